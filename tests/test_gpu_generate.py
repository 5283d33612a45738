"""``generate`` / ``generate_batched`` (device-side sampling inside the captured step) against the loop every caller wrote
before: ``decode_graph_step`` -> logits to the host -> the contract's token rule (tests/_sampling_ref.py) -> next id.

Greedy tokens are compared under the contract's greedy rule (largest 16-bit key, ties to the lowest index), not with
``torch.argmax``: fp16 logit ties are not rare at this vocabulary and argmax does not promise which of them it returns."""
import numpy as np
import pytest
import torch

import _sampling_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VOCAB, PAGE, MAX_LEN, BUDGET = 1000, 16, 512, 96
NAME = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def _model(dtype=torch.float16, n_seqs=None):
    """A tiny random checkpoint (3 layers: 2 dense + 1 sparse, hidden 256, GQA 2), built as the other model tests build theirs."""
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(vocab_size=VOCAB, hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=4,
                      num_key_value_heads=2)
    torch.manual_seed(11)
    with torch.device(DEV):
        m = LlamaForCausalLM(cfg).to(dtype)
    for p_ in m.parameters():
        p_.data.normal_(0, 0.05)
    if n_seqs is None:
        m.quest_init(PAGE, MAX_LEN, token_budget=BUDGET, dtype=dtype)
    else:
        m.quest_init_batched(n_seqs, PAGE, MAX_LEN, token_budget=BUDGET, dtype=dtype)
    return m


def _prompt(length: int, salt: int = 0) -> torch.Tensor:
    return ((torch.arange(length, device=DEV)[None] * 7 + salt * 131) % VOCAB)


PROMPTS = [(300, 0), (275, 1), (330, 2)]  # unequal lengths; the runs cross page and metadata-page boundaries


def _bits(logits: torch.Tensor) -> np.ndarray:
    """``[.., V]`` fp16 / bf16 logits -> ``[rows, V]`` stored bits on the host."""
    return logits.reshape(-1, logits.size(-1)).view(torch.int16).cpu().numpy().view(np.uint16)


def _host_loop(dtype, fused, n_new, choose, prompts=None):
    """The existing way: prefill, capture (no sampler), then per token logits -> host -> ``choose(seq, step, bits)`` ->
    next id.  -> (tokens ``[n][n_new]``, logits bits ``[n_new][n, V]``)."""
    batched = prompts is not None
    prompts = prompts or [PROMPTS[0]]
    m = _model(dtype, len(prompts) if batched else None)
    with torch.inference_mode():
        if batched:
            logits = torch.cat([m.prefill_sequence(i, _prompt(*p)).view(1, -1) for i, p in enumerate(prompts)])
            m.capture_decode_graph_batched(fused_layers=fused)
        else:
            logits = m(input_ids=_prompt(*prompts[0])).view(1, -1)
            m.capture_decode_graph(fused_layers=fused)
        tokens, seen = [[] for _ in prompts], []
        for t in range(n_new):
            b = _bits(logits)
            seen.append(b)
            ids = [choose(i, t, b[i]) for i in range(len(prompts))]
            for i, tok in enumerate(ids):
                tokens[i].append(tok)
            if t + 1 < n_new:
                if batched:
                    logits = m.decode_graph_step_batched(torch.tensor(ids, device=DEV))
                else:
                    logits = m.decode_graph_step(input_ids=torch.tensor([[ids[0]]], device=DEV))
    return tokens, seen


@pytest.mark.parametrize("dtype,fused", [(torch.float16, False), (torch.float16, True), (torch.bfloat16, False)],
                         ids=["module-path", "fused-layers", "bf16"])
def test_greedy_generate_equals_the_host_loop(dtype, fused):
    n_new = 40
    want, _ = _host_loop(dtype, fused, n_new, lambda i, t, b: ref.greedy_token(b))
    m = _model(dtype)
    got = m.generate(_prompt(*PROMPTS[0]), n_new, fused_layers=fused)
    assert m.fused_layers == fused
    assert got.tolist() == want[0]


def test_greedy_generate_batched_equals_the_host_loop():
    n_new = 24
    want, _ = _host_loop(torch.float16, None, n_new, lambda i, t, b: ref.greedy_token(b), prompts=PROMPTS)
    m = _model(torch.float16, len(PROMPTS))
    got = m.generate_batched([_prompt(*p) for p in PROMPTS], n_new)
    assert [g.tolist() for g in got] == want
    assert len({tuple(w) for w in want}) == len(PROMPTS)  # three different sequences


def test_sampled_tokens_are_the_restatements_choice_from_the_host_loops_logits():
    """T = 0.8, top_k 50, top_p 0.9: feed ``generate``'s tokens back through the existing loop and check each one against
    the restatement on that step's logits -- decided steps exactly, undecided ones (at most 1 % of the draws) within the
    contract's allowance."""
    from quest_amd.utils import SamplingParams

    n_new, seed, L = 40, 0x5EED0123456789AB, PROMPTS[0][0]
    m = _model()
    got = m.generate(_prompt(*PROMPTS[0]), n_new, sampling=SamplingParams(0.8, 50, 0.9, seed), fused_layers=True).tolist()
    assert len(got) == n_new
    _, seen = _host_loop(torch.float16, True, n_new, lambda i, t, b: got[t])
    rows = [ref.sample_row(seen[t][0], "fp16", 0.8, 50, 0.9, seed, L + t) for t in range(n_new)]
    problems = [f"step {t}: {msg}" for t, r in enumerate(rows) if (msg := ref.check_token(r, got[t]))]
    assert not problems, "\n".join(problems)
    undecided = sum(ref.is_undecided(r) for r in rows)
    print(f"{undecided} undecided of {n_new} draws; kept sets of {min(r.kept for r in rows)}..{max(r.kept for r in rows)} tokens")
    assert undecided <= ref.MAX_UNDECIDED * n_new
    assert len(set(got)) > n_new // 2 and max(r.kept for r in rows) > 1  # a real draw, not a greedy run in disguise


def _sampled_steps(m, ctl, prompts, params, n_new, seq_of_interest, fused):
    """Drive the captured step with a sampler by hand, keeping each step's logits: -> (tokens, logits bits) of one sequence."""
    from quest_amd.utils import Sampler

    batched = len(prompts) > 1
    sampler = Sampler(len(prompts), VOCAB, DEV, max_tokens=n_new)
    for i, p in enumerate(params):
        sampler.set_params(i, p)
    with torch.inference_mode():
        if batched:
            logits = torch.cat([m.prefill_sequence(i, _prompt(*p)).view(1, -1) for i, p in enumerate(prompts)])
        else:
            logits = m(input_ids=_prompt(*prompts[0])).view(1, -1)
        seen = [_bits(logits)[seq_of_interest]]
        first = torch.empty(len(prompts), 1, 256, dtype=torch.float16, device=DEV)
        sampler.sample(logits, positions=torch.tensor([p[0] for p in prompts], dtype=torch.int32, device=DEV),
                       embed=m.model.embed_tokens.weight, next_input=first.view(len(prompts), -1))
        (m.capture_decode_graph_batched if batched else m.capture_decode_graph)(fused_layers=fused, sampler=sampler)
        m.graph_input.copy_(first)
        for _ in range(1, n_new):
            m._graph.replay()
            ctl(m).prepare_metadata(1)
            seen.append(_bits(m.graph_logits)[seq_of_interest])
    return sampler.sequences()[seq_of_interest].tolist(), seen


@pytest.mark.parametrize("fused", [False, True], ids=["module-path", "fused-layers"])
def test_a_sequence_samples_the_same_alone_and_inside_a_batch_while_the_logits_agree(fused):
    """Same prompt, parameters and seed alone and as sequence 1 of a batch of three: the tokens are equal for as long as
    the two runs' logits agree bit for bit (the draw depends on seed, position and token index only).  The prompt's
    logits always do -- both runs prefill through the single-sequence path -- so the first token is always compared.
    From the first decode step on the alone run takes the batch-1 projection launches (GEMV, or rocBLAS with one row)
    and the batch the n-token ones, whose sums round in another order: where their logits differ in the last bits the
    comparison ends (the step is printed).  On an MI355X the module path's logits agree for all 16 steps here (rocBLAS
    rounds one row and three alike at these shapes); the fused layers' agree for the first 4 and then differ in the last
    bits, the n-token kernels against the batch-1 GEMVs -- the 16 tokens were equal in both runs all the same."""
    from quest_amd.utils import SamplingParams

    n_new = 16
    mine = SamplingParams(0.8, 50, 0.9, 77)
    alone_t, alone_l = _sampled_steps(_model(), lambda m: m.model.iController, [PROMPTS[1]], [mine], n_new, 0, fused)
    batch_t, batch_l = _sampled_steps(_model(n_seqs=3), lambda m: m.model.bController, PROMPTS,
                                      [SamplingParams(1.0, 0, 1.0, 5), mine, SamplingParams(0.0)], n_new, 1, fused)
    assert np.array_equal(alone_l[0], batch_l[0]), "both runs prefill sequence 1 the same way"
    agree = 0
    while agree < n_new and np.array_equal(alone_l[agree], batch_l[agree]):
        assert alone_t[agree] == batch_t[agree], agree
        agree += 1
    same = sum(a == b for a, b in zip(alone_t, batch_t))
    print(f"logits agree bit for bit for {agree} of {n_new} steps; {same} of {n_new} tokens equal")
    assert agree >= 1


def test_generate_stops_at_the_eos_and_a_batch_runs_on():
    n_new = 24
    greedy = lambda i, t, b: ref.greedy_token(b)
    want, _ = _host_loop(torch.float16, None, n_new, greedy)
    eos = want[0][5]
    cut = lambda toks: toks[:toks.index(eos) + 1] if eos in toks else toks
    assert len(cut(want[0])) <= 6
    m = _model()
    got = m.generate(_prompt(*PROMPTS[0]), n_new, eos_token_id=eos, sync_every=4)
    assert got.tolist() == cut(want[0])
    assert m.model.iController.kv_cache.seqlen < PROMPTS[0][0] + n_new  # it did stop stepping early
    # in a batch: sequence 0 ends at its eos, the others run on (a finished sequence steps on with the pad id unseen)
    want, _ = _host_loop(torch.float16, None, n_new, greedy, prompts=PROMPTS)
    eos = want[0][5]
    m = _model(n_seqs=len(PROMPTS))
    got = m.generate_batched([_prompt(*p) for p in PROMPTS], n_new, eos_token_id=[eos], sync_every=4)
    assert got[0].tolist() == cut(want[0]) and len(got[0]) <= 6
    # (the others' logits do not depend on sequence 0's input: no data is shared between the sequences of a launch)
    assert [g.tolist() for g in got[1:]] == [cut(w) for w in want[1:]]
    assert max(len(g) for g in got[1:]) > 6


def test_a_graph_captured_without_a_sampler_still_serves_decode_graph_step():
    """``sampler=None`` is the graph as it was: after a ``generate`` the same model re-captures without one and its
    ``decode_graph_step`` gives the logits of a model that never saw a sampler."""
    n_new = 8
    want, seen = _host_loop(torch.float16, True, n_new, lambda i, t, b: ref.greedy_token(b))
    m = _model()
    assert m.generate(_prompt(*PROMPTS[0]), n_new, fused_layers=True).tolist() == want[0]
    m.quest_clear()
    with torch.inference_mode():
        logits = m(input_ids=_prompt(*PROMPTS[0]))
        m.capture_decode_graph(fused_layers=True)
        assert m._graph_sampler is None
        for t in range(n_new - 1):
            assert np.array_equal(_bits(logits)[0], seen[t][0]), t
            logits = m.decode_graph_step(input_ids=torch.tensor([[want[0][t]]], device=DEV))
