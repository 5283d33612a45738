"""The MODEL's Quest sparse decode against a float64 restatement of the same model (tests/_quest_model_ref.py, made
trustworthy by tests/test_quest_model_ref_host.py): layer skip, the re-plan with the real budget in the middle of a forward,
``token_budget // page_size`` pages including the current one, the last page always attended and never scored, metadata
kept from the prefill into 24 decode tokens across page boundaries, the change from "attend everything" to sparse during
graph replay, the device-state planner of captured and batched steps, Qwen3's q/k norm on the sparse path, bf16.

The selection is discrete, so a free-running reference diverges at the first near-tie.  Instead, per decode token:
the device step runs; its selection is read (eager module path: every ``decode_topk`` call; captured steps: the handler's
selection output = the last sparse layer's) and translated to logical pages; the float64 model and a yardstick (the same
code in the model's dtype) run the same token FORCED to that selection; the next token is float64's argmax.  Checked:

1. each head selected B - 1 distinct logical pages in [0, P - 2];
2. the selection is valid against float64: with delta = max |yardstick score - float64 score| over the (step, layer) block,
   no unselected page beats a selected one by more than 3 delta in float64 (two scores, each allowed 1.5 x the yardstick's
   own deviation), and the device's selected values are within 1.5 delta + one ulp of the float64 scores of their pages;
3. that is not vacuous: the share of (step, layer, head) rows whose float64 gap at the cut exceeds 3 delta -- the selection
   is then forced -- is at least 70 % in fp16 and 20 % in bf16 (computed from reference and yardstick alone);
4. logits of the prefill's last position and of every token: rel(got, r64) <= 1.5 rel(yardstick, r64) + 2e-3, finite;
5. at the end, per layer, the device's K (after RoPE) and V rows against the reference's by the same rule.

Measured on an MI355X (seed 11; worst rel over prefill, tokens and caches; delta as a share of the block's score spread,
mean; decided = rows whose float64 gap at the cut exceeds 3 delta; other = rows whose device set is not float64's own top-k):

  case                                   rel(got, r64)  rel(yardstick, r64)  delta / spread  decided        other
  eager llama fp16, 4 layers             1.9e-3         2.2e-3               0.23 %          163 / 192 85 %  1
  eager qwen3 fp16, 4 layers             2.9e-3         3.7e-3               0.30 %          160 / 192 83 %  2
  eager mistral fp16, 4 layers           2.4e-3         2.7e-3               0.30 %          147 / 192 77 %  3
  eager llama bf16, 4 layers             1.5e-2         1.7e-2               1.68 %           76 / 192 40 %  14
  captured llama fp16, module path       1.8e-3         2.0e-3               0.19 %           89 / 96  93 %  1
  captured llama fp16, fused layers      1.5e-3         2.0e-3               0.19 %           89 / 96  93 %  2
  captured qwen3 fp16, fused, NHD_ROT    1.8e-3         3.0e-3               0.31 %           81 / 96  84 %  1
  captured mistral fp16, fused           1.8e-3         2.4e-3               0.25 %           79 / 96  82 %  0
  captured qwen3 bf16, fused layers      1.5e-2         2.2e-2               2.28 %           28 / 96  29 %  9
  entering the sparse regime (60 tokens) 1.5e-3         1.8e-3               0.22 %           79 / 80  99 %  0
  batched, 200 tokens                    1.6e-3         2.0e-3               0.19 %           89 / 96  93 %  2
  batched, 77 tokens                     1.4e-3         1.8e-3               0.23 %           91 / 96  95 %  0
  batched, 40 tokens (never sparse)      1.3e-3         1.8e-3               --               --             --
"""
import copy

import pytest
import torch

from _quest_model_ref import QuestModelRef

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
PAGE, BUDGET, VOCAB, STEPS = 16, 4, 320, 24   # token_budget 64 = 4 pages, the current one included
SEED = 11


def _config(kind, layers):
    from quest_amd.models.llama import LlamaConfig

    common = dict(vocab_size=VOCAB, intermediate_size=1024, num_hidden_layers=layers, num_attention_heads=4,
                  num_key_value_heads=2, max_position_embeddings=1024)
    if kind == "llama":    # GQA 4 / 2 x 128, the kernels' RoPE formula
        return LlamaConfig(hidden_size=512, **common)
    if kind == "qwen3":    # 4 / 2 x 64 at hidden 512, per-head q/k norm, theta 1e6 through the frequency table
        return LlamaConfig(hidden_size=512, head_dim=64, qk_norm=True, model_type="qwen3", rms_norm_eps=1e-6,
                           rope_theta=1e6, **common)
    assert kind == "mistral"  # 4 / 2 x 128 at hidden 640
    return LlamaConfig(hidden_size=640, head_dim=128, model_type="mistral", rope_theta=1e6, **common)


def _model(kind, layers, dtype, fused=True):
    """Seeded weights normal(0, 0.04), norm weights ones, q/k norm weights uniform 0.5 .. 1.5 (drawn on the CPU: the same
    for every model of a (kind, layers, dtype))."""
    from quest_amd.models.llama import LlamaForCausalLM

    cfg = _config(kind, layers)
    with torch.device(DEV):
        m = LlamaForCausalLM(cfg, fused=fused).to(dtype)
    g = torch.Generator().manual_seed(SEED)
    for n, p in m.named_parameters():
        if "q_norm" in n or "k_norm" in n:
            w = 0.5 + torch.rand(p.shape, generator=g)
        elif "norm" in n:
            w = torch.ones(p.shape)
        else:
            w = torch.randn(p.shape, generator=g) * 0.04
        p.data.copy_(w)
    return m.eval(), cfg


def _prompt(n, i=0):
    return (torch.arange(n) * (37 + 2 * i) + 11 + i) % VOCAB


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _ulp(x, dtype):
    bits = 10 if dtype == torch.float16 else 7
    return 2.0 ** (torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14))) - bits)


_PREFILLED = {}  # (kind, layers, dtype, prompt) -> the two restatements after the prompt and their logits: computed once


class _Sequence:
    """The float64 model and the yardstick of one sequence, and the running figures of its checks."""

    def __init__(self, model, cfg, kind, dtype, prompt, name):
        key = (kind, cfg.num_hidden_layers, dtype, tuple(prompt.tolist()))
        if key not in _PREFILLED:
            sd = model.state_dict()
            refs = [QuestModelRef(sd, cfg, PAGE, BUDGET, dtype=t) for t in (torch.float64, dtype)]
            _PREFILLED[key] = (refs, [r.prefill(prompt)[-1] for r in refs])
        (self.r64, self.yard), self.first = copy.deepcopy(_PREFILLED[key])
        assert torch.equal(self.r64.w["model.layers.0.mlp.up_proj.weight"],
                           model.model.layers[0].mlp.up_proj.weight.detach().cpu().double())
        self.name, self.dtype, self.layers, self.hq = name, dtype, cfg.num_hidden_layers, cfg.num_attention_heads
        self.rows = self.forced_rows = self.differ = self.sparse_steps = 0
        self.delta_rel, self.worst = [], [0.0, 0.0]

    def _check(self, got, yard, r64, what):
        got, yard = got.detach().float().cpu().double().reshape(-1), yard.double()
        e, y = _rel(got, r64), _rel(yard, r64)
        print(f"{self.name} {what}: rel(got, r64)={e:.4e} rel(yardstick, r64)={y:.4e} rel(got, yardstick)={_rel(got, yard):.4e}")
        self.worst = [max(self.worst[0], e), max(self.worst[1], y)]
        assert torch.isfinite(got).all(), what
        assert e <= 1.5 * y + 2e-3, f"{self.name} {what}: {e:.4e} vs the yardstick's {y:.4e}"

    def prefill(self, got) -> int:
        self._check(got, self.first[1], self.first[0], "prefill, last position")
        return int(self.first[0].argmax())

    def step(self, token, got, observed, table, t) -> int:
        """``observed``: layer -> (physical pages ``[Hq, B - 1]``, selected values or None) as read from the device after its
        step on ``token``; ``table``: the sequence's page table (logical -> physical).  Returns the next token."""
        n_pages = -(-(self.r64.seqlen + 1) // PAGE)
        sparse = n_pages > BUDGET
        what = f"token {t} ({self.r64.seqlen + 1} tokens, {n_pages} pages)"
        forced = {}
        if sparse:
            assert len(table) == n_pages
            assert sorted(observed) == list(range(2, self.layers)), f"{what}: selections of layers {sorted(observed)}"
            logical = {int(p): j for j, p in enumerate(table)}
            for layer, (phys, _) in observed.items():
                # 1. shape: B - 1 distinct logical pages in [0, P - 2] per head
                assert tuple(phys.shape) == (self.hq, BUDGET - 1), f"{what} layer {layer}: {tuple(phys.shape)}"
                rows = [[logical.get(int(p), -1) for p in row] for row in phys.tolist()]
                for h, row in enumerate(rows):
                    assert len(set(row)) == BUDGET - 1 and min(row) >= 0 and max(row) <= n_pages - 2, \
                        f"{what} layer {layer} head {h}: physical pages {phys[h].tolist()} = logical {row}"
                forced[layer] = torch.tensor(rows)
        else:
            assert not observed, f"{what}: the budget covers the cache, yet layers {sorted(observed)} selected pages"
        l64, i64 = self.r64.step(token, forced)
        ly, iy = self.yard.step(token, forced)
        assert sorted(i64) == sorted(iy) == sorted(forced)
        for layer in sorted(i64):
            # 2. validity against float64, 3. how many rows the float64 scores decide
            s64, sy, pages = i64[layer].scores, iy[layer].scores.double(), i64[layer].pages
            delta = float((sy - s64).abs().max())
            sel = torch.zeros_like(s64, dtype=torch.bool).scatter_(1, pages, True)
            worst_sel = s64.masked_fill(~sel, float("inf")).min(1).values
            best_unsel = s64.masked_fill(sel, float("-inf")).max(1).values
            top = s64.sort(dim=1, descending=True).values
            decided = (top[:, BUDGET - 2] - top[:, BUDGET - 1]) > 3 * delta
            own = [set(r) != set(o) for r, o in zip(pages.tolist(), i64[layer].own.tolist())]
            self.rows += self.hq
            self.forced_rows += int(decided.sum())
            self.differ += sum(own)
            self.delta_rel.append(delta / float(s64.max() - s64.min()))
            over = float((best_unsel - worst_sel).max())
            print(f"{self.name} {what} layer {layer}: delta={delta:.3e} ({self.delta_rel[-1]:.2%} of the spread) "
                  f"unselected - selected <= {over:.3e} decided rows {int(decided.sum())}/{self.hq} other than float64's {sum(own)}")
            assert over <= 3 * delta, f"{what} layer {layer}: an unselected page beats a selected one by {over:.3e} > 3 x {delta:.3e}"
            val = observed[layer][1]
            if val is not None:
                val = val.double()
                err = (val - s64.gather(1, pages)).abs()
                bound = 1.5 * delta + _ulp(val, self.dtype)
                assert bool((err <= bound).all()), f"{what} layer {layer}: selected values off by {float(err.max()):.3e}"
        self.sparse_steps += bool(i64)
        self._check(got, ly, l64, what)
        return int(l64.argmax())

    def finish(self, ctl, kv_layer, seqlen):
        """5. the caches, per layer, and 3. the floor; prints the case's figures."""
        from quest_amd.utils.utils import TensorLayout

        assert ctl.kv_cache.seqlen == seqlen == self.r64.seqlen == self.yard.seqlen
        idx = torch.tensor(list(ctl.kv_cache.indicies), device=DEV)
        for layer in range(self.layers):
            pages = TensorLayout.to_logical(kv_layer(layer)[idx].view(torch.int16), ctl.layout).view(self.dtype)
            n, _, S, H, D = pages.shape
            for slot, name, ref in ((0, "K", "k"), (1, "V", "v")):
                got = pages[:, slot].reshape(n * S, H, D)[:seqlen]
                self._check(got, getattr(self.yard, ref)[layer].reshape(-1), getattr(self.r64, ref)[layer].reshape(-1),
                            f"layer {layer} {name} cache")
        share = self.forced_rows / max(self.rows, 1)
        mean_delta = sum(self.delta_rel) / max(len(self.delta_rel), 1)
        print(f"{self.name} SUMMARY: rel(got, r64) <= {self.worst[0]:.3e} rel(yardstick, r64) <= {self.worst[1]:.3e} "
              f"delta / spread {mean_delta:.2%} decided rows {self.forced_rows}/{self.rows} = {share:.0%} "
              f"rows other than float64's own top-k {self.differ} sparse steps {self.sparse_steps}")
        return share


class _SelectionOut:
    """The handler's selection output ``[n, Hq, B - 1]`` at the head of twice the memory: what lies behind stays untouched
    if the launches write B - 1 entries per head and no more."""

    def __init__(self, handler, n, hq, dtype):
        size = n * hq * (BUDGET - 1)
        self._idx = torch.full((2 * size + 64,), -1, dtype=torch.int32, device=DEV)
        self._val = torch.zeros(2 * size + 64, dtype=dtype, device=DEV)
        self.idx, self.val = self._idx[:size].view(n, hq, BUDGET - 1), self._val[:size].view(n, hq, BUDGET - 1)
        self.size, self.handler = size, handler
        handler.set_selection_out(self.val, self.idx)

    def reset(self):
        self.idx.fill_(-1)

    def read(self, i):
        return self.idx[i].cpu(), self.val[i].cpu()

    def close(self):
        self.handler.set_selection_out(None, None)

    def check_guard(self):
        assert bool((self._idx[self.size:] == -1).all()) and bool((self._val[self.size:] == 0).all()), \
            "the launches wrote more than B - 1 selections per head"


def _floor(share, dtype):
    assert share >= (0.70 if dtype == torch.float16 else 0.20), \
        f"only {share:.0%} of the rows are decided by the float64 scores: choose another seed"


# ---------------------------------------------------------------------------- eager module path: every sparse layer observed
@pytest.mark.parametrize("kind,dtype", [("llama", torch.float16), ("qwen3", torch.float16), ("mistral", torch.float16),
                                        ("llama", BF)], ids=["llama", "qwen3", "mistral", "llama_bf16"])
def test_eager_module_path(kind, dtype, monkeypatch):
    """4 layers: two dense, two sparse -- layer 3 must score with its own query against its own metadata.  ``decode_topk`` is
    never called from layers 0 and 1 and exactly once per token from layers 2 and 3."""
    import quest_amd.utils as qutils

    dev = torch.device(DEV)
    m, cfg = _model(kind, 4, dtype, fused=False)
    m.quest_init(PAGE, 512, token_budget=PAGE * BUDGET, dtype=dtype)
    ctl = m.model.iController
    prompt = _prompt(200)
    seq = _Sequence(m, cfg, kind, dtype, prompt, f"eager {kind} {dtype}")
    current, calls, real = {}, [], qutils.decode_topk
    for i, layer in enumerate(m.model.layers):
        layer.self_attn.register_forward_pre_hook(lambda mod, args, i=i: current.__setitem__("layer", i))

    def spy(scores, controller):
        real(scores, controller)
        calls.append((current["layer"], controller.topk_dindices_buffer.cpu(), controller.topk_dout_buffer.cpu()))

    monkeypatch.setattr(qutils, "decode_topk", spy)
    with torch.inference_mode():
        tok = seq.prefill(m(input_ids=prompt[None].to(dev))[0, -1])
        assert not calls
        for t in range(STEPS):  # 201 .. 224 tokens: token 209 opens the 14th page, token 224 fills it
            calls.clear()
            got = m(input_ids=torch.tensor([[tok]], device=dev))[0, -1]
            assert [c[0] for c in calls] == [2, 3], f"token {t}: decode_topk called from layers {[c[0] for c in calls]}"
            tok = seq.step(tok, got, {c[0]: (c[1], c[2]) for c in calls}, ctl.kv_cache.indicies, t)
    assert seq.sparse_steps == STEPS
    _floor(seq.finish(ctl, ctl.kv_layer, 200 + STEPS), dtype)


# ---------------------------------------------------------------------------- captured steps: the last sparse layer observed
def _captured(kind, dtype, fused_layers, expect_fused, kv_layout="NHD", prompt_len=200):
    dev = torch.device(DEV)
    m, cfg = _model(kind, 3, dtype)
    m.quest_init(PAGE, 512, token_budget=PAGE * BUDGET, dtype=dtype, kv_layout=kv_layout)
    ctl = m.model.iController
    prompt = _prompt(prompt_len)
    seq = _Sequence(m, cfg, kind, dtype, prompt, f"captured {kind} {dtype} {kv_layout} fused_layers={fused_layers}")
    with torch.inference_mode():
        tok = seq.prefill(m(input_ids=prompt[None].to(dev))[0, -1])
        out = _SelectionOut(ctl._decode_handler, 1, cfg.num_attention_heads, dtype)
        try:
            m.capture_decode_graph(fused_layers=fused_layers)
            assert m.fused_layers is expect_fused
            for t in range(STEPS):
                out.reset()
                got = m.decode_graph_step(input_ids=torch.tensor([[tok]], device=dev))[0, -1]
                sparse = len(ctl.kv_cache.indicies) > BUDGET
                tok = seq.step(tok, got, {2: out.read(0)} if sparse else {}, ctl.kv_cache.indicies, t)
        finally:
            out.close()
    out.check_guard()
    share = seq.finish(ctl, ctl.kv_layer, prompt_len + STEPS)
    return seq, share


def test_captured_module_path():
    seq, share = _captured("llama", torch.float16, False, False)
    assert seq.sparse_steps == STEPS
    _floor(share, torch.float16)


@pytest.mark.parametrize("kind,kv_layout", [("llama", "NHD"), ("qwen3", "NHD_ROT"), ("mistral", "NHD")])
def test_captured_fused_layers_default(kind, kv_layout):
    seq, share = _captured(kind, torch.float16, None, True, kv_layout)
    assert seq.sparse_steps == STEPS
    _floor(share, torch.float16)


def test_captured_fused_layers_bf16():
    seq, share = _captured("qwen3", BF, True, True)
    assert seq.sparse_steps == STEPS
    _floor(share, BF)


def test_entering_the_sparse_regime_during_replay():
    """60 prompt tokens = 4 pages: captured while the budget covers the cache; token 65 opens the fifth page and the same
    graph starts to select 3 of 4 pages, token 81 the sixth (3 of 5)."""
    seq, _ = _captured("llama", torch.float16, None, True, prompt_len=60)
    assert seq.sparse_steps == STEPS - 4 and seq.rows > 0  # every sparse step has P - 1 > B - 1 candidates


def test_batched_three_ragged_prompts():
    """200, 77 and 40 tokens over the shared pools, fused n-token launches: the 40-token sequence stays within the budget
    (its selection rows are ignored, its logits and caches still checked)."""
    dev = torch.device(DEV)
    lens, dtype = (200, 77, 40), torch.float16
    m, cfg = _model("llama", 3, dtype)
    m.quest_init_batched(len(lens), PAGE, 512, token_budget=PAGE * BUDGET)
    b = m.model.bController
    seqs = [_Sequence(m, cfg, "llama", dtype, _prompt(L, i), f"batched sequence {i}") for i, L in enumerate(lens)]
    with torch.inference_mode():
        toks = [s.prefill(m.prefill_sequence(i, _prompt(L, i)[None].to(dev))[0, -1]) for i, (s, L) in enumerate(zip(seqs, lens))]
        out = _SelectionOut(b._decode_handler, len(lens), cfg.num_attention_heads, dtype)
        try:
            m.capture_decode_graph_batched()
            assert m.fused_layers
            for t in range(STEPS):
                out.reset()
                got = m.decode_graph_step_batched(torch.tensor(toks, device=dev))
                for i, (s, c) in enumerate(zip(seqs, b.seqs)):
                    sparse = len(c.kv_cache.indicies) > BUDGET
                    toks[i] = s.step(toks[i], got[i, -1], {2: out.read(i)} if sparse else {}, c.kv_cache.indicies, t)
        finally:
            out.close()
    out.check_guard()
    shares = [s.finish(c, b.kv_layer, L + STEPS) for s, c, L in zip(seqs, b.seqs, lens)]
    assert [s.sparse_steps for s in seqs] == [STEPS, STEPS, 0]
    rows, decided = sum(s.rows for s in seqs), sum(s.forced_rows for s in seqs)
    print(f"batched: decided rows {decided}/{rows}, per sequence {shares}")
    _floor(decided / rows, dtype)
