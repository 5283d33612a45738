"""What makes tests/_quest_model_ref.py trustworthy as the reference of tests/test_gpu_model_sparse_reference.py (CPU):

* dense, in float64, it reproduces transformers' Llama (GQA, linear RoPE), Mistral (own head_dim) and Qwen3 (q/k norm,
  tied embeddings, theta 1e6) -- prefill at all positions and 20 greedy tokens -- at 1e-9 relative: float64 rounding
  (2^-53 per operation, a few thousand operations deep) and nothing else;
* its page scores equal the oracle's estimate on metadata the oracle's append built from the same fp16 K, at fp16
  rounding of the float64 score, and its pages equal the oracle's top-k on rows without a tie at the cut;
* properties of the decode rule: forcing its own selection changes nothing, a budget that covers the cache is dense
  attention, the last page is always attended and never scored, the first two layers attend everything.
* the fp16 / bf16 yardstick really computes in its type: a few unit roundoffs from float64, no less and no more.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _quest_model_ref import QuestModelRef

PAGE = 16
N_NEW = 20


def _rel(a, b):
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------- dense against transformers
def _hf_model(kind, transformers):
    """The families of tests/test_gpu_hf_checkpoint.py / test_gpu_model_families.py (``_hf_class``), and what the
    restatement needs to know of their configs."""
    common = dict(vocab_size=320, intermediate_size=1024, num_hidden_layers=3, max_position_embeddings=1024)
    if kind == "llama":  # GQA 4 / 2, linear position interpolation
        rope = {"rope_type": "linear", "factor": 4.0, "rope_theta": 10000.0}
        cls, hcfg = transformers.LlamaForCausalLM, transformers.LlamaConfig(
            hidden_size=512, num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=1e-5, rope_parameters=rope, **common)
        cfg = dict(hidden_size=512, head_dim=None, rms_norm_eps=1e-5, qk_norm=False, rope_theta=1e4, rope_scaling=rope)
    elif kind == "qwen3":  # head_dim 64 at hidden 512 with 4 heads, q/k norm, tied embeddings, eps 1e-6
        cls, hcfg = transformers.Qwen3ForCausalLM, transformers.Qwen3Config(
            hidden_size=512, head_dim=64, num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=1e-6,
            tie_word_embeddings=True, rope_parameters={"rope_type": "default", "rope_theta": 1000000.0}, **common)
        cfg = dict(hidden_size=512, head_dim=64, rms_norm_eps=1e-6, qk_norm=True, rope_theta=1e6, rope_scaling=None)
    else:  # mistral: head_dim 128 at hidden 640 with 4 heads
        cls, hcfg = transformers.MistralForCausalLM, transformers.MistralConfig(
            hidden_size=640, head_dim=128, num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=1e-5,
            sliding_window=None, rope_parameters={"rope_type": "default", "rope_theta": 1000000.0}, **common)
        cfg = dict(hidden_size=640, head_dim=128, rms_norm_eps=1e-5, qk_norm=False, rope_theta=1e6, rope_scaling=None)
    torch.manual_seed(3)
    hcfg._attn_implementation = "eager"
    hf = cls(hcfg)
    for p in hf.parameters():
        p.data.mul_(2.0)
    g = torch.Generator().manual_seed(9)
    for n, p in hf.named_parameters():
        if "q_norm" in n or "k_norm" in n:
            p.data.copy_(0.5 + torch.rand(p.shape, generator=g))
        elif "norm" in n:
            p.data.fill_(1.0)
    return hf.double().eval(), SimpleNamespace(num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2, **cfg)


@pytest.mark.parametrize("kind", ["llama", "mistral", "qwen3"])
def test_dense_float64_matches_transformers(kind):
    """transformers keeps the RMSNorm statistics, the softmax and the rotary table in float32 whatever the model's type, a
    ``.double()`` model included, so it is compared with the restatement's ``acc_dtype=float32`` form: every float32
    expression is the same torch expression on the same values, and what is left is float64 rounding.  The all-float64
    reference then differs from that form by float32 rounding of those three only."""
    transformers = pytest.importorskip("transformers")
    hf, cfg = _hf_model(kind, transformers)
    if kind == "qwen3":
        assert hf.lm_head.weight.data_ptr() == hf.model.embed_tokens.weight.data_ptr()
    prompt = (torch.arange(150) * 37 + 11) % 320
    sd = {k: v for k, v in hf.state_dict().items() if not (kind == "qwen3" and k == "lm_head.weight")}
    ref = QuestModelRef(sd, cfg, PAGE, 1 << 20, dtype=torch.float64, acc_dtype=torch.float32)
    r64 = QuestModelRef(sd, cfg, PAGE, 1 << 20, dtype=torch.float64)
    with torch.no_grad():
        out = hf(input_ids=prompt[None], use_cache=True)
    got, got64 = ref.prefill(prompt), r64.prefill(prompt)
    worst = _rel(got, out.logits[0])
    wide = _rel(got64, got)
    assert _rel(got[-1], out.logits[0, -1]) <= 1e-9
    past, tok = out.past_key_values, out.logits[0, -1].argmax()
    for t in range(N_NEW):
        with torch.no_grad():
            out = hf(input_ids=tok.view(1, 1), past_key_values=past, use_cache=True)
        past = out.past_key_values
        got, info = ref.step(int(tok))
        got64, _ = r64.step(int(tok))
        assert not info
        worst, wide = max(worst, _rel(got, out.logits[0, -1])), max(wide, _rel(got64, got))
        tok = out.logits[0, -1].argmax()
    print(f"{kind}: rel(restatement, transformers) <= {worst:.3e}; float64 against float32 statistics <= {wide:.3e}")
    assert ref.seqlen == r64.seqlen == 150 + N_NEW
    assert worst <= 1e-9
    # float32 rounding (6e-8) of two norms, one softmax and one rotary table per layer, 3 layers and the final norm
    assert wide <= 1e-5


# ---------------------------------------------------------------------------- a small random model
def _state(cfg, seed, vocab=320, inter=256, tied=False):
    g = torch.Generator().manual_seed(seed)
    d = cfg.head_dim or cfg.hidden_size // cfg.num_attention_heads
    hid, hq, hkv = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads

    def w(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * 0.04

    sd = {"model.embed_tokens.weight": w(vocab, hid), "model.norm.weight": torch.ones(hid, dtype=torch.float64)}
    if not tied:
        sd["lm_head.weight"] = w(vocab, hid)
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        sd.update({p + "self_attn.q_proj.weight": w(hq * d, hid), p + "self_attn.k_proj.weight": w(hkv * d, hid),
                   p + "self_attn.v_proj.weight": w(hkv * d, hid), p + "self_attn.o_proj.weight": w(hid, hq * d),
                   p + "mlp.gate_proj.weight": w(inter, hid), p + "mlp.up_proj.weight": w(inter, hid),
                   p + "mlp.down_proj.weight": w(hid, inter),
                   p + "input_layernorm.weight": torch.ones(hid, dtype=torch.float64),
                   p + "post_attention_layernorm.weight": torch.ones(hid, dtype=torch.float64)})
        if cfg.qk_norm:
            sd[p + "self_attn.q_norm.weight"] = 0.5 + torch.rand(d, generator=g, dtype=torch.float64)
            sd[p + "self_attn.k_norm.weight"] = 0.5 + torch.rand(d, generator=g, dtype=torch.float64)
    return sd


def _cfg(qk_norm=False, layers=4):
    return SimpleNamespace(hidden_size=256, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
                           head_dim=64, rms_norm_eps=1e-5, qk_norm=qk_norm, rope_theta=1e4, rope_scaling=None)


class _Recording(QuestModelRef):
    """Keeps, per decode step, the cache rows every layer attended."""

    def _attend(self, layer, q, tokens):
        self.attended[layer] = tokens.clone()
        return super()._attend(layer, q, tokens)

    def step(self, token, forced=None):
        self.attended = {}
        return super().step(token, forced)


@pytest.mark.parametrize("qk_norm", [False, True])
def test_decode_rule_properties(qk_norm):
    cfg = _cfg(qk_norm)
    sd = _state(cfg, 5, tied=qk_norm)
    B = 4
    prompt = (torch.arange(60) * 37 + 11) % 320  # 4 pages: within the budget until token 65 opens the fifth
    free, forced, dense = (_Recording(sd, cfg, PAGE, b) for b in (B, B, 1 << 20))
    lg = [r.prefill(prompt) for r in (free, forced, dense)]
    assert torch.equal(lg[0], lg[1]) and torch.equal(lg[0], lg[2])
    tok, sparse_steps = int(lg[0][-1].argmax()), 0
    for t in range(24):  # tokens 61 .. 84: P = 4, then 5 from token 65 and 6 from token 81
        a, info = free.step(tok)
        b, info_b = forced.step(tok, forced={l: s.own for l, s in info.items()})
        c, info_c = dense.step(tok)
        n_tok = 60 + t + 1
        P = -(-n_tok // PAGE)
        assert free.seqlen == n_tok and not info_c
        assert torch.equal(a, b), "forcing its own selection changes nothing"
        every = torch.arange(n_tok)[None].expand(4, -1)
        for l in (0, 1):  # the first two layers attend everything
            assert torch.equal(free.attended[l], every)
        if P <= B:  # a budget that covers the cache is dense attention
            assert not info and torch.equal(a, c)
            assert all(torch.equal(free.attended[l], every) for l in range(4))
            tok = int(a.argmax())
            continue
        sparse_steps += 1
        assert sorted(info) == [2, 3] and sorted(info_b) == [2, 3]
        assert not torch.equal(a, c)
        last = set(range((P - 1) * PAGE, n_tok))
        for l, s in info.items():
            assert s.n_pages == P and s.scores.shape == (4, P - 1)         # the last page is never scored
            assert s.own.shape == (4, B - 1) and torch.equal(s.own, s.pages)
            assert int(s.own.max()) <= P - 2 and int(s.own.min()) >= 0
            assert torch.equal(info_b[l].scores, s.scores)
            for h in range(4):
                rows = set(free.attended[l][h].tolist())
                assert len(rows) == free.attended[l].shape[1] == (B - 1) * PAGE + len(last)
                want = {p * PAGE + i for p in s.own[h].tolist() for i in range(PAGE)} | last
                assert rows == want                                         # ... and always attended
                top = s.scores[h].sort(descending=True).values
                assert float(s.scores[h][s.own[h]].min()) == float(top[B - 2])
        # layers 2 and 3 score with their own query and their own cache
        assert not torch.equal(info[2].scores, info[3].scores)
        tok = int(a.argmax())
    assert sparse_steps == 20


def test_forced_selection_is_what_is_attended():
    """Another selection than its own gives other logits (``forced`` is not ignored), in the layer it is given for only."""
    cfg = _cfg()
    sd = _state(cfg, 6)
    prompt = (torch.arange(100) * 37 + 11) % 320
    a, b = _Recording(sd, cfg, PAGE, 4), _Recording(sd, cfg, PAGE, 4)
    tok = int(a.prefill(prompt)[-1].argmax())
    b.prefill(prompt)
    la, info = a.step(tok)
    worst = info[3].scores.topk(3, dim=-1, largest=False).indices
    lb, info_b = b.step(tok, forced={3: worst})
    assert torch.equal(info_b[2].pages, info[2].own) and torch.equal(info_b[3].pages, worst)
    assert torch.equal(info_b[3].own, info[3].own) and not torch.equal(la, lb)
    assert torch.equal(a.attended[2], b.attended[2]) and not torch.equal(a.attended[3], b.attended[3])


# ---------------------------------------------------------------------------- the Quest rule against the oracle
@pytest.mark.parametrize("L,Hq,Hkv,D,B", [(16 * 21 + 5, 4, 2, 128, 4), (16 * 40 + 16, 8, 8, 64, 9), (16 * 17 + 1, 4, 1, 128, 6)])
def test_page_scores_and_pages_match_the_oracle(L, Hq, Hkv, D, B):
    import oracle
    from oracle import synth

    q = synth.normal_f16(31, (1, Hq, D))
    k, v = synth.normal_f16(32, (L, Hkv, D)), synth.normal_f16(33, (L, Hkv, D))
    P = -(-L // PAGE)
    MP = -(-P // PAGE)
    kv = oracle.Paged(np.zeros((P, 2, PAGE, Hkv, D), np.float16), np.arange(P, dtype=np.int32), L - (P - 1) * PAGE)
    meta = oracle.Paged(np.zeros((MP, 2, PAGE, Hkv, D), np.float16), np.arange(MP, dtype=np.int32), P - (MP - 1) * PAGE)
    oracle.append_prefill(kv, meta, k, v)
    est = torch.from_numpy(oracle.estimate(q, meta).astype(np.float64))  # [Hq, P - 1], fp16 values

    cfg = SimpleNamespace(hidden_size=Hq * D, num_hidden_layers=1, num_attention_heads=Hq, num_key_value_heads=Hkv,
                          head_dim=D, rms_norm_eps=1e-5, qk_norm=False, rope_theta=1e4, rope_scaling=None)
    ref = QuestModelRef({"model.embed_tokens.weight": torch.zeros(1, Hq * D)}, cfg, PAGE, B)
    ref.k[0], ref.v[0] = torch.from_numpy(k.astype(np.float64)), torch.from_numpy(v.astype(np.float64))
    q64 = torch.from_numpy(q[0].astype(np.float64))
    s64 = ref.page_scores(0, q64)
    assert s64.shape == est.shape == (Hq, P - 1)
    # the oracle multiplies in fp32 (exact for fp16 factors), adds D terms in fp32 and rounds once to fp16: half an fp16 ulp
    # of the result plus D fp32 roundings of partial sums no larger than the sum of the terms' magnitudes
    pages = ref.k[0][: (P - 1) * PAGE].view(P - 1, PAGE, Hkv, D)
    kvh = torch.arange(Hq) // (Hq // Hkv)
    terms = torch.maximum(q64[None] * pages.amax(1)[:, kvh], q64[None] * pages.amin(1)[:, kvh])
    assert torch.equal(terms.sum(-1).t(), s64)
    half_ulp = 2.0 ** (torch.floor(torch.log2(est.abs().clamp_min(2.0 ** -14))) - 11)
    bound = half_ulp + D * 2.0 ** -24 * terms.abs().sum(-1).t()
    err = (est - s64).abs()
    print(f"estimate: max |oracle - float64| / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())

    # pages: rows whose float64 gap at the cut exceeds two fp16 ulps cannot be reordered by the fp16 rounding
    cols = np.tile(np.arange(P - 1, dtype=np.int32), (Hq, 1))
    _, o_idx = oracle.topk(est.numpy().astype(np.float16), cols, B - 1)
    own = ref.top_pages(s64)
    top = s64.sort(dim=-1, descending=True).values
    clear = (top[:, B - 2] - top[:, B - 1]) > 2 * 2.0 ** (torch.floor(torch.log2(top[:, B - 2].abs())) - 10)
    assert int(clear.sum()) >= Hq // 2, "too many near-ties at the cut: choose other inputs"
    for h in range(Hq):
        if clear[h]:
            assert sorted(own[h].tolist()) == sorted(o_idx[h].tolist()), f"head {h}"


@pytest.mark.parametrize("dtype,u", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)], ids=["fp16", "bf16"])
def test_yardstick_runs_in_its_type(dtype, u):
    """The yardstick is the same code with weights, activations and caches in ``dtype``: forced to float64's selection its
    logits sit a few unit roundoffs ``u`` from float64's -- some ten roundings of up to u per layer, adding like a random
    walk over 4 layers.  Below u / 2 it would not be computing in its type, beyond 16 u it would be broken."""
    cfg = _cfg(qk_norm=True)
    sd = {k: v.to(dtype) for k, v in _state(cfg, 7).items()}
    r64, yard = QuestModelRef(sd, cfg, PAGE, 4), QuestModelRef(sd, cfg, PAGE, 4, dtype=dtype)
    prompt = (torch.arange(100) * 37 + 11) % 320
    a, b = r64.prefill(prompt), yard.prefill(prompt)
    assert b.dtype == dtype and yard.k[3].dtype == dtype and r64.k[3].dtype == torch.float64
    rels = [_rel(b[-1].double(), a[-1])]
    tok = int(a[-1].argmax())
    for t in range(8):
        a, info = r64.step(tok)
        b, info_y = yard.step(tok, forced={l: s.own for l, s in info.items()})
        assert b.dtype == dtype and info_y[3].scores.dtype == dtype and torch.equal(info_y[3].pages, info[3].own)
        rels.append(_rel(b.double(), a))
        tok = int(a.argmax())
    print(f"{dtype}: rel(yardstick, float64) {min(rels):.3e} .. {max(rels):.3e} = {min(rels) / u:.1f} .. {max(rels) / u:.1f} u")
    assert u / 2 <= min(rels) and max(rels) <= 16 * u
