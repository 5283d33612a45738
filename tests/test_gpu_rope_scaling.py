"""Scaled RoPE (llama3 / yarn) through the kernels' frequency-table form: the eager / state / batched rope launch against
transformers (tests/golden/hf_rope_scaling_golden.npz), the fused q/k/v+RoPE launches against fp32, the fused decode graph
against the module path, and Hugging Face checkpoints with llama3 and yarn scaling against transformers' logits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.synth import normal_f16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from test_rope_scaling import CONFIGS, GOLDEN, _cfg  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _table(name):
    from quest_amd.models import rope

    return rope.device_rope_parameters(_cfg(name), torch.device(DEV))


def _inputs(golden, ci, i, n, d):
    seed = 900 + 10 * ci + i
    hq, hkv = int(golden["seeds_base"][2]), int(golden["seeds_base"][3])
    q = torch.from_numpy(normal_f16(seed * 3, (n, hq, d))).to(DEV)
    k = torch.from_numpy(normal_f16(seed * 3 + 1, (n, hkv, d))).to(DEV)
    return q, k


@pytest.mark.parametrize("ci,name", list(enumerate(CONFIGS)))
def test_table_rope_matches_transformers(golden, ci, name):
    """Every (past, n) of the fixture -- the last row at position 131071 -- in one launch and in prefill chunks, at the
    reference rope test's bar (rtol = atol = 5e-3, atol scaled by attention_factor)."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    d = CONFIGS[name][0]
    inv_freq, factor = _table(name)
    tol = dict(rtol=5e-3, atol=5e-3 * factor)
    for i, (past, n) in enumerate(golden["cases"].tolist()):
        want_q = torch.from_numpy(golden[f"{name}_q_{past}_{n}"].astype(np.float32))
        want_k = torch.from_numpy(golden[f"{name}_k_{past}_{n}"].astype(np.float32))
        q, k = _inputs(golden, ci, i, n, d)
        _kernels.apply_rope_in_place_freqs(q, k, inv_freq, factor, past_kv_len=past)
        torch.testing.assert_close(q.float().cpu(), want_q, **tol)
        torch.testing.assert_close(k.float().cpu(), want_k, **tol)
        # prefill chunks through the utils entry: same bits as the one launch
        q2, k2 = _inputs(golden, ci, i, n, d)
        for lo in range(0, n, 24):
            hi = min(n, lo + 24)
            qc, kc = q2[lo:hi].contiguous(), k2[lo:hi].contiguous()
            qu.apply_rope_in_place(qc, kc, past + lo, rope_freqs=(inv_freq, factor))
            q2[lo:hi], k2[lo:hi] = qc, kc
        assert torch.equal(q2, q) and torch.equal(k2, k)


@pytest.mark.parametrize("name", ["llama31_8b", "llama32_1b", "yarn_llama2_7b_128k"])
def test_state_form_equals_the_eager_form(name):
    """states[i].seq_len - 1 as the position of row i: one sequence, and several of different lengths, bit for bit the
    eager launch at the same positions."""
    from quest_amd import _kernels

    d = CONFIGS[name][0]
    inv_freq, factor = _table(name)
    g = torch.Generator(device=DEV).manual_seed(7)
    for lens in ([131072], [1, 4096, 8192, 131072, 77, 32760]):
        n = len(lens)
        q = torch.randn(n, 8, d, generator=g, device=DEV).half()
        k = torch.randn(n, 2, d, generator=g, device=DEV).half()
        states = torch.zeros(n, 8, dtype=torch.int32, device=DEV)
        states[:, 0] = torch.tensor(lens, dtype=torch.int32)
        qs, ks = q.clone(), k.clone()
        _kernels.apply_rope_in_place_freqs(qs, ks, inv_freq, factor, states=states)
        for i, L in enumerate(lens):
            qe, ke = q[i:i + 1].clone(), k[i:i + 1].clone()
            _kernels.apply_rope_in_place_freqs(qe, ke, inv_freq, factor, past_kv_len=L - 1)
            assert torch.equal(qs[i:i + 1], qe) and torch.equal(ks[i:i + 1], ke), (name, L)


def _weights(g, hidden, hq, hkv, d):
    s = 1.0 / hidden ** 0.5
    h = torch.randn(hidden, generator=g, device=DEV, dtype=torch.float16)
    gamma = (1 + 0.1 * torch.randn(hidden, generator=g, device=DEV, dtype=torch.float16)).contiguous()
    w = [(torch.randn(r * d, hidden, generator=g, device=DEV, dtype=torch.float16) * s).contiguous() for r in (hq, hkv, hkv)]
    return h, gamma, w


def _rms(x, g, eps):
    x = x.float()
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g.float()).half().float()


def _rope_ref(x, pos, inv_freq, factor, d):
    """fp32 rotate-half with the table: angle = pos * inv_freq[i] (one fp32 product, as transformers)."""
    x = x.reshape(-1, d)
    ang = torch.tensor(float(pos), device=DEV) * inv_freq
    c, sn = torch.cos(ang) * factor, torch.sin(ang) * factor
    a, b = x[:, : d // 2], x[:, d // 2:]
    return torch.cat([a * c - b * sn, b * c + a * sn], 1)


@pytest.mark.parametrize("name,hq,hkv", [("llama31_8b", 32, 8), ("llama32_1b", 32, 8), ("yarn_llama2_7b_128k", 8, 8)])
@pytest.mark.parametrize("pos", [8191, 131071])
def test_qkv_rope_freqs_vs_fp32(name, hq, hkv, pos):
    from quest_amd import _kernels

    d = CONFIGS[name][0]
    inv_freq, factor = _table(name)
    hidden = hq * d
    g = torch.Generator(device=DEV).manual_seed(pos + d)
    h, gamma, (wq, wk, wv) = _weights(g, hidden, hq, hkv, d)
    q = torch.empty(1, hq, d, device=DEV, dtype=torch.float16)
    k = torch.empty(1, hkv, d, device=DEV, dtype=torch.float16)
    v = torch.empty(1, hkv, d, device=DEV, dtype=torch.float16)
    state = torch.tensor([pos + 1, 1, 1, 0, 1, 1, 0, 0], dtype=torch.int32, device=DEV)
    _kernels.decode_qkv_rope_freqs(h, gamma, 1e-5, wq, wk, wv, q, k, v, d, inv_freq, factor, state)
    n = _rms(h, gamma, 1e-5)
    tol = dict(rtol=5e-3, atol=8e-3 * factor)
    torch.testing.assert_close(q.float().view(-1, d), _rope_ref(wq.float() @ n, pos, inv_freq, factor, d), **tol)
    torch.testing.assert_close(k.float().view(-1, d), _rope_ref(wk.float() @ n, pos, inv_freq, factor, d), **tol)
    torch.testing.assert_close(v.float().view(-1), wv.float() @ n, **tol)


@pytest.mark.parametrize("n", [1, 4, 8, 16])
@pytest.mark.parametrize("name,hidden,hq,hkv,persistent", [
    ("llama31_8b", 4096, 32, 8, 1),           # Llama-3.1-8B shapes: the persistent kernel
    ("yarn_llama2_7b_128k", 8704, 8, 2, 0),   # inputs too long for its LDS: the inputs-from-L2 kernel
    ("llama32_1b", 2048, 32, 8, 1),           # head_dim 64
])
def test_qkv_rope_batched_freqs_vs_fp32(n, name, hidden, hq, hkv, persistent):
    from quest_amd import _kernels
    from quest_amd._lib import lib

    d = CONFIGS[name][0]
    info = (ctypes.c_uint32 * 6)()
    assert lib.quest_decode_batched_plan(hidden, (hq + 2 * hkv) * d, n, 1, info) == persistent
    inv_freq, factor = _table(name)
    g = torch.Generator(device=DEV).manual_seed(hidden + n)
    _, gamma, (wq, wk, wv) = _weights(g, hidden, hq, hkv, d)
    h = torch.randn(n, hidden, generator=g, device=DEV, dtype=torch.float16)
    q = torch.empty(n, hq, d, device=DEV, dtype=torch.float16)
    k = torch.empty(n, hkv, d, device=DEV, dtype=torch.float16)
    v = torch.empty(n, hkv, d, device=DEV, dtype=torch.float16)
    pos = [(131071, 8191, 0, 4095, 70000)[i % 5] - (i // 5) for i in range(n)]
    states = torch.zeros(n, 8, dtype=torch.int32, device=DEV)
    states[:, 0] = torch.tensor(pos, dtype=torch.int32) + 1
    _kernels.decode_qkv_rope_batched_freqs(h, gamma, 1e-5, wq, wk, wv, q, k, v, d, inv_freq, factor, states)
    nrm = _rms(h, gamma, 1e-5)
    tol = dict(rtol=5e-3, atol=8e-3 * factor)
    for t in range(n):
        torch.testing.assert_close(q[t].float().view(-1, d), _rope_ref(wq.float() @ nrm[t], pos[t], inv_freq, factor, d),
                                   **tol)
        torch.testing.assert_close(k[t].float().view(-1, d), _rope_ref(wk.float() @ nrm[t], pos[t], inv_freq, factor, d),
                                   **tol)
        torch.testing.assert_close(v[t].float().view(-1), wv.float() @ nrm[t], **tol)


def test_shim_argument_errors():
    from quest_amd import _kernels

    inv_freq, factor = _table("llama31_8b")
    q = torch.zeros(2, 4, 128, device=DEV, dtype=torch.float16)
    k = torch.zeros(2, 2, 128, device=DEV, dtype=torch.float16)
    for bad in (inv_freq.half(), inv_freq[:32].clone(), inv_freq.cpu(), torch.cat([inv_freq, inv_freq])[::2]):
        with pytest.raises(RuntimeError):
            _kernels.apply_rope_in_place_freqs(q, k, bad, factor)
    with pytest.raises(RuntimeError):  # states of the wrong size
        _kernels.apply_rope_in_place_freqs(q, k, inv_freq, factor, states=torch.ones(1, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):  # QUEST_EINVAL from the entry
        _kernels.apply_rope_in_place_freqs(q, k, inv_freq, 0.0)
    with pytest.raises(ValueError):
        _kernels.apply_rope_in_place_freqs(q, k, inv_freq, float("inf"))
    hidden = 512
    g = torch.Generator(device=DEV).manual_seed(1)
    _, gamma, (wq, wk, wv) = _weights(g, hidden, 4, 2, 128)
    h = torch.zeros(hidden, device=DEV, dtype=torch.float16)
    qo, ko, vo = (torch.empty(1, r, 128, device=DEV, dtype=torch.float16) for r in (4, 2, 2))
    state = torch.tensor([10, 1, 1, 0, 1, 1, 0, 0], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        _kernels.decode_qkv_rope_freqs(h, gamma, 1e-5, wq, wk, wv, qo, ko, vo, 128, inv_freq[:63].clone(), factor, state)
    with pytest.raises(ValueError):
        _kernels.decode_qkv_rope_freqs(h, gamma, 1e-5, wq, wk, wv, qo, ko, vo, 128, inv_freq, float("nan"), state)
    hb = torch.zeros(2, hidden, device=DEV, dtype=torch.float16)
    qb, kb, vb = (torch.empty(2, r, 128, device=DEV, dtype=torch.float16) for r in (4, 2, 2))
    states = state.repeat(2, 1).contiguous()
    with pytest.raises(RuntimeError):
        _kernels.decode_qkv_rope_batched_freqs(hb, gamma, 1e-5, wq, wk, wv, qb, kb, vb, 128, inv_freq.double(), factor,
                                               states)
    with pytest.raises(ValueError):
        _kernels.decode_qkv_rope_batched_freqs(hb, gamma, 1e-5, wq, wk, wv, qb, kb, vb, 128, inv_freq, -1.0, states)
    torch.cuda.synchronize()


SCALINGS = {
    "llama3": ({"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                "original_max_position_embeddings": 256}, 500000.0),
    "yarn": ({"type": "yarn", "factor": 4.0, "original_max_position_embeddings": 256}, 10000.0),
}


@pytest.mark.parametrize("kind", list(SCALINGS))
def test_fused_decode_graph_matches_the_module_path(kind):
    """test_gpu_decode_layer.py::test_fused_decode_graph_matches_the_unfused_module_path with a scaled RoPE: the fused
    q/k/v+RoPE launch (table form) vs the module path (nn.Linear + the table rope launch), full attention, 24 positions."""
    from quest_amd.models.llama import LlamaConfig, LlamaForCausalLM
    import quest_amd.utils as qu

    sc, theta = SCALINGS[kind]
    dev = torch.device(DEV)
    cfg = LlamaConfig(vocab_size=1000, hidden_size=512, intermediate_size=1376, num_hidden_layers=4, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=4096, rope_scaling=dict(sc), rope_theta=theta)
    torch.manual_seed(3)
    with torch.device(dev):
        ref_model = LlamaForCausalLM(cfg).half()
    for p in ref_model.parameters():
        p.data.normal_(0, 0.05)
    for m in ref_model.modules():
        if hasattr(m, "variance_epsilon"):
            m.weight.data.uniform_(0.8, 1.2)
    ctx, steps, D = 16 * 20 + 5, 24, 128
    g = torch.Generator(device=dev).manual_seed(4)
    kc = torch.randn(cfg.num_hidden_layers, ctx, 2, D, generator=g, device=dev, dtype=torch.float16)
    vc = torch.randn(cfg.num_hidden_layers, ctx, 2, D, generator=g, device=dev, dtype=torch.float16)
    embs = torch.randn(steps, 1, 1, 512, generator=g, device=dev, dtype=torch.float16) * 0.3
    logits = {}
    for fused in (False, True):
        with torch.device(dev):
            model = LlamaForCausalLM(cfg).half()
        model.load_state_dict(ref_model.state_dict())
        model.quest_init(16, ctx + steps + 64, token_budget=16 * 64)
        tables = {id(l.self_attn.rope_freqs[0]) for l in model.model.layers}
        assert len(tables) == 1 and model.model.layers[0].self_attn.rope_freqs[0].dtype == torch.float32
        ctl = model.model.iController
        ctl.prepare_metadata(ctx)
        ctl.begin_forward(ctx)
        for l in range(cfg.num_hidden_layers):
            qu.append_kv(kc[l], vc[l], ctl, l)
        ctl.end_forward()
        model.capture_decode_graph(fused_layers=fused)
        assert model.fused_layers == fused
        outs = []
        with torch.inference_mode():
            for t in range(steps):
                outs.append(model.decode_graph_step(inputs_embeds=embs[t]).float().clone())
        torch.cuda.synchronize()
        logits[fused] = torch.stack(outs)
    assert torch.isfinite(logits[True]).all()
    scale = float(logits[False].abs().max())
    err = (logits[True] - logits[False]).abs().flatten(1).max(1).values
    assert float(err.max()) < 1e-2 * scale, (err.tolist(), scale)


HF_ROPE = {
    "llama3": {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
               "original_max_position_embeddings": 64, "rope_theta": 500000.0},
    "yarn": {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 256, "rope_theta": 10000.0},
}


@pytest.mark.parametrize("kind", list(HF_ROPE))
def test_hf_checkpoint_with_scaled_rope_matches_transformers(tmp_path, kind):
    """test_gpu_hf_checkpoint.py for llama3 / yarn checkpoints: transformers' logits over the prefill and 20
    graph-decoded tokens (full attention); on the Quest sparse path eager == graph bit for bit; a 3-sequence batch of
    different prompt lengths (quest_init_batched) against the single-sequence model."""
    transformers = pytest.importorskip("transformers")
    from quest_amd.models.llama import LlamaForCausalLM

    dev = torch.device(DEV)
    hcfg = transformers.LlamaConfig(vocab_size=320, hidden_size=512, intermediate_size=1024, num_hidden_layers=3,
                                    num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=1024,
                                    rms_norm_eps=1e-5, rope_parameters=dict(HF_ROPE[kind]))
    torch.manual_seed(3)
    hf = transformers.LlamaForCausalLM(hcfg)
    for p in hf.parameters():
        p.data.mul_(2.0)
    for n, p in hf.named_parameters():
        if "norm" in n:
            p.data.fill_(1.0)
    d = str(tmp_path / "ckpt")
    hf.half().save_pretrained(d, safe_serialization=True)
    hf32 = transformers.LlamaForCausalLM.from_pretrained(d, dtype=torch.float32, attn_implementation="eager").eval()
    hf16 = transformers.LlamaForCausalLM.from_pretrained(d, dtype=torch.float16, attn_implementation="eager").to(dev).eval()
    assert hf32.model.rotary_emb.rope_type == kind

    def rel(a, b):
        return float((a - b).norm() / b.norm())

    def check(got, r16, r32, what):
        got, r16 = got.float().cpu(), r16.float().cpu()
        assert rel(got, r32) <= 1.5 * rel(r16, r32) + 2e-3, f"{what}: {rel(got, r32):.4f} vs HF fp16 {rel(r16, r32):.4f}"
        assert rel(got, r16) <= 1e-2, f"{what}: {rel(got, r16):.4f} from transformers' fp16 logits"

    m = LlamaForCausalLM.from_pretrained(d, device=dev)
    a = m.model.layers[0].self_attn
    assert a.rope_table and a.rope_scale == 1.0
    m.quest_init(16, 512, token_budget=16 * 1024)
    prompt = (torch.arange(150)[None] * 37 + 11) % 320
    with torch.no_grad():
        ref32 = hf32(input_ids=prompt, use_cache=True)
        ref16 = hf16(input_ids=prompt.to(dev), use_cache=True)
    with torch.inference_mode():
        got_all = m.lm_head(m.model(input_ids=prompt.to(dev)))[0]
    check(got_all, ref16.logits[0], ref32.logits[0], "prefill, all positions")
    past32, past16, tok = ref32.past_key_values, ref16.past_key_values, ref32.logits[0, -1].argmax()
    m.capture_decode_graph()
    assert m.fused_layers
    for t in range(20):
        with torch.no_grad():
            ref32 = hf32(input_ids=tok.view(1, 1), past_key_values=past32, use_cache=True)
            ref16 = hf16(input_ids=tok.view(1, 1).to(dev), past_key_values=past16, use_cache=True)
        past32, past16 = ref32.past_key_values, ref16.past_key_values
        with torch.inference_mode():
            got = m.decode_graph_step(input_ids=tok.view(1, 1).to(dev))
        check(got[0, -1], ref16.logits[0, -1], ref32.logits[0, -1], f"decode token {t}")
        tok = ref32.logits[0, -1].argmax()
    del m, hf16

    # Quest sparse path (4 pages of 16 tokens): eager == graph replay of the module-by-module step, bit for bit
    outs = []
    for graph in (False, True):
        q = LlamaForCausalLM.from_pretrained(d, device=dev)
        q.quest_init(16, 512, token_budget=64)
        with torch.inference_mode():
            lg = q(input_ids=prompt.to(dev))
            if graph:
                q.capture_decode_graph(fused_layers=False)
            seq = []
            for t in range(12):
                tk = lg[0, -1].argmax().view(1, 1)
                lg = q.decode_graph_step(input_ids=tk) if graph else q(input_ids=tk)
                seq.append(lg.float().clone())
        assert q.model.iController.need_estimate()
        outs.append(torch.stack(seq))
        del q
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])

    # a batch of 3 prompts of different lengths vs each alone (test_gpu_batched.py's bars: M = 3 GEMMs round differently)
    prompts = [((torch.arange(L)[None] * (7 + i) + i) % 320).to(dev) for i, L in enumerate((150, 97, 201))]
    n_new = 10
    toks, logits = [], []
    for pr in prompts:
        s = LlamaForCausalLM.from_pretrained(d, device=dev)
        s.quest_init(16, 512, token_budget=96)
        with torch.inference_mode():
            first = s(input_ids=pr)
        s.capture_decode_graph()
        tk, lg = [int(first.argmax(-1))], [first.float().clone()]
        with torch.inference_mode():
            for _ in range(n_new):
                out = s.decode_graph_step(input_ids=torch.tensor([[tk[-1]]], device=dev))
                lg.append(out.float().clone())
                tk.append(int(out.argmax(-1)))
        toks.append(tk)
        logits.append(lg)
        del s
    mb = LlamaForCausalLM.from_pretrained(d, device=dev)
    mb.quest_init_batched(len(prompts), 16, 512, token_budget=96)
    with torch.inference_mode():
        for i, pr in enumerate(prompts):
            assert torch.equal(mb.prefill_sequence(i, pr).float(), logits[i][0]), "prefill over the shared pool differs"
    mb.capture_decode_graph_batched()
    assert mb.fused_layers
    errs = []
    with torch.inference_mode():
        for t in range(n_new):
            ids = torch.tensor([toks[i][t] for i in range(len(prompts))], device=dev)
            out = mb.decode_graph_step_batched(ids).float()
            for i in range(len(prompts)):
                errs.append(float((out[i].reshape(-1) - logits[i][t + 1][0].reshape(-1)).abs().max()))
    errs = torch.tensor(errs)
    assert float(errs.median()) < 3e-2 and float((errs < 3e-2).float().mean()) >= 0.8 and float(errs.max()) < 0.5, errs.tolist()
