"""bf16 end to end: the MFMA flash prefill on bf16 pools against fp64, and a bf16 Llama checkpoint whose weights, keys and
values do not fit fp16 through ``from_pretrained(dtype=torch.bfloat16)`` -> ``quest_init(dtype=torch.bfloat16)`` -> prefill
-> graph-replayed decode, against transformers.

Bars.  Prefill: the error of a bf16 P matrix is not derived here, it is MEASURED against a yardstick that is not the code
under test -- the same attention computed by torch in bf16 on the GPU (matmul, fp32 softmax, matmul); the kernel's max-abs
and relative-norm errors against fp64 must be at most 1.5 x the yardstick's (the factor tests/test_gpu_hf_checkpoint.py
uses for "our pipeline vs the framework's own pipeline in the same type").  Model: rel(got, hf_fp32) <= 1.5 *
rel(hf_bf16, hf_fp32) + 2e-3 with hf_bf16 = transformers' own bf16 run on the same GPU; on the sparse path eager == graph
and NHD == NHD_ROT bit for bit, all logits finite."""
import math

import numpy as np
import pytest
import torch

from _bf16 import record
from oracle import torch_ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda:0"


def _torch_bf16_attention(q, k, v, causal=True):
    """The yardstick: torch's own bf16 pipeline -- bf16 matmul (scores rounded to bf16), fp32 softmax, P rounded to bf16,
    bf16 matmul."""
    n, Hq, D = q.shape
    kv_len, Hkv, _ = k.shape
    qh = q.transpose(0, 1)
    kh = k.repeat_interleave(Hq // Hkv, 1).transpose(0, 1)
    vh = v.repeat_interleave(Hq // Hkv, 1).transpose(0, 1)
    s = torch.matmul(qh, kh.transpose(1, 2)).float() / math.sqrt(D)
    if causal:
        keep = torch.ones(n, kv_len, dtype=torch.bool, device=q.device).tril(diagonal=kv_len - n)
        s = s.masked_fill(~keep, float("-inf"))
    p = torch.softmax(s, dim=-1).to(BF)
    return torch.matmul(p, vh).transpose(0, 1)


@pytest.mark.parametrize("n_q,kv_len,Hq,Hkv,D,page,layout", [
    (300, 300, 8, 8, 128, 16, 0),      # whole prompt, MHA
    (200, 1000, 8, 2, 128, 16, 2),     # a chunk over a longer cache, GQA, row-rotated pool
    (257, 700, 4, 4, 64, 16, 1),       # head_dim 64, HND
    (130, 400, 4, 2, 256, 8, 0),       # head_dim 256, the generic page walk
    (64, 2100, 8, 4, 128, 16, 0),      # many key tiles per query row
])
def test_prefill_bf16_against_fp64_with_torch_bf16_as_yardstick(n_q, kv_len, Hq, Hkv, D, page, layout):
    import quest_amd.utils as qu

    g = torch.Generator(device=DEV).manual_seed(n_q + kv_len)
    q = torch.randn(n_q, Hq, D, generator=g, device=DEV).to(BF)
    k = torch.randn(kv_len, Hkv, D, generator=g, device=DEV).to(BF)
    v = torch.randn(kv_len, Hkv, D, generator=g, device=DEV).to(BF)
    ctl = qu.InferenceController(1, Hq, D, page, 4, kv_len + 4 * page, BF, torch.device(DEV), num_kv_heads=Hkv,
                                 layout=layout, shuffle_seed=n_q)
    chunks = [kv_len] if kv_len == n_q else [kv_len - n_q, n_q]
    t = 0
    for c in chunks:
        ctl.prepare_metadata(c)
        ctl.begin_forward(c)
        qu.append_kv(k[t:t + c], v[t:t + c], ctl, 0)
        t += c
        if t < kv_len:
            ctl.end_forward()
    o = qu.prefill_forward(q, ctl, 0)
    ctl.end_forward()
    assert o.dtype == BF and o.shape == q.shape
    ref = torch_ref.prefill_attention(q, k, v, causal=True, dtype=torch.float64)
    yard = _torch_bf16_attention(q, k, v)

    def errs(x):
        d = x.double() - ref
        return float(d.abs().max()), float(d.norm() / ref.norm())

    (k_abs, k_rel), (y_abs, y_rel) = errs(o), errs(yard)
    record(f"prefill n_q={n_q} kv_len={kv_len} Hq={Hq} Hkv={Hkv} D={D} page={page} layout={layout}: "
          f"kernel max_abs={k_abs:.3e} rel_norm={k_rel:.3e} | torch bf16 max_abs={y_abs:.3e} rel_norm={y_rel:.3e}")
    assert torch.isfinite(o.float()).all()
    assert k_abs <= 1.5 * y_abs, (k_abs, y_abs)
    assert k_rel <= 1.5 * y_rel, (k_rel, y_rel)


ROPE = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
        "original_max_position_embeddings": 64, "rope_theta": 500000.0}


def _checkpoint(tmp_path):
    """A tiny random Llama (GQA, llama3 RoPE) saved as bf16, rescaled by exact powers of two so that it does not fit fp16
    while computing the same function: v_proj x 2^22 / o_proj x 2^-22 (weights of ~1.7e5 > 65504, cached values of ~1e6),
    k_proj x 2^18 / q_proj x 2^-18 (cached keys, hence page maxima / minima, of ~1e5 and beyond)."""
    transformers = pytest.importorskip("transformers")
    hcfg = transformers.LlamaConfig(vocab_size=320, hidden_size=512, intermediate_size=1024, num_hidden_layers=3,
                                    num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=1024,
                                    rms_norm_eps=1e-5, rope_parameters=dict(ROPE))
    torch.manual_seed(3)
    hf = transformers.LlamaForCausalLM(hcfg)
    for p in hf.parameters():
        p.data.mul_(2.0)
    big = 0.0
    for n, p in hf.named_parameters():
        if "norm" in n:
            p.data.fill_(1.0)
        for key, e in (("v_proj", 22), ("o_proj", -22), ("k_proj", 18), ("q_proj", -18)):
            if key in n:
                p.data.mul_(2.0 ** e)
        big = max(big, float(p.data.abs().max()))
    assert big > 65504
    d = str(tmp_path / "ckpt")
    hf.to(BF).save_pretrained(d, safe_serialization=True)
    hf32 = transformers.LlamaForCausalLM.from_pretrained(d, dtype=torch.float32, attn_implementation="eager").eval()
    hfbf = transformers.LlamaForCausalLM.from_pretrained(d, dtype=BF, attn_implementation="eager").to(DEV).eval()
    return d, hf32, hfbf


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _check(got, rbf, r32, what):
    got, rbf = got.float().cpu(), rbf.float().cpu()
    e, y = _rel(got, r32), _rel(rbf, r32)
    record(f"model {what}: rel(got, hf_fp32)={e:.4e} rel(hf_bf16, hf_fp32)={y:.4e}")
    assert torch.isfinite(got).all(), what
    assert e <= 1.5 * y + 2e-3, f"{what}: {e:.4f} vs HF bf16 {y:.4f}"


def _hf_run(hf32, hfbf, prompt, n_new):
    """transformers' logits (fp32 on the CPU, bf16 on the GPU) for the prompt's positions and n_new greedy tokens (the fp32
    model's choice feeds both)."""
    with torch.no_grad():
        r32 = hf32(input_ids=prompt.cpu(), use_cache=True)
        rbf = hfbf(input_ids=prompt.to(DEV), use_cache=True)
    first = (r32.logits[0], rbf.logits[0])
    p32, pbf, tok = r32.past_key_values, rbf.past_key_values, r32.logits[0, -1].argmax()
    toks, steps = [], []
    for _ in range(n_new):
        toks.append(int(tok))
        with torch.no_grad():
            r32 = hf32(input_ids=tok.view(1, 1), past_key_values=p32, use_cache=True)
            rbf = hfbf(input_ids=tok.view(1, 1).to(DEV), past_key_values=pbf, use_cache=True)
        p32, pbf = r32.past_key_values, rbf.past_key_values
        steps.append((r32.logits[0, -1], rbf.logits[0, -1]))
        tok = r32.logits[0, -1].argmax()
    return first, toks, steps


def test_bf16_checkpoint_single_sequence(tmp_path):
    from quest_amd.models.llama import LlamaForCausalLM

    d, hf32, hfbf = _checkpoint(tmp_path)
    dev = torch.device(DEV)
    # the fp16 load still refuses what does not fit, and now says where to go
    with pytest.raises(ValueError, match=r"overflow torch\.float16.*dtype=torch\.bfloat16"):
        LlamaForCausalLM.from_pretrained(d, device=dev)
    prompt = (torch.arange(150)[None] * 37 + 11) % 320
    n_new = 20  # crosses the 160-token page boundary
    first, toks, steps = _hf_run(hf32, hfbf, prompt, n_new)

    m = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
    assert m.lm_head.weight.dtype == BF and m.model.layers[0].self_attn.rope_table
    m.quest_init(16, 512, token_budget=16 * 1024, dtype=BF)  # budget >= pages: full attention, comparable with HF
    ctl = m.model.iController
    assert ctl.kv_cache.buf_layer(0).dtype == BF and ctl.metadata_cache.buf_layer(0).dtype == BF
    with torch.inference_mode():
        got_all = m.lm_head(m.model(input_ids=prompt.to(dev)))[0]
    _check(got_all, first[1], first[0], "prefill, all positions")
    _check(got_all[-1], first[1][-1], first[0][-1], "prefill, last position")
    # the cache really holds what fp16 cannot: values beyond 65504 in the KV pool and in the page maxima
    assert float(ctl.kv_cache.buf_layer(0)[ctl.kv_cache.indicies[0]].float().abs().max()) > 65504
    assert float(ctl.metadata_cache.buf_layer(0)[ctl.metadata_cache.indicies[0], 0, :2].float().abs().max()) > 65504
    m.capture_decode_graph()
    assert not m.fused_layers  # the fused projection launches are fp16-only: the module path
    assert m._graph_scores.dtype == BF
    for t in range(n_new):
        with torch.inference_mode():
            got = m.decode_graph_step(input_ids=torch.tensor([[toks[t]]], device=dev))
        _check(got[0, -1], steps[t][1], steps[t][0], f"decode token {t}")
    assert ctl.kv_cache.seqlen == 150 + n_new
    del m

    # the Quest sparse path, budget 4 pages of 16 tokens: eager == graph replay, NHD == NHD_ROT, bit for bit; finite
    outs = []
    for graph, kv_layout in ((False, "NHD"), (True, "NHD"), (True, "NHD_ROT")):
        s = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
        s.quest_init(16, 512, token_budget=64, dtype=BF, kv_layout=kv_layout)
        with torch.inference_mode():
            lg = s(input_ids=prompt.to(dev))
            if graph:
                s.capture_decode_graph()
            seq = []
            for t in range(12):
                tk = lg[0, -1].argmax().view(1, 1)
                lg = s.decode_graph_step(input_ids=tk) if graph else s(input_ids=tk)
                seq.append(lg.float().clone())
        assert s.model.iController.need_estimate() or graph
        outs.append(torch.stack(seq))
        del s
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])


def test_bf16_checkpoint_batch_of_three(tmp_path):
    from quest_amd.models.llama import LlamaForCausalLM

    d, hf32, hfbf = _checkpoint(tmp_path)
    dev = torch.device(DEV)
    prompts = [((torch.arange(L)[None] * (7 + i) + i) % 320) for i, L in enumerate((150, 97, 201))]
    n_new = 20  # the first sequence crosses a page boundary at 160, the third at 208
    refs = [_hf_run(hf32, hfbf, pr, n_new) for pr in prompts]
    mb = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
    mb.quest_init_batched(len(prompts), 16, 512, token_budget=16 * 1024, dtype=BF)
    with torch.inference_mode():
        for i, pr in enumerate(prompts):
            lg = mb.prefill_sequence(i, pr.to(dev))
            _check(lg[0, -1], refs[i][0][1][-1], refs[i][0][0][-1], f"sequence {i} prefill, last position")
    mb.capture_decode_graph_batched()
    assert not mb.fused_layers and mb.model.bController.one_launch_layers is False
    with torch.inference_mode():
        for t in range(n_new):
            ids = torch.tensor([refs[i][1][t] for i in range(len(prompts))], device=dev)
            out = mb.decode_graph_step_batched(ids)
            for i in range(len(prompts)):
                _check(out[i, -1], refs[i][2][t][1], refs[i][2][t][0], f"sequence {i} decode token {t}")
    del mb

    # sparse path (4 pages): the captured batched step on the NHD and on the row-rotated pool, bit for bit; finite
    outs = []
    for kv_layout in ("NHD", "NHD_ROT"):
        s = LlamaForCausalLM.from_pretrained(d, device=dev, dtype=BF)
        s.quest_init_batched(len(prompts), 16, 512, token_budget=64, dtype=BF, kv_layout=kv_layout)
        with torch.inference_mode():
            ids = torch.stack([s.prefill_sequence(i, pr.to(dev))[0, -1].argmax() for i, pr in enumerate(prompts)])
            s.capture_decode_graph_batched()
            seq = []
            for t in range(12):
                lg = s.decode_graph_step_batched(ids)
                seq.append(lg.float().clone())
                ids = lg[:, -1].argmax(-1)
        outs.append(torch.stack(seq))
        del s
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
