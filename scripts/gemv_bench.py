#!/usr/bin/env python3
"""Per-launch time of the fused decoder-layer GEMV launches at Llama-2-7B shapes (rotating weight sets past the Infinity
Cache, hipGraph + HIP events).  QUEST_GEMV_CFG="RW,U" forces a workgroup shape.   python scripts/gemv_bench.py
With --tokens N (2..16): the N-token launches (csrc/decode_layer.hip skinny_kernel; QUEST_SKINNY_CFG="NW,U") next to
torch.nn.functional.linear on the same [N, in] inputs (hipBLASLt).
With --rope-ab: the q/k/v+RoPE launch at Llama-3.1-8B shapes (hidden 4096, 32 / 8 heads, head_dim 128), batch 1 and 8
tokens, RoPE formula (rope_scale / rope_theta) vs the llama3 frequency table, alternating A B A B.
With --qk-norm-ab: Qwen3-8B shapes (hidden 4096, 32 / 8 heads of 128), batch 1 and 8 tokens: the rotating q/k/v launch
(frequency table) beside the unrotated one (quest_decode_qkv*) and the per-head q/k norm + RoPE launch that follows it,
alternating A B A B.
With --dtype bf16 (default f16): every tensor of the runs above in that element type (the entries' dtype argument).
With --dtype-ab: fp16 against bf16 in ONE process, alternating A B A B, the four launches of a layer at Llama-2-7B and
Qwen3-8B shapes at 1, 4, 8 and 16 tokens: per launch the four times of each type, the medians, the fp16 runs' own spread
(max - min) and the difference of the medians.  The bytes are the same; a difference inside the spread is none."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from quest_amd import _kernels
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
from kbench_reference_rows import graph_time

dev = torch.device("cuda", 0)
DT = {"f16": torch.float16, "bf16": torch.bfloat16}[sys.argv[sys.argv.index("--dtype") + 1] if "--dtype" in sys.argv else "f16"]
H, I, NSET = 4096, 11008, 8
g = torch.Generator(device=dev).manual_seed(0)
def w(o, i): return [(torch.randn(o, i, generator=g, device=dev, dtype=DT) * 0.02) for _ in range(NSET)]
x = torch.randn(H, generator=g, device=dev, dtype=DT)
xi = torch.randn(I, generator=g, device=dev, dtype=DT)
gamma = torch.ones(H, device=dev, dtype=DT)
h = torch.zeros(H, device=dev, dtype=DT)
act = torch.empty(I, device=dev, dtype=DT)
q = torch.empty(1, 32, 128, device=dev, dtype=DT); k = torch.empty_like(q); v = torch.empty_like(q)
state = torch.tensor([1000, 1, 1, 0, 1, 1, 0, 0], dtype=torch.int32, device=dev)
wo, wd, wg, wu, wq, wk, wv = w(H, H), w(H, I), w(I, H), w(I, H), w(H, H), w(H, H), w(H, H)
rows = []
rows.append(("o_proj+res    32 MiB", graph_time(lambda i: _kernels.decode_gemv_residual(x, wo[i], h), NSET, 20), 32))
rows.append(("down+res      86 MiB", graph_time(lambda i: _kernels.decode_gemv_residual(xi, wd[i], h), NSET, 20), 86))
rows.append(("gate/up+silu 172 MiB", graph_time(lambda i: _kernels.decode_mlp_gate_up(x, gamma, 1e-5, wg[i], wu[i], act), NSET, 20), 172))
rows.append(("qkv+rope      96 MiB", graph_time(lambda i: _kernels.decode_qkv_rope(x, gamma, 1e-5, wq[i], wk[i], wv[i], q, k, v, 128, 1.0, 1e4, state), NSET, 20), 96))
print(str(DT)[6:], os.environ.get("QUEST_GEMV_CFG", "default"), " | ".join(f"{n}: {t:6.2f} us {m * 1.048576 / t:5.2f} TB/s" for n, t, m in rows))

if "--tokens" in sys.argv:
    n = int(sys.argv[sys.argv.index("--tokens") + 1])
    X = torch.randn(n, H, generator=g, device=dev, dtype=DT)
    XI = torch.randn(n, I, generator=g, device=dev, dtype=DT)
    HB = torch.zeros(n, H, device=dev, dtype=DT)
    ACT = torch.empty(n, I, device=dev, dtype=DT)
    Q = torch.empty(n, 32, 128, device=dev, dtype=DT); K = torch.empty_like(Q); V = torch.empty_like(Q)
    ST = torch.tensor([[1000 + 17 * i, 1, 1, 0, 1, 1, 0, 0] for i in range(n)], dtype=torch.int32, device=dev)
    rows = []
    rows.append(("o_proj+res    32 MiB", graph_time(lambda i: _kernels.decode_gemv_residual_batched(X, wo[i], HB), NSET, 20), 32))
    rows.append(("down+res      86 MiB", graph_time(lambda i: _kernels.decode_gemv_residual_batched(XI, wd[i], HB), NSET, 20), 86))
    rows.append(("gate/up+silu 172 MiB", graph_time(lambda i: _kernels.decode_mlp_gate_up_batched(X, gamma, 1e-5, wg[i], wu[i], ACT), NSET, 20), 172))
    rows.append(("qkv+rope      96 MiB", graph_time(lambda i: _kernels.decode_qkv_rope_batched(X, gamma, 1e-5, wq[i], wk[i], wv[i], Q, K, V, 128, 1.0, 1e4, ST), NSET, 20), 96))
    print(f"{n} tokens", os.environ.get("QUEST_SKINNY_CFG", "default"), " | ".join(f"{nm}: {t:6.2f} us {m * 1.048576 / t:5.2f} TB/s" for nm, t, m in rows))
    lin = torch.nn.functional.linear
    rows = []
    rows.append(("linear o_proj  32 MiB", graph_time(lambda i: lin(X, wo[i]), NSET, 20), 32))
    rows.append(("linear down    86 MiB", graph_time(lambda i: lin(XI, wd[i]), NSET, 20), 86))
    rows.append(("linear gate    86 MiB", graph_time(lambda i: lin(X, wg[i]), NSET, 20), 86))
    print(f"{n} tokens torch ", " | ".join(f"{nm}: {t:6.2f} us {m * 1.048576 / t:5.2f} TB/s" for nm, t, m in rows))

if "--rope-ab" in sys.argv:
    from quest_amd.models import rope as qrope
    from types import SimpleNamespace
    cfg31 = SimpleNamespace(hidden_size=4096, num_attention_heads=32, max_position_embeddings=131072, rope_theta=500000.0,
                            rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                          "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    inv_freq, factor = qrope.device_rope_parameters(cfg31, dev)
    wk8, wv8 = w(1024, H), w(1024, H)
    k8 = torch.empty(1, 8, 128, device=dev, dtype=DT); v8 = torch.empty_like(k8)
    X8 = torch.randn(8, H, generator=g, device=dev, dtype=DT)
    Q8 = torch.empty(8, 32, 128, device=dev, dtype=DT); K8 = torch.empty(8, 8, 128, device=dev, dtype=DT)
    V8 = torch.empty_like(K8)
    ST8 = torch.tensor([[100000 + 17 * i, 1, 1, 0, 1, 1, 0, 0] for i in range(8)], dtype=torch.int32, device=dev)
    st1 = torch.tensor([100000, 1, 1, 0, 1, 1, 0, 0], dtype=torch.int32, device=dev)
    launches = {
        ("batch 1", "formula"): lambda i: _kernels.decode_qkv_rope(x, gamma, 1e-5, wq[i], wk8[i], wv8[i], q, k8, v8, 128, 1.0,
                                                                 500000.0, st1),
        ("batch 1", "table"): lambda i: _kernels.decode_qkv_rope_freqs(x, gamma, 1e-5, wq[i], wk8[i], wv8[i], q, k8, v8, 128,
                                                                     inv_freq, factor, st1),
        ("8 tokens", "formula"): lambda i: _kernels.decode_qkv_rope_batched(X8, gamma, 1e-5, wq[i], wk8[i], wv8[i], Q8, K8, V8,
                                                                          128, 1.0, 500000.0, ST8),
        ("8 tokens", "table"): lambda i: _kernels.decode_qkv_rope_batched_freqs(X8, gamma, 1e-5, wq[i], wk8[i], wv8[i], Q8, K8,
                                                                              V8, 128, inv_freq, factor, ST8),
    }
    times = {key: [] for key in launches}
    for _ in range(4):  # A B A B
        for key, fn in launches.items():
            times[key].append(graph_time(fn, NSET, 20))
    for key, ts in times.items():
        print(f"qkv+rope Llama-3.1-8B {key[0]:8s} {key[1]:7s}: " + " ".join(f"{t:6.2f}" for t in ts)
              + f"  us (median {sorted(ts)[len(ts) // 2]:6.2f}, 48 MiB: {48 * 1.048576 / sorted(ts)[len(ts) // 2]:5.2f} TB/s)")

if "--qk-norm-ab" in sys.argv:
    from quest_amd.models import rope as qrope
    from types import SimpleNamespace
    cfgq = SimpleNamespace(hidden_size=4096, num_attention_heads=32, head_dim=128, max_position_embeddings=40960,
                           rope_theta=1e6, rope_scaling=None, model_type="qwen3")
    inv_freq, factor = qrope.device_rope_parameters(cfgq, dev)
    wk8, wv8 = w(1024, H), w(1024, H)
    qn = (1 + 0.1 * torch.randn(128, generator=g, device=dev)).to(DT)
    kn = (1 + 0.1 * torch.randn(128, generator=g, device=dev)).to(DT)
    k8 = torch.empty(1, 8, 128, device=dev, dtype=DT); v8 = torch.empty_like(k8)
    X8 = torch.randn(8, H, generator=g, device=dev, dtype=DT)
    Q8 = torch.empty(8, 32, 128, device=dev, dtype=DT); K8 = torch.empty(8, 8, 128, device=dev, dtype=DT)
    V8 = torch.empty_like(K8)
    ST8 = torch.tensor([[32768 + 17 * i, 1, 1, 0, 1, 1, 0, 0] for i in range(8)], dtype=torch.int32, device=dev)
    st1 = torch.tensor([[32768, 1, 1, 0, 1, 1, 0, 0]], dtype=torch.int32, device=dev)
    # the norm + RoPE launch rewrites q / k in place: the values wander, the time does not depend on them
    launches = {
        ("batch 1", "q/k/v + RoPE (table)"): lambda i: _kernels.decode_qkv_rope_freqs(x, gamma, 1e-6, wq[i], wk8[i], wv8[i], q, k8, v8,
                                                                                     128, inv_freq, factor, st1),
        ("batch 1", "q/k/v unrotated"): lambda i: _kernels.decode_qkv(x, gamma, 1e-6, wq[i], wk8[i], wv8[i], q, k8, v8),
        ("batch 1", "q/k norm + RoPE"): lambda i: _kernels.apply_qk_norm_rope_in_place(q, k8, qn, kn, 1e-6, inv_freq=inv_freq,
                                                                                      attention_factor=factor, states=st1),
        ("batch 1", "RoPE alone"): lambda i: _kernels.apply_rope_in_place_freqs(q, k8, inv_freq, factor, states=st1),
        ("8 tokens", "q/k/v + RoPE (table)"): lambda i: _kernels.decode_qkv_rope_batched_freqs(X8, gamma, 1e-6, wq[i], wk8[i], wv8[i],
                                                                                              Q8, K8, V8, 128, inv_freq, factor, ST8),
        ("8 tokens", "q/k/v unrotated"): lambda i: _kernels.decode_qkv_batched(X8, gamma, 1e-6, wq[i], wk8[i], wv8[i], Q8, K8, V8),
        ("8 tokens", "q/k norm + RoPE"): lambda i: _kernels.apply_qk_norm_rope_in_place(Q8, K8, qn, kn, 1e-6, inv_freq=inv_freq,
                                                                                       attention_factor=factor, states=ST8),
        ("8 tokens", "RoPE alone"): lambda i: _kernels.apply_rope_in_place_freqs(Q8, K8, inv_freq, factor, states=ST8),
    }
    times = {key: [] for key in launches}
    for _ in range(4):  # A B A B
        for key, fn in launches.items():
            times[key].append(graph_time(fn, NSET, 20))
    for key, ts in times.items():
        print(f"Qwen3-8B {key[0]:8s} {key[1]:22s}: " + " ".join(f"{t:6.2f}" for t in ts)
              + f"  us (median {sorted(ts)[len(ts) // 2]:6.2f})")

if "--dtype-ab" in sys.argv:
    del wo, wd, wg, wu, wq, wk, wv
    torch.cuda.empty_cache()
    SHAPES = {"Llama-2-7B": (4096, 11008, 32, 32), "Qwen3-8B": (4096, 12288, 32, 8)}  # hidden, intermediate, q heads, kv heads (of 128)
    TYPES = (("f16", torch.float16), ("bf16", torch.bfloat16))
    for model, (Hd, Id, hq, hkv) in SHAPES.items():
        def ws(o, i):  # the same numbers in both types
            base = [(torch.randn(o, i, generator=g, device=dev) * 0.02) for _ in range(NSET)]
            return {nm: [t.to(dt) for t in base] for nm, dt in TYPES}
        Wo, Wd, Wg, Wu, Wq, Wk, Wv = ws(Hd, hq * 128), ws(Hd, Id), ws(Id, Hd), ws(Id, Hd), ws(hq * 128, Hd), ws(hkv * 128, Hd), ws(hkv * 128, Hd)
        mib = {"o_proj+res": Hd * hq * 128, "down+res": Hd * Id, "gate/up+silu": 2 * Id * Hd, "qkv+rope": (hq + 2 * hkv) * 128 * Hd}
        for n in (1, 4, 8, 16):
            launches = {}
            for nm, dt in TYPES:
                shp = (lambda *d: d[1:]) if n == 1 else (lambda *d: d)
                X = torch.randn(*shp(n, Hd), generator=g, device=dev).to(dt)
                XA = torch.randn(*shp(n, hq * 128), generator=g, device=dev).to(dt)
                XI = torch.randn(*shp(n, Id), generator=g, device=dev).to(dt)
                HB, ACT = torch.zeros(*shp(n, Hd), device=dev, dtype=dt), torch.empty(*shp(n, Id), device=dev, dtype=dt)
                GM = torch.ones(Hd, device=dev, dtype=dt)
                Q, K, V = (torch.empty(n, hh, 128, device=dev, dtype=dt) for hh in (hq, hkv, hkv))
                ST = torch.tensor([[1000 + 17 * i, 1, 1, 0, 1, 1, 0, 0] for i in range(n)], dtype=torch.int32, device=dev)
                res, gu, rope = ((_kernels.decode_gemv_residual, _kernels.decode_mlp_gate_up, _kernels.decode_qkv_rope) if n == 1 else
                                 (_kernels.decode_gemv_residual_batched, _kernels.decode_mlp_gate_up_batched, _kernels.decode_qkv_rope_batched))
                ST = ST[0] if n == 1 else ST
                launches[("o_proj+res", nm)] = lambda i, f=res, a=XA, w_=Wo[nm], o=HB: f(a, w_[i], o)
                launches[("down+res", nm)] = lambda i, f=res, a=XI, w_=Wd[nm], o=HB: f(a, w_[i], o)
                launches[("gate/up+silu", nm)] = lambda i, f=gu, a=X, gm=GM, w1=Wg[nm], w2=Wu[nm], o=ACT: f(a, gm, 1e-5, w1[i], w2[i], o)
                launches[("qkv+rope", nm)] = (lambda i, f=rope, a=X, gm=GM, w1=Wq[nm], w2=Wk[nm], w3=Wv[nm], q_=Q, k_=K, v_=V, st=ST:
                                              f(a, gm, 1e-5, w1[i], w2[i], w3[i], q_, k_, v_, 128, 1.0, 1e6, st))
            times = {key: [] for key in launches}
            for _ in range(4):  # A B A B
                for key, fn in launches.items():
                    times[key].append(graph_time(fn, NSET, 20))
            med = lambda ts: sorted(ts)[len(ts) // 2]
            for name in mib:
                tf, tb = times[(name, "f16")], times[(name, "bf16")]
                print(f"{model:10s} {n:2d} tokens {name:13s} f16 " + " ".join(f"{t:6.2f}" for t in tf) + "  bf16 " + " ".join(f"{t:6.2f}" for t in tb)
                      + f"  us | median f16 {med(tf):6.2f} ({mib[name] * 2e-6 / med(tf):5.2f} TB/s) bf16 {med(tb):6.2f}, f16 spread {max(tf) - min(tf):5.2f},"
                      + f" bf16 - f16 {med(tb) - med(tf):+6.2f}", flush=True)
        del Wo, Wd, Wg, Wu, Wq, Wk, Wv
        torch.cuda.empty_cache()
