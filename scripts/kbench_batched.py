"""Per-op timing of the batched state-driven launches (8 sequences, cfg-3 shapes): append+estimate,
top-k+attention(+merge), and the whole layer, for a sweep of pages-per-chunk.

    python scripts/kbench_batched.py --dtype bf16     fp16 against bf16 pools, A B A B in one process: the append+estimate launch and the
                                                      top-k+attention(+merge) launch at cfg-3 (32 heads, 1 sequence) and cfg-5 (32 / 8
                                                      heads, 8 sequences) shapes on NHD_ROT pools of random contents
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def compare_dtypes(layers: int, rounds: int = 2, reps: int = 20) -> None:
    """fp16 vs bf16, the same launches on pools of the same shape: both move the same bytes."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    dev = torch.device("cuda:0")
    D, page, seqlen, budget = 128, 16, 32768, 2048 // 16
    for label, n, hq, hkv in (("cfg-3 shapes (32 heads, 1 sequence)", 1, 32, 32), ("cfg-5 shapes (32 / 8 heads, 8 sequences)", 8, 32, 8)):
        work = {}
        for dt in (torch.float16, torch.bfloat16):
            b = qu.BatchedInferenceController(n, layers, hq, D, page, budget, seqlen + 4 * page, dt, dev, num_kv_heads=hkv,
                                              layout="NHD_ROT", shuffle_seed=3)
            b.prepare_metadata(seqlen)  # reserve the pages; the pools get random contents instead of a prefill
            g = torch.Generator(device=dev).manual_seed(1)
            for pool in (b.kv_pool, b.metadata_pool):
                for l in range(layers):
                    pool.layer(l).copy_(torch.randn(pool.layer(l).shape, generator=g, device=dev, dtype=torch.float16))
            b.enable_device_state()
            b.begin_graph_decode()
            q = torch.randn(layers, n, hq, D, generator=g, device=dev, dtype=torch.float16).to(dt)
            k = torch.randn(layers, n, hkv, D, generator=g, device=dev, dtype=torch.float16).to(dt)
            v = torch.randn(layers, n, hkv, D, generator=g, device=dev, dtype=torch.float16).to(dt)
            o, scores = torch.empty_like(q), qu.score_scratch(b)
            max_n = b.max_pages - 1
            qu.step_advance_batched(b)

            def ae(l, b=b, q=q, k=k, v=v, scores=scores, max_n=max_n):
                _kernels.append_estimate_batched(k[l], v[l], b.kv_layer(l), b.kv_tables, q[l], scores, b.metadata_layer(l),
                                                 b.meta_tables, b.step_states, max_n, b.layout)

            def ts(l, b=b, q=q, o=o, scores=scores, max_n=max_n):
                b._decode_handler.forward_fused_topk_batched(q[l], o[l], b.kv_layer(l), b.kv_tables, scores, b.step_states, max_n)

            work[dt] = (ae, ts, b)
        print(f"# {label}: seqlen {seqlen}, budget {budget} pages, {layers} layers (pools) per graph, NHD_ROT, us per launch")
        for r in range(rounds):
            for dt in (torch.float16, torch.bfloat16):
                ae, ts, b = work[dt]
                t_ae = bench.time_kernel_loop(ae, layers, reps)
                t_ts = bench.time_kernel_loop(ts, layers, reps)
                info = b._decode_handler.last_launch_info()
                print(f"round {r} {str(dt).replace('torch.', ''):8s}: append+estimate {t_ae:7.2f}   top-k+attention(+merge) {t_ts:7.2f}   "
                      f"(front end {info['front_end_variant']}, {info['workgroups_per_head']} workgroup(s) per head)")
        del work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16", help="bf16: fp16 vs bf16 pools, A B A B (see above)")
    ap.add_argument("--seqs", type=int, default=8)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--ppc", type=int, nargs="*", default=[0, 16, 32, 64, 128])
    x = ap.parse_args()
    if x.dtype == "bf16":
        compare_dtypes(x.layers)
        return
    sys.argv = [sys.argv[0]]
    a = bench.parse()
    a.layers, a.steps, a.warmup = x.layers, 8, 2
    dev = torch.device("cuda:0")
    from quest_amd import _kernels
    import quest_amd.utils as qu

    w = bench.BatchedWorkload(a, dev, x.seqs)
    b = w.ctl
    bpl = bench.bytes_per_layer(a)
    max_n = b.max_pages - 1

    def ae(l):
        _kernels.append_estimate_batched(w.k1[l], w.v1[l], b.kv_layer(l), b.kv_tables, w.q[l], w.scores,
                                         b.metadata_layer(l), b.meta_tables, b.step_states, max_n, b.layout)

    def ts(l):
        b._decode_handler.forward_fused_topk_batched(w.q[l], w.o[l], b.kv_layer(l), b.kv_tables, w.scores,
                                                     b.step_states, max_n)

    def both(l):
        ae(l)
        ts(l)

    qu.step_advance_batched(b)
    t_ae = bench.time_kernel_loop(ae, a.layers, 10)
    print(f"append+estimate batched: {t_ae:.1f} us per launch = {t_ae / x.seqs:.2f} us/seq, "
          f"{x.seqs * (bpl['append'] + bpl['estimate']) / t_ae / 1e3:.0f} GB/s")
    for ppc in x.ppc:
        b._decode_handler.set_pages_per_chunk(ppc)
        try:
            b.begin_graph_decode()
            t_ts = bench.time_kernel_loop(ts, a.layers, 10)
            t_l = bench.time_kernel_loop(both, a.layers, 10)
        except Exception as e:  # unsupported split
            print(f"ppc {ppc}: {e}")
            continue
        print(f"ppc {ppc:3d} plan {b._decode_handler.plan_info()}: topk+attn(+merge) {t_ts:.1f} us = {t_ts / x.seqs:.2f} us/seq, "
              f"{x.seqs * bpl['attn'] / t_ts / 1e3:.0f} GB/s; layer {t_l:.1f} us = {t_l / x.seqs:.2f} us/seq")


if __name__ == "__main__":
    main()
