"""Group-shared page selection against per-head selection, same process, A B A B (profiles/group_selection_cfg5.txt is this
script's output):

    A  the per-head two-launch layer:  append+estimate | top-k+attention(+merge), one selection per QUERY head
    B  the group-shared layer:         append+estimate | group-selection launch(+merge), one selection per KV head

on pools of random contents, state-driven launches as a captured step issues them, at
    cfg5_8seq_gqa   8 sequences x 32K tokens, 32 / 8 heads x 128, page 16, budget 2048 tokens (128 pages)
    llama31_8b_1seq one sequence of the same head shape at 32K

Per shape and round: us per sequence-layer of the chain and of the attention launch alone, and the algorithmic bytes of each
(metadata read once per kv head; selected K/V once per query head in A, once per kv head in B) over the time as a fraction
of 8 TB/s.  ``--ppc`` adds rounds of B with forced pages per workgroup (0 = the planner's split).

    python scripts/kbench_group_selection.py [--layers 8] [--rounds 3] [--reps 20] [--ppc 0 129]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

PEAK = 8.0e12  # bytes / s


def shape_bytes(hq, hkv, d, page, pages, budget):
    """Algorithmic bytes per sequence-layer: (metadata, selected K/V per-head, selected K/V group-shared)."""
    meta = (pages - 1) * hkv * 2 * d * 2
    kv_head = budget * page * d * 2 * 2
    return meta, hq * kv_head, hkv * kv_head


def run(label, n, hq, hkv, layers, rounds, reps, ppcs):
    import quest_amd.utils as qu
    from quest_amd import _kernels

    dev = torch.device("cuda:0")
    d, page, seqlen, budget = 128, 16, 32768, 2048 // 16
    b = qu.BatchedInferenceController(n, layers, hq, d, page, budget, seqlen + 4 * page, torch.float16, dev, num_kv_heads=hkv,
                                      layout="NHD_ROT", shuffle_seed=3, group_selection=True)
    b.prepare_metadata(seqlen)  # reserve the pages; the pools get random contents instead of a prefill
    g = torch.Generator(device=dev).manual_seed(1)
    for pool in (b.kv_pool, b.metadata_pool):
        for l in range(layers):
            pool.layer(l).copy_(torch.randn(pool.layer(l).shape, generator=g, device=dev, dtype=torch.float16))
    b.enable_device_state()
    b.begin_graph_decode()
    q = torch.randn(layers, n, hq, d, generator=g, device=dev, dtype=torch.float16)
    k = torch.randn(layers, n, hkv, d, generator=g, device=dev, dtype=torch.float16)
    v = torch.randn(layers, n, hkv, d, generator=g, device=dev, dtype=torch.float16)
    o, scores = torch.empty_like(q), qu.score_scratch(b)
    max_n = b.max_pages - 1
    h = b._decode_handler
    qu.step_advance_batched(b)
    pages = seqlen // page + 1
    meta, kv_a, kv_b = shape_bytes(hq, hkv, d, page, pages, budget)

    def ae(l):
        _kernels.append_estimate_batched(k[l], v[l], b.kv_layer(l), b.kv_tables, q[l], scores, b.metadata_layer(l), b.meta_tables,
                                         b.step_states, max_n, b.layout)

    def att_a(l):
        h.forward_fused_topk_batched(q[l], o[l], b.kv_layer(l), b.kv_tables, scores, b.step_states, max_n)

    def att_b(l):
        assert h.forward_group_topk(q[l], o[l], b.kv_layer(l), b.kv_tables, scores, b.step_states, max_n)

    def chain(att):
        def f(l):
            ae(l)
            att(l)
        return f

    print(f"# {label}: {n} sequence(s) x {seqlen} tokens, {hq} / {hkv} heads x {d}, page {page}, budget {budget} pages, NHD_ROT pools, "
          f"{layers} layers per graph, {reps} replays; us per sequence-layer")
    print(f"# algorithmic bytes per sequence-layer: metadata {meta / 1e6:.2f} MB; selected K/V per-head {kv_a / 1e6:.2f} MB, "
          f"group-shared {kv_b / 1e6:.2f} MB; chain A {(meta + kv_a) / 1e6:.2f} MB, chain B {(meta + kv_b) / 1e6:.2f} MB")
    for ppc in ppcs:
        h.set_pages_per_chunk(ppc)
        b.begin_graph_decode()
        for r in range(rounds):
            for name, att, kv_bytes in (("A per-head", att_a, kv_a), ("B group   ", att_b, kv_b)):
                if ppc and name.startswith("A"):
                    continue  # the forced split is B's sweep; A runs the planner's split
                t_att = bench.time_kernel_loop(att, layers, reps) / n
                t_chain = bench.time_kernel_loop(chain(att), layers, reps) / n
                info = h.last_launch_info()
                print(f"{label} ppc {ppc:3d} round {r} {name}: chain {t_chain:6.2f} us ({(meta + kv_bytes) / (t_chain * 1e-6) / PEAK:5.1%} "
                      f"of 8 TB/s)   attention(+merge) {t_att:6.2f} us ({kv_bytes / (t_att * 1e-6) / PEAK:5.1%})   "
                      f"front end {info['front_end_variant']}, {info['workgroups_per_head']} workgroup(s) per "
                      f"{'kv head' if info['front_end_variant'] == 9 else 'head'}")
    h.set_pages_per_chunk(0)
    del b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ppc", type=int, nargs="*", default=[0])
    x = ap.parse_args()
    run("cfg5_8seq_gqa", 8, 32, 8, x.layers, x.rounds, x.reps, x.ppc)
    run("llama31_8b_1seq", 1, 32, 8, x.layers, x.rounds, x.reps, x.ppc)


if __name__ == "__main__":
    main()
