"""Batched long-row decode, whole-row front end (A) vs tiles front end (B): BASELINE configs[3] shapes (Hq 32 / Hkv 8 /
D 128, 128K context, budget 4096 tokens) with 2, 4 and 8 sequences per GPU, a few layers each (a sequence's pools are
0.5 GiB per layer).  Per launch and per sequence-layer: append+estimate without / with tile maxima, top-k+attention
whole-row / tiles, the two-launch layer, and a captured step (advance + every layer) of each form.

A and B alternate (A B A B ...) inside this one process on the same controller, the same plan and the same pools; both
forms are warmed first (time_kernel_loop runs every launch once before it captures).  A is the path of
decode_layer_batched(tiles=False): the launches a batch took before the tiles entries existed, bit for bit.

    python scripts/kbench_batched_tiles.py [--seqs 2 4 8] [--layers 4] [--rounds 3] [--reps 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

PEAK_BPS = 8e12  # MI355X HBM3E peak, the denominator VERDICT.md uses


def run(a, dev, seqs, rounds, reps):
    from quest_amd import _kernels
    import quest_amd.utils as qu

    w = bench.BatchedWorkload(a, dev, seqs)
    b, h = w.ctl, w.ctl._decode_handler
    bpl = bench.bytes_per_layer(a)
    max_n = b.max_pages - 1
    assert w.scores.size(2) >= _kernels.tiles_row_stride(max_n), "the scratch has no room for the tile maxima"
    print(f"== {seqs} sequences x {a.layers} layers, {bpl['pages']} pages each, budget {bpl['budget_pages']} pages, "
          f"capacity {b.max_pages} pages, plan (pages per workgroup, workgroups per head) {h.plan_info()}, "
          f"tiles_min_pages {b.tiles_min_pages}", flush=True)

    def ae(tiles):
        def fn(l):
            ok = _kernels.append_estimate_batched(w.k1[l], w.v1[l], b.kv_layer(l), b.kv_tables, w.q[l], w.scores,
                                                  b.metadata_layer(l), b.meta_tables, b.step_states, max_n, b.layout, tiles=tiles)
            assert ok
        return fn

    def ts(tiles):
        def fn(l):
            ok = h.forward_fused_topk_batched(w.q[l], w.o[l], b.kv_layer(l), b.kv_tables, w.scores, b.step_states, max_n,
                                              b.page_budgets, tiles=tiles)
            assert ok
        return fn

    def layer(tiles):
        def fn(l):
            qu.decode_layer_batched(w.q[l], w.k1[l], w.v1[l], b, l, w.scores, out=w.o[l], one_launch=False, tiles=tiles)
        return fn

    qu.step_advance_batched(b)
    ae(True)(0)  # the maxima of layer 0 are in the scratch before either attention form is timed on it
    variants = {}
    for tiles in (False, True):
        ts(tiles)(0)
        variants[tiles] = h.last_launch_info()
    print(f"   A whole-row launch: {variants[False]}\n   B tiles launch:     {variants[True]}", flush=True)
    assert variants[True]["front_end_variant"] == 8 and variants[False]["front_end_variant"] != 8
    torch.cuda.synchronize()

    rows = [("append+estimate", ae, bpl["append"] + bpl["estimate"]),
            ("top-k+attention(+merge)", ts, bpl["topk"] + bpl["attn"]),
            ("two-launch layer", layer, bpl["chain"])]
    results = {}
    for name, make, nbytes in rows:
        t = {False: [], True: []}
        for _ in range(rounds):
            for tiles in (False, True):  # A B A B
                if make is ts:
                    ae(tiles)(0)  # (every layer's scores / maxima are in place: the scratch is shared by the layers)
                t[tiles].append(bench.time_kernel_loop(make(tiles), a.layers, reps))
        results[name] = t
        for tiles in (False, True):
            best = min(t[tiles])
            print(f"   {name:26s} {'B tiles    ' if tiles else 'A whole-row'}: rounds " + " ".join(f"{x:7.2f}" for x in t[tiles])
                  + f" us per launch; best {best:7.2f} = {best / seqs:6.2f} us per sequence-layer, "
                  f"{seqs * nbytes / best / 1e3:6.0f} GB/s", flush=True)
        sa = max(t[False]) - min(t[False])
        print(f"   {name:26s} B - A (best): {min(t[True]) - min(t[False]):+.2f} us per launch; spread of the A rounds {sa:.2f} us",
              flush=True)

    # a captured step of each form: advance + every layer.  Each replay appends a token per sequence, so the replays are
    # counted against the pools' capacity.
    def step_graph(tiles):
        def step():
            qu.step_advance_batched(b)
            for l in range(a.layers):
                qu.decode_layer_batched(w.q[l], w.k1[l], w.v1[l], b, l, w.scores, out=w.o[l], one_launch=False, tiles=tiles)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        return g

    graphs = {tiles: step_graph(tiles) for tiles in (False, True)}
    room = b.max_pages * a.page_size - int(b.step_states[:, 0].max()) - 2
    step_reps = max(1, min(reps, room // (2 * rounds) - 2))
    t = {False: [], True: []}
    for _ in range(rounds):
        for tiles in (False, True):
            g = graphs[tiles]
            g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(step_reps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            t[tiles].append(e0.elapsed_time(e1) * 1e3 / step_reps)
    assert int(b.step_states[:, 0].max()) < b.max_pages * a.page_size
    for tiles in (False, True):
        best = min(t[tiles])
        frac = seqs * a.layers * bpl["chain"] / (best * 1e-6) / PEAK_BPS
        print(f"   captured step ({step_reps} replays)  {'B tiles    ' if tiles else 'A whole-row'}: rounds "
              + " ".join(f"{x:8.2f}" for x in t[tiles])
              + f" us per step; best {best:8.2f} = {best / (seqs * a.layers):6.2f} us per sequence-layer, chain "
              f"{frac:.3f} of {PEAK_BPS / 1e12:.0f} TB/s", flush=True)
    sa = max(t[False]) - min(t[False])
    print(f"   captured step              B - A (best): {min(t[True]) - min(t[False]):+.2f} us per step; spread of the A rounds "
          f"{sa:.2f} us", flush=True)
    results["captured step"] = t
    del graphs, w
    torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    x = ap.parse_args()
    a = bench.parse(["--config", "4"])
    a.layers, a.steps, a.warmup = x.layers, 200, 2  # (steps sizes the pools' spare capacity: 2 tokens per step)
    dev = torch.device("cuda:0")
    print(f"{torch.cuda.get_device_name(dev)}; config 4: Hq {a.heads} / Hkv {a.kv_heads} / D {a.head_dim}, {a.seqlen} tokens, "
          f"budget {a.token_budget} tokens, layout {a.layout}")
    for seqs in x.seqs:
        run(a, dev, seqs, x.rounds, x.reps)


if __name__ == "__main__":
    main()
