"""The ``lse`` output of the attention entries (include/quest_hip.h ``float* lse``), reached through the handler's ``lse_out``.

The device writes it at five places, each through the per-sequence row offset of ``select_sequence``: the one-workgroup
tail of the per-head kernel, ``merge_head_fast`` (2 to 32 partials per head), the generic merge (more than 32), the
group-shared kernel's tail, and the one-launch layer.  Every one is run here and named by an assertion on the plan.

Bit-equalities (no number involved): NHD_ROT == NHD; graph replay == eager; sequence i of a batched launch == that sequence
alone under the same split; fused top-k launch == index-tensor launch under the same waves; a launch that also carries the
armed step advance == the same launch without it.  (Poisoned pool == zero pool is in test_gpu_uninitialised_pools.py.)
Around every LSE buffer sit NaN guards: after a launch all ``n_seqs * Hq`` values are finite and the guards are untouched;
with ``lse_out = None`` nothing is written.

Against a reference: ``oracle.torch_ref.lse_f64`` -- float64 numpy, ``log sum exp(q.k / sqrt(D))`` over the tokens of the
selected pages plus the valid tokens of the current page, read from the oracle's pools as stored.  The page sets are fixed
by the test (random per head; crafted score rows make the fused top-k select exactly them), so the reference does not
depend on a device result.  Tolerance: the yardstick is the same formula in float32 on the CPU (``torch.logsumexp`` of
float32 scores, ``lse_f32``); the kernel may be off by FOUR times the yardstick's largest error against float64 over this
module's own cases -- it sums per lane row, per wave and per chunk, in another order, and takes exp2 / log2 from the
hardware at one ulp each -- and never by less than one float32 ulp of the value.
Measured on an MI355X (profiles/lse_parity.txt; the values lie between about 4 and 7, where one float32 ulp is 4.8e-07): the
yardstick's largest error 5.17e-07, so the bound is 2.07e-06; the kernels' largest error 9.05e-07 (group-shared kernel, one
workgroup per head), 8.1e-07 through the merges, 4.9e-07 at budget 4.

One property test of what the LSE is for: the attention over pages A u B equals the LSE-weighted merge, in float64, of the
attention over A and over B, at the suite's attention tolerance (atol 2e-3; rtol 2e-3 fp16 / 2^-8 bf16)."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import torch_ref
import _bf16
import _harness as H
from test_gpu_uninitialised_pools import GUARD, _Lse, _dev, _f32, _fill, _same_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# head_dim, page, Hq, Hkv, bf16, layout
CASES = [(64, 16, 4, 2, False, 0), (128, 16, 3, 3, True, 1), (256, 16, 4, 2, False, 2), (128, 7, 4, 2, True, 0),
         (64, 7, 3, 3, False, 1), (256, 7, 3, 3, True, 2), (128, 16, 4, 2, False, 2), (64, 16, 3, 3, True, 0)]
_id = lambda c: "D%d_S%d_Hq%d_Hkv%d_%s_layout%d" % (c[0], c[1], c[2], c[3], "bf16" if c[4] else "fp16", c[5])
PAGES = (42, 44, 47)   # three sequences of ragged lengths; the current page holds 5 / S / 1 tokens
# name, selected pages, pages per workgroup, workgroups per head: the tail of the attention kernel | merge_head_fast | the
# generic merge (40 selected pages + the current one at one page per workgroup, ~ 770 tokens at page 16).  In this order
# every plan has another budget than the one before (the batched controller plans again when the budget changes).
PLANS = (("one_workgroup", 3, 4, 1), ("merge_generic", 40, 1, 41), ("merge_fast", 3, 2, 2))


def _lens(S):
    return tuple((p - 1) * S + l for p, l in zip(PAGES, (5, S, 1)))


def record(line: str) -> None:
    """A measured figure: printed, and appended to the file QUEST_LSE_PARITY_FILE names (profiles/lse_parity.txt is such a
    file, as these tests wrote it)."""
    print(line)
    path = os.environ.get("QUEST_LSE_PARITY_FILE")
    if path:
        new = not os.path.exists(path)
        with open(path, "a") as f:
            if new:
                f.write("# written by tests/test_gpu_lse.py (record()) with QUEST_LSE_PARITY_FILE=<this file> pytest tests/test_gpu_lse.py -m gpu\n"
                        "# one line per measurement: <test case> | <figures>; how the bound is set is in the module's docstring\n")
            case = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].replace("tests/", "")
            f.write(f"{case} | {line}\n")


# ------------------------------------------------------------------------------------------------ the reference
def _keys(kv_o, pages, n_tokens, hk):
    """Keys of kv head ``hk`` over the logical ``pages`` (the last one holding the tail), as stored in the oracle's pool."""
    return H.gather_entries(kv_o.data, pages, n_tokens, 0)[0][:, hk]


def _lse_pair(q, kv_o, sel, L, S, group):
    """(float64 reference, float32 yardstick) ``[Hq]`` for per-head logical page lists ``sel`` + the current page."""
    last, lpl = (L - 1) // S, (L - 1) % S + 1
    keys = np.stack([_keys(kv_o, [int(p) for p in sel[h]] + [last], len(sel[h]) * S + lpl, h // group) for h in range(q.shape[1])])
    return torch_ref.lse_f64(q[0], keys), torch_ref.lse_f32(q[0].astype(np.float32), keys.astype(np.float32)).numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Inputs, page sets and references of a case, computed once on the CPU: per plan random per-head page sets, every page
    (the dense launches), and the oracle's own selection for budget 4 (the one-launch layer computes its scores itself)."""
    D, S, Hq, Hkv, bf16, layout = case
    rng = np.random.default_rng(D * 1000 + S * 10 + Hq)
    lens = _lens(S)
    data = [_bf16.inputs(900 + D + S + i, L, Hq, Hkv, D) for i, L in enumerate(lens)]
    ref = {"data": data, "sel": {}, "lse": {}, "yard": {}}
    pools = []
    for (q, k, v), L in zip(data, lens):
        n_pages = -(-L // S)
        kv = oracle.Paged(np.zeros((n_pages, 2, S, Hkv, D), np.float16), np.arange(n_pages, dtype=np.int32), (L - 1) % S + 1, 0)
        meta = oracle.Paged(np.zeros((-(-n_pages // S), 2, S, Hkv, D), np.float16), np.arange(-(-n_pages // S), dtype=np.int32),
                            (n_pages - 1) % S + 1, 0)
        oracle.append_prefill(kv, meta, k, v)
        pools.append((kv, meta))
    sets = {name: [np.stack([np.sort(rng.choice(p - 1, n_sel, replace=False)) for _ in range(Hq)]) for p in PAGES]
            for name, n_sel, _, _ in PLANS}
    sets["dense"] = [np.tile(np.arange(p - 1), (Hq, 1)) for p in PAGES]
    # union property: per head A (3 pages) and B (3 pages + one page b0 common to the heads, which that launch is handed as
    # its "current" page), disjoint
    sets["b0"] = [int(rng.integers(p - 1)) for p in PAGES]
    ab = [np.stack([rng.choice(np.delete(np.arange(p - 1), b0), 6, replace=False) for _ in range(Hq)])
          for p, b0 in zip(PAGES, sets["b0"])]
    sets["A"], sets["B"] = [x[:, :3] for x in ab], [x[:, 3:] for x in ab]
    sets["layer"] = []
    for (q, k, v), (kv, meta), p in zip(data, pools, PAGES):
        _, ei = oracle.topk(oracle.estimate(q, meta), np.tile(np.arange(p - 1, dtype=np.int32), (Hq, 1)), 3)
        sets["layer"].append(ei)
    for name, per_seq in sets.items():
        if name in ("A", "B", "b0"):
            continue
        pairs = [_lse_pair(d[0], kv, sel, L, S, Hq // Hkv) for d, (kv, _), sel, L in zip(data, pools, per_seq, lens)]
        ref["lse"][name], ref["yard"][name] = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    ref["sel"] = sets
    return ref


@functools.lru_cache(maxsize=None)
def _yardstick():
    """Largest error of the float32 yardstick against float64 over every case of this module."""
    return max(float(np.abs(r["yard"][name] - r["lse"][name]).max()) for r in map(_reference, CASES) for name in r["lse"])


def _check(got, want, what):
    """``got`` float32 device LSE against the float64 reference: within 4 x the yardstick's largest error, at least one
    float32 ulp of the value."""
    got = np.asarray(got, np.float32).reshape(want.shape)
    err = np.abs(got.astype(np.float64) - want)
    bound = np.maximum(4 * _yardstick(), np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    record(f"{what}: kernel max err {err.max():.3e} (worst err / bound {float((err / bound).max()):.3f}); yardstick (float32 logsumexp) "
           f"max err over the module's cases {_yardstick():.3e}; bound {4 * _yardstick():.3e}, at least 1 float32 ulp")
    assert (err <= bound).all(), (what, float(err.max()), float(bound.min()))


# ------------------------------------------------------------------------------------------------ device side
def _single(case, i, budget=4, layout=None, seed=11):
    """Sequence i of a case alone in its own pools, all but its last token appended."""
    import quest_amd.utils as qu

    D, S, Hq, Hkv, bf16, lay = case
    L = _lens(S)[i]
    _, k, v = _reference(case)["data"][i]
    c = qu.InferenceController(1, Hq, D, S, budget, L + 3 * S, torch.bfloat16 if bf16 else torch.float16, torch.device(DEV),
                               num_kv_heads=Hkv, layout=lay if layout is None else layout, shuffle_seed=seed + i)
    _fill(c, _dev(k, bf16), _dev(v, bf16), [L - 1])
    c.end_forward()
    return c


def _batch(case, budget=4):
    import quest_amd.utils as qu

    D, S, Hq, Hkv, bf16, layout = case
    lens = _lens(S)
    b = qu.BatchedInferenceController(len(lens), 1, Hq, D, S, budget, max(lens) + 3 * S, torch.bfloat16 if bf16 else torch.float16,
                                      torch.device(DEV), num_kv_heads=Hkv, layout=layout, shuffle_seed=3)
    for c, (_, k, v), L in zip(b.seqs, _reference(case)["data"], lens):
        _fill(c, _dev(k, bf16), _dev(v, bf16), [L - 1])
        c.end_forward()
    b.enable_device_state()
    return b


def _step_inputs(case):
    D, S, Hq, Hkv, bf16, layout = case
    data, lens = _reference(case)["data"], _lens(S)
    return (torch.cat([_dev(d[0], bf16) for d in data]), torch.cat([_dev(d[1][L - 1:L], bf16) for d, L in zip(data, lens)]),
            torch.cat([_dev(d[2][L - 1:L], bf16) for d, L in zip(data, lens)]))


def _phys(c, logical):
    table = np.array(c.kv_cache.indicies, np.int32)
    return table[np.asarray(logical)]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_index_tensor_launches_at_every_merge_form(case):
    """forward_batched over fixed page sets of three ragged sequences with 1, 2 and 41 workgroups per head: the attention
    kernel's tail, merge_head_fast and the generic merge write the LSE; each against float64, and row i bit for bit the
    launch of sequence i alone under the same split."""
    import quest_amd.utils as qu

    D, S, Hq, Hkv, bf16, layout = case
    ref, lens, n = _reference(case), _lens(S), len(PAGES)
    qd, kd, vd = _step_inputs(case)
    b = _batch(case)
    h = b._decode_handler
    singles = [_single(case, i) for i in range(n)]
    for step, (name, n_sel, ppc, chunks) in enumerate(PLANS):
        b.set_page_budgets([n_sel + 1] * n)
        h.set_pages_per_chunk(ppc)
        if step == 0:
            b.prepare_metadata(1)
        b.begin_forward()
        assert h.plan_info() == (ppc, chunks), (name, h.plan_info())
        if step == 0:
            qu.append_kv_batched(kd, vd, b, 0)
        idx = _i32(np.stack([_phys(c, ref["sel"][name][i]) for i, c in enumerate(b.seqs)]))
        lse = _Lse(h, n * Hq)
        o = qu.decode_sparse_attn_batched(qd, b, 0, idx)
        info = h.last_launch_info()
        assert info["keys_per_thread"] == 0 and info["workgroups_per_head"] == chunks and info["n_seqs"] == n, (name, info)
        got = lse.take().reshape(n, Hq)
        _check(got, ref["lse"][name], f"forward_batched, {name}")
        h.lse_out = None   # no LSE asked for: the buffer (NaN again after take()) stays as it is
        o_none = qu.decode_sparse_attn_batched(qd, b, 0, idx)
        assert bool(torch.isnan(lse.buf).all()) and _same_bytes(_bf16.bits(o_none), _bf16.bits(o))
        for i, c in enumerate(singles):
            hc = c._decode_handler
            if step == 0:
                c.prepare_metadata(1)
            c.set_page_budget(n_sel + 1)
            hc.set_pages_per_chunk(ppc)
            c.begin_forward(1)
            assert hc.plan_info() == (ppc, chunks)
            if step == 0:
                qu.append_kv(kd[i:i + 1], vd[i:i + 1], c, 0)
            lse_s = _Lse(hc, Hq)
            o_s = qu.decode_sparse_attn(qd[i:i + 1], c, 0, _i32(_phys(c, ref["sel"][name][i])))
            assert hc.last_launch_info()["workgroups_per_head"] == chunks
            assert _same_bytes(lse_s.take(), got[i]), f"{name}: sequence {i} alone"
            assert _same_bytes(_bf16.bits(o_s[0]), _bf16.bits(o[i])), f"{name}: sequence {i} alone (output)"
            hc.lse_out = None
            c.end_forward()


@pytest.mark.parametrize("case", CASES[:6], ids=_id)
def test_layouts_graph_replay_and_fused_topk_leave_the_same_bits(case):
    """Sequence 0 alone in an NHD and an NHD_ROT pool: index-tensor launch, fused top-k launch (same waves) and a graph
    replay of the index-tensor launch all write the same LSE bits, in both layouts."""
    import quest_amd.utils as qu

    D, S, Hq, Hkv, bf16, _ = case
    q, k, v = _reference(case)["data"][0]
    L = _lens(S)[0]
    qd, kd, vd = _dev(q, bf16), _dev(k[L - 1:L], bf16), _dev(v[L - 1:L], bf16)
    per_layout = []
    for layout in (0, 2):
        c = _single(case, 0, layout=layout)
        h = c._decode_handler
        h.set_pages_per_chunk(2)
        c.prepare_metadata(1)
        c.begin_forward(1)
        assert h.plan_info() == (2, 2)
        lse = _Lse(h, Hq)
        est = qu.decode_append_estimate(qd, kd, vd, c, 0)
        qu.decode_topk(est, c)
        idx = c.topk_dindices_buffer.clone()
        o1 = qu.decode_sparse_attn(qd, c, 0, idx)
        waves = h.last_launch_info()["waves"]
        l1 = lse.take()
        o2 = qu.decode_topk_sparse_attn(qd, est, c, 0)
        info = h.last_launch_info()
        assert info["keys_per_thread"] > 0 and info["waves"] == waves and info["workgroups_per_head"] == 2, info
        assert _same_bytes(lse.take(), l1) and _same_bytes(_bf16.bits(o2), _bf16.bits(o1)), "fused top-k vs index tensor"
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            qu.decode_sparse_attn(qd, c, 0, idx)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        lse.take()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            o3 = qu.decode_sparse_attn(qd, c, 0, idx)
        lse.buf.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bytes(lse.take(), l1) and _same_bytes(_bf16.bits(o3), _bf16.bits(o1)), "graph replay vs eager"
        h.lse_out = None
        c.end_forward()
        per_layout.append((l1, _bf16.bits(o1), idx.cpu().numpy()))
    for a, b_ in zip(*per_layout):  # (same shuffle seed: same physical pages)
        assert _same_bytes(a, b_), "NHD_ROT vs NHD"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_state_driven_fused_launch_with_and_without_the_armed_advance(case):
    """forward_fused_topk_batched of one sequence on crafted score rows (ones at the fixed page set: the top-k selects exactly
    it), two workgroups per head: the merge launch writes the LSE; with the step advance armed the same launch also moves
    the state one token on, and writes the same bits."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    D, S, Hq, Hkv, bf16, layout = case
    ref, L = _reference(case), _lens(S)[0]
    q, k, v = ref["data"][0]
    qd = _dev(q, bf16)
    c = _single(case, 0)
    c.enable_device_state()
    h = c._decode_handler
    h.set_pages_per_chunk(2)
    c.begin_graph_decode()
    assert h.plan_info() == (2, 2)
    qu.step_advance_dyn(c)
    _kernels.append_kv_cache_decode_batched(_dev(k[L - 1:L], bf16), _dev(v[L - 1:L], bf16), c.kv_layer(0), c.kv_tables,
                                            c.metadata_layer(0), c.meta_tables, c.step_states, c.layout)
    scores = qu.score_scratch(c).zero_()
    sel = ref["sel"]["merge_fast"][0]
    for hq in range(Hq):
        scores[hq, torch.from_numpy(sel[hq]).to(DEV)] = 1.0
    sel_i = torch.full((1, Hq, 3), -1, dtype=torch.int32, device=DEV)
    h.set_selection_out(None, sel_i)
    lse, o = _Lse(h, Hq), torch.empty_like(qd)
    launch = lambda: h.forward_fused_topk_batched(qd, o, c.kv_layer(0), c.kv_tables, scores, c.step_states, c.max_pages - 1)
    launch()
    info = h.last_launch_info()
    assert info["keys_per_thread"] > 0 and info["workgroups_per_head"] == 2, info
    assert np.array_equal(sel_i[0].cpu().numpy(), _phys(c, sel))
    l1, o1 = lse.take(), _bf16.bits(o)
    assert c.step_state.cpu().tolist()[0] == L
    _check(l1, ref["lse"]["merge_fast"][0], "forward_fused_topk_batched, merge_fast")
    h.arm_step_advance(c.step_states, c.kv_tables, c.meta_tables, c.page_size)
    launch()
    h.set_selection_out(None, None)
    assert _same_bytes(lse.take(), l1) and _same_bytes(_bf16.bits(o), o1), "merge launch that carries the step advance"
    c.prepare_metadata(1)
    c.prepare_metadata(1)
    kvc, mc = c.kv_cache, c.metadata_cache
    assert c.step_state.cpu().tolist()[:7] == [L + 1, len(kvc.indicies), kvc.last_page_len, kvc.indicies[-1], len(mc.indicies),
                                               mc.last_page_len, mc.indicies[-1]]
    h.lse_out = None


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dense_launches_and_the_one_launch_layer(case):
    """append_forward_shared_batched (the group-shared kernel where it serves the shape: page 16, head_dim 64 / 128; else the
    append launch + the per-head kernel on the one table) over every page of three ragged sequences with 1, 7 and 50
    workgroups per head; and, where it exists (fp16, page 16, head_dim 64 / 128), the one-launch layer against the oracle's
    selection."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    D, S, Hq, Hkv, bf16, layout = case
    ref, n = _reference(case), len(PAGES)
    qd, kd, vd = _step_inputs(case)
    b = _batch(case)
    b.begin_graph_decode(dense_layers=True)
    dh = b._dense_handler
    qu.step_advance_batched(b)
    b.prepare_metadata(1)   # (host mirror of the reservation)
    shared_shape = S == 16 and D in (64, 128)
    for ppc in (64, 8, 1):
        dh.set_pages_per_chunk(ppc)
        b.begin_graph_decode(dense_layers=True)
        chunks = -(-b.max_pages // ppc)
        assert dh.plan_info()[1] == chunks and chunks in (1, 7, 50), dh.plan_info()
        lse, o = _Lse(dh, n * Hq), torch.empty_like(qd)
        ok = dh.append_forward_shared_batched(kd, vd, b.metadata_layer(0), b.meta_tables, qd, o, b.kv_layer(0), b.kv_tables,
                                              b.step_states)
        assert ok == shared_shape
        if not ok:
            _kernels.append_kv_cache_decode_batched(kd, vd, b.kv_layer(0), b.kv_tables, b.metadata_layer(0), b.meta_tables,
                                                    b.step_states, b.layout)
            dh.forward_shared_batched(qd, o, b.kv_layer(0), b.kv_tables, b.step_states)
            assert dh.last_launch_info()["workgroups_per_head"] == chunks
        _check(lse.take().reshape(n, Hq), ref["lse"]["dense"],
               f"{'group-shared' if ok else 'per-head'} kernel over every page, {chunks} workgroups per head")
        dh.lse_out = None
    if not bf16 and shared_shape:
        h = b._decode_handler
        h.set_pages_per_chunk(4)
        b.begin_graph_decode(dense_layers=True)
        assert h.plan_info() == (4, 1)
        got = []
        for one in (True, False):
            sel_i = torch.full((n, Hq, 3), -1, dtype=torch.int32, device=DEV)
            h.set_selection_out(None, sel_i)
            lse = _Lse(h, n * Hq)
            o = qu.decode_layer_batched(qd, kd, vd, b, 0, qu.score_scratch(b).zero_(), one_launch=one, tiles=False)
            h.set_selection_out(None, None)
            info = h.last_launch_info()
            assert (info["front_end_variant"] == 7) == one and info["workgroups_per_head"] == 1 and info["n_seqs"] == n, info
            for i, c in enumerate(b.seqs):
                assert np.array_equal(sel_i[i].cpu().numpy(), _phys(c, ref["sel"]["layer"][i])), (one, i)
            got.append((lse.take(), _bf16.bits(o)))
            h.lse_out = None
        # (8-wave and 4-wave gathers fold a head's pages in another order: the two forms are not compared bit for bit here;
        # test_gpu_batched.py does that at a capacity where both gather with 8 waves)
        _check(got[0][0].reshape(n, Hq), ref["lse"]["layer"], "one-launch layer")
        _check(got[1][0].reshape(n, Hq), ref["lse"]["layer"], "two-launch layer, one workgroup per head")


@pytest.mark.parametrize("case", CASES[:6], ids=_id)
def test_attention_over_a_union_is_the_lse_weighted_merge(case):
    """What the LSE is for: o(A u B) == (o_A e^lse_A + o_B e^lse_B) / (e^lse_A + e^lse_B), computed in float64 from two
    launches' outputs, against ONE launch over the union.  Per head A = 3 pages + the current page; B = 3 + 1 full pages,
    the one handed over as that launch's "current" page; the union = 7 pages + the current page."""
    import quest_amd.utils as qu

    D, S, Hq, Hkv, bf16, layout = case
    ref, L = _reference(case), _lens(S)[0]
    q, k, v = ref["data"][0]
    qd = _dev(q, bf16)
    c = _single(case, 0)
    h = c._decode_handler
    c.prepare_metadata(1)
    A, Bp = _phys(c, ref["sel"]["A"][0]), _phys(c, ref["sel"]["B"][0])
    b0 = _phys(c, np.full((Hq, 1), ref["sel"]["b0"][0]))
    buf, cur, lpl = c.kv_cache.buf_layer(0), c.kv_cache.indicies[-1], c.kv_cache.last_page_len
    res = {}
    for name, idx, last, last_len in (("A", A, cur, lpl), ("B", Bp, b0[0, 0], S), ("AB", np.concatenate([A, Bp, b0], 1), cur, lpl)):
        c.set_page_budget(idx.shape[1] + 1)
        c.begin_forward(1)
        if name == "A":
            qu.append_kv(_dev(k[L - 1:L], bf16), _dev(v[L - 1:L], bf16), c, 0)
        lse, o = _Lse(h, Hq), torch.empty_like(qd)
        h.forward(qd, o, buf, _i32(idx), c.kv_indptr_for_approx_decode, last_len, int(last))
        res[name] = (_f32(_bf16.bits(o), bf16)[0].astype(np.float64), lse.take().astype(np.float64))
        h.lse_out = None
        c.end_forward()
    (oa, la), (ob, lb), (ou, lu) = res["A"], res["B"], res["AB"]
    m = np.maximum(la, lb)
    wa, wb = np.exp(la - m)[:, None], np.exp(lb - m)[:, None]
    merged = (oa * wa + ob * wb) / (wa + wb)
    bound = 2e-3 + (2.0 ** -8 if bf16 else 2e-3) * np.abs(ou)
    assert (np.abs(merged - ou) <= bound).all(), float((np.abs(merged - ou) / bound).max())
    # the merged LSE is the union's: its error is at most the larger of the two parts' errors (their weights sum to one)
    # plus the union launch's own, so twice the bound of one LSE
    lm = m + np.log(wa + wb)[:, 0]
    assert (np.abs(lm - lu) <= 2 * np.maximum(4 * _yardstick(), np.spacing(np.abs(lu).astype(np.float32)))).all(), float(np.abs(lm - lu).max())
