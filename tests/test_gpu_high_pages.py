"""Every KV-pool kernel on pages beyond 4 GiB and beyond 8 GiB of a pool layer.

Every kernel that touches the paged KV pool computes ``pool + page * st.page + ...`` in 16-bit elements from int32 page
ids and uint32 strides and walk offsets, each site with its own widening cast (append.hip, append_device.cuh,
decode_device.cuh, decode_kernels_typed.cuh, layer_device.cuh, group_topk_kernels_typed.cuh, prefill_kernel_typed.cuh).
A narrowed cast does not crash: it reads or writes somebody else's page.  These tests hold the casts in place.

The pool (tests/_high_pages.py): 2 layers, every launch on layer 1, each layer a little over 8 GiB (the batched cases:
9 GiB), filled with 0x7fff -- a NaN in both element types -- before the first append.  LINE A is element offset 2^31 of a
layer (byte 2^32), LINE B element offset 2^32 (8 GiB); pages are ``low`` / ``mid`` / ``high`` by where they start.  Layer
0 is the guard: a sign-extended negative offset lands there, not outside the allocation.  The metadata pool keeps its
ordinary size.

Placement is chosen by the test and asserted from ``kv_cache.indicies``: a single sequence gets its pages from a ``KvPool``
whose LIFO free list was driven with ``alloc_block`` / ``free_block`` into a crafted order that interleaves the three
bands, includes the pages just below and above both lines and the pool's last page, and puts the page of the decode
append and the page a step opens next above B in one case and into ``mid`` in another; the sequences of an unshuffled
``BatchedInferenceController`` own consecutive ranges of 4096 pages, which start in ``mid`` from sequence 16 and in
``high`` from sequence 32 (Hkv 8 / head_dim 128, Hkv 4 / head_dim 256 or Hkv 16 / head_dim 64: pages of 64 KiB).  Geometries with 3 or 6 kv
heads or pages of 7 tokens put both lines INSIDE a page; those pages are in the table and attended.

Each case checks: (1) pools, scores, selections and outputs against the oracle restated on the sequence's pages gathered
on the device into a compact pool with the table renumbered (pool bits and selections exact, o and lse within 2e-3 for
fp16, 2e-3 + 2^-8 |x| for bf16); (2) every output bit and the compact pools against a LOW TWIN -- same data, shapes and
plan in an ordinary small pool: addresses are the only difference, so any differing bit is an address bug; (3) a scan of
both layers of the big pool on the device: only owned pages hold anything but the pattern, the stale slots of owned pages
still hold it, layer 0 holds it throughout; (4) once per single-sequence geometry the detector itself:
``quest_decode_forward`` over the selection with every mid / high page id replaced by the page a wrapped offset would
reach (``p mod pA``, or ``p - pB``: asserted to be pages the sequence does not own and that hold the pattern -- but for
the edge page just below B, which wraps onto the edge page just below A, another page's live data) must NOT give the
expected output.  Where a line falls inside a page (3 or 6 kv heads) the detector is approximate: a wrapped
element offset is not page-aligned there, so the alias page stands for the two pattern-filled pages it would touch.

Out of scope: a metadata pool beyond 4 GiB.  It is 1/16 of the KV pool and would need 64 GiB of KV per layer; the metadata
pool's address sites stay pinned by review only.  Larger KV pools than these are not measured either.

The module skips only on a device with less than 64 GiB; a failed allocation is reported."""
import time

import numpy as np
import pytest
import torch

import oracle
from oracle import synth, torch_ref
import _bf16
import _high_pages as HP
from _group_selection import expand, group_topk

pytestmark = pytest.mark.gpu
DEV = HP.DEV
S16 = 16
PEAK_GIB = 24    # the module's peak device memory stays under this


@pytest.fixture(scope="module", autouse=True)
def _module():
    total = torch.cuda.get_device_properties(0).total_memory
    if total < 64 << 30:
        pytest.skip(f"the device has {total >> 30} GiB: pools beyond 8 GiB per layer need a 64 GiB part")
    HP.release()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    for line in HP.summary_lines():
        HP.record("summary", line)
    allocated, reserved = torch.cuda.max_memory_allocated() / 2 ** 30, torch.cuda.max_memory_reserved() / 2 ** 30
    HP.record("summary", f"module wall time {time.time() - t0:.1f} s, peak device memory {allocated:.2f} GiB allocated, "
                         f"{reserved:.2f} GiB reserved (ceiling {PEAK_GIB} GiB)")
    assert reserved < PEAK_GIB, f"the module's peak device memory {reserved:.2f} GiB is not under {PEAK_GIB} GiB"


def _id(row):
    flat = [y for x in row for y in (x if isinstance(x, tuple) else (x,))]
    return "-".join(str(x) for x in flat)


def _controller(geo, cap_pages, budget, **kw):
    import quest_amd.utils as qu

    return qu.InferenceController(2, geo.Hq, geo.D, geo.S, budget, cap_pages * geo.S, geo.dtype, torch.device(DEV),
                                  num_kv_heads=geo.Hkv, layout=geo.layout, **kw)


def _fill(ctl, kd, vd, chunks, start=0):
    """Append device k / v rows ``start ..`` to layer 1 in pieces: > 1 token the prefill append, 1 token the decode append.
    Every piece but the last is closed with ``end_forward``."""
    import quest_amd.utils as qu

    t = start
    chunks = [n for n in chunks if n > 0]
    for i, n in enumerate(chunks):
        ctl.prepare_metadata(n)
        ctl.begin_forward(n)
        qu.append_kv(kd[t:t + n], vd[t:t + n], ctl, 1)
        t += n
        if i != len(chunks) - 1:
            ctl.end_forward()
    return t


def _prefix_chunks(n, S):
    """A chunked prefill of n tokens whose first chunk ends inside a page, so that the second one crosses pages and reads
    the existing metadata entry."""
    return [S + 3, n - S - 3] if n >= S + 5 else [n]


class _Result:
    pass


def _high_and_twin(geo, cap_pages, budget, body, tail_at=(), tail="high", what="", **kw):
    """``body(ctl) -> (L, outputs)`` on a sequence whose pages the crafted free list hands out, then on its low twin.
    ``outputs``: name -> numpy array; names starting with ``sel_i`` hold physical page ids and are compared as logical pages.
    Checks placement, the scan of both pools and twin equality; returns the high run for the oracle's checks."""
    runs = {}
    for which in ("high", "twin"):
        if which == "high":
            pool = HP.big_pool(geo)
            order = HP.crafted_order(geo, cap_pages, tail_at, tail, seed=cap_pages)
            HP.drive_free_list(pool, order)
            ctl = _controller(geo, cap_pages, budget, kv_pool=pool, **kw)
        else:
            ctl = _controller(geo, cap_pages, budget, shuffle_seed=3, **kw)
            pool = ctl.kv_cache.pool
            HP.poison(pool)
        HP.poison(ctl.metadata_cache.pool)
        L, out = body(ctl)
        torch.cuda.synchronize()
        r = _Result()
        r.L, r.table = L, list(ctl.kv_cache.indicies)
        assert ctl.kv_cache.seqlen == L and len(r.table) == -(-L // geo.S)
        if which == "high":
            assert r.table == order[:len(r.table)], "the pool did not hand out the crafted order"
            r.counts = HP.assert_placement(geo, r.table, [j for j in tail_at if j < len(r.table)], tail)
        HP.assert_only_owned_written(pool, r.table, f"{what} {which}: KV pool")
        HP.assert_only_owned_written(ctl.metadata_cache.pool, ctl.metadata_cache.indicies, f"{what} {which}: metadata pool")
        r.out = {n: (HP.logical(a, r.table) if n.startswith("sel_i") else a) for n, a in out.items()}
        assert all((a >= 0).all() for n, a in r.out.items() if n.startswith("sel_i")), "a selected page is not the sequence's"
        r.out["kv_pool"], r.out["meta_pool"] = HP.compact(ctl.kv_cache), HP.compact(ctl.metadata_cache)
        if ctl.step_state is not None:
            ctl.invalidate_device_state()
        runs[which] = r
        del ctl, pool
        HP.release()
    HP.assert_twin_equal(runs["high"].out, runs["twin"].out, what)
    return runs["high"]


def _selected_bands(geo, table, logical_idx, what, family):
    """The selected pages (all heads) include at least 2 in each band."""
    pages = {table[j] for j in np.unique(logical_idx)}
    counts = HP.band_counts(geo, pages)
    assert all(counts[b] >= 2 for b in HP.BANDS), (what, counts)
    return counts


def _check_sequence(geo, r, q, k, v, L, family, what, est=None, sel=(), sparse=(), dense=(), group_sel=(), k_sel=None,
                    pools=True, table=None):
    """Outputs of a run over ``L`` tokens against the oracle on the compact pool (logical page numbers)."""
    out = r.out
    kv_o, meta_o = HP.oracle_compact(geo, k, v, L)
    if pools:
        HP.assert_compact_is_oracle(geo, out["kv_pool"], out["meta_pool"], kv_o, meta_o, L)
    if est is None:
        return {}
    table = r.table if table is None else table
    n = -(-L // geo.S)
    lpl = (L - 1) % geo.S + 1
    logical_table = np.arange(n, dtype=np.int32)
    e0 = out[est[0]]
    for name in est:
        HP.check_scores(out[name], q, meta_o, geo.bf16)
        assert np.array_equal(out[name], e0), name   # every estimate launch: the same bits
    o_err = lse_err = 0.0
    counts = {}
    if sel:
        ev, ei = oracle.topk(e0.view(np.float16), np.tile(logical_table[:-1], (geo.Hq, 1)), k_sel)
        counts = _selected_bands(geo, table, ei, what, family)
        eo, el = oracle.sparse_attn(q, kv_o, ei, k_sel, n - 1, lpl)
        for name in sel:
            assert np.array_equal(out["sel_i_" + name], ei), f"{name}: selected pages"
            assert np.array_equal(out["sel_v_" + name], ev.view(np.uint16)), f"{name}: selected values"
        for name in sparse:
            o_err = max(o_err, HP.close(out["o_" + name], eo, geo.bf16, f"{what} {name}"))
            lse_err = max(lse_err, HP.close_lse(out["lse_" + name], el, f"{what} {name}"))
    for name in group_sel:
        group = geo.Hq // geo.Hkv
        gv, gi = group_topk(e0.view(np.float16), logical_table, group, k_sel)
        assert np.array_equal(out["sel_i_" + name], gi) and np.array_equal(out["sel_v_" + name], gv.view(np.uint16)), name
        _selected_bands(geo, table, gi, what + " " + name, family)
        eo, el = oracle.sparse_attn(q, kv_o, expand(gi, group), k_sel, n - 1, lpl)
        o_err = max(o_err, HP.close(out["o_" + name], eo, geo.bf16, f"{what} {name}"))
        lse_err = max(lse_err, HP.close_lse(out["lse_" + name], el, f"{what} {name}"))
    if dense:
        full = np.tile(logical_table[:-1], (geo.Hq, 1))
        eo, el = oracle.sparse_attn(q, kv_o, full, n - 1, n - 1, lpl)
        for name in dense:
            o_err = max(o_err, HP.close(out["o_" + name], eo, geo.bf16, f"{what} {name}"))
            lse_err = max(lse_err, HP.close_lse(out["lse_" + name], el, f"{what} {name}"))
    HP.note_errors(family, o_err, lse_err)
    return {"selected": counts, "o_err": o_err, "lse_err": lse_err}


def _ppc(split, budget):
    """Pages per workgroup that cut ``budget`` pages into one workgroup per head / into several."""
    return budget if split == "one" else max(2, budget // 4)


# ------------------------------------------------------------------------------------------------ 1. append
# (bf16, layout, Hq, Hkv, head_dim, page), pages, band of the page that receives the decode appends and of the one they open
APPEND = [((False, 2, 8, 8, 128, 16), 40, "high"), ((True, 1, 12, 6, 64, 16), 47, "mid"), ((True, 0, 4, 4, 256, 7), 55, "high"),
          ((False, 1, 4, 2, 256, 16), 41, "mid"), ((False, 0, 8, 8, 64, 5), 64, "high"), ((True, 2, 6, 3, 128, 32), 40, "mid")]


@pytest.mark.parametrize("row", APPEND, ids=_id)
def test_append(row):
    """Prefill append in chunks that cross pages, a decode token that fills its page and a decode token that opens one."""
    geo, pages, tail = HP.Geo(*row[0]), row[1], row[2]
    S = geo.S
    L = (pages - 1) * S + 1          # the last decode token opens page `pages - 1`; the one before fills page `pages - 2`
    _, k, v = _bf16.inputs(7 + geo.D + S + pages, L, geo.Hq, geo.Hkv, geo.D)

    def body(c):
        assert _fill(c, HP.dev(k, geo.bf16), HP.dev(v, geo.bf16), [S + 3, L - 2 - (S + 3), 1, 1]) == L
        c.end_forward()
        return L, {}

    r = _high_and_twin(geo, pages + 2, 9, body, (pages - 2, pages - 1), tail, f"append {geo.name()}")
    _check_sequence(geo, r, None, k, v, L, "append", geo.name())
    HP.record("append", f"{geo.name()} pages {pages} tail {tail}: bands {r.counts}, pools exact, twin exact, scan clean")


# ------------------------------------------------------------------------------------------------ 2. eager chain
# (bf16, layout, Hq, Hkv, head_dim), pages, last_page_len, work split, budget, band of the decode append's page
EAGER = [((False, 0, 8, 8, 128), 43, 5, "one", 9, "high"), ((True, 1, 6, 3, 128), 61, 16, "several", 17, "mid"),
         ((False, 2, 16, 4, 64), 100, 1, "several", 33, "high"), ((True, 2, 32, 4, 64), 40, 9, "one", 9, "mid"),
         ((False, 1, 4, 2, 256), 52, 3, "several", 12, "high"), ((True, 0, 8, 8, 64), 300, 15, "several", 33, "mid"),
         ((True, 1, 16, 2, 128), 46, 8, "one", 12, "high")]
assert {(r[0][3] and r[0][2] // r[0][3], r[0][4]) for r in EAGER} >= {(1, 128), (2, 128), (4, 64), (8, 64), (1, 64), (8, 128)}


@pytest.mark.parametrize("row", EAGER, ids=_id)
def test_eager_chain_of_one_sequence(row):
    """decode append | decode_estimate | decode_topk | decode_sparse_attn on the index rows | append + estimate and top-k +
    attention as single launches | forward_group_topk (head_dim 64 / 128) | attention over every page (the group-shared
    launch where it serves the shape) | the detector: the index-row launch over wrapped page ids."""
    import quest_amd.utils as qu

    geo = HP.Geo(*row[0], S16)
    pages, lpl, split, budget, tail = row[1:]
    S, Hq, Hkv, D = S16, geo.Hq, geo.Hkv, geo.D
    L = (pages - 1) * S + lpl
    n_out, k_sel = pages - 1, budget - 1
    ppc = _ppc(split, budget)
    q, k, v = _bf16.inputs(11 + D + lpl + pages, L, Hq, Hkv, D)
    grouped = D in (64, 128)
    detector = {}

    def body(c):
        qd, kd, vd = HP.dev(q, geo.bf16), HP.dev(k, geo.bf16), HP.dev(v, geo.bf16)
        _fill(c, kd, vd, _prefix_chunks(L - 1, S))
        c.end_forward()
        h = c._decode_handler
        h.set_pages_per_chunk(ppc)
        c.prepare_metadata(1)
        c.begin_forward(1)
        assert c.need_estimate()
        out = {"plan": np.array(h.plan_info())}
        assert (out["plan"][1] == 1) == (split == "one"), out["plan"]
        lse = HP.Lse(h, Hq)

        def taken(name, o):
            out["sel_v_" + name], out["sel_i_" + name] = _bf16.bits(c.topk_dout_buffer), c.topk_dindices_buffer.cpu().numpy()
            out["o_" + name], out["lse_" + name] = _bf16.bits(o), lse.take()

        qu.append_kv(kd[L - 1:L], vd[L - 1:L], c, 1)
        est = qu.decode_estimate(qd, c, 1)
        out["est_eager"] = _bf16.bits(est)
        qu.decode_topk(est, c)
        o = qu.decode_sparse_attn(qd, c, 1, c.topk_dindices_buffer)
        info = h.last_launch_info()
        assert info["keys_per_thread"] == 0 and info["n_seqs"] == 1, info
        taken("index", o)
        # the detector: the same launch over the pages a wrapped offset would reach
        table = list(c.kv_cache.indicies)
        if geo.band(max(table)) == "high":
            idx = c.topk_dindices_buffer.cpu().numpy()
            alias = np.vectorize(lambda p: p - geo.pB if p >= geo.pB else p % geo.pA, otypes=[np.int32])(idx)
            changed = sorted(set(alias[alias != idx].tolist()))
            # (the required edge page pB - 1 wraps onto the required edge page pA - 1 where pB = 2 pA: the one owned alias)
            assert changed and set(changed) & set(table) <= {geo.pA - 1}, "an alias is one of the sequence's own pages"
            changed = [p for p in changed if p != geo.pA - 1]
            held = c.kv_layer(1)[torch.tensor(changed, device=DEV)].view(torch.int16)
            assert bool((held == HP.PATTERN).all()), "an alias page does not hold the pattern"
            o2 = qu.decode_sparse_attn(qd, c, 1, torch.from_numpy(alias).to(DEV))
            lse.drop()
            detector["differs"] = not np.array_equal(_bf16.bits(o2), out["o_index"])
            detector["rows"] = int((alias != idx).any(axis=1).sum())
        # append + estimate in one launch, top-k + attention in one launch
        c.topk_dindices_buffer.fill_(-7)
        est2 = qu.decode_append_estimate(qd, kd[L - 1:L], vd[L - 1:L], c, 1)
        out["est_fused"] = _bf16.bits(est2)
        o = qu.decode_topk_sparse_attn(qd, est2, c, 1, write_topk=True)
        info = h.last_launch_info()
        assert info["keys_per_thread"] > 0 and (info["workgroups_per_head"] == 1) == (split == "one"), info
        taken("fused", o)
        if grouped:   # one selection per kv head, attended by the heads of its group
            sel_v = torch.zeros((1, Hkv, k_sel), dtype=geo.dtype, device=DEV)
            sel_i = torch.full((1, Hkv, k_sel), -7, dtype=torch.int32, device=DEV)
            h.set_selection_out(sel_v, sel_i)
            o = torch.empty_like(qd)
            ok = h.forward_group_topk(qd, o, c.kv_layer(1), c.kv_indices_with_last, est2, None, n_out,
                                      paged_kv_last_page_len=c.kv_cache.last_page_len, paged_kv_last_page_idx=c.kv_last_page_idx)
            h.set_selection_out(None, None)
            assert ok and h.last_launch_info()["front_end_variant"] == 9, h.last_launch_info()
            out["sel_v_group"], out["sel_i_group"] = _bf16.bits(sel_v[0]), sel_i[0].cpu().numpy()
            out["o_group"], out["lse_group"] = _bf16.bits(o), lse.take()
        # every page
        c.end_forward()
        c.set_page_budget(pages)
        c.begin_forward(1)
        o = torch.empty_like(qd)
        shared = h.forward_shared(qd, o, c.kv_layer(1), c.kv_indices_with_last[:pages - 1], c.kv_cache.last_page_len,
                                  c.kv_last_page_idx)
        assert shared == grouped
        if not shared:
            o = qu.decode_sparse_attn(qd, c, 1, c.kv_indices_without_last)
        out["o_dense"], out["lse_dense"] = _bf16.bits(o), lse.take()
        c.end_forward()
        lse.off()
        return L, out

    what = f"{geo.name()} pages {pages} lpl {lpl} budget {budget} split {split}"
    r = _high_and_twin(geo, pages + 2, budget, body, (pages - 1,), tail, f"eager {what}")
    assert detector["differs"] and detector["rows"] > 0, f"a wrapped read would go unnoticed: {detector}"
    res = _check_sequence(geo, r, q, k, v, L, "eager chain", what, est=("est_eager", "est_fused"), sel=("index", "fused"),
                          sparse=("index", "fused"), dense=("dense",), group_sel=("group",) if grouped else (), k_sel=k_sel)
    HP.record("eager chain", f"{what} tail {tail} plan {r.out['plan'].tolist()}: bands {r.counts}, selected {res['selected']}, "
                             f"|o - oracle| {res['o_err']:.3e}, |lse - oracle| {res['lse_err']:.3e}, detector rows {detector['rows']}")


# ------------------------------------------------------------------------------------------------ 3. state-driven layers
# (bf16, layout, Hq, Hkv, head_dim), pages, last_page_len, work split, budget, band of the append's page and the next one.
# last_page_len 16: the armed advance opens a new page, which the second step's folded append then writes.  The first two
# rows (fp16 MHA, head_dim 128) read their scores from sign planes, whose append role writes the KV pool.
STATE = [((False, 0, 8, 8, 128), 43, 16, "one", 9, "high"), ((False, 2, 8, 8, 128), 58, 16, "several", 17, "mid"),
         ((True, 1, 6, 3, 128), 40, 7, "several", 9, "high"), ((True, 2, 16, 4, 64), 70, 16, "one", 33, "high"),
         ((False, 1, 4, 2, 256), 45, 16, "several", 12, "mid"), ((True, 0, 8, 8, 64), 64, 2, "one", 9, "high")]


@pytest.mark.parametrize("row", STATE, ids=_id)
def test_state_driven_layers_of_one_sequence(row):
    """decode_layer_dyn (whole rows and tiles) and decode_layer_dense_dyn with and without the folded append on the token
    the device-side step reserved; the last layer carries the armed advance, and a second step runs on the token it
    reserved -- on a page the advance opened above B (or in mid) where the first token filled its page."""
    import quest_amd.utils as qu

    geo = HP.Geo(*row[0], S16)
    pages, lpl, split, budget, tail = row[1:]
    S, Hq, Hkv, D = S16, geo.Hq, geo.Hkv, geo.D
    L = (pages - 1) * S + lpl          # the first step's token; the second step's is L + 1
    k_sel = budget - 1
    ppc = _ppc(split, budget)
    q, k, v = _bf16.inputs(13 + D + lpl + pages, L + 1, Hq, Hkv, D)
    q2 = _bf16.mask3(synth.normal_f16(17 + D + pages, (1, Hq, D)))
    planes = not geo.bf16 and Hq == Hkv and D == 128
    dense_advance = row[0][1] == 1      # which layer carries the armed advance

    def body(c):
        qd, q2d, kd, vd = HP.dev(q, geo.bf16), HP.dev(q2, geo.bf16), HP.dev(k, geo.bf16), HP.dev(v, geo.bf16)
        _fill(c, kd, vd, _prefix_chunks(L - 1, S))
        c.end_forward()
        c.enable_device_state()
        h = c._decode_handler
        h.set_pages_per_chunk(ppc)
        c.begin_graph_decode(dense_layers=True)
        assert c._planes_registered == planes
        out = {"plan": np.array(h.plan_info())}
        assert (out["plan"][1] == 1) == (split == "one"), out["plan"]
        lse = HP.Lse(h, Hq)
        qu.step_advance_dyn(c)
        scores = qu.score_scratch(c)

        def sparse(name, qx, t, tiles, advance=False):
            n_out = -(-t // S) - 1
            scores.view(torch.int16).fill_(-1)
            sel_v = torch.zeros((1, Hq, k_sel), dtype=geo.dtype, device=DEV)
            sel_i = torch.full((1, Hq, k_sel), -7, dtype=torch.int32, device=DEV)
            h.set_selection_out(sel_v, sel_i)
            o = qu.decode_layer_dyn(qx, kd[t - 1:t], vd[t - 1:t], c, 1, scores, tiles=tiles, advance_after=advance)
            h.set_selection_out(None, None)
            info = h.last_launch_info()
            assert (info["front_end_variant"] == 8) == tiles and (info["workgroups_per_head"] == 1) == (split == "one"), info
            out["est_" + name] = _bf16.bits(scores[:, :n_out])
            out["sel_v_" + name], out["sel_i_" + name] = _bf16.bits(sel_v[0]), sel_i[0].cpu().numpy()
            out["o_" + name], out["lse_" + name] = _bf16.bits(o), lse.take()

        sparse("rows", qd, L, False)
        sparse("tiles", qd, L, True)
        lse.off()
        dh = c._dense_handler
        lse = HP.Lse(dh, Hq)
        for fuse in (True, False):
            o = qu.decode_layer_dense_dyn(qd, kd[L - 1:L], vd[L - 1:L], c, 1, fuse_append=fuse)
            out[f"o_dense_fuse{int(fuse)}"], out[f"lse_dense_fuse{int(fuse)}"] = _bf16.bits(o), lse.take()
        if dense_advance:
            o = qu.decode_layer_dense_dyn(qd, kd[L - 1:L], vd[L - 1:L], c, 1, advance_after=True)
            out["o_dense_armed"], out["lse_dense_armed"] = _bf16.bits(o), lse.take()
        lse.off()
        lse = HP.Lse(h, Hq)
        if not dense_advance:
            sparse("armed", qd, L, False, advance=True)
        c.prepare_metadata(1)
        torch.cuda.synchronize()
        c.prepare_metadata(1)            # host mirror of the armed advance
        st = c.step_state.cpu().tolist()
        kv = c.kv_cache
        assert st[:4] == [L + 1, len(kv.indicies), kv.last_page_len, kv.indicies[-1]], st
        sparse("step2", q2d, L + 1, False)
        lse.off()
        return L + 1, out

    what = f"{geo.name()} pages {pages} lpl {lpl} budget {budget} split {split}"
    tail_at = (pages - 1, pages) if lpl == S else (pages - 1,)
    r = _high_and_twin(geo, pages + 3, budget, body, tail_at, tail, f"state {what}")
    assert len(r.table) == pages + (lpl == S)
    armed = ("o_dense_armed",) if dense_advance else ()
    sp = ("rows", "tiles") + (() if dense_advance else ("armed",))
    table1 = r.table[:pages]
    res = _check_sequence(geo, r, q, k, v, L, "state-driven", what, est=tuple("est_" + n for n in sp), sel=sp, sparse=sp,
                          dense=("dense_fuse1", "dense_fuse0") + tuple(n[2:] for n in armed), k_sel=k_sel, pools=False,
                          table=table1)
    res2 = _check_sequence(geo, r, q2, k, v, L + 1, "state-driven", what + " step 2", est=("est_step2",), sel=("step2",),
                           sparse=("step2",), k_sel=k_sel)
    HP.record("state-driven", f"{what} tail {tail} planes {planes} armed on {'dense' if dense_advance else 'sparse'} layer: "
                              f"bands {r.counts}, selected {res['selected']} / {res2['selected']}, "
                              f"|o - oracle| {max(res['o_err'], res2['o_err']):.3e}, "
                              f"|lse - oracle| {max(res['lse_err'], res2['lse_err']):.3e}")


# ------------------------------------------------------------------------------------------------ 3b. a captured step
# (bf16, layout, Hq, Hkv, head_dim), pages, last_page_len after the prefill, work split, budget, band of the page the
# replayed appends fill and of the page the captured advance opens.  The fp16 MHA rows read their scores from sign planes.
GRAPH = [((False, 0, 8, 8, 128), 40, 13, "one", 9, "high"), ((True, 1, 8, 2, 128), 44, 14, "several", 12, "high"),
         ((False, 2, 8, 8, 128), 41, 13, "several", 9, "mid"), ((True, 2, 16, 4, 64), 47, 12, "one", 17, "mid")]
STEPS = 6


@pytest.mark.parametrize("row", GRAPH, ids=_id)
def test_captured_step_replayed_across_a_page_boundary(row):
    """One step (device-side advance, append + estimate, top-k + attention) captured once and replayed for 6 tokens: the
    first ones fill the last page, the next opens a page the captured advance takes from the table -- above B, or in mid --
    and the rest land there."""
    import quest_amd.utils as qu

    geo = HP.Geo(*row[0], S16)
    pages, lpl0, split, budget, tail = row[1:]
    S, Hq, Hkv, D = S16, geo.Hq, geo.Hkv, geo.D
    L0 = (pages - 1) * S + lpl0
    assert pages * S < L0 + STEPS - 1, "the replays must cross the page boundary and go on behind it"
    k_sel = budget - 1
    ppc = _ppc(split, budget)
    _, k, v = _bf16.inputs(31 + D + lpl0 + pages, L0 + STEPS, Hq, Hkv, D)
    qs = _bf16.mask3(synth.normal_f16(37 + D + pages, (STEPS, 1, Hq, D)))
    planes = not geo.bf16 and Hq == Hkv and D == 128

    def body(c):
        qd, kd, vd = HP.dev(qs, geo.bf16), HP.dev(k, geo.bf16), HP.dev(v, geo.bf16)
        _fill(c, kd, vd, _prefix_chunks(L0, S))
        c.end_forward()
        c.enable_device_state()
        h = c._decode_handler
        h.set_pages_per_chunk(ppc)
        c.begin_graph_decode()
        assert c._planes_registered == planes
        out = {"plan": np.array(h.plan_info())}
        qb, kb, vb = torch.empty_like(qd[0]), torch.empty_like(kd[:1]), torch.empty_like(vd[:1])
        scores = qu.score_scratch(c)
        scores.view(torch.int16).fill_(-1)
        sel_v = torch.zeros((1, Hq, k_sel), dtype=geo.dtype, device=DEV)
        sel_i = torch.full((1, Hq, k_sel), -7, dtype=torch.int32, device=DEV)
        h.set_selection_out(sel_v, sel_i)
        lse = HP.Lse(h, Hq)
        obuf = [None]

        def step():
            qu.step_advance_dyn(c)
            obuf[0] = qu.decode_layer_dyn(qb, kb, vb, c, 1, scores)

        # the warm-up advances the state and writes the first token: the state is set back, the token is written again
        qb.copy_(qd[0]); kb.copy_(kd[L0:L0 + 1]); vb.copy_(vd[L0:L0 + 1])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        c.sync_device_state()
        lse.drop()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        for t in range(STEPS):
            qb.copy_(qd[t]); kb.copy_(kd[L0 + t:L0 + t + 1]); vb.copy_(vd[L0 + t:L0 + t + 1])
            graph.replay()
            c.prepare_metadata(1)       # host mirror of what the graph's first node did on the device
            torch.cuda.synchronize()
            kv = c.kv_cache
            assert c.step_state.cpu().tolist()[:4] == [L0 + t + 1, len(kv.indicies), kv.last_page_len, kv.indicies[-1]]
            out[f"est_{t}"] = _bf16.bits(scores[:, :len(kv.indicies) - 1])
            out[f"sel_v_{t}"], out[f"sel_i_{t}"] = _bf16.bits(sel_v[0]), sel_i[0].cpu().numpy()
            out[f"o_{t}"], out[f"lse_{t}"] = _bf16.bits(obuf[0]), lse.take()
        h.set_selection_out(None, None)
        lse.off()
        return L0 + STEPS, out

    what = f"{geo.name()} pages {pages}+1 lpl {lpl0} budget {budget} split {split}"
    r = _high_and_twin(geo, pages + 3, budget, body, (pages - 1, pages), tail, f"graph {what}")
    assert len(r.table) == pages + 1 and geo.band(r.table[pages]) == tail
    o_err = lse_err = 0.0
    for t in range(STEPS):
        L = L0 + t + 1
        res = _check_sequence(geo, r, qs[t], k, v, L, "captured step", f"{what} token {t}", est=(f"est_{t}",), sel=(str(t),),
                              sparse=(str(t),), k_sel=k_sel, pools=t == STEPS - 1, table=r.table[:-(-L // S)])
        o_err, lse_err = max(o_err, res["o_err"]), max(lse_err, res["lse_err"])
    HP.record("captured step", f"{what} tail {tail} planes {planes} plan {r.out['plan'].tolist()}: {STEPS} replays, page "
                               f"{r.table[pages]} ({tail}) opened by the captured advance, bands {r.counts}, selected (last token) "
                               f"{res['selected']}, |o - oracle| {o_err:.3e}, |lse - oracle| {lse_err:.3e}")


# ------------------------------------------------------------------------------------------------ 4. prefill
# (bf16, layout, Hq, Hkv, head_dim, page), kv pages, last_page_len, query rows (a chunk after a prefix), band of the last page
PREFILL = [((False, 0, 8, 8, 128, 16), 40, 5, 37, "high"), ((True, 1, 4, 4, 64, 16), 50, 16, 100, "mid"),
           ((False, 2, 4, 2, 256, 16), 41, 9, 33, "high"), ((True, 2, 4, 4, 128, 7), 45, 3, 50, "mid"),
           ((False, 1, 8, 8, 64, 7), 60, 7, 29, "high"), ((True, 0, 4, 2, 256, 7), 40, 1, 64, "mid")]


@pytest.mark.parametrize("row", PREFILL, ids=_id)
def test_prefill(row):
    """prefill_with_paged_kv_cache, causal, a chunk of query rows after a prefix: page 16 (the fast walk) and page 7 (the
    generic walk, both lines inside a page)."""
    from quest_amd import _kernels

    geo = HP.Geo(*row[0])
    pages, lpl, nq, tail = row[1:]
    S, Hq, Hkv, D = geo.S, geo.Hq, geo.Hkv, geo.D
    kv_len = (pages - 1) * S + lpl
    _, k, v = _bf16.inputs(19 + kv_len + D, kv_len, Hq, Hkv, D)
    q = _bf16.mask3(synth.normal_f16(23 + kv_len + D, (nq, Hq, D)))

    def body(c):
        _fill(c, HP.dev(k, geo.bf16), HP.dev(v, geo.bf16), _prefix_chunks(kv_len - nq, S) + [nq])
        # every page is attended: causal, the queries are the LAST nq rows, and the launch gets the whole table
        assert 0 < nq <= kv_len and c.kv_indices_with_last.tolist() == c.kv_cache.indicies and len(c.kv_cache.indicies) == pages
        o = _kernels.prefill_with_paged_kv_cache(HP.dev(q, geo.bf16), c.kv_layer(1), c.kv_indices_with_last,
                                                 c.kv_cache.last_page_len, True, c.layout, False, 1.0, 1e4)
        c.end_forward()
        return kv_len, {"o_prefill": _bf16.bits(o)}

    what = f"{geo.name()} kv {kv_len} q {nq}"
    r = _high_and_twin(geo, pages + 2, 9, body, (pages - 1,), tail, f"prefill {what}")
    _check_sequence(geo, r, None, k, v, kv_len, "prefill", what)
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    ref = torch_ref.prefill_attention(f(q), f(k), f(v), True).numpy()
    err = HP.close(r.out["o_prefill"], ref, geo.bf16, f"prefill {what}")
    HP.note_errors("prefill", err, 0.0)
    HP.record("prefill", f"{what} tail {tail}: bands {r.counts}, every page attended, |o - reference| {err:.3e}")


# ------------------------------------------------------------------------------------------------ 5. a batch
# 36 sequences of 4096 pages of 64 KiB over an unshuffled shared pool of 9 GiB per layer: sequence i owns pages
# i * 4096 ..; line A is the start of sequence 16, line B the start of sequence 32.  Checked against the oracle and the
# twin: EVERY sequence that starts at or above line A (16 in mid, 4 in high: each of the four data rows below in both
# bands), one in the middle of low and the last one below A.
N_SEQS, SEQ_PAGES = 36, 4096
CHECKED = (5, 15) + tuple(range(16, N_SEQS))
BATCH_PAGES = (41, 75, 120, 52)             # pages of sequence i before the step: BATCH_PAGES[i % 4]
BATCH_LPL = (16, 3, 9, 1)                   # 16: the step's token opens a page
BATCH_BUDGETS = (33, 9, 17, 12)
# (bf16, layout, Hq, Hkv, head_dim), work split, group selection
BATCH = [((False, 0, 8, 8, 128), "one", False), ((True, 2, 16, 8, 128), "several", False), ((True, 1, 16, 8, 128), "several", True),
         ((False, 1, 4, 4, 256), "several", False), ((False, 2, 8, 8, 128), "several", True),
         ((False, 2, 16, 16, 64), "one", False), ((True, 0, 32, 16, 64), "several", True)]


def _batch_data(geo):
    data = []
    for r in range(4):
        L = (BATCH_PAGES[r] - 1) * S16 + BATCH_LPL[r]
        data.append((L,) + _bf16.inputs(29 + r + geo.D, L + 1, geo.Hq, geo.Hkv, geo.D))
    return data


@pytest.mark.parametrize("row", BATCH, ids=_id)
def test_batched_operators_and_layers(row):
    """append_kv_batched | decode_estimate_batched | decode_topk_batched | decode_sparse_attn_batched with per-sequence
    budgets | decode_layer_batched as two launches and (fp16 MHA) as one | decode_layer_dense_batched with and without the
    folded append; with group selection: the append + estimate launch and the group-selection launch with per-sequence
    budgets.  The twin holds the checked sequences alone."""
    import quest_amd.utils as qu

    geo = HP.Geo(*row[0], S16)
    split, group_selection = row[1:]
    Hq, Hkv, D = geo.Hq, geo.Hkv, geo.D
    assert geo.P * SEQ_PAGES * 16 == HP.LINE_A, "sequence 16 starts at line A, sequence 32 at line B"
    data = _batch_data(geo)
    ppc = _ppc(split, max(BATCH_BUDGETS))
    one_launch = not geo.bf16 and Hq == Hkv and D in (64, 128) and split == "one" and not group_selection
    names = ["rows"] if group_selection else ["eager", "rows"] + (["one"] if one_launch else [])
    def run(which):
        seq_ids = list(range(N_SEQS)) if which == "high" else list(CHECKED)
        n = len(seq_ids)
        b = qu.BatchedInferenceController(n, 2, Hq, D, S16, max(BATCH_BUDGETS), SEQ_PAGES * S16, geo.dtype, torch.device(DEV),
                                          num_kv_heads=Hkv, layout=geo.layout, group_selection=group_selection)
        HP.poison(b.kv_pool)
        HP.poison(b.metadata_pool)
        if which == "high":
            assert b.kv_pool.layer(1).numel() > HP.LINE_B
        dev_data = [tuple(HP.dev(a, geo.bf16) for a in d[1:]) for d in data]
        for c, i in zip(b.seqs, seq_ids):
            L, (_, kd, vd) = data[i % 4][0], dev_data[i % 4]
            _fill(c, kd, vd, _prefix_chunks(L, S16))
            c.end_forward()
        lens = [data[i % 4][0] for i in seq_ids]
        qd = torch.stack([dev_data[i % 4][0][0] for i in seq_ids])
        kd = torch.stack([dev_data[i % 4][1][L] for i, L in zip(seq_ids, lens)])
        vd = torch.stack([dev_data[i % 4][2][L] for i, L in zip(seq_ids, lens)])
        b.set_page_budgets([BATCH_BUDGETS[i % 4] for i in seq_ids])
        b.enable_device_state()
        h = b._decode_handler
        h.set_pages_per_chunk(ppc)
        pick = [seq_ids.index(i) for i in CHECKED]
        out = {}
        k_max = max(BATCH_BUDGETS) - 1

        def take(name, o, lse, sel=None):
            o = _bf16.bits(o)
            sel = (_bf16.bits(sel[0]), sel[1].cpu().numpy()) if sel is not None else None
            for i, j in zip(CHECKED, pick):
                out[f"o_{name}_{i}"], out[f"lse_{name}_{i}"] = o[j:j + 1], lse[j * Hq:(j + 1) * Hq]
                if sel is not None:   # (a row's entries past its own k are not the launch's to write)
                    k_i = min(BATCH_BUDGETS[i % 4] - 1, data[i % 4][0] // S16)
                    out[f"sel_v_{name}_{i}"], out[f"sel_i_{name}_{i}"] = sel[0][j][:, :k_i], sel[1][j][:, :k_i]

        def live(sc, name):
            sc = _bf16.bits(sc)
            for i, j in zip(CHECKED, pick):
                out[f"est_{name}_{i}"] = sc[j, :, :len(b.seqs[j].kv_cache.indicies) - 1]

        if group_selection:
            b.begin_graph_decode()
            qu.step_advance_batched(b)
            lse = HP.Lse(h, n * Hq)
            scores = qu.score_scratch(b)
            scores.view(torch.int16).fill_(-1)
            sel_v = torch.zeros((n, Hkv, k_max), dtype=geo.dtype, device=DEV)
            sel_i = torch.full((n, Hkv, k_max), -7, dtype=torch.int32, device=DEV)
            h.set_selection_out(sel_v, sel_i)
            o = qu.decode_layer_batched(qd, kd, vd, b, 1, scores)
            h.set_selection_out(None, None)
            info = h.last_launch_info()
            assert info["front_end_variant"] == 9 and info["n_seqs"] == n, info
            b.prepare_metadata(1)
            live(scores, "rows")
            take("rows", o, lse.take(), (sel_v, sel_i))
            lse.off()
        else:
            b.prepare_metadata(1)
            b.begin_forward()
            lse = HP.Lse(h, n * Hq)
            qu.append_kv_batched(kd, vd, b, 1)
            sc = qu.score_scratch(b)
            sc.view(torch.int16).fill_(-1)
            est = qu.decode_estimate_batched(qd, b, 1, out=sc)
            live(est, "eager")
            qu.decode_topk_batched(est, b)
            o = qu.decode_sparse_attn_batched(qd, b, 1, b.topk_dindices_buffer)
            info = h.last_launch_info()
            assert info["keys_per_thread"] == 0 and info["n_seqs"] == n, info
            take("eager", o, lse.take(), (b.topk_dout_buffer, b.topk_dindices_buffer))
            for name in names[1:]:
                scores = qu.score_scratch(b)
                scores.view(torch.int16).fill_(-1)
                sel_v = torch.zeros((n, Hq, k_max), dtype=geo.dtype, device=DEV)
                sel_i = torch.full((n, Hq, k_max), -7, dtype=torch.int32, device=DEV)
                h.set_selection_out(sel_v, sel_i)
                o = qu.decode_layer_batched(qd, kd, vd, b, 1, scores, one_launch=name == "one", tiles=False, write_scores=True)
                h.set_selection_out(None, None)
                info = h.last_launch_info()
                assert (info["front_end_variant"] == 7) == (name == "one") and info["n_seqs"] == n, (name, info)
                assert b.last_layer_launches == (1 if name == "one" else 2)
                live(scores, name)
                take(name, o, lse.take(), (sel_v, sel_i))
            lse.off()
            b.begin_graph_decode(dense_layers=True)
            dh = b._dense_handler
            lse = HP.Lse(dh, n * Hq)
            for fuse in (True, False):
                o = qu.decode_layer_dense_batched(qd, kd, vd, b, 1, fuse_append=fuse)
                take(f"dense_fuse{int(fuse)}", o, lse.take())
            lse.off()
        out["plan"] = np.array(h.plan_info())
        torch.cuda.synchronize()
        r = _Result()
        r.tables = {i: list(b.seqs[j].kv_cache.indicies) for i, j in zip(CHECKED, pick)}
        if which == "high":   # the placement the case relies on
            for j, c in enumerate(b.seqs):
                assert c.kv_cache.indicies == list(range(j * SEQ_PAGES, j * SEQ_PAGES + len(c.kv_cache.indicies)))
            for i in CHECKED:   # a sequence's pages all lie in the band its range starts in
                want = "low" if i < 16 else "mid" if i < 32 else "high"
                assert {geo.band(p) for p in r.tables[i]} == {want}, (i, want)
            assert r.tables[16][0] == geo.pA and r.tables[32][0] == geo.pB
            assert r.tables[N_SEQS - 1][0] == (N_SEQS - 1) * SEQ_PAGES and b.kv_pool.capacity == N_SEQS * SEQ_PAGES
            assert {i for i in range(N_SEQS) if geo.band(i * SEQ_PAGES) != "low"} <= set(CHECKED)
            assert all({i % 4 for i in CHECKED if geo.band(i * SEQ_PAGES) == band} == {0, 1, 2, 3} for band in ("mid", "high"))
        HP.assert_only_owned_written(b.kv_pool, [p for c in b.seqs for p in c.kv_cache.indicies], f"batch {which}: KV pool")
        HP.assert_only_owned_written(b.metadata_pool, [p for c in b.seqs for p in c.metadata_cache.indicies],
                                     f"batch {which}: metadata pool")
        r.out = {}
        for name, a in out.items():
            r.out[name] = HP.logical(a, r.tables[int(name.rsplit("_", 1)[1])]) if name.startswith("sel_i") else a
        for i, j in zip(CHECKED, pick):
            r.out[f"kv_pool_{i}"], r.out[f"meta_pool_{i}"] = HP.compact(b.seqs[j].kv_cache), HP.compact(b.seqs[j].metadata_cache)
        return r

    runs = {}
    for which in ("high", "twin"):
        runs[which] = run(which)   # (its pools die with its frame)
        HP.release()
    what = f"{geo.name()} split {split} group_selection {group_selection}"
    HP.assert_twin_equal(runs["high"].out, runs["twin"].out, f"batch {what}")
    r = runs["high"]
    group = Hq // Hkv
    o_err = lse_err = 0.0
    selected = set()
    expected = {}   # per data row: the oracle's pools, selection and outputs, as logical pages (computed once, never changed)
    for res in sorted({i % 4 for i in CHECKED}):
        L, q, k, v = data[res]
        L += 1
        n_pages = -(-L // S16)
        k_sel = min(BATCH_BUDGETS[res] - 1, n_pages - 1)
        kv_o, meta_o = HP.oracle_compact(geo, k, v, L)
        logical_table = np.arange(n_pages, dtype=np.int32)
        expected[res] = (L, q, kv_o, meta_o, n_pages, k_sel, logical_table)
    sparse_ref = {}
    for i in CHECKED:
        L, q, kv_o, meta_o, n_pages, k_sel, logical_table = expected[i % 4]
        HP.assert_compact_is_oracle(geo, r.out[f"kv_pool_{i}"], r.out[f"meta_pool_{i}"], kv_o, meta_o, L)
        e0 = r.out[f"est_{names[0]}_{i}"]
        for name in names:
            HP.check_scores(r.out[f"est_{name}_{i}"], q, meta_o, geo.bf16)
            assert np.array_equal(r.out[f"est_{name}_{i}"], e0), (i, name)
        key = (i % 4, e0.tobytes())   # the oracle's selection over the device's own score bits: the same for equal rows
        if key not in sparse_ref:
            if group_selection:
                ev, ei = group_topk(e0.view(np.float16), logical_table, group, k_sel)
                rows = expand(ei, group)
            else:
                ev, ei = oracle.topk(e0.view(np.float16), np.tile(logical_table[:-1], (Hq, 1)), k_sel)
                rows = ei
            sparse_ref[key] = (ev, ei) + oracle.sparse_attn(q, kv_o, rows, k_sel, n_pages - 1, (L - 1) % S16 + 1)
            if not group_selection:
                full = np.tile(logical_table[:-1], (Hq, 1))
                sparse_ref[key] += oracle.sparse_attn(q, kv_o, full, n_pages - 1, n_pages - 1, (L - 1) % S16 + 1)
        ev, ei, eo, el = sparse_ref[key][:4]
        selected |= {r.tables[i][j] for j in np.unique(ei)}
        for name in names:
            assert np.array_equal(r.out[f"sel_i_{name}_{i}"], ei), (i, name)
            assert np.array_equal(r.out[f"sel_v_{name}_{i}"], ev.view(np.uint16)), (i, name)
            o_err = max(o_err, HP.close(r.out[f"o_{name}_{i}"], eo, geo.bf16, f"batch {what} seq {i} {name}"))
            lse_err = max(lse_err, HP.close_lse(r.out[f"lse_{name}_{i}"], el, f"batch {what} seq {i} {name}"))
        if not group_selection:
            eo, el = sparse_ref[key][4:]
            for name in ("dense_fuse1", "dense_fuse0"):
                o_err = max(o_err, HP.close(r.out[f"o_{name}_{i}"], eo, geo.bf16, f"batch {what} seq {i} {name}"))
                lse_err = max(lse_err, HP.close_lse(r.out[f"lse_{name}_{i}"], el, f"batch {what} seq {i} {name}"))
    counts = HP.band_counts(geo, selected)
    assert all(counts[b] >= 2 for b in HP.BANDS), counts
    HP.note_errors("batch", o_err, lse_err)
    HP.record("batch", f"{what} launches {names} plan {r.out['plan'].tolist()}: {len(CHECKED)} sequences checked "
                       f"(5 and 15 in low, 16-31 in mid, 32-{N_SEQS - 1} in high: every sequence at or above line A); selected pages per band {counts}, |o - oracle| {o_err:.3e}, "
                       f"|lse - oracle| {lse_err:.3e}")
