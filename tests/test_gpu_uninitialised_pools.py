"""Every pool operator on pools whose unwritten bytes are poison.

``KvPool`` allocates with ``torch.empty``: in service the slots of a sequence's last page past ``last_page_len``, the
entries of its last metadata page past ``meta_last_page_len`` and every reserved page hold arbitrary bytes.  The contract
("Unowned pool bytes"): a launch may READ any byte of an allocated page, no unowned byte may influence a result,
and a launch WRITES only the bytes ``_harness.valid_mask`` names.

Each case runs twice with the same inputs, ``shuffle_seed`` and plan -- on a zero-filled pool and on a pool filled with one
16-bit pattern (``_harness.poison_pools``) -- and the two runs must agree BIT FOR BIT on every score, selected page and
value, attention output, LSE and valid pool byte; after the poisoned run every other pool byte still holds the pattern.
No tolerance is involved.  Two patterns per element type, because they catch different mistakes: 0x7fff (a NaN in fp16 and
in bf16) catches a stale row multiplied by a zero weight instead of selected away; +inf (0x7c00 / 0x7f80) catches a stale
row that gets into a running maximum or a page's (max, min) entry, which a NaN cannot (v_max_f32 / fmaxf drop a NaN
operand and the metadata fold suppresses it).  The zero run of every case is also compared with the oracle once, so the
test stays honest about what it runs; ``last_launch_info`` / ``plan_info`` pin the kernel a sub-path names.

Shapes: a load covers R = 512 / head_dim rows (8 / 4 / 2 for head_dim 64 / 128 / 256): ``last_page_len`` in
{1, R, R + 1, 15, 16} at page 16; pages of 5, 7 (no multiple of R: the clamped-row branch of the gather) and 32 for the
generic walk; 5-12 pages (18 where the tiles form needs 17 columns), budget 4 for the sparse launches; (Hq, Hkv) = (4, 2)
and (3, 3); three layouts; fp16 and bf16.  The data are fp16 values that bf16 holds exactly (tests/_bf16.py), so one
fp16 oracle referees both element types."""
import numpy as np
import pytest
import torch

import oracle
from oracle import synth, torch_ref
import _bf16
import _harness as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN16 = 0x7FFF
INF16 = {False: 0x7C00, True: 0x7F80}
MARK_V, MARK_I, GUARD, B = 0x5A5A, -7, 8, 4   # marker of pre-filled output rows; NaN guards around the LSE; page budget
# (element type, pattern, layout) triples dealt over the rows of every table: six consecutive rows meet both element
# types, both patterns and all three layouts; any four consecutive ones both types, both patterns, HND and NHD_ROT
COMBOS = [(False, "nan", 0), (True, "inf", 1), (False, "inf", 2), (True, "nan", 2), (False, "nan", 1), (True, "inf", 0)]


def _deal(rows, shift=0):
    return [pytest.param(r, *COMBOS[(i + shift) % 6], id=f"{'-'.join(str(x) for x in r)}-{'bf16' if COMBOS[(i + shift) % 6][0] else 'fp16'}-"
                         f"{COMBOS[(i + shift) % 6][1]}-layout{COMBOS[(i + shift) % 6][2]}") for i, r in enumerate(rows)]


def _pattern(bf16, kind):
    return NAN16 if kind == "nan" else INF16[bf16]


def _dev(a, bf16):
    return _bf16.dev16(a) if bf16 else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _f32(bits_, bf16):
    return _bf16.bf16_bits_to_f32(bits_) if bf16 else bits_.view(np.float16).astype(np.float32)


def _controller(bf16, cap, Hq, Hkv, D, S, layout, seed):
    import quest_amd.utils as qu

    return qu.InferenceController(1, Hq, D, S, B, cap, torch.bfloat16 if bf16 else torch.float16, torch.device(DEV),
                                  num_kv_heads=Hkv, layout=layout, shuffle_seed=seed)


def _fill(ctl, kd, vd, chunks, start=0):
    """Append device k / v rows ``start ..`` in pieces: > 1 token the prefill append, 1 token the decode append.  Every piece
    but the last is closed with ``end_forward``."""
    import quest_amd.utils as qu

    t = start
    chunks = [n for n in chunks if n > 0]
    for i, n in enumerate(chunks):
        ctl.prepare_metadata(n)
        ctl.begin_forward(n)
        qu.append_kv(kd[t:t + n], vd[t:t + n], ctl, 0)
        t += n
        if i != len(chunks) - 1:
            ctl.end_forward()
    return t


def _prefix_chunks(n, S):
    """A chunked prefill of n tokens whose first chunk ends inside a page, so that the second chunk reads the existing
    metadata entry (one call where n is too short for that)."""
    return [S + 3, n - S - 3] if n >= S + 5 else [n]


def _marked(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16).fill_(MARK_V)
    return t


def _poisoned_scratch(ctl):
    """Score scratch whose every word is 0xffff (as a tile key the largest there is), as in test_gpu_tiles_batched.py."""
    import quest_amd.utils as qu

    sc = qu.score_scratch(ctl)
    sc.view(torch.int16).fill_(-1)
    return sc


class _Lse:
    """A NaN-filled float32 buffer with guards, handed to a handler; ``take`` checks the guards and returns the values."""

    def __init__(self, handler, n):
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        self.n = n
        handler.lse_out = self.buf[GUARD:GUARD + n]

    def take(self):
        a = self.buf.cpu().numpy().copy()
        self.buf.fill_(float("nan"))
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + self.n:]).all(), "LSE guard written"
        assert np.isfinite(a[GUARD:GUARD + self.n]).all(), "LSE not written or not finite"
        return a[GUARD:GUARD + self.n]


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _twice(run, pattern):
    """``run(pattern) -> (controller, lengths, outputs)`` on a zero pool and on a poisoned pool: same bits everywhere the
    contract names; returns the zero run."""
    c0, L0, r0 = run(0)
    c1, L1, r1 = run(pattern)
    assert L0 == L1 and r0.keys() == r1.keys()
    bad = [name for name in r0 if not _same_bytes(r0[name], r1[name])]
    for p0, p1, m, what in zip(H._pools(c0), H._pools(c1), H.valid_mask(c1, L1), ("KV pool", "metadata pool")):
        b0, b1 = H.pool_bits(p0)[0], H.pool_bits(p1)[0]
        if not np.array_equal(b0[m], b1[m]):
            bad.append(f"valid bytes of the {what}")
        if not (b1[m] != pattern).all():
            bad.append(f"owned bytes of the {what} left unwritten")
        if not (b0[~m] == 0).all():
            bad.append(f"unowned bytes of the zero-filled {what} written")
        if not (b1[~m] == pattern).all():
            w = np.argwhere((b1 != pattern) & ~m)
            bad.append(f"{len(w)} unowned elements of the poisoned {what} written, first at {w[0].tolist()}")
    assert H.unowned_bytes_untouched(c1, L1, pattern) or bad
    assert not bad, f"zero pool vs pool of 0x{pattern:04x}: {bad}"
    return c0, r0


# ------------------------------------------------------------------------------------------------ the oracle's side
def _oracle_pools(c, k, v, L):
    kvc, mc = c.kv_cache, c.metadata_cache
    kv = oracle.Paged(np.zeros(tuple(kvc.buf_layer(0).shape), np.float16), np.array(kvc.indicies, np.int32),
                      kvc.last_page_len, c.layout)
    meta = oracle.Paged(np.zeros(tuple(mc.buf_layer(0).shape), np.float16), np.array(mc.indicies, np.int32),
                        mc.last_page_len, c.layout)
    assert kvc.seqlen == L
    oracle.append_prefill(kv, meta, k[:L], v[:L])
    return kv, meta


def _pools_equal_oracle(c, bf16, kv_o, meta_o, L):
    if bf16:
        return all(_bf16.pools_equal_oracle(c, kv_o, meta_o, L).values())
    return H.pools_match(c, kv_o, meta_o, L)


def _close(o_bits, eo_f16, bf16, what, extra=0.0):
    """Attention output against the oracle's: atol 2e-3 as everywhere in the suite, rtol 2e-3 (fp16) / 2^-8 (bf16: half an
    ulp of the output format, tests/test_gpu_bf16_kernels.py); ``extra``: a term the caller derives for its kernel."""
    got, want = _f32(o_bits, bf16).astype(np.float64), eo_f16.astype(np.float64)
    bound = 2e-3 + (2.0 ** -8 if bf16 else 2e-3) * np.abs(want) + extra
    assert (np.abs(got - want) <= bound).all(), (what, float((np.abs(got - want) / bound).max()))


def _check_scores(est_bits, q, meta_o, bf16):
    e = oracle.estimate(q, meta_o)
    if bf16:
        _bf16.check_scores(est_bits, e, max_undecided=1.0)  # (a handful of scores: the share of midpoints is not a statistic here)
    else:
        assert np.array_equal(est_bits, e.view(np.uint16)), "estimate differs from the oracle's"


def _check_sequence(c, bf16, q, k, v, L, est=None, sel=(), sparse=(), dense=(), k_sel=B - 1):
    """Zero run of one sequence against the oracle: pools, scores, selections (oracle top-k over the device's own score
    bits), outputs over the selected pages (``sparse``) and over every page (``dense``)."""
    kv_o, meta_o = _oracle_pools(c, k, v, L)
    assert _pools_equal_oracle(c, bf16, kv_o, meta_o, L), "pools differ from the oracle's"
    if est is None:
        return
    table = np.array(c.kv_cache.indicies, np.int32)
    Hq = q.shape[1]
    for name, e in est.items():
        _check_scores(e, q, meta_o, bf16)
    e0 = next(iter(est.values()))
    for name, e in est.items():
        assert np.array_equal(e, e0), name   # every estimate launch: the same bits
    ev, ei = oracle.topk(e0.view(np.float16), np.tile(table[:-1], (Hq, 1)), k_sel)
    for name, (sv, si) in sel.items():
        assert np.array_equal(si[:, :k_sel], ei) and np.array_equal(sv[:, :k_sel], ev.view(np.uint16)), name
        assert (si[:, k_sel:] == MARK_I).all() and (sv[:, k_sel:] == MARK_V).all(), f"{name}: row written past its k entries"
    eo, _ = oracle.sparse_attn(q, kv_o, ei, k_sel, int(table[-1]), kv_o.last_page_len)
    for name, o in sparse.items():
        _close(o, eo, bf16, name)
    if dense:
        full = np.tile(table[:-1], (Hq, 1))
        eo, _ = oracle.sparse_attn(q, kv_o, full, len(table) - 1, int(table[-1]), kv_o.last_page_len)
        for name, o in dense.items():
            _close(o, eo, bf16, name)


# ------------------------------------------------------------------------------------------------ 1. append
# head_dim, page, Hq, Hkv, pages, mode: "one" = the prompt in one prefill append; "chunked" = a chunk that ends inside a
# page, a chunk that reads that page's metadata entry, a decode token that fills its page, a decode token that opens one
APPEND = [(D, S, Hq, Hkv, pages, mode)
          for (D, S, Hq, Hkv, pages) in ((64, 16, 4, 2, 5), (128, 16, 3, 3, 6), (256, 16, 4, 2, 5), (128, 5, 4, 2, 9),
                                         (128, 7, 3, 3, 8), (64, 32, 4, 2, 5))
          for mode in ("one", "chunked")]


@pytest.mark.parametrize("row,bf16,kind,layout", _deal(APPEND))
def test_append(row, bf16, kind, layout):
    D, S, Hq, Hkv, pages, mode = row
    L = (pages - 1) * S + (1 if mode == "chunked" else S // 2 + 1)
    _, k, v = _bf16.inputs(7 + D + S, L, Hq, Hkv, D)
    chunks = [L] if mode == "one" else [S + 3, L - 2 - (S + 3), 1, 1]

    def run(pattern):
        c = _controller(bf16, L + 3 * S, Hq, Hkv, D, S, layout, seed=L)
        H.poison_pools(c, pattern)
        assert _fill(c, _dev(k, bf16), _dev(v, bf16), chunks) == L
        c.end_forward()
        torch.cuda.synchronize()
        return c, L, {}

    c0, _ = _twice(run, _pattern(bf16, kind))
    _check_sequence(c0, bf16, None, k, v, L)


# ------------------------------------------------------------------------------------------------ 2. one sequence
# head_dim, page, Hq, Hkv, pages, last_page_len, pages per workgroup (4: one workgroup per head; 2: two, and a merge)
R = {64: 8, 128: 4, 256: 2}
SEQ = [(D, 16, Hq, Hkv, pages, lpl, ppc) for D, Hq, Hkv, shapes in (
    (64, 4, 2, ((8, 1, 4), (9, 8, 2), (10, 9, 4), (5, 15, 2), (18, 16, 4))),
    (128, 3, 3, ((9, 1, 2), (8, 4, 4), (18, 5, 2), (12, 15, 4), (10, 16, 2))),
    (256, 4, 2, ((10, 1, 4), (18, 2, 2), (8, 3, 4), (9, 15, 2), (6, 16, 4)))) for pages, lpl, ppc in shapes]
SEQ += [(128, 5, 4, 2, 9, 3, 2), (128, 7, 3, 3, 12, 7, 4), (64, 7, 4, 2, 8, 1, 2), (128, 32, 3, 3, 5, 17, 4), (256, 5, 4, 2, 11, 5, 2)]
assert all(lpl in (1, R[D], R[D] + 1, 15, 16) for D, S, _, _, _, lpl, _ in SEQ if S == 16)
assert {p - 1 for _, S, _, _, p, _, _ in SEQ if S == 16} >= {7, 8, 9, 17}   # the tiles form's n_out: a partly live last run of 8


def _prompt(row, bf16, layout, pattern):
    """Controller of a row over pools filled with ``pattern``, and the row's final length."""
    D, S, Hq, Hkv, pages, lpl, ppc = row
    L = (pages - 1) * S + lpl
    c = _controller(bf16, L + 3 * S, Hq, Hkv, D, S, layout, seed=L + D)
    H.poison_pools(c, pattern)
    return c, L


@pytest.mark.parametrize("row,bf16,kind,layout", _deal(SEQ))
def test_eager_operators_of_one_sequence(row, bf16, kind, layout):
    """append (chunked prefill + a decode token that continues or opens a page) | estimate, eager and fused with the append |
    top-k into marker-filled rows | attention on the index tensor, fused with the top-k under front ends 1, 2, 3 and
    automatic, and over every page (the group-shared launch where it serves the shape)."""
    import quest_amd.utils as qu

    D, S, Hq, Hkv, pages, lpl, ppc = row
    L = (pages - 1) * S + lpl
    q, k, v = _bf16.inputs(11 + D + S + lpl, L, Hq, Hkv, D)
    dt = torch.bfloat16 if bf16 else torch.float16

    def run(pattern):
        c, _ = _prompt(row, bf16, layout, pattern)
        qd, kd, vd = _dev(q, bf16), _dev(k, bf16), _dev(v, bf16)
        _fill(c, kd, vd, _prefix_chunks(L - 1, S))
        c.end_forward()
        h = c._decode_handler
        h.set_pages_per_chunk(ppc)
        c.prepare_metadata(1)
        c.begin_forward(1)
        assert c.need_estimate() and h.plan_info() == (ppc, B // ppc), h.plan_info()
        lse = _Lse(h, Hq)
        out = {}

        def mark_topk():
            c.topk_dout_buffer.view(torch.int16).fill_(MARK_V)
            c.topk_dindices_buffer.fill_(MARK_I)

        def taken(name, o):
            out["sel_v_" + name], out["sel_i_" + name] = _bf16.bits(c.topk_dout_buffer), c.topk_dindices_buffer.cpu().numpy()
            out["o_" + name], out["lse_" + name] = _bf16.bits(o), lse.take()

        # the operators one by one
        qu.append_kv(kd[L - 1:L], vd[L - 1:L], c, 0)
        est = qu.decode_estimate(qd, c, 0)
        out["est_eager"] = _bf16.bits(est)
        mark_topk()
        qu.decode_topk(est, c)
        o = qu.decode_sparse_attn(qd, c, 0, c.topk_dindices_buffer)
        info = h.last_launch_info()
        assert info["keys_per_thread"] == 0 and info["workgroups_per_head"] == B // ppc and info["n_seqs"] == 1, info
        taken("index", o)
        # append + estimate in one launch, top-k + attention in one launch: every front end
        for fe in (1, 2, 3, 0):
            h.set_front_end(fe)
            est2 = qu.decode_append_estimate(qd, kd[L - 1:L], vd[L - 1:L], c, 0)
            out[f"est_fused{fe}"] = _bf16.bits(est2)
            mark_topk()
            o = qu.decode_topk_sparse_attn(qd, est2, c, 0, write_topk=True)
            info = h.last_launch_info()
            assert info["keys_per_thread"] > 0 and info["workgroups_per_head"] == B // ppc, (fe, info)
            assert (info["front_end_variant"] == 2) == (fe in (2, 3)), (fe, info)
            taken(f"fused{fe}", o)
        # every page: the group-shared launch where it serves the shape, else the per-head launch on the repeated table
        c.end_forward()
        c.set_page_budget(pages)
        c.begin_forward(1)
        lse = _Lse(h, Hq)
        o = torch.empty_like(qd)
        shared = h.forward_shared(qd, o, c.kv_cache.buf_layer(0), c.kv_indices_with_last[:pages - 1],
                                  c.kv_cache.last_page_len, c.kv_last_page_idx)
        assert shared == (S == 16 and D in (64, 128))
        if not shared:
            o = qu.decode_sparse_attn(qd, c, 0, c.kv_indices_without_last)
        out["o_dense"], out["lse_dense"] = _bf16.bits(o), lse.take()
        c.end_forward()
        h.lse_out = None
        torch.cuda.synchronize()
        return c, L, out

    c0, r = _twice(run, _pattern(bf16, kind))
    names = ["index"] + [f"fused{fe}" for fe in (1, 2, 3, 0)]
    _check_sequence(c0, bf16, q, k, v, L, est={n: r[n] for n in r if n.startswith("est_")},
                    sel={n: (r["sel_v_" + n], r["sel_i_" + n]) for n in names}, sparse={n: r["o_" + n] for n in names},
                    dense={"dense": r["o_dense"]})


@pytest.mark.parametrize("row,bf16,kind,layout", _deal(SEQ, shift=3))
def test_state_driven_layers_of_one_sequence(row, bf16, kind, layout):
    """decode_layer_dyn whole-row and tiles (score scratch poisoned too; the tile maxima behind a partly live run of 8) and
    decode_layer_dense_dyn with and without the folded append, all on the token the device-side step reserved."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    D, S, Hq, Hkv, pages, lpl, ppc = row
    L = (pages - 1) * S + lpl
    n_out = pages - 1
    q, k, v = _bf16.inputs(13 + D + S + lpl, L, Hq, Hkv, D)
    dt = torch.bfloat16 if bf16 else torch.float16

    def run(pattern):
        c, _ = _prompt(row, bf16, layout, pattern)
        qd, kd, vd = _dev(q, bf16), _dev(k, bf16), _dev(v, bf16)
        _fill(c, kd, vd, _prefix_chunks(L - 1, S))
        c.end_forward()
        c.enable_device_state()
        h = c._decode_handler
        h.set_pages_per_chunk(ppc)
        c.begin_graph_decode(dense_layers=True)
        assert h.plan_info() == (ppc, B // ppc), h.plan_info()
        lse = _Lse(h, Hq)
        out = {}
        qu.step_advance_dyn(c)
        for tiles in (False, True) if S == 16 else (False,):
            name = "tiles" if tiles else "rows"
            scores = _poisoned_scratch(c)
            sel_v, sel_i = _marked((1, Hq, B - 1), dt), torch.full((1, Hq, B - 1), MARK_I, dtype=torch.int32, device=DEV)
            h.set_selection_out(sel_v, sel_i)
            o = qu.decode_layer_dyn(qd, kd[L - 1:L], vd[L - 1:L], c, 0, scores, tiles=tiles)
            h.set_selection_out(None, None)
            info = h.last_launch_info()
            assert (info["front_end_variant"] == 8) == tiles and info["workgroups_per_head"] == B // ppc, (tiles, info)
            out["est_" + name] = _bf16.bits(scores[:, :n_out])
            out["sel_v_" + name], out["sel_i_" + name] = _bf16.bits(sel_v[0]), sel_i[0].cpu().numpy()
            out["o_" + name], out["lse_" + name] = _bf16.bits(o), lse.take()
            if tiles:
                off = _kernels.tile_max_offset(c.max_pages - 1)
                out["tile_maxima"] = _bf16.bits(scores[:, off:off + (n_out + 7) // 8])
        h.lse_out = None
        dh = c._dense_handler
        lse = _Lse(dh, Hq)
        for fuse in (True, False):
            o = qu.decode_layer_dense_dyn(qd, kd[L - 1:L], vd[L - 1:L], c, 0, fuse_append=fuse)
            out[f"o_dense_fuse{int(fuse)}"], out[f"lse_dense_fuse{int(fuse)}"] = _bf16.bits(o), lse.take()
        dh.lse_out = None
        c.prepare_metadata(1)
        torch.cuda.synchronize()
        st = c.step_state.cpu().tolist()
        assert st[:3] == [L, pages, lpl], st
        return c, L, out

    c0, r = _twice(run, _pattern(bf16, kind))
    names = ["rows", "tiles"] if S == 16 else ["rows"]
    _check_sequence(c0, bf16, q, k, v, L, est={n: r["est_" + n] for n in names},
                    sel={n: (r["sel_v_" + n], r["sel_i_" + n]) for n in names}, sparse={n: r["o_" + n] for n in names},
                    dense={n: r[n] for n in ("o_dense_fuse1", "o_dense_fuse0")})
    if S == 16:  # per run of 8 columns the largest key of the row's live scores; a column past n_out counts as key 0
        keys = np.zeros((Hq, (n_out + 7) // 8 * 8), np.uint32)
        keys[:, :n_out] = oracle.half_key(r["est_tiles"].view(np.float16))
        assert np.array_equal(r["tile_maxima"], keys.reshape(Hq, -1, 8).max(axis=2).astype(np.uint16))


# ------------------------------------------------------------------------------------------------ 3. a batch
# head_dim, page, Hq, Hkv, pages per workgroup.  Three sequences over shared pools, (pages, last_page_len) before the step:
# 9 pages; TWO pages (fewer than its budget: it attends all of them and its top-k row keeps its tail); 6 full pages (the
# step's token opens the 7th).  Budgets 4 / 4 / 3.  Workgroups whose chunk lies past a sequence's live pages have nothing
# but wholly poisoned reserved pages behind their table entries.
BATCH = [(128, 16, 4, 2, 4), (64, 16, 3, 3, 2), (256, 16, 4, 2, 4), (128, 7, 3, 3, 2), (128, 5, 4, 2, 4), (64, 32, 4, 2, 2),
         (128, 16, 3, 3, 4), (64, 16, 4, 2, 4), (128, 16, 4, 2, 2), (64, 16, 3, 3, 4), (256, 16, 3, 3, 2), (128, 16, 3, 3, 2)]
BUDGETS = (4, 4, 3)


@pytest.mark.parametrize("row,bf16,kind,layout", _deal(BATCH, shift=2))
def test_batched_operators_and_layers(row, bf16, kind, layout):
    """append_kv_batched with ragged lengths | decode_estimate_batched into a poisoned scratch | decode_topk_batched into
    marker-filled rows | decode_sparse_attn_batched with a budget per sequence | decode_layer_batched as two launches
    (whole rows, tiles) and as one (fp16, page 16, head_dim 64 / 128, one workgroup per head) | decode_layer_dense_batched
    with and without the folded append -- all on the same step's token (the append is idempotent)."""
    import quest_amd.utils as qu

    D, S, Hq, Hkv, ppc = row
    R_ = R[D] if S == 16 else 2
    lens = (8 * S + R_, S + 1, 6 * S)              # before the step: its token is row R + 1 of the first sequence's page
    n = len(lens)
    data = [_bf16.inputs(17 + D + S + i, L + 1, Hq, Hkv, D) for i, L in enumerate(lens)]
    dt = torch.bfloat16 if bf16 else torch.float16
    one_launch = not bf16 and S == 16 and D in (64, 128) and ppc == B
    k_i = [min(BUDGETS[i] - 1, -(-(L + 1) // S) - 1) for i, L in enumerate(lens)]
    assert k_i == [3, 1, 2]

    def run(pattern):
        b = qu.BatchedInferenceController(n, 1, Hq, D, S, B, max(lens) + 3 * S, dt, torch.device(DEV), num_kv_heads=Hkv,
                                          layout=layout, shuffle_seed=5 + D)
        b.tiles_min_pages = 1   # score_scratch leaves room for the tile maxima
        H.poison_pools(b, pattern)
        for i, L in enumerate(lens):
            _fill(b.seqs[i], _dev(data[i][1], bf16), _dev(data[i][2], bf16), _prefix_chunks(L, S))
            b.seqs[i].end_forward()
        qd = torch.cat([_dev(d[0], bf16) for d in data])
        kd = torch.cat([_dev(d[1][L:L + 1], bf16) for d, L in zip(data, lens)])
        vd = torch.cat([_dev(d[2][L:L + 1], bf16) for d, L in zip(data, lens)])
        b.set_page_budgets(BUDGETS)
        b.enable_device_state()
        h = b._decode_handler
        h.set_pages_per_chunk(ppc)
        b.prepare_metadata(1)
        b.begin_forward()
        assert h.plan_info() == (ppc, B // ppc), h.plan_info()
        lse = _Lse(h, n * Hq)
        out = {}
        live = lambda sc: np.concatenate([_bf16.bits(sc[i, :, :len(c.kv_cache.indicies) - 1]).ravel() for i, c in enumerate(b.seqs)])
        # the four operators one by one
        qu.append_kv_batched(kd, vd, b, 0)
        est = qu.decode_estimate_batched(qd, b, 0, out=_poisoned_scratch(b))
        out["est_eager"] = live(est)
        b.topk_dout_buffer.view(torch.int16).fill_(MARK_V)
        b.topk_dindices_buffer.fill_(MARK_I)
        qu.decode_topk_batched(est, b)
        out["sel_v_eager"], out["sel_i_eager"] = _bf16.bits(b.topk_dout_buffer), b.topk_dindices_buffer.cpu().numpy()
        o = qu.decode_sparse_attn_batched(qd, b, 0, b.topk_dindices_buffer)
        info = h.last_launch_info()
        assert info["keys_per_thread"] == 0 and info["workgroups_per_head"] == B // ppc and info["n_seqs"] == n, info
        out["o_eager"], out["lse_eager"] = _bf16.bits(o), lse.take()
        # the layer as two launches (whole rows, tiles) and as one
        for name in ("rows", "tiles", "one"):
            if (name == "tiles" and S != 16) or (name == "one" and not one_launch):
                continue
            scores = _poisoned_scratch(b)
            sel_v, sel_i = _marked((n, Hq, B - 1), dt), torch.full((n, Hq, B - 1), MARK_I, dtype=torch.int32, device=DEV)
            h.set_selection_out(sel_v, sel_i)
            o = qu.decode_layer_batched(qd, kd, vd, b, 0, scores, one_launch=name == "one", tiles=name == "tiles",
                                        write_scores=True)
            h.set_selection_out(None, None)
            info = h.last_launch_info()
            assert info["front_end_variant"] == {"tiles": 8, "one": 7}.get(name, info["front_end_variant"]), (name, info)
            assert (info["front_end_variant"] in (7, 8)) == (name != "rows") and info["n_seqs"] == n, (name, info)
            assert b.last_layer_launches == (1 if name == "one" else 2) and info["workgroups_per_head"] == B // ppc
            out["est_" + name] = live(scores)
            out["sel_v_" + name], out["sel_i_" + name] = _bf16.bits(sel_v), sel_i.cpu().numpy()
            out["o_" + name], out["lse_" + name] = _bf16.bits(o), lse.take()
        h.lse_out = None
        # every page of every sequence
        b.begin_graph_decode(dense_layers=True)
        dh = b._dense_handler
        lse = _Lse(dh, n * Hq)
        for fuse in (True, False):
            o = qu.decode_layer_dense_batched(qd, kd, vd, b, 0, fuse_append=fuse)
            out[f"o_dense_fuse{int(fuse)}"], out[f"lse_dense_fuse{int(fuse)}"] = _bf16.bits(o), lse.take()
        dh.lse_out = None
        b.end_forward()
        torch.cuda.synchronize()
        return b, tuple(L + 1 for L in lens), out

    b0, r = _twice(run, _pattern(bf16, kind))
    names = ["eager", "rows"] + (["tiles"] if S == 16 else []) + (["one"] if one_launch else [])
    off = 0
    for i, L in enumerate(lens):
        c = b0.seqs[i]
        n_out = len(c.kv_cache.indicies) - 1
        cut = lambda a: a[off:off + Hq * n_out].reshape(Hq, n_out)
        _check_sequence(c, bf16, data[i][0], data[i][1], data[i][2], L + 1, est={m: cut(r["est_" + m]) for m in names},
                        sel={m: (r["sel_v_" + m][i], r["sel_i_" + m][i]) for m in names},
                        sparse={m: r["o_" + m][i:i + 1] for m in names},
                        dense={m: r[m][i:i + 1] for m in ("o_dense_fuse1", "o_dense_fuse0")}, k_sel=k_i[i])
        off += Hq * n_out


# ------------------------------------------------------------------------------------------------ 4. prefill
# kv_len, query rows (1 or kv_len), causal; page and head_dim dealt over the rows: the page-16 path reads the stale slots of
# the last page (and re-reads that page for key rows past the end); pages 5 and 7 take the generic walk
PREFILL = [(kv, nq, causal, (16, 5, 7)[i % 3], (128, 64, 256, 128)[i % 4], *((4, 2) if i % 2 else (3, 3)))
           for i, (kv, nq, causal) in enumerate((kv, nq, causal) for kv in (1, 15, 17, 65, 100) for nq in (1, kv)
                                                for causal in (True, False))]
PREFILL += [(100, 100, True, 16, 64, 4, 2), (65, 1, True, 16, 256, 3, 3), (17, 17, False, 16, 128, 4, 2), (15, 15, True, 16, 64, 3, 3)]


@pytest.mark.parametrize("row,bf16,kind,layout", _deal(PREFILL, shift=1))
def test_prefill(row, bf16, kind, layout):
    from quest_amd import _kernels

    kv_len, nq, causal, S, D, Hq, Hkv = row
    q, k, v = _bf16.inputs(19 + kv_len + D, kv_len, Hq, Hkv, D)
    q = _bf16.mask3(synth.normal_f16(23 + kv_len + D, (nq, Hq, D)))

    def run(pattern):
        c = _controller(bf16, kv_len + 3 * S, Hq, Hkv, D, S, layout, seed=kv_len + S)
        H.poison_pools(c, pattern)
        _fill(c, _dev(k, bf16), _dev(v, bf16), _prefix_chunks(kv_len - nq, S) + [nq] if nq < kv_len else [kv_len])
        o = _kernels.prefill_with_paged_kv_cache(_dev(q, bf16), c.kv_cache.buf_layer(0), c.kv_indices_with_last,
                                                 c.kv_cache.last_page_len, causal, c.layout, False, 1.0, 1e4)
        c.end_forward()
        torch.cuda.synchronize()
        return c, kv_len, {"o": _bf16.bits(o)}

    c0, r = _twice(run, _pattern(bf16, kind))
    _check_sequence(c0, bf16, None, k, v, kv_len)
    f = lambda a: torch.from_numpy(a.astype(np.float32))
    ref = torch_ref.prefill_attention(f(q), f(k), f(v), causal).numpy()
    # the prefill hands P to the MFMA in the element type: every weight p_j carries a relative rounding error of half an ulp
    # (2^-9 bf16, 2^-12 fp16), so the output may move by that times sum_j p_j |v_j| -- the same attention over |v|
    p_abs_v = torch_ref.prefill_attention(f(q), f(k), f(np.abs(v)), causal).numpy().astype(np.float64)
    _close(r["o"], ref, bf16, "prefill", extra=2.0 ** (-9 if bf16 else -12) * p_abs_v)
