"""bf16 as the second element type of the attention path: append, estimate, top-k, sparse / shared attention, RoPE and
RMSNorm on bf16 pools, refereed by the frozen fp16 oracle on data every value of which is a bf16 value (tests/_bf16.py).

Bars: pools and metadata bit for bit; scores = the oracle's fp32 sum rounded to bf16 (decided where the oracle's fp16
value is not a bf16 midpoint, a neighbour elsewhere, undecidable share <= 20 %); selections bit for bit on the device's
own score bits; attention within atol 2e-3 (the fp16 bar of test_gpu_fuzz.py, for the fp32 arithmetic) and rtol 2^-8
(bf16 output rounding 2^-9 + the oracle's fp16 rounding 2^-11); batched == single, NHD_ROT == NHD, graph == eager bit for
bit; RoPE / RMSNorm within one bf16 ulp of an fp64 restatement."""
import numpy as np
import pytest
import torch

import oracle
from _bf16 import (BF16_MAX, BF16_NEG_MAX, bf16_bits_to_f32, bits, check_scores, dev16, f16_to_bf16_bits, f32_to_bf16_bits,
                   fill, inputs, make_controller, oracle_pools, pools_equal_oracle, record, to_dev)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ATOL, RTOL = 2e-3, 2.0 ** -8


def _f16view(b):
    """bf16 bit patterns handed to the oracle's top-k as 16-bit patterns (it orders keys of bits, whatever the format)."""
    return np.ascontiguousarray(b, np.uint16).view(np.float16)


def _close(o_dev, eo_f16):
    got = bf16_bits_to_f32(bits(o_dev)).astype(np.float64)
    want = eo_f16.astype(np.float64)
    err = np.abs(got - want)
    bound = ATOL + RTOL * np.abs(want)
    record(f"attention: max abs err {err.max():.3e}, worst err / bound {float((err / bound).max()):.3f} (bound atol 2e-3 + rtol 2^-8)")
    assert (err <= bound).all(), float((err / bound).max())


# ------------------------------------------------------------------------------------------------ 1. append
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("Hq,Hkv,D,page,chunks", [
    (4, 4, 128, 16, [300, 1]),                 # prefill + decode append (the reference harness)
    (8, 2, 64, 16, [37, 120, 1, 1, 1]),        # chunked prefill, then three decode tokens (one opens a page)
    (4, 4, 256, 8, [15, 1, 1, 40, 1]),         # decode tokens between prefill chunks, page boundaries in both
])
def test_append_pools_equal_the_oracles(layout, Hq, Hkv, D, page, chunks):
    L = sum(chunks)
    _, k, v = inputs(11 + layout, L, Hq, Hkv, D)
    ctl = make_controller(L, Hq, Hkv, D, page, 4, layout=layout, shuffle_seed=3)
    fill(ctl, k, v, chunks)
    ctl.end_forward()
    kv_o, meta_o = oracle_pools(ctl, k, v)
    eq = pools_equal_oracle(ctl, kv_o, meta_o, L)
    assert all(eq.values()), eq


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_append_state_driven_single_and_batched(layout):
    """The state-driven appends (``*_dyn`` = the batch of one, ``*_batched``) leave the oracle's pools as well."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    Hq, Hkv, D, page = 8, 4, 128, 16
    lens = (16 * 5 + 16, 16 * 3 + 7, 9)   # the first sequence's next token opens a page
    dev = torch.device("cuda:0")
    data = [inputs(20 + i, L + 2, Hq, Hkv, D) for i, L in enumerate(lens)]
    # single sequence, two state-driven decode appends
    _, k, v = data[0]
    L = lens[0]
    ctl = make_controller(L + 2, Hq, Hkv, D, page, 4, layout=layout, shuffle_seed=5)
    fill(ctl, k[:L], v[:L], [L])
    ctl.end_forward()
    for t in range(L, L + 2):
        ctl.prepare_metadata(1)
        ctl.enable_device_state()
        _kernels.append_kv_cache_decode_batched(dev16(k[t:t + 1]), dev16(v[t:t + 1]), ctl.kv_layer(0), ctl.kv_tables,
                                                ctl.metadata_layer(0), ctl.meta_tables, ctl.step_states, ctl.layout)
    kv_o, meta_o = oracle_pools(ctl, k, v)
    eq = pools_equal_oracle(ctl, kv_o, meta_o, L + 2)
    assert all(eq.values()), eq
    # a batch of three over shared pools
    b = qu.BatchedInferenceController(len(lens), 1, Hq, D, page, 4, max(lens) + 64, BF, dev, num_kv_heads=Hkv, layout=layout,
                                      shuffle_seed=7)
    for i, L in enumerate(lens):
        fill(b.seqs[i], data[i][1][:L], data[i][2][:L], [L])
        b.seqs[i].end_forward()
    b.enable_device_state()
    for t in range(2):
        b.prepare_metadata(1)
        b.begin_forward()
        kk = torch.cat([dev16(data[i][1][L + t:L + t + 1]) for i, L in enumerate(lens)])
        vv = torch.cat([dev16(data[i][2][L + t:L + t + 1]) for i, L in enumerate(lens)])
        qu.append_kv_batched(kk, vv, b, 0)
        b.end_forward()
    for i, L in enumerate(lens):
        kv_o, meta_o = oracle_pools(b.seqs[i], data[i][1], data[i][2])
        eq = pools_equal_oracle(b.seqs[i], kv_o, meta_o, L + 2)
        assert all(eq.values()), (i, eq)


def _rule_max(a, b, nan_above=0x7F80):
    """The metadata rule restated: NaN-suppressing, -0 < +0, order of sign-magnitude patterns (both NaN -> 0x7fff)."""
    an, bn = (a & 0x7FFF) > nan_above, (b & 0x7FFF) > nan_above
    key = lambda x: (~x & 0xFFFF) if x & 0x8000 else (x | 0x8000)
    if an:
        return 0x7FFF if bn else b
    if bn:
        return a
    return a if key(a) >= key(b) else b


def _rule_min(a, b, nan_above=0x7F80):
    an, bn = (a & 0x7FFF) > nan_above, (b & 0x7FFF) > nan_above
    key = lambda x: (~x & 0xFFFF) if x & 0x8000 else (x | 0x8000)
    if an:
        return 0x7FFF if bn else b
    if bn:
        return a
    return a if key(a) <= key(b) else b


@pytest.mark.parametrize("layout", [0, 2])
def test_append_metadata_of_values_fp16_cannot_hold(layout):
    """Keys beyond +-65504 (bf16 only), NaN, -0 and +0: the page entries follow the rule above with bf16's NaN threshold
    (patterns above 0x7f80) and start from -/+ the largest finite bf16, not from -/+65504."""
    from _harness import gather_entries

    H, D, page, L = 4, 64, 4, 4 * 6 + 3
    special = np.array([0x0000, 0x8000, 0x7FC0, 0xFFC1, 0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x4780, 0xC780, 0x5000, 0xD123,
                        0x0001, 0x8001, 0x3F80, 0xBF80, 0x7E00, 0xFE00], np.uint16)  # 0x4780 = 65536, 0x7e00 ~ 2.7e38
    rng = np.random.default_rng(4)
    kb = special[rng.integers(0, len(special), (L, H, D))]
    kb[0:4, 0, 0] = 0x7FC0                      # a page of NaN only: every fold drops the NaN, the entry keeps the finite values it started from
    kb[4:8, 1, 1] = [0x8000, 0x0000, 0x8000, 0x0000]  # -0 < +0
    vb = special[rng.integers(0, len(special), (L, H, D))]
    ctl = make_controller(L, H, H, D, page, 4, layout=layout, shuffle_seed=1)
    kc, vc = to_dev(kb), to_dev(vb)
    for n, t0 in ((10, 0), (1, 10), (1, 11), (1, 12), (L - 13, 13)):
        ctl.prepare_metadata(n)
        ctl.begin_forward(n)
        import quest_amd.utils as qu
        qu.append_kv(kc[t0:t0 + n], vc[t0:t0 + n], ctl, 0)
        ctl.end_forward()
    n_pages = len(ctl.kv_cache.indicies)
    dk, dv = gather_entries(bits(ctl.kv_cache.buf_layer(0)), ctl.kv_cache.indicies, L, ctl.layout)
    assert np.array_equal(dk, kb) and np.array_equal(dv, vb)
    dmx, dmn = gather_entries(bits(ctl.metadata_cache.buf_layer(0)), ctl.metadata_cache.indicies, n_pages, ctl.layout)
    for p in range(n_pages):
        for h in range(H):
            for d in range(D):
                mx, mn = BF16_NEG_MAX, BF16_MAX
                for t in range(p * page, min(L, (p + 1) * page)):
                    mx, mn = _rule_max(mx, int(kb[t, h, d])), _rule_min(mn, int(kb[t, h, d]))
                assert (int(dmx[p, h, d]), int(dmn[p, h, d])) == (mx, mn), (p, h, d, hex(dmx[p, h, d]), hex(mx), hex(dmn[p, h, d]), hex(mn))


# ------------------------------------------------------------------------------------------------ 2. estimate, 3. top-k, 4. attention
CHAIN = [
    # Hq, Hkv, D, page, L, budget (pages)
    (8, 8, 128, 16, 16 * 255 + 9, 12),
    (8, 2, 128, 16, 16 * 130 + 16, 9),
    (8, 4, 64, 16, 16 * 90 + 2, 17),
    (4, 2, 256, 16, 16 * 70 + 5, 6),
    (16, 2, 128, 16, 16 * 64 + 3, 8),   # group of 8
    (6, 3, 128, 8, 8 * 77 + 2, 10),     # the generic page walk
]


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("case", CHAIN, ids=lambda c: "Hq%d_Hkv%d_D%d_S%d_L%d_B%d" % c)
def test_chain_estimate_topk_attention(case, layout):
    import quest_amd.utils as qu
    from quest_amd import _kernels

    Hq, Hkv, D, page, L, B = case
    q, k, v = inputs(31 + Hq + D, L, Hq, Hkv, D)
    ctl = make_controller(L, Hq, Hkv, D, page, B, layout=layout, shuffle_seed=L)
    fill(ctl, k, v, [L - 1, 1])
    kv_o, meta_o = oracle_pools(ctl, k, v)
    eq = pools_equal_oracle(ctl, kv_o, meta_o, L)
    assert all(eq.values()), eq
    assert ctl.need_estimate()
    table = np.array(ctl.kv_cache.indicies, np.int32)
    qd = dev16(q)
    # ---- estimate (plain launch)
    est = qu.decode_estimate(qd, ctl, 0)
    assert est.dtype == BF
    e_est = oracle.estimate(q, meta_o)
    est_b = bits(est)
    check_scores(est_b, e_est)
    # ---- top-k on the device's own score bits: standalone, then fused with the attention
    qu.decode_topk(est, ctl)
    ev, ei = oracle.topk(_f16view(est_b), np.tile(table[:-1], (Hq, 1)), B - 1)
    assert ctl.topk_dout_buffer.dtype == BF
    assert np.array_equal(ctl.topk_dindices_buffer.cpu().numpy(), ei)
    assert np.array_equal(bits(ctl.topk_dout_buffer), ev.view(np.uint16))
    # ---- attention over the oracle's indices (index-list launch)
    o = qu.decode_sparse_attn(qd, ctl, 0, torch.from_numpy(ei).to("cuda:0"))
    eo, _ = oracle.sparse_attn(q, kv_o, ei, B - 1, int(table[-1]), kv_o.last_page_len)
    _close(o, eo)
    ctl.topk_dindices_buffer.zero_()
    o2 = qu.decode_topk_sparse_attn(qd, est, ctl, 0, write_topk=True)
    assert np.array_equal(ctl.topk_dindices_buffer.cpu().numpy(), ei)
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16))
    # ---- full attention over every page: the group-shared launch (page 16, head_dim 64 / 128) or its fallback
    full = np.tile(table[:-1], (Hq, 1))
    o_full = torch.empty_like(qd)
    ctl.end_forward()
    ctl.set_page_budget(len(table))
    ctl.begin_forward(1, updateTensor=True)
    o_full = qu.decode_sparse_attn(qd, ctl, 0, ctl.kv_indices_without_last)
    eo_full, _ = oracle.sparse_attn(q, kv_o, full, len(table) - 1, int(table[-1]), kv_o.last_page_len)
    _close(o_full, eo_full)
    ctl.end_forward()
    ctl.set_page_budget(B)
    # ---- state-driven launches: rewind one token on the device state and decode it again, every front end
    ctl.enable_device_state()
    st = ctl.step_state.cpu().tolist()
    assert st[2] > 1
    st[0] -= 1
    st[2] -= 1
    ctl.begin_graph_decode()
    n_out = len(table) - 1
    for gen in (1, 2, 3, "tiles", 0):
        tiles = gen == "tiles" and page == 16
        scores = (torch.zeros(Hq, ctl.max_pages | 1, dtype=BF, device="cuda:0") if gen == 1 else qu.score_scratch(ctl).zero_())
        assert scores.dtype == BF
        ctl._decode_handler.set_front_end(gen if isinstance(gen, int) else 0)
        ctl.step_state.copy_(torch.tensor(st, dtype=torch.int32))
        sel_i = torch.full((1, Hq, B - 1), -1, dtype=torch.int32, device="cuda:0")
        sel_v = torch.zeros(1, Hq, B - 1, dtype=BF, device="cuda:0")
        ctl._decode_handler.set_selection_out(sel_v, sel_i)
        qu.step_advance_dyn(ctl)
        o3 = qu.decode_layer_dyn(qd, dev16(k[L - 1:L]), dev16(v[L - 1:L]), ctl, 0, scores, tiles=tiles)
        ctl._decode_handler.set_selection_out(None, None)
        info = ctl._decode_handler.last_launch_info()
        assert (info["front_end_variant"] == 8) == tiles, info
        assert np.array_equal(bits(scores[:, :n_out]), est_b)           # the fused append+estimate: the plain launch's bits
        assert np.array_equal(sel_i[0].cpu().numpy(), ei) and np.array_equal(bits(sel_v[0]), ev.view(np.uint16))
        eq = pools_equal_oracle(ctl, kv_o, meta_o, L)
        assert all(eq.values()), eq
        _close(o3, eo)
        if tiles:  # the tile maxima: per run of 8 columns the largest key of the row's scores
            off = _kernels.tile_max_offset(ctl.max_pages - 1)
            keys = oracle.half_key(_f16view(est_b)).astype(np.uint32)
            pad = np.zeros((Hq, (n_out + 7) // 8 * 8), np.uint32)
            pad[:, :n_out] = keys
            want = pad.reshape(Hq, -1, 8).max(axis=2)
            got = bits(scores[:, off:off + want.shape[1]])
            assert np.array_equal(got, want.astype(np.uint16))


def test_topk_ties_nan_and_signed_zero_rows():
    """Crafted rows in bf16 encoding: ties straddling the k-th boundary, NaN of both signs, +-0, +-inf -- the selection is
    the oracle's on the same 16-bit patterns (lowest columns first among equal keys, ascending column order)."""
    from quest_amd import _kernels

    n, k = 200, 16
    rows = np.zeros((5, n), np.uint16)
    rows[0, :] = 0x3F80                        # all equal: the first k columns
    rows[1, :] = 0x3F80
    rows[1, [7, 50, 199]] = 0x4000             # three above a sea of ties
    rows[2, :] = np.where(np.arange(n) % 2 == 0, 0x0000, 0x8000)   # +0 > -0
    rows[3, :] = 0xBF80
    rows[3, [3, 9, 100]] = [0x7FC0, 0xFFC0, 0x7F80]   # +NaN on top, -NaN at the bottom, +inf
    rows[3, [20, 21]] = [0xFF80, 0x7F7F]
    rng = np.random.default_rng(0)
    rows[4, :] = f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32).round(1))  # many exact ties
    idx = np.tile(np.arange(1000, 1000 + n, dtype=np.int32), (5, 1))
    ev, ei = oracle.topk(_f16view(rows), idx, k)
    d_out = torch.zeros(5, k, dtype=BF, device="cuda:0")
    i_out = torch.zeros(5, k, dtype=torch.int32, device="cuda:0")
    _kernels.topk_filtering(to_dev(rows), torch.from_numpy(idx).to("cuda:0"), d_out, i_out, None, k)
    assert np.array_equal(i_out.cpu().numpy(), ei)
    assert np.array_equal(bits(d_out), ev.view(np.uint16))


def _crafted_rows(n):
    """Five score rows in bf16 encoding: all ties; three values above a sea of ties; +0 against -0; NaN of both signs, the
    infinities and the largest finite value among ties; many exact ties of random values."""
    rows = np.zeros((5, n), np.uint16)
    rows[0, :] = 0x3F80
    rows[1, :] = 0x3F80
    rows[1, [7, 50, n - 1]] = 0x4000
    rows[2, :] = np.where(np.arange(n) % 2 == 0, 0x0000, 0x8000)
    rows[3, :] = 0xBF80
    rows[3, [3, 9, 100]] = [0x7FC0, 0xFFC0, 0x7F80]
    rows[3, [20, 21]] = [0xFF80, 0x7F7F]
    rows[4, :] = f32_to_bf16_bits(np.random.default_rng(0).standard_normal(n).astype(np.float32).round(1))
    return rows


@pytest.mark.parametrize("layout", [0, 2])
def test_crafted_rows_through_the_fused_front_ends(layout):
    """The crafted rows of the test above as the score rows of the FUSED launches: the eager top-k + attention launch and the
    state-driven one with every front end (first generation, second generation without / with its pre-filter, tiles with
    the rows' tile maxima, the automatic choice) select what the oracle selects on the same 16-bit patterns."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    Hq, D, page, n, B = 5, 128, 16, 200, 17
    L = n * page + 5                                       # n full pages + the current one
    rows = _crafted_rows(n)
    q, k, v = inputs(61, L, Hq, Hq, D)
    ctl = make_controller(L, Hq, Hq, D, page, B, layout=layout, shuffle_seed=6)
    fill(ctl, k, v, [L - 1, 1])
    table = np.array(ctl.kv_cache.indicies, np.int32)
    assert len(table) == n + 1
    ev, ei = oracle.topk(_f16view(rows), np.tile(table[:-1], (Hq, 1)), B - 1)
    qd = dev16(q)
    # eager fused launch: scores as a [:, :n] view of 16-byte padded rows, like decode_append_estimate's
    sc = torch.zeros(Hq, (n + 7) // 8 * 8, dtype=BF, device="cuda:0")
    sc[:, :n] = to_dev(rows)
    ctl.topk_dindices_buffer.zero_()
    qu.decode_topk_sparse_attn(qd, sc[:, :n], ctl, 0, write_topk=True)
    assert np.array_equal(ctl.topk_dindices_buffer.cpu().numpy(), ei)
    assert np.array_equal(bits(ctl.topk_dout_buffer), ev.view(np.uint16))
    ctl.end_forward()
    # state-driven fused launch on the same rows
    ctl.enable_device_state()
    ctl.begin_graph_decode()
    h = ctl._decode_handler
    max_n = ctl.max_pages - 1
    for gen in (1, 2, 3, "tiles", 0):
        tiles = gen == "tiles"
        scores = (torch.zeros(Hq, ctl.max_pages | 1, dtype=BF, device="cuda:0") if gen == 1 else qu.score_scratch(ctl).zero_())
        scores[:, :n] = to_dev(rows)
        if tiles:  # the rows' tile maxima, as the estimate leaves them: per run of 8 columns the largest key
            pad = np.zeros((Hq, (n + 7) // 8 * 8), np.uint32)
            pad[:, :n] = oracle.half_key(_f16view(rows))
            off = _kernels.tile_max_offset(max_n)
            mx = pad.reshape(Hq, -1, 8).max(axis=2).astype(np.uint16)
            scores[:, off:off + mx.shape[1]] = to_dev(mx)
        h.set_front_end(gen if isinstance(gen, int) else 0)
        sel_i = torch.full((1, Hq, B - 1), -1, dtype=torch.int32, device="cuda:0")
        sel_v = torch.zeros(1, Hq, B - 1, dtype=BF, device="cuda:0")
        h.set_selection_out(sel_v, sel_i)
        o = torch.empty_like(qd)
        assert h.forward_fused_topk_dyn(qd, o, ctl.kv_layer(0), ctl.kv_tables, scores, ctl.step_states, max_n, tiles=tiles)
        h.set_selection_out(None, None)
        info = h.last_launch_info()
        assert (info["front_end_variant"] == 8) == tiles, info
        assert np.array_equal(sel_i[0].cpu().numpy(), ei), gen
        assert np.array_equal(bits(sel_v[0]), ev.view(np.uint16)), gen
    with pytest.raises(RuntimeError, match="dispatch with dtype"):  # fp16 score rows are not this handler's keys
        h.forward_fused_topk_dyn(qd, o, ctl.kv_layer(0), ctl.kv_tables, scores.half(), ctl.step_states, max_n)
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        h.set_selection_out(sel_v.half(), sel_i)


@pytest.mark.parametrize("layout", [0, 2])
@pytest.mark.parametrize("Hq,Hkv,D", [(8, 8, 128), (8, 2, 128)])
def test_batched_launches_against_the_oracle(Hq, Hkv, D, layout):
    """One batched step of three sequences of unequal length, refereed directly: every sequence's scores by the estimate
    rule, its selection by the oracle's top-k on the device's score bits, its pools bit for bit, its output within the bar."""
    import quest_amd.utils as qu

    dev = torch.device("cuda:0")
    lens, B, page = (16 * 40 + 9, 16 * 21 + 16, 16 * 12 + 2), 7, 16
    data = [inputs(70 + i, L, Hq, Hkv, D) for i, L in enumerate(lens)]
    b = qu.BatchedInferenceController(len(lens), 1, Hq, D, page, B, max(lens) + 64, BF, dev, num_kv_heads=Hkv, layout=layout,
                                      shuffle_seed=11)
    for i, L in enumerate(lens):
        fill(b.seqs[i], data[i][1][:L - 1], data[i][2][:L - 1], [L - 1])
        b.seqs[i].end_forward()
    b.enable_device_state()
    b.begin_graph_decode()
    qd = torch.cat([dev16(d_[0]) for d_ in data])
    kd = torch.cat([dev16(d_[1][L - 1:L]) for d_, L in zip(data, lens)])
    vd = torch.cat([dev16(d_[2][L - 1:L]) for d_, L in zip(data, lens)])
    scores = qu.score_scratch(b).zero_()
    sel_i = torch.full((len(lens), Hq, B - 1), -1, dtype=torch.int32, device=dev)
    sel_v = torch.zeros(len(lens), Hq, B - 1, dtype=BF, device=dev)
    b._decode_handler.set_selection_out(sel_v, sel_i)
    qu.step_advance_batched(b)
    o = qu.decode_layer_batched(qd, kd, vd, b, 0, scores, tiles=False)
    b._decode_handler.set_selection_out(None, None)
    b.prepare_metadata(1)
    assert b.last_layer_launches == 2
    for i, L in enumerate(lens):
        c = b.seqs[i]
        kv_o, meta_o = oracle_pools(c, data[i][1], data[i][2])
        eq = pools_equal_oracle(c, kv_o, meta_o, L)
        assert all(eq.values()), (i, eq)
        table = np.array(c.kv_cache.indicies, np.int32)
        n_out = len(table) - 1
        est_b = bits(scores[i, :, :n_out])
        check_scores(est_b, oracle.estimate(data[i][0], meta_o))
        ev, ei = oracle.topk(_f16view(est_b), np.tile(table[:-1], (Hq, 1)), B - 1)
        assert np.array_equal(sel_i[i].cpu().numpy(), ei) and np.array_equal(bits(sel_v[i]), ev.view(np.uint16)), i
        eo, _ = oracle.sparse_attn(data[i][0], kv_o, ei, B - 1, int(table[-1]), kv_o.last_page_len)
        _close(o[i:i + 1], eo)


@pytest.mark.parametrize("Hq,Hkv,D", [(4, 4, 128), (8, 2, 128)])
def test_rotated_layout_equals_nhd(Hq, Hkv, D):
    """NHD_ROT moves vectors, not values: scores, selection and attention output bit for bit those of the NHD pool."""
    import quest_amd.utils as qu

    L, B = 16 * 60 + 7, 9
    q, k, v = inputs(77, L, Hq, Hkv, D)
    out = []
    for layout in (0, 2):
        ctl = make_controller(L, Hq, Hkv, D, 16, B, layout=layout, shuffle_seed=2)
        fill(ctl, k, v, [L - 1, 1])
        est = qu.decode_append_estimate(dev16(q), dev16(k[L - 1:]), dev16(v[L - 1:]), ctl, 0)
        o = qu.decode_topk_sparse_attn(dev16(q), est, ctl, 0)
        out.append((bits(est), ctl.topk_dindices_buffer.cpu().numpy().copy(), bits(o)))
        ctl.end_forward()
    # (physical page ids are the same: same shuffle seed, same allocation order)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("layout", [0, 2])
@pytest.mark.parametrize("Hq,Hkv,D", [(8, 8, 128), (8, 2, 128), (8, 4, 64)])
def test_batched_equals_single_and_graph_equals_eager(Hq, Hkv, D, layout):
    """A batch of three sequences of unequal length, decoded for several tokens across page boundaries: per sequence the
    batched launches leave the single-sequence launches' scores, pools and outputs bit for bit (same work split), and
    the captured step replays the eager step bit for bit."""
    import quest_amd.utils as qu

    dev = torch.device("cuda:0")
    lens, B, steps, page = (16 * 31 + 10, 16 * 20 + 16, 16 * 9 + 1), 7, 20, 16
    n = len(lens)
    cap = max(lens) + steps + 40
    data = [inputs(50 + i, L, Hq, Hkv, D) for i, L in enumerate(lens)]
    g = torch.Generator(device=dev).manual_seed(5)
    new_q = torch.randn(steps, n, Hq, D, generator=g, device=dev, dtype=torch.float16).to(BF)
    new_k = torch.randn(steps, n, Hkv, D, generator=g, device=dev, dtype=torch.float16).to(BF)
    new_v = torch.randn(steps, n, Hkv, D, generator=g, device=dev, dtype=torch.float16).to(BF)

    singles, single_out, single_sc = [], [], []
    for i, L in enumerate(lens):
        c = qu.InferenceController(1, Hq, D, page, B, cap, BF, dev, num_kv_heads=Hkv, layout=layout, shuffle_seed=40 + i)
        fill(c, data[i][1], data[i][2], [L])
        c.end_forward()
        c.enable_device_state()
        c._decode_handler.set_pages_per_chunk(2)
        c.begin_graph_decode()
        singles.append(c)
    for t in range(steps):
        outs, scs = [], []
        for i, c in enumerate(singles):
            qu.step_advance_dyn(c)
            sc = qu.score_scratch(c).zero_()
            q, k = new_q[t, i:i + 1].clone(), new_k[t, i:i + 1].clone()
            outs.append(qu.decode_layer_dyn(q, k, new_v[t, i:i + 1], c, 0, sc, apply_rope=True, tiles=False))
            c.prepare_metadata(1)
            scs.append(sc)
        single_out.append(torch.cat(outs))
        single_sc.append(scs)

    def batched(graph):
        b = qu.BatchedInferenceController(n, 1, Hq, D, page, B, cap, BF, dev, num_kv_heads=Hkv, layout=layout, shuffle_seed=9)
        assert b.one_launch_layers is False
        for i, L in enumerate(lens):
            fill(b.seqs[i], data[i][1], data[i][2], [L])
            b.seqs[i].end_forward()
        b.enable_device_state()
        b._decode_handler.set_pages_per_chunk(2)
        b.begin_graph_decode()
        qbuf, kbuf, vbuf = torch.empty_like(new_q[0]), torch.empty_like(new_k[0]), torch.empty_like(new_v[0])
        scores = qu.score_scratch(b).zero_()
        obuf = torch.empty_like(new_q[0])

        def step():
            qu.step_advance_batched(b)
            qu.decode_layer_batched(qbuf, kbuf, vbuf, b, 0, scores, apply_rope=True, out=obuf, tiles=False)

        gr = None
        if graph:
            qbuf.copy_(new_q[0]); kbuf.copy_(new_k[0]); vbuf.copy_(new_v[0])
            pool = b.metadata_pool
            saved_m, saved_kv = pool.buf.clone(), b.kv_pool.buf.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()  # warm-up: a real step, undone below
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            pool.buf.copy_(saved_m); b.kv_pool.buf.copy_(saved_kv)
            b.sync_device_state()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                step()
            pool.buf.copy_(saved_m); b.kv_pool.buf.copy_(saved_kv)
            b.sync_device_state()
        outs, scs = [], []
        for t in range(steps):
            qbuf.copy_(new_q[t]); kbuf.copy_(new_k[t]); vbuf.copy_(new_v[t])
            if gr is not None:
                gr.replay()
            else:
                step()
            b.prepare_metadata(1)
            outs.append(obuf.clone())
            scs.append(scores.clone())
        torch.cuda.synchronize()
        return b, outs, scs

    b, outs, scs = batched(graph=False)
    for t in range(steps):
        assert torch.equal(outs[t].view(torch.int16), single_out[t].view(torch.int16)), t
        for i, c in enumerate(singles):
            n_out = (lens[i] + t + 1 + page - 1) // page - 1
            assert torch.equal(scs[t][i, :, :n_out].view(torch.int16), single_sc[t][i][:, :n_out].view(torch.int16)), (t, i)
    from test_gpu_batched import _gather
    for i, c in enumerate(singles):
        Lf = lens[i] + steps
        for a, bb in zip(_gather(c.kv_layer(0), c.kv_cache.indicies, Lf, layout),
                         _gather(b.kv_layer(0), b.seqs[i].kv_cache.indicies, Lf, layout)):
            assert torch.equal(a.view(torch.int16), bb.view(torch.int16))
        npg = len(c.kv_cache.indicies)
        for a, bb in zip(_gather(c.metadata_layer(0), c.metadata_cache.indicies, npg, layout),
                         _gather(b.metadata_layer(0), b.seqs[i].metadata_cache.indicies, npg, layout)):
            assert torch.equal(a.view(torch.int16), bb.view(torch.int16))
    _, outs_g, scs_g = batched(graph=True)
    for t in range(steps):
        assert torch.equal(outs_g[t].view(torch.int16), outs[t].view(torch.int16)), t


def test_tiles_launches_on_rows_beyond_4096_pages():
    """A pool of more than 4096 pages, GQA: the tiles launches (tile maxima from the estimate, two short selection passes)
    select what the oracle selects on the device's score bits, any chunk split, and attend within the bar."""
    import quest_amd.utils as qu

    Hq, Hkv, D, page, B = 4, 2, 128, 16, 64
    L = 16 * 4200 + 5
    q, k, v = inputs(91, L, Hq, Hkv, D)
    ctl = make_controller(L, Hq, Hkv, D, page, B, layout=2, shuffle_seed=8, max_seq_len=L + 64)
    fill(ctl, k, v, [L - 1, 1])
    kv_o, meta_o = oracle_pools(ctl, k, v)
    table = np.array(ctl.kv_cache.indicies, np.int32)
    ctl.end_forward()
    ctl.enable_device_state()
    st = ctl.step_state.cpu().tolist()
    st[0] -= 1
    st[2] -= 1
    n_out = len(table) - 1
    e_est = oracle.estimate(q, meta_o)
    ref = None
    for ppc in (0, 5, 64):
        ctl._decode_handler.set_pages_per_chunk(ppc)
        ctl.begin_graph_decode()
        ctl.step_state.copy_(torch.tensor(st, dtype=torch.int32))
        scores = qu.score_scratch(ctl).zero_()
        sel_i = torch.full((1, Hq, B - 1), -1, dtype=torch.int32, device="cuda:0")
        sel_v = torch.zeros(1, Hq, B - 1, dtype=BF, device="cuda:0")
        ctl._decode_handler.set_selection_out(sel_v, sel_i)
        qu.step_advance_dyn(ctl)
        o = qu.decode_layer_dyn(dev16(q), dev16(k[L - 1:L]), dev16(v[L - 1:L]), ctl, 0, scores)
        ctl._decode_handler.set_selection_out(None, None)
        assert ctl._decode_handler.last_launch_info()["front_end_variant"] == 8
        est_b = bits(scores[:, :n_out])
        check_scores(est_b, e_est)
        ev, ei = oracle.topk(_f16view(est_b), np.tile(table[:-1], (Hq, 1)), B - 1)
        assert np.array_equal(sel_i[0].cpu().numpy(), ei) and np.array_equal(bits(sel_v[0]), ev.view(np.uint16))
        eo, _ = oracle.sparse_attn(q, kv_o, ei, B - 1, int(table[-1]), kv_o.last_page_len)
        _close(o, eo)
        ref = ref if ref is not None else est_b
        assert np.array_equal(est_b, ref)


# ------------------------------------------------------------------------------------------------ 5. RoPE, RMSNorm
def _ulp_bf16(x64):
    """One bf16 ulp at |x| (8 significant bits), never below the smallest normal's."""
    e = np.floor(np.log2(np.maximum(np.abs(x64), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def _rope_ref(x_bits, pos, inv_freq32, attn):
    """Rotate-half in fp64 of the kernel's OWN fp32 angle: float32(pos) * float32(freq), one fp32 rounding, as the kernel
    forms it.  Returns (reference [n, H, D], |angle| [n, 1, D], |x1| + |x2| [n, H, D])."""
    x = bf16_bits_to_f32(x_bits).astype(np.float64)          # [n, H, D]
    n, H, D = x.shape
    ang32 = pos.astype(np.float32)[:, None] * inv_freq32.astype(np.float32)[None, :]      # [n, D/2], fp32 product
    ang = ang32.astype(np.float64)
    c, s = np.cos(ang) * attn, np.sin(ang) * attn
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    ref = np.concatenate([x1 * c[:, None, :] - x2 * s[:, None, :], x2 * c[:, None, :] + x1 * s[:, None, :]], axis=-1)
    mag = np.abs(x1) + np.abs(x2)
    return ref, np.abs(np.concatenate([ang, ang], axis=-1))[:, None, :], np.concatenate([mag, mag], axis=-1)


@pytest.mark.parametrize("D", [64, 128, 256])
def test_rope_all_four_entries_within_one_ulp(D):
    """The formula and table forms, eager positions and positions from step states, on bf16 q / k, against an fp64
    restatement of the rotation of the kernel's own fp32 angle (``_rope_ref``).

    Bound, per element: one bf16 ulp of the reference value + (|x1| + |x2|) * attention_factor * e.  The second term is a
    DEVIATION from the issue's "one bf16 ulp of the reference value", which cannot hold literally: an output is
    x1 c -+ x2 s computed in fp32, and where the two terms cancel the result (and its ulp) is arbitrarily small while the
    fp32 error of the terms is not.  e is derived, not fitted:
      * table form: e = 2^-21 -- the frequency is the table's fp32 value and the angle the same fp32 product as the
        kernel's, so what is left is sincosf (a few fp32 ulp of values <= 1, ulp 2^-24), the fp32 products with the
        attention factor and the two products and one sum of the rotation (2^-24 relative each): 8 x 2^-24 covers them;
      * formula form: e = 2^-21 + 2^-22 |angle| -- the frequency comes from the device's exp2f, here of an argument that is
        bit-identical in numpy (theta = 2^19 and a power-of-two scale make -log2f(theta) and every product exact in any
        libm), so it differs from numpy's exp2 by at most two fp32 ulp (2^-22 relative) and the angle by |angle| 2^-22.
    For |x| ~ 1 the term is 5e-7 (table) against a bf16 ulp of 4e-3 to 8e-3: the bar is one ulp wherever nothing cancels."""
    from quest_amd import _kernels

    n, Hq, Hk, past = 5, 6, 2, 700
    rng = np.random.default_rng(D)
    qb = f32_to_bf16_bits(rng.standard_normal((n, Hq, D)).astype(np.float32))
    kb = f32_to_bf16_bits(rng.standard_normal((n, Hk, D)).astype(np.float32))
    theta, scale = 2.0 ** 19, 2.0
    formula = ((np.float32(1.0) / np.float32(scale)) * np.exp2(np.float32(-np.log2(np.float32(theta))) *
                                                               (2 * np.arange(D // 2)).astype(np.float32) / np.float32(D))).astype(np.float32)
    table = (1.0 / (1e4 ** (np.arange(0, D, 2, dtype=np.float64) / D)) * np.where(np.arange(D // 2) % 3 == 0, 0.25, 1.0)).astype(np.float32)
    attn = 1.25
    states = torch.zeros(n, 8, dtype=torch.int32)
    seq_lens = np.array([past + 1 + 37 * i for i in range(n)])
    states[:, 0] = torch.from_numpy(seq_lens.astype(np.int32))
    states = states.to("cuda:0")
    inv_dev = torch.from_numpy(table).to("cuda:0")
    runs = {
        "formula": (lambda q, k: _kernels.apply_rope_in_place(q, k, past, scale, theta), past + np.arange(n), formula, 1.0, 2.0 ** -22),
        "formula_states": (lambda q, k: _kernels.apply_rope_in_place_batched(q, k, scale, theta, states), seq_lens - 1, formula, 1.0, 2.0 ** -22),
        "table": (lambda q, k: _kernels.apply_rope_in_place_freqs(q, k, inv_dev, attn, past_kv_len=past), past + np.arange(n), table, attn, 0.0),
        "table_states": (lambda q, k: _kernels.apply_rope_in_place_freqs(q, k, inv_dev, attn, states=states), seq_lens - 1, table, attn, 0.0),
    }
    for name, (run, pos, freq, af, freq_rel) in runs.items():
        q, k = to_dev(qb), to_dev(kb)
        run(q, k)
        for got_t, src in ((q, qb), (k, kb)):
            ref, ang, mag = _rope_ref(src, pos, freq, af)
            got = bf16_bits_to_f32(bits(got_t)).astype(np.float64)
            bound = _ulp_bf16(ref) + mag * af * (2.0 ** -21 + freq_rel * ang)
            err = np.abs(got - ref)
            record(f"rope {name} D={D}: worst err / bound {float((err / bound).max()):.3f}, worst err / ulp {float((err / _ulp_bf16(ref)).max()):.3f}")
            assert (err <= bound).all(), (name, int((err > bound).sum()), float((err / bound).max()))


def test_rms_norm_within_one_ulp():
    from quest_amd import _kernels

    rng = np.random.default_rng(3)
    rows, cols, eps = 7, 4096, 1e-5
    xb = f32_to_bf16_bits((rng.standard_normal((1, rows, cols)) * 3).astype(np.float32))
    wb = f32_to_bf16_bits((1 + 0.1 * rng.standard_normal(cols)).astype(np.float32))
    x, w = to_dev(xb), to_dev(wb)
    out = torch.empty_like(x)
    _kernels.rms_norm_forward(x, w, out, eps)
    x64, w64 = bf16_bits_to_f32(xb).astype(np.float64), bf16_bits_to_f32(wb).astype(np.float64)
    ref = x64 / np.sqrt((x64 ** 2).mean(axis=-1, keepdims=True) + eps) * w64
    got = bf16_bits_to_f32(bits(out)).astype(np.float64)
    bound = _ulp_bf16(ref)  # one bf16 ulp of the reference value
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())


# ------------------------------------------------------------------------------------------------ dtype discipline on the GPU
def test_mixed_and_foreign_dtypes_are_refused():
    from quest_amd import _kernels

    dev = "cuda:0"
    q16 = torch.zeros(1, 4, 128, dtype=torch.float16, device=dev)
    k_bf = torch.zeros(1, 4, 128, dtype=BF, device=dev)
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        _kernels.apply_rope_in_place(q16, k_bf, 0, 1.0, 1e4)
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        _kernels.apply_rope_in_place(q16.float(), k_bf.float(), 0, 1.0, 1e4)
    ctl = make_controller(64, 4, 4, 128, 16, 4)
    with pytest.raises(RuntimeError, match="dispatch with dtype"):   # fp16 token into a bf16 pool
        ctl.prepare_metadata(1)
        ctl.begin_forward(1)
        import quest_amd.utils as qu
        qu.append_kv(q16, q16, ctl, 0)
