"""Every tile-shape cell of the estimate launch (tests/_estimate_cells.py: two- / four-wave workgroups x kv heads per tile x
entries per tile x pool walk x table-load branch x tiles on / off) against the CPU oracle, bit for bit, through the C ABI's
Python wrappers; tests/test_estimate_cells_host.py shows that the cases are in the cells they claim and that no reachable
cell is missing.  One test per (head_dim, group); per case

* the state-driven appending entry (``append_estimate_dyn``; the tiles form in a tiles cell) appends the sequence's last
  token and scores: scores == oracle, pools == oracle after the append (the append blocks sit behind the estimate blocks and
  their count follows the workgroup width), columns beyond the live length keep a sentinel, tile maxima == the host keys of
  every run of 8 scores and nothing else is written.  Then the same entry with the state rewound to each shorter length of
  the case (1, below a tile, whole tiles): the appended token is the one already there, so the pools must not change;
* whole-row cells: ``decode_estimate`` and the eager entry over each shorter prefix of the page table == oracle;
* one query element zeroed in one head of the last head tile: only that tile takes the literal form, same bits as the oracle;
* flagged cases again as a batch of three ragged sequences (shorter than a tile, a single page, across a metadata page):
  every row == the oracle and == the sequence's own eager launch;
* bf16 cases: decided scores equal, midpoint scores a neighbour (tests/_bf16.py), the undecidable share pooled over the test
  at most 0.20 (the host test computes the same share from the oracle alone).

No tolerance anywhere: fp16 comparisons are on bit patterns."""
import numpy as np
import pytest
import torch

import _bf16
import _estimate_cells as E
import _harness
import oracle

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A
BUDGET = 4


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class _Checker:
    """Score comparison of one case: fp16 on bits; bf16 by ``_bf16.check_scores`` without its per-call cap -- the oracle
    scores are pooled and the cap applied to the pool."""

    def __init__(self, bf16):
        self.bf16 = bf16

    def __call__(self, dev_bits, want_f16, what):
        if not self.bf16:
            assert np.array_equal(dev_bits, np.ascontiguousarray(want_f16).view(np.uint16)), what
            return
        if want_f16.size:
            _bf16.check_scores(dev_bits, np.ascontiguousarray(want_f16), max_undecided=1.0)


def _sentinel_scratch(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda:0")
    t.view(torch.int16).fill_(SENTINEL)
    return t


def _check_row_block(buf_bits, n_out, max_n, tiles, check, want, what):
    """``buf_bits`` ``[Hq, stride]`` of one sequence after a state-driven launch: live scores, tile maxima, sentinel elsewhere."""
    from quest_amd import _kernels

    check(buf_bits[:, :n_out], want[:, :n_out], what + ": scores")
    if not tiles:
        assert (buf_bits[:, n_out:] == SENTINEL).all(), what + ": columns beyond the live length"
        return
    off, runs = _kernels.tile_max_offset(max_n), (n_out + 7) // 8
    assert (buf_bits[:, n_out:off] == SENTINEL).all(), what + ": between the live scores and the maxima"
    assert (buf_bits[:, off + runs:] == SENTINEL).all(), what + ": behind the live maxima"
    assert np.array_equal(buf_bits[:, off:off + runs], E.tile_maxima(buf_bits[:, :n_out])), what + ": tile maxima"


def _fill(c, ctl, k, v):
    """All but the last token: prefill, then two decode appends; the last token is the appending launch's."""
    n = k.shape[0] - 1
    if c.bf16:
        _bf16.fill(ctl, k[:n], v[:n], [n - 2, 1, 1])
    else:
        _harness.fill(ctl, k[:n], v[:n], split=n - 2)
    ctl.end_forward()


def _pools_equal(c, ctl, kv_o, meta_o, L):
    if c.bf16:
        return all(_bf16.pools_equal_oracle(ctl, kv_o, meta_o, L).values())
    return _harness.pools_match(ctl, kv_o, meta_o, L)


def _run_case(c, pooled):
    import quest_amd.utils as qu
    from quest_amd import _kernels

    cell, Hkv, S, L = c.cell, c.kv_heads, c.page_size, E.seq_len(c)
    Hq, D, what = Hkv * cell.group, cell.head_dim, E.case_id(c)
    mk, up = (_bf16, _bf16.dev16) if c.bf16 else (_harness, _harness.cuda)
    check = _Checker(c.bf16)
    q, k, v = E.case_inputs(c)
    q0 = E.zeroed_query(c, q)
    ctl = mk.make_controller(L, Hq, Hkv, D, S, BUDGET, layout=c.layout, shuffle_seed=c.seed)
    _fill(c, ctl, k, v)
    ctl.enable_device_state()
    qu.step_advance_dyn(ctl)
    max_n, lengths = ctl.max_pages - 1, E.n_outs(c)
    kd, vd, qd, q0d = up(k), up(v), up(q), up(q0)
    kvb, mb = ctl.kv_cache.buf_layer(0), ctl.metadata_cache.buf_layer(0)

    def dyn(query, token, scores):
        assert _kernels.append_estimate_dyn(kd[token:token + 1], vd[token:token + 1], kvb, ctl.kv_table_full, query, scores, mb,
                                            ctl.meta_table_full, ctl.step_state, max_n, ctl.layout, cell.tiles), what

    # the appending launch proper: the last token goes into the pools here
    scores = _sentinel_scratch((Hq, _kernels.tiles_row_stride(max_n)), ctl.dtype)
    dyn(qd, L - 1, scores)
    ctl.prepare_metadata(1)  # host mirror of the device-side reservation
    ctl.begin_forward(1)
    assert [int(x) for x in ctl.step_state.cpu()[:7]] == [L, lengths[-1] + 1, ctl.kv_cache.last_page_len,
                                                          ctl.kv_cache.indicies[-1], len(ctl.metadata_cache.indicies),
                                                          ctl.metadata_cache.last_page_len, ctl.metadata_cache.indicies[-1]], what
    kv_o, meta_o = mk.oracle_pools(ctl, k, v)
    want, want0 = oracle.estimate(q, meta_o), oracle.estimate(q0, meta_o)
    assert want.shape == (Hq, lengths[-1])
    _check_row_block(_bits(scores), lengths[-1], max_n, cell.tiles, check, want, what + " appending launch")
    assert _pools_equal(c, ctl, kv_o, meta_o, L), what + ": pools after the appending launch"

    # the literal form in one tile: whole rows through the eager entry, a tiles cell through its own entry (the append of
    # the token that is already there changes nothing)
    if cell.tiles:
        scores0 = _sentinel_scratch(tuple(scores.shape), ctl.dtype)
        dyn(q0d, L - 1, scores0)
        _check_row_block(_bits(scores0), lengths[-1], max_n, True, check, want0, what + " zeroed query element")
    else:
        check(_bits(qu.decode_estimate(q0d, ctl, 0)), want0, what + " zeroed query element")
        # whole rows, eager entry: the full length, then every shorter one over a prefix of the page table
        check(_bits(qu.decode_estimate(qd, ctl, 0)), want, what + " decode_estimate")
        for n in lengths[:-1]:
            o = _sentinel_scratch((Hq, n), ctl.dtype)
            _kernels.estimate_attn_score(qd, o, mb, ctl.metadata_indices, ctl.metadata_indptr_for_append,
                                         ctl.metadata_cache.last_page_len, ctl.metadata_last_page_idx, ctl.layout)
            check(_bits(o), want[:, :n], f"{what} eager n_out {n}")
    if c.bf16:
        pooled += [want, want0]  # what the cap of 0.20 is applied to, per test
    ctl.end_forward()

    # the state rewound to each shorter length: n pages scored, the "current" page n full, its last token appended again
    table, mtable = ctl.kv_cache.indicies, ctl.metadata_cache.indicies
    live = ctl.step_state.clone()
    for n in lengths[:-1]:
        state = [(n + 1) * S, n + 1, S, table[n], n // S + 1, n % S + 1, mtable[n // S], 0]
        ctl.step_state.copy_(torch.tensor(state, dtype=torch.int32))
        scores_n = _sentinel_scratch(tuple(scores.shape), ctl.dtype)
        dyn(qd, (n + 1) * S - 1, scores_n)
        _check_row_block(_bits(scores_n), n, max_n, cell.tiles, check, want, f"{what} state-driven n_out {n}")
    ctl.step_state.copy_(live)
    assert _pools_equal(c, ctl, kv_o, meta_o, L), what + ": pools after the rewound launches"
    if c.batched:
        _run_batch(c)


def _run_batch(c):
    """Three ragged sequences in one launch of the appending entry: each row == the oracle == the sequence's eager launch."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    cell, Hkv, S, what = c.cell, c.kv_heads, c.page_size, E.case_id(c) + " batch"
    Hq, D, lens = Hkv * cell.group, cell.head_dim, E.batch_lens(c)
    data = [E.case_inputs(c, L, salt=i + 1) for i, L in enumerate(lens)]
    b = qu.BatchedInferenceController(len(lens), 1, Hq, D, S, BUDGET, max(lens) + 4 * S, torch.float16, torch.device("cuda:0"),
                                      num_kv_heads=Hkv, layout=c.layout, shuffle_seed=c.seed + 1)
    for ctl, (_, k, v) in zip(b.seqs, data):
        n = k.shape[0] - 1
        ctl.prepare_metadata(n)
        ctl.begin_forward(n)
        qu.append_kv(_harness.cuda(k[:n]), _harness.cuda(v[:n]), ctl, 0)
        ctl.end_forward()
    b.enable_device_state()
    qu.step_advance_batched(b)
    max_n = b.max_pages - 1
    scores = _sentinel_scratch((len(lens), Hq, _kernels.tiles_row_stride(max_n)), torch.float16)
    stack = lambda j: _harness.cuda(np.concatenate([d[j][-1:] if j else d[j] for d in data]))
    qs = stack(0)
    assert _kernels.append_estimate_batched(stack(1), stack(2), b.kv_layer(0), b.kv_tables, qs, scores, b.metadata_layer(0),
                                            b.meta_tables, b.step_states, max_n, b.layout, cell.tiles), what
    b.prepare_metadata(1)
    rows = _bits(scores)
    check = _Checker(False)
    for i, (ctl, (q, k, v), L) in enumerate(zip(b.seqs, data, lens)):
        n_out = -(-L // S) - 1
        kv_o, meta_o = _harness.oracle_pools(ctl, k, v)
        want = oracle.estimate(q, meta_o)
        assert want.shape == (Hq, n_out)
        _check_row_block(rows[i], n_out, max_n, cell.tiles, check, want, f"{what} sequence {i}")
        assert _harness.pools_match(ctl, kv_o, meta_o, L), f"{what} sequence {i}: pools"
        if n_out:
            ctl.begin_forward(1)
            single = qu.decode_estimate(qs[i:i + 1], ctl, 0)
            ctl.end_forward()
            assert np.array_equal(_bits(single), rows[i][:, :n_out]), f"{what} sequence {i}: its single-sequence result"


@pytest.mark.parametrize("head_dim,group", [(D, G) for D in E.HEAD_DIMS for G in E.GROUPS])
def test_estimate_cells_match_the_oracle(head_dim, group):
    cases = [c for c in E.CASES if (c.cell.head_dim, c.cell.group) == (head_dim, group)]
    assert cases
    pooled = []
    for c in cases:
        _run_case(c, pooled)
    if pooled:
        share = E.midpoint_share(pooled)
        _bf16.record(f"estimate cells D{head_dim} G{group}: undecidable share {share:.4f} of {sum(a.size for a in pooled)} pooled "
                     f"bf16 scores (bar {E.BF16_MIDPOINT_CAP})")
        assert share <= E.BF16_MIDPOINT_CAP, share


@pytest.mark.parametrize("Hkv", [4, 12])
def test_refused_shapes_are_refused_by_every_entry_and_served_on_nhd(Hkv):
    """head_dim 256, group 8, kv heads a multiple of 4: QUEST_EUNSUPPORTED from every estimate entry for the row-rotated
    layout -- the Python surface raises RuntimeError (the tiles form returns False: its caller has another route), nothing is
    launched, output and pools stay untouched -- while the same pool read as NHD is served, bit-equal to the oracle."""
    import quest_amd.utils as qu
    from quest_amd import _kernels

    Hq, D, S, L, ROT = Hkv * 8, 256, 16, 16 * 3 + 5, E.NHD_ROT
    assert E.plan(D, Hq, Hkv, ROT, False)[0] == E.plan(D, Hq, Hkv, ROT, True)[0] == E.EUNSUPPORTED
    with pytest.raises(ValueError, match="layouts that serve this shape: NHD, HND"):
        _harness.make_controller(L, Hq, Hkv, D, S, BUDGET, layout=ROT)
    q, k, v = _harness.inputs(77 + Hkv, L, Hq, Hkv, D)
    ctl = _harness.make_controller(L, Hq, Hkv, D, S, BUDGET, layout=E.NHD, shuffle_seed=3)
    _harness.fill(ctl, k, v)
    kv_o, meta_o = _harness.oracle_pools(ctl, k, v)
    want = oracle.estimate(q, meta_o)
    n_out = want.shape[1]
    qd, k1, v1 = _harness.cuda(q), _harness.cuda(k[-1:]), _harness.cuda(v[-1:])
    kvb, mb = ctl.kv_cache.buf_layer(0), ctl.metadata_cache.buf_layer(0)
    before = (_bits(kvb), _bits(mb))
    o = _sentinel_scratch((Hq, n_out), torch.float16)
    a = qu._append_args(ctl, 0)
    ctl.end_forward()
    ctl.enable_device_state()
    max_n = ctl.max_pages - 1
    wide = _sentinel_scratch((1, Hq, _kernels.tiles_row_stride(max_n)), torch.float16)
    dyn = (k1, v1, kvb, ctl.kv_table_full, qd, wide[0], mb, ctl.meta_table_full, ctl.step_state, max_n)
    refused = [
        lambda: _kernels.estimate_attn_score(qd, o, mb, ctl.metadata_indices, ctl.metadata_indptr_for_append,
                                             ctl.metadata_cache.last_page_len, ctl.metadata_last_page_idx, ROT),
        lambda: _kernels.append_estimate(k1, v1, a[0], a[1], a[2], a[3], a[4], qd, o, a[5], a[6], a[7], a[8], a[9], ROT),
        lambda: _kernels.estimate_attn_score_batched(qd, wide, mb, ctl.meta_tables, ctl.step_states, max_n, ROT),
        lambda: _kernels.append_estimate_batched(*dyn, ROT),
        lambda: _kernels.append_estimate_dyn(*dyn, ROT),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(RuntimeError, match="error code -2"):
            call()
        torch.cuda.synchronize()
        assert (_bits(o) == SENTINEL).all() and (_bits(wide) == SENTINEL).all(), f"entry {i} wrote its output"
    assert _kernels.append_estimate_dyn(*dyn, ROT, tiles=True) is False
    assert _kernels.append_estimate_batched(*dyn, ROT, tiles=True) is False
    assert (_bits(wide) == SENTINEL).all()
    assert np.array_equal(_bits(kvb), before[0]) and np.array_equal(_bits(mb), before[1]), "a refused launch wrote a pool"
    # the same shape on NHD: served (a two-wave tile of one kv head), bit-equal
    ctl.begin_forward(1)
    assert np.array_equal(_bits(qu.decode_estimate(qd, ctl, 0)), want.view(np.uint16))
    _kernels.append_estimate_dyn(*dyn, E.NHD)  # the state describes the filled cache: the last token once more
    assert np.array_equal(_bits(wide[0])[:, :n_out], want.view(np.uint16))
    ctl.end_forward()
    assert _harness.pools_match(ctl, kv_o, meta_o, L)
