"""The case table of tests/_estimate_cells.py against the estimate launch's real planner (quest_estimate_plan needs no GPU and
is the function launch_estimate plans with): which planner cells tests/test_gpu_estimate_cells.py reaches is stated here,
not left to its shapes.  Also the refusals: which shapes every estimate entry refuses, that the header says so, and that the
controllers refuse them at construction."""
import collections
import ctypes
import os

import pytest
import torch

import _estimate_cells as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from quest_amd._lib import lib
    return lib


def _plan(D, Hq, Hkv, layout, tiles):
    info = (ctypes.c_uint32 * 3)(77, 77, 77)
    code = _lib().quest_estimate_plan(D, Hq, Hkv, layout, int(tiles), info)
    if code:
        assert tuple(info) == (77, 77, 77)  # a refusal leaves info alone
        return code, None
    return 0, tuple(info)


def test_cases_are_well_formed():
    ids = [E.case_id(c) for c in E.CASES]
    assert len(set(ids)) == len(ids)
    for c in E.CASES:
        k = c.cell
        assert c.kv_heads in E.PREFERRED_KV_HEADS and c.kv_heads % k.hw == 0, c
        assert c.page_size == E.PAGE or c.page_size == E.second_page_size(k.ew, 0) or c.page_size == E.second_page_size(k.ew, 1), c
        assert not (k.tiles and c.page_size != E.PAGE), c
        # lengths: 1, below a tile, whole tiles, k tiles + 3 with k >= 2; the longest spans two metadata pages
        n = E.n_outs(c)
        assert n[0] == 1 and max(1, k.ew - 1) in n and (n[-1] - 3) % k.ew == 0 and (n[-1] - 3) // k.ew >= 2 and n[-1] - 3 in n, (c, n)
        assert n[-1] + 1 > c.page_size, (c, n)
        L = E.seq_len(c)
        assert -(-L // c.page_size) == n[-1] + 1 and L <= 9000, (c, L)
        pool_bytes = (n[-1] + 1 + 5) * 2 * c.page_size * c.kv_heads * k.head_dim * 2
        assert pool_bytes <= 24 << 20, (c, pool_bytes)
        qh, d = E.zeroed_element(c)
        assert qh // (k.hw * k.group) == c.kv_heads // k.hw - 1 and d < k.head_dim, c  # a head of the last head tile
        if c.batched:
            lens = E.batch_lens(c)
            pages = [-(-l // c.page_size) for l in lens]
            assert c.page_size == E.PAGE and not c.bf16
            assert 1 <= pages[0] - 1 < max(2, k.ew) and pages[1] == 1 and pages[2] - 1 > c.page_size, (c, pages)


def test_every_case_is_in_the_cell_the_table_claims():
    for c in E.CASES:
        k = c.cell
        code, shape = _plan(k.head_dim, c.kv_heads * k.group, c.kv_heads, c.layout, k.tiles)
        assert code == 0 and shape == (k.waves, k.hw, k.ew), (E.case_id(c), code, shape)
        assert E.walk(c.kv_heads, c.layout) == k.walk and E.branch(c.page_size, k.ew) == k.branch, E.case_id(c)
        # the rotation the walk names is the pool's: quest_pool_slot moves head 0 of entry e to slot e & rot
        if c.layout == E.NHD_ROT:
            rot = int(k.walk[3:])
            assert [_lib().quest_pool_slot(2, c.kv_heads, 0, e, 0) for e in range(4)] == [e & rot for e in range(4)]


def test_restatement_equals_the_planner_over_the_whole_grid():
    served = refused = 0
    for D, G, H, layout, tiles in E.grid():
        mine, theirs = E.plan(D, H * G, H, layout, tiles), _plan(D, H * G, H, layout, tiles)
        assert mine == theirs, ((D, G, H, layout, tiles), mine, theirs)
        served += mine[0] == 0
        refused += mine[0] != 0
    assert served == 3 * 4 * 32 * 3 * 2 - len(E.REFUSED) and refused == len(E.REFUSED)
    # outside the grid: the codes every estimate entry returns
    for args in [(96, 8, 8, 0, 0), (128, 24, 8, 0, 0), (128, 48, 3, 1, 0), (512, 4, 4, 2, 1),   # unsupported head_dim / group
                 (128, 8, 8, 3, 0), (128, 0, 8, 0, 0), (128, 8, 0, 0, 0), (128, 9, 8, 0, 0), (96, 9, 8, 7, 1)]:  # malformed
        assert E.plan(*args) == _plan(*args), args
        assert E.plan(*args)[0] == (E.EUNSUPPORTED if args in [(96, 8, 8, 0, 0), (128, 24, 8, 0, 0), (128, 48, 3, 1, 0),
                                                                (512, 4, 4, 2, 1)] else E.EINVAL), args
    assert _lib().quest_estimate_plan(128, 8, 8, 0, 0, None) == E.EINVAL


def test_the_refused_set_is_head_dim_256_group_8_on_the_rotated_pool_with_kv_heads_in_fours():
    got = [g for g in E.grid() if _plan(g[0], g[1] * g[2], g[2], g[3], g[4])[0] != 0]
    assert sorted(got) == sorted(E.REFUSED)
    assert all(_plan(g[0], g[1] * g[2], g[2], g[3], g[4])[0] == E.EUNSUPPORTED for g in got)
    # the ten a sweep over the usual head counts finds; the other layouts serve every one of them, both forms
    usual = [g for g in got if g[2] in (1, 2, 3, 4, 6, 8, 12, 16, 32)]
    assert len(usual) == 10 and len(got) == 16
    for D, G, H, _, tiles in got:
        for layout in (E.NHD, E.HND):
            assert _plan(D, H * G, H, layout, tiles)[0] == 0
    # no shape is refused in the tiles form alone: a controller that cannot take the tiles form has the whole-row one
    for D, G, H, layout, _ in E.grid():
        assert (_plan(D, H * G, H, layout, True)[0] == 0) == (_plan(D, H * G, H, layout, False)[0] == 0)


def test_every_reachable_cell_has_a_case(capsys):
    cells, left_out = E.served_cells()
    covered = collections.Counter(c.cell for c in E.CASES if not c.bf16)
    missing = [c for c in cells if not covered[c]]
    assert not missing, missing
    assert set(covered) == set(cells)
    # the grid's cells come from the planner itself, not only from its restatement
    for D, G, H, layout, tiles in E.grid():
        planned = _plan(D, H * G, H, layout, tiles)
        if planned[0] == 0:
            for S in (E.PAGE, E.second_page_size(planned[1][2])):
                cell = E.cell_of(D, G, H, layout, tiles, S, planned)
                assert cell in cells or cell in left_out, cell
    # cells left out, by name: only the branch a tiles cell cannot reach at page size 16
    for cell, why in left_out.items():
        assert cell.tiles and cell.branch != E.branch(E.PAGE, cell.ew) and "page size 16 only" in why, cell
    with capsys.disabled():
        print(f"\nestimate cells: {len(cells)} served cells covered by {len(E.CASES)} cases "
              f"({sum(c.bf16 for c in E.CASES)} bf16, {sum(c.batched for c in E.CASES)} also as a batch); "
              f"{len(left_out)} left out, all '<tiles cell> at the other table-load branch': the tiles form runs at page size "
              f"16 only")
        by_shape = collections.Counter((c.waves, c.hw, c.ew) for c in cells)
        print("  cells per (waves, kv heads per tile, entries per tile): " +
              ", ".join(f"{k}: {v}" for k, v in sorted(by_shape.items())))


def test_four_wave_cells_and_head_tile_counts_are_reached():
    cells, _ = E.served_cells()
    f16 = [c for c in E.CASES if not c.bf16]
    # the bench's default layout: 32 / 4 heads x 128 on the row-rotated pool is a four-wave cell
    llama70 = E.cell_of(128, 8, 4, E.NHD_ROT, False, 16)
    assert llama70.waves == 4 and any(c.cell == llama70 and c.kv_heads == 4 for c in f16)
    four = {c for c in cells if c.waves == 4}
    assert four and four <= {c.cell for c in f16}
    assert {(c.head_dim, c.group) for c in four} == {(128, 8), (256, 1), (256, 2), (256, 4), (256, 8)}
    # every tile width of every (head_dim, group): with one head tile, and with a count > 1 that is no power of two,
    # wherever a preferred head count gives the planner that
    want = collections.defaultdict(set)
    for D, G, H, layout, tiles in E.grid():
        if H in E.PREFERRED_KV_HEADS:
            code, shape = E.plan(D, H * G, H, layout, tiles)
            if code == 0:
                t = H // shape[1]
                want[(D, G, shape[0], shape[1])].add("one" if t == 1 else "odd" if t & (t - 1) else "pow2")
    have = collections.defaultdict(set)
    for c in f16:
        t = c.kv_heads // c.cell.hw
        have[(c.cell.head_dim, c.cell.group, c.cell.waves, c.cell.hw)].add("one" if t == 1 else "odd" if t & (t - 1) else "pow2")
    for key, kinds in want.items():
        assert kinds & {"one", "odd"} <= have[key], (key, kinds, have[key])
    # bf16 and the batch: once per (waves, kv heads per tile, entries per tile, layout)
    shapes = {(c.waves, c.hw, c.ew, E._layout_of(c.walk)) for c in cells}
    assert {(c.cell.waves, c.cell.hw, c.cell.ew, c.layout) for c in E.CASES if c.bf16} == shapes
    assert {(c.cell.waves, c.cell.hw, c.cell.ew, c.layout) for c in E.CASES if c.batched} == shapes
    assert any(c.kv_heads == 32 and c.cell.group == 8 and c.cell.head_dim == 256 for c in f16)  # 256 query heads x 256


def test_bf16_midpoint_share_of_each_gpu_test_is_within_the_cap():
    """The bf16 cases' oracle scores (the query and its zeroed variant, the scores the GPU test pools per (head_dim, group)):
    the share that sits on a bf16 midpoint -- where the oracle cannot decide the device's rounding -- is at most 0.20 for the
    chosen seeds, so the cap is known to hold before any GPU runs."""
    import oracle

    pooled = collections.defaultdict(list)
    for c in E.CASES:
        if c.bf16:
            q, k, v = E.case_inputs(c)
            _, meta = E.plain_oracle_pools(c, k, v)
            pooled[(c.cell.head_dim, c.cell.group)] += [oracle.estimate(q, meta), oracle.estimate(E.zeroed_query(c, q), meta)]
    assert pooled
    for key, arrays in sorted(pooled.items()):
        share = E.midpoint_share(arrays)
        assert share <= E.BF16_MIDPOINT_CAP, (key, share, sum(a.size for a in arrays))


def test_the_header_states_the_refused_shapes():
    text = " ".join(open(os.path.join(ROOT, "include", "quest_hip.h")).read().replace("*", " ").split())
    assert "REFUSED" in text and "head_dim 256 with group 8 on QUEST_LAYOUT_NHD_ROT when the number of kv heads is a multiple of 4" in text
    assert "int quest_estimate_plan(uint32_t head_dim, uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t layout, int tiles," in text


@pytest.mark.parametrize("Hkv", [4, 8, 12, 32])
def test_controllers_refuse_at_construction_what_the_estimate_refuses(Hkv):
    import quest_amd.utils as qu

    Hq, D = Hkv * 8, 256
    for make in (lambda layout: qu.InferenceController(1, Hq, D, 16, 4, 64, torch.float16, "cpu", num_kv_heads=Hkv, layout=layout),
                 lambda layout: qu.BatchedInferenceController(2, 1, Hq, D, 16, 4, 64, torch.float16, "cpu", num_kv_heads=Hkv,
                                                              layout=layout)):
        for layout in (2, "NHD_ROT"):
            with pytest.raises(ValueError) as exc:
                make(layout)
            msg = str(exc.value)
            assert f"{Hq} query heads / {Hkv} kv heads x head_dim 256" in msg and "NHD_ROT" in msg, msg
            assert "layouts that serve this shape: NHD, HND" in msg, msg
        for layout in (0, 1):  # the same shape on the reference's layouts: served, so constructed
            assert make(layout).layout == layout


def test_controllers_still_construct_what_the_estimate_serves_or_no_layout_serves():
    import quest_amd.utils as qu

    # neighbours of the refused shapes on the rotated pool: kv heads 2 and 6 (rotation 1), group 4, head_dim 128
    for Hq, Hkv, D in [(16, 2, 256), (48, 6, 256), (16, 4, 256), (32, 4, 128), (32, 32, 256)]:
        assert qu.InferenceController(1, Hq, D, 16, 4, 64, torch.float16, "cpu", num_kv_heads=Hkv, layout=2).layout == 2
    # a group no layout serves is not this check's business: the operators refuse it when asked, as before
    assert qu.InferenceController(1, 48, 128, 16, 4, 64, torch.float16, "cpu", num_kv_heads=3, layout=2).num_heads == 48
