"""The estimate launch's planner, restated, and the case table of tests/test_gpu_estimate_cells.py.

``launch_estimate`` (quest_amd/csrc/estimate.hip) picks, per shape: a two-wave or a four-wave workgroup, a tile of 1, 2, 4
or 8 kv heads (narrower when the launch also writes tile maxima), or a refusal.  Each combination changes index arithmetic
of ``estimate_tile`` (estimate_device.cuh): the q staging count HW*G*D/8, the ``hl ^= e_in & rot`` head fix-up,
``blockIdx.x / head_tiles``, the LDS offsets of ``neg_s`` / ``out_s``, the scalar versus per-row page-table load
``(S & (EW-1)) == 0``, and the number of append blocks (EWV*64 threads each) behind the estimate blocks.

``plan`` below is that planner in plain Python; tests/test_estimate_cells_host.py holds it to ``quest_estimate_plan`` (the
function the launch plans with) over the whole grid.  A CELL is one combination

    (head_dim, group, walk, tiles, waves, kv heads per tile, entries per tile, table-load branch)

with walk = "NHD", "HND" or "ROT<rot>" (QUEST_LAYOUT_NHD_ROT with its rotation 0 / 1 / 3) and branch = "scalar" (page size a
multiple of the tile's entries: one wave-uniform table load) or "rows" (one table load per row).  The element type is a field
of the CASE: every cell has an fp16 case, and one bf16 case runs per (waves, heads per tile, entries per tile, layout) --
bf16 changes the tile's LDS offsets (no sign masks) and always takes the literal form, not the planner's choice.

A case names its cell and a small shape.  Page size 16 is the default; the second page size sits on the other side of
``(S & (EW-1)) == 0``: 5 or 7 where EW <= 16 (per-row loads), EW itself where EW is 32 or 64 (scalar load).  The tiles form
runs at page size 16 only (the launch that consumes the maxima serves no other), so a tiles cell has the one branch page
size 16 gives it.  kv heads come from PREFERRED_KV_HEADS, so that every tile width runs with one head tile and with a number
of head tiles that is larger than one and no power of two wherever the cell has such a head count.

Lengths follow from EW (``n_outs``): the pool is built once, for the longest one -- k*EW + 3 pages scored with k >= 2 and
more than one metadata page, page ids shuffled -- and the shorter ones (1, < EW, k*EW) are launches over a prefix of its
page table: the estimate takes n_out as an argument and a page's score does not depend on the others.
"""
from collections import namedtuple

NHD, HND, NHD_ROT = 0, 1, 2
LAYOUT_NAMES = {NHD: "NHD", HND: "HND", NHD_ROT: "NHD_ROT"}
EINVAL, EUNSUPPORTED = -1, -2
HEAD_DIMS, GROUPS, KV_HEADS = (64, 128, 256), (1, 2, 4, 8), tuple(range(1, 33))
PREFERRED_KV_HEADS = (1, 3, 2, 6, 4, 12, 8, 32)
WAVE, VEC, LOADS_PER_WAVE = 64, 8, 4  # lanes, elements per 16-byte load, load rounds per wave (QUEST_EST_ITER[_GQA])
PAGE = 16

Cell = namedtuple("Cell", "head_dim group walk tiles waves hw ew branch")
Case = namedtuple("Case", "cell kv_heads layout page_size bf16 batched seed")


def rotation(num_heads, layout):
    """``rot`` of PoolStrides (quest_common.cuh): min(largest power of two dividing the head count, 4) - 1 on NHD_ROT."""
    if layout != NHD_ROT:
        return 0
    return min(num_heads & -num_heads, 4) - 1


def _tile_shape(D, G, H, rot, tiles, waves):
    """kv heads per tile of a ``waves``-wave workgroup, or None where that width does not serve the shape."""
    lanes_per_row = D // VEC
    rows = waves * LOADS_PER_WAVE * (WAVE // lanes_per_row)
    staging = 2 * waves * WAVE  # 16-byte query vectors one staging pass holds
    hw = 1
    for cand in (8, 4, 2):
        if H % cand == 0 and cand * G * lanes_per_row <= staging:
            hw = cand
            break
    while tiles and hw > 1 and (rows // hw) % 8:
        hw //= 2
    if tiles and (rows // hw) % 8:
        return None
    if rot >= hw:
        return None
    if hw * G * lanes_per_row > staging:
        return None
    return hw, rows // hw


def plan(D, Hq, Hkv, layout, tiles):
    """What quest_estimate_plan answers: ``(0, (waves, kv heads per tile, entries per tile))`` or ``(error code, None)``."""
    if layout not in (NHD, HND, NHD_ROT) or Hkv == 0 or Hq == 0 or Hq % Hkv:
        return EINVAL, None
    G = Hq // Hkv
    if D not in HEAD_DIMS or G not in GROUPS:
        return EUNSUPPORTED, None
    for waves in (2, 4):
        shape = _tile_shape(D, G, Hkv, rotation(Hkv, layout), bool(tiles), waves)
        if shape:
            return 0, (waves,) + shape
    return EUNSUPPORTED, None


def walk(Hkv, layout):
    return "ROT%d" % rotation(Hkv, layout) if layout == NHD_ROT else LAYOUT_NAMES[layout]


def branch(page_size, ew):
    return "scalar" if page_size & (ew - 1) == 0 else "rows"


def second_page_size(ew, salt=0):
    """The page size on the other side of ``(S & (EW-1)) == 0`` from 16."""
    return (5, 7)[salt % 2] if ew <= 16 else ew


def cell_of(D, G, Hkv, layout, tiles, page_size, planned=None):
    code, shape = plan(D, Hkv * G, Hkv, layout, tiles) if planned is None else planned
    if code:
        return None
    waves, hw, ew = shape
    return Cell(D, G, walk(Hkv, layout), bool(tiles), waves, hw, ew, branch(page_size, ew))


def grid():
    """Every (head_dim, group, kv heads, layout, tiles) of the planner's domain."""
    for D in HEAD_DIMS:
        for G in GROUPS:
            for H in KV_HEADS:
                for layout in (NHD, HND, NHD_ROT):
                    for tiles in (False, True):
                        yield D, G, H, layout, tiles


def served_cells():
    """cell -> kv head counts that land in it, for page size 16 and the second page size of the cell's EW; plus the cells
    left out and why."""
    cells, left_out = {}, {}
    for D, G, H, layout, tiles in grid():
        code, shape = plan(D, H * G, H, layout, tiles)
        if code:
            continue
        ew = shape[2]
        for S in (PAGE, second_page_size(ew)):
            c = cell_of(D, G, H, layout, tiles, S)
            if tiles and S != PAGE:
                left_out[c] = "the tiles form runs at page size 16 only (the attention launch that reads the maxima serves no other)"
                continue
            cells.setdefault(c, []).append(H)
    for c in cells:
        left_out.pop(c, None)
    return cells, left_out


REFUSED = [(256, 8, H, NHD_ROT, tiles) for H in KV_HEADS if H % 4 == 0 for tiles in (False, True)]
"""The refused shapes (QUEST_EUNSUPPORTED from every estimate entry): head_dim 256, group 8, kv heads % 4 == 0 on the
row-rotated pool, whole rows and tiles form alike.  Over kv heads 1..32 that is 8 head counts x 2 forms = 16 grid points; the
ten of them with kv heads in (4, 8, 12, 16, 32) are the ones a sweep over the usual head counts finds."""


def _layout_of(walk_name):
    return {"NHD": NHD, "HND": HND}.get(walk_name, NHD_ROT)


def _build_cases():
    cells, _ = served_cells()
    # bf16 and the batch run once per (waves, kv heads per tile, entries per tile, layout), at page size 16: the cell that
    # carries them is picked by a fixed rule that spreads them over the (head_dim, group) tests
    by_shape = {}
    for c in sorted(cells):
        if branch(PAGE, c.ew) == c.branch:
            by_shape.setdefault((c.waves, c.hw, c.ew, _layout_of(c.walk)), []).append(c)
    extras = {v[(7 * k[0] + 3 * k[1] + k[2] + 5 * k[3]) % len(v)] for k, v in by_shape.items()}
    cases = []
    for n, c in enumerate(sorted(cells)):
        heads = [h for h in PREFERRED_KV_HEADS if h in cells[c]]
        assert heads, c  # every cell holds one of the preferred head counts
        one_tile = [h for h in heads if h == c.hw]
        odd_tiles = [h for h in heads if h // c.hw > 1 and (h // c.hw) & (h // c.hw - 1)]
        # the scalar-branch case of a cell takes a single head tile, the per-row one a non-power-of-two number of them;
        # 32 kv heads (flip 28 on the rotated pool, 256 query heads at group 8) ride as a third case where the cell has them
        first = (one_tile or heads) if c.branch == "scalar" else (odd_tiles or heads[::-1])
        picks = [first[0]] + ([32] if 32 in heads and first[0] != 32 and c.branch == "scalar" and not c.tiles else [])
        if c.tiles:  # a tiles cell has one branch only: both kinds of head-tile count run in it
            picks += [h for h in (one_tile[:1] + odd_tiles[:1]) if h not in picks]
        layout = _layout_of(c.walk)
        S = PAGE if branch(PAGE, c.ew) == c.branch else second_page_size(c.ew, n)
        for i, H in enumerate(picks):
            extra = c in extras and i == 0
            cases.append(Case(c, H, layout, S, False, extra, 1000 + len(cases)))
            if extra:
                cases.append(Case(c, H, layout, S, True, False, 1000 + len(cases)))
    return cases


CASES = _build_cases()


def case_id(c):
    k = c.cell
    return "D%d_G%d_%s_%s_w%d_hw%d_ew%d_%s_H%d_S%d_%s" % (k.head_dim, k.group, k.walk, "tiles" if k.tiles else "rows", k.waves,
                                                          k.hw, k.ew, k.branch, c.kv_heads, c.page_size,
                                                          "bf16" if c.bf16 else "f16")


def n_outs(c):
    """Scored-page counts of a case, ascending: 1, one below a tile, k tiles, k tiles + 3 (k >= 2, and enough for the
    metadata entries to span two metadata pages: entry n_out, the current page's, lies in the second one at the least)."""
    ew, S = c.cell.ew, c.page_size
    k = max(2, -(-(S - 2) // ew))
    full = k * ew + 3
    assert full > S and k >= 2
    return sorted({1, max(1, ew - 1), k * ew, full})


def seq_len(c):
    """Tokens of the case's sequence: n_outs(c)[-1] + 1 pages; the last token opens the last page in the per-row cases (the
    appending launch then starts a page and a metadata entry), and lands inside it otherwise."""
    pages, S = n_outs(c)[-1] + 1, c.page_size
    last = 1 if c.cell.branch == "rows" else 2 + c.seed % (S - 1)
    return (pages - 1) * S + last


def batch_lens(c):
    """Three ragged sequences of a batched case: shorter than a tile, a single page (nothing to score), across a metadata
    page."""
    S = c.page_size
    short = max(1, c.cell.ew - 1)
    return [short * S + 3, 5, seq_len(c)]


def zeroed_element(c):
    """(query head, feature) zeroed for the literal-form run: a head of the LAST head tile, not its first."""
    k = c.cell
    tile_heads = k.hw * k.group
    qh = (c.kv_heads // k.hw - 1) * tile_heads + (tile_heads - 1 if tile_heads > 1 else 0)
    return qh, (7 * c.seed + 3) % k.head_dim


def case_inputs(c, length=None, salt=0):
    """q ``[1, Hq, D]``, k / v ``[L, Hkv, D]`` of a case as fp16 arrays: N(0,1), for a bf16 case restricted to bf16 values."""
    import _bf16
    import _harness

    make = _bf16.inputs if c.bf16 else _harness.inputs
    return make(c.seed + 7919 * salt, seq_len(c) if length is None else length, c.kv_heads * c.cell.group, c.kv_heads,
                c.cell.head_dim)


def zeroed_query(c, q):
    q2 = q.copy()
    qh, d = zeroed_element(c)
    q2[0, qh, d] = 0
    return q2


def plain_oracle_pools(c, k, v):
    """The oracle's pools of one sequence on an identity page table (scores do not depend on the physical page ids)."""
    import numpy as np

    import oracle

    L, S, H, D = k.shape[0], c.page_size, c.kv_heads, c.cell.head_dim
    pages = -(-L // S)
    meta_pages = -(-pages // S)
    shape = (lambda n: (n, 2, H, S, D)) if c.layout == HND else (lambda n: (n, 2, S, H, D))
    kv = oracle.Paged(np.zeros(shape(pages), np.float16), np.arange(pages, dtype=np.int32), L - (pages - 1) * S, c.layout)
    meta = oracle.Paged(np.zeros(shape(meta_pages), np.float16), np.arange(meta_pages, dtype=np.int32),
                        pages - (meta_pages - 1) * S, c.layout)
    oracle.append_prefill(kv, meta, k, v)
    return kv, meta


BF16_MIDPOINT_CAP = 0.20  # tests/_bf16.py check_scores: share of oracle scores that sit on a bf16 midpoint


def midpoint_share(score_arrays):
    """Share of the fp16 oracle scores whose bf16 rounding the oracle value does not decide (``bits & 7 == 4``), over all
    the arrays together."""
    import numpy as np

    bits = np.concatenate([np.ascontiguousarray(a, np.float16).view(np.uint16).ravel() for a in score_arrays])
    return float(((bits & 7) == 4).mean()) if bits.size else 0.0


def half_keys(bits_u16):
    """Order-preserving 16-bit keys of sign-magnitude 16-bit patterns (csrc/quest_common.cuh half_key)."""
    import numpy as np

    b = bits_u16.astype(np.uint32)
    return np.where(b & 0x8000, (~b) & 0xffff, b | 0x8000).astype(np.uint16)


def tile_maxima(bits_u16):
    """Per row the largest key of every run of 8 scores (missing columns of the last run count as key 0)."""
    import numpy as np

    rows, n = bits_u16.shape
    runs = (n + 7) // 8
    padded = np.zeros((rows, runs * 8), np.uint16)
    padded[:, :n] = half_keys(bits_u16)
    return padded.reshape(rows, runs, 8).max(axis=2)
