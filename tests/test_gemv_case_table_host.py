"""The case table of tests/_gemv_exact.py against the real n-token planner (quest_decode_batched_plan needs no GPU: it assumes
256 workgroups, an MI355X's compute units) and against the conditions the table exists for: which cells of the planner and
of the batch-1 dispatch the GPU file test_gpu_decode_layer_exact.py reaches is stated here, not left to its shapes."""
import ctypes

import numpy as np
import pytest
import torch

import _gemv_exact as G

PERSIST = [c for c in G.CASES if c.cell[0] == "persist"]
FALLBACK = [c for c in G.CASES if c.cell[0] == "fallback"]
TGS, KSS = (1, 2, 4), (1, 2, 4, 8, 16)


def _lib():
    from quest_amd._lib import lib
    return lib


def _quads_per_round(ks):
    return G.WORKGROUPS * 16 // ks


def _last_round_full(c):
    quads = (G.virtual_rows(c) + 3) // 4
    return quads == c.cell[3] * _quads_per_round(c.cell[2])


def _spp(c):
    return (c.in_dim + 127) // 128


def test_case_ids_are_unique_and_cases_well_formed():
    assert len({G.case_id(c) for c in G.CASES}) == len(G.CASES)
    for c in G.CASES:
        assert c.entry in G.ENTRIES and c.in_dim % 8 == 0 and 0 <= c.n <= 16, c
        assert (c.n == 0) == (c.cell[0] == "batch1"), c
        assert G.virtual_rows(c) * c.in_dim * 2 <= 70 << 20, c     # weights of a case: tens of MB at the most
        if c.entry in ("rope", "rope_table"):
            assert c.head_dim % 16 == 0 and c.rows[0] % c.head_dim == 0 and c.rows[1] % c.head_dim == 0, c
        G.bit_budget(c)


def test_every_n_token_case_is_in_the_cell_the_table_claims():
    lib = _lib()
    for c in G.N_TOKEN_CASES:
        cell, info = G.planner_cell(lib, c)
        assert cell == c.cell, (G.case_id(c), cell)
        if cell[0] == "persist":
            assert info[3] == G.WORKGROUPS and info[4] == _spp(c) and info[5] == 4, (G.case_id(c), info)
        assert c.cell[1] == G.token_groups(c.n)


def test_persistent_cells_cover_every_tg_ks_round_shape():
    lib = _lib()
    for tg in TGS:
        for ks in KSS:
            mine = [c for c in PERSIST if c.cell[1:3] == (tg, ks)]
            rounds = {c.cell[3] for c in mine}
            assert 1 in rounds and any(r >= 3 and r % 2 for r in rounds), (tg, ks, rounds)
            if (tg, ks) not in ((2, 16), (4, 16)):
                assert 2 in rounds, (tg, ks, rounds)
            assert {_last_round_full(c) for c in mine} == {True, False}, (tg, ks)
            assert {c.entry for c in mine} == set(G.ENTRIES), (tg, ks)
    for ks in KSS:
        assert any(c.cell[3] >= 4 and c.cell[3] % 2 == 0 for c in PERSIST if c.cell[2] == ks), ks
    # (TG 2 | 4, ks 16) has no even round count to test: more than 4 tokens fit the kernel up to in_dim 4096, where ks = 16
    # is only ever the planner's move from ks = 8 to a fuller last round, and 2 m rounds of 256 quads fill exactly as
    # well as m rounds of 512.  Every such row length, every quad count up to 20 rounds:
    info = (ctypes.c_uint32 * 6)()
    for n in (8, 16):
        for spp in range(17, 33):
            for quads in range(1, 20 * 256 + 1):
                if lib.quest_decode_batched_plan(spp * 128, 4 * quads, n, 0, info) == 1 and info[0] == 16:
                    assert info[1] % 2 == 1, (n, spp, quads, list(info))
        assert lib.quest_decode_batched_plan(33 * 128, 4096, n, 0, info) == 0


def test_fallback_cells_cover_every_entry_and_tg():
    for tg in TGS:
        assert {c.entry for c in FALLBACK if c.cell[1] == tg} == set(G.ENTRIES), tg


def test_cases_that_must_be_present():
    assert any(c.in_dim % 128 for c in PERSIST)
    assert any(_spp(c) % c.cell[2] for c in PERSIST)
    assert {-(-_spp(c) // c.cell[2]) for c in PERSIST} >= {2, 3, 4}
    assert {c.n for c in PERSIST} >= {1, 3, 4, 5, 8, 9, 13, 16} and {c.n for c in FALLBACK} >= {1, 3, 4, 5, 8, 9, 13, 16}
    # ks = 16 with 17 k steps: 15 slices hold one step and one holds two (dead fragments of issue / consume)
    assert any(c.cell[2] == 16 and _spp(c) == 17 for c in PERSIST)
    # hidden sizes between 4096 and 8192 at both ends of the token group that fits
    assert {(c.in_dim, c.n) for c in PERSIST} >= {(5120, 1), (5120, 4), (8192, 1), (8192, 4)}
    for kind in (PERSIST, FALLBACK):
        for entry in ("plain_norm", "plain", "residual"):
            assert {c.rows[0] % 4 for c in kind if c.entry == entry} & {1, 2, 3}, entry
        assert {c.rows[0] % 4 for c in kind if c.entry in ("plain_norm", "plain", "residual")} >= {1, 2, 3}
        assert any(c.rows[0] % 2 for c in kind if c.entry == "gate_up")
        assert any(c.rows[0] % 4 and c.rows[1] % 4 for c in kind if c.entry == "qkv")   # a quad straddles two matrices
    assert {c.in_dim for c in FALLBACK} >= {8, 40}                                    # fewer k steps than waves
    big = {c.cell[1] for c in FALLBACK if c.in_dim > 8192 and c.in_dim % 128}
    assert big >= {1, 4}
    assert any(c.head_dim == 512 for c in FALLBACK if c.entry == "rope")
    assert any(c.head_dim == 512 for c in FALLBACK if c.entry == "rope_table")
    # rotation at head_dim 512 would otherwise be a persistent-kernel shape: the route, not the planner, sends it away
    info = (ctypes.c_uint32 * 6)()
    assert any(_lib().quest_decode_batched_plan(c.in_dim, G.virtual_rows(c), c.n, 1, info) == 1
               for c in FALLBACK if c.head_dim == 512)


def test_batch1_cases_cover_the_dispatch():
    for c in G.BATCH1_CASES:
        assert G.batch1_cell(c.entry, G.virtual_rows(c), c.in_dim) == c.cell, G.case_id(c)
        assert c.in_dim <= 30720
    # the thresholds themselves
    assert G.batch1_cell("plain", 8191, 512) == ("batch1", 1, 8) and G.batch1_cell("plain", 8192, 512) == ("batch1", 2, 4)
    assert G.batch1_cell("residual", 16383, 8) == ("batch1", 2, 4) and G.batch1_cell("residual", 16384, 8) == ("batch1", 4, 2)
    assert G.batch1_cell("gate_up", 16383, 8) == ("batch1", 2, 4) and G.batch1_cell("rope", 16384, 8) == ("batch1", 4, 2)
    # RW = 1 beyond 7 rounds of U = 8: both sides of the switch are cases
    assert {(c.in_dim, c.cell) for c in G.BATCH1_CASES} >= {(28672, ("batch1", 1, 8)), (28680, ("batch1", 1, 4))}
    classes = {"plain": ("plain_norm", "plain", "qkv"), "residual": ("residual",), "gate_up": ("gate_up",),
               "rotation": ("rope", "rope_table")}
    for name, entries in classes.items():
        shapes = ((1, 8), (2, 4), (4, 2)) if name in ("plain", "residual") else ((2, 4), (4, 2))
        for rw, u in shapes:
            mine = [c for c in G.BATCH1_CASES if c.entry in entries and c.cell == ("batch1", rw, u) and c.in_dim < 28672]
            rnd = u * 512
            assert any(c.in_dim < rnd and c.in_dim > 8 for c in mine), (name, rw, u)            # full == 0
            assert any(c.in_dim % rnd == 0 for c in mine), (name, rw, u)                        # whole rounds only
            assert any(c.in_dim > rnd and (c.in_dim % rnd) // 8 % 64 for c in mine), (name, rw, u)  # ragged tail
            assert any(c.in_dim == 8 for c in mine), (name, rw, u)
    assert {c.entry for c in G.BATCH1_CASES} == set(G.ENTRIES)
    for rw, u in ((1, 4), (2, 4)):                                                              # the staging limit
        assert any(c.in_dim == 30720 and c.cell == ("batch1", rw, u) for c in G.BATCH1_CASES)
    assert any(c.entry in ("rope", "rope_table") and c.cell == ("batch1", 4, 2) for c in G.BATCH1_CASES)


def _widest(in_dim=None, entry=None):
    """the table's case of that row length and / or entry with the longest rows and the most tokens"""
    return max((c for c in G.CASES if in_dim in (None, c.in_dim) and entry in (None, c.entry)), key=lambda c: (c.in_dim, c.n))


@pytest.mark.parametrize("case", [_widest(520), _widest(4104), _widest(11008), _widest(entry="gate_up"),
                                  _widest(entry="residual"), _widest(entry="rope_table")], ids=G.case_id)
def test_the_input_recipe_is_exact_in_every_order(case):
    """The construction the GPU file rests on, in numpy on the recipe's own tensors: fp32 sums of the products in three
    random orders equal the float64 sum; 1 / rms perturbed by +-2 fp32 ulp -- and computed with eps 0, 1e-6, 1e-5 --
    leaves the fp16 normalised input unchanged; mean(x ** 2) = 4 s_t ** 2 exactly."""
    d = G.make_inputs(case, "cpu", 7)
    x = d["x"].numpy()
    n, in_dim = x.shape
    s = np.array([2.0 ** (t % 4 - 1) for t in range(n)])
    assert np.array_equal((x.astype(np.float64) ** 2).mean(-1), 4 * s * s)
    assert not (x == 0).any()
    if d["gamma"] is not None:
        gam = d["gamma"].numpy().astype(np.float32)
        exact = (x.astype(np.float64) / (2 * s[:, None]) * gam.astype(np.float64)).astype(np.float16)
        assert np.array_equal(exact.astype(np.float64), x.astype(np.float64) / (2 * s[:, None]) * gam.astype(np.float64))
        for eps in (0.0, 1e-6, 1e-5):
            inv = (1.0 / np.sqrt((x.astype(np.float32) ** 2).mean(-1, dtype=np.float32) + np.float32(eps))).astype(np.float32)
            for k in (-2, -1, 0, 1, 2):
                inv_k = inv.copy()
                for _ in range(abs(k)):
                    inv_k = np.nextafter(inv_k, np.float32(np.inf if k > 0 else 0), dtype=np.float32)
                xn = (x.astype(np.float32) * inv_k[:, None] * gam).astype(np.float16)
                assert np.array_equal(xn, exact), (eps, k)
            assert np.array_equal(G.normalised(d["x"], d["gamma"], eps).numpy(), exact.astype(np.float64))
        xn = exact
    else:
        xn = x
    rng = np.random.default_rng(3)
    inexact = 0
    for w in d["w"]:
        w = w.numpy()[:24]
        for t in range(n):
            prod32 = xn[t].astype(np.float32)[None, :] * w.astype(np.float32)
            prod64 = xn[t].astype(np.float64)[None, :] * w.astype(np.float64)
            assert np.array_equal(prod32.astype(np.float64), prod64)
            want = prod64.sum(-1)
            for _ in range(3):
                perm = rng.permutation(in_dim)
                got = np.cumsum(prod32[:, perm], axis=-1, dtype=np.float32)      # sequential fp32, every partial sum
                assert np.array_equal(got[:, -1].astype(np.float64), want)
                assert np.array_equal(got.astype(np.float64), np.cumsum(prod64[:, perm], axis=-1))
            if case.entry == "residual":
                h = d["h"].numpy()[t, :24]
                tot = h.astype(np.float32) + want.astype(np.float32)
                assert np.array_equal(tot.astype(np.float64), h.astype(np.float64) + want)
                want = tot.astype(np.float64)
            inexact += int((want.astype(np.float16).astype(np.float64) != want).sum())
    if case.in_dim >= 11008:
        assert inexact > 0   # the final fp32 -> fp16 convert really rounds at these lengths


def test_reference_helpers():
    a = torch.tensor([1.0, -1.0, 0.0, -0.0, 2.0], dtype=torch.float16)
    b = torch.tensor([1.0009765625, -1.0, -0.0, 0.0, 2.0], dtype=torch.float16)
    assert G.ulp_distance(a, b).tolist() == [1, 0, 0, 0, 0]
    tiny = torch.tensor([6e-8, -6e-8], dtype=torch.float16)
    assert G.ulp_distance(tiny[:1], tiny[1:]).tolist() == [2]
    c = next(c for c in G.CASES if c.entry == "gate_up" and c.in_dim == 264)
    d = G.make_inputs(c, "cpu", 1)
    (ref,) = G.reference(c, d)
    xn = G.normalised(d["x"], d["gamma"])
    g, u = xn @ d["w"][0].double().T, xn @ d["w"][1].double().T
    assert torch.equal(ref, (torch.nn.functional.silu(g) * u).float().half())
    v = torch.arange(32, dtype=torch.float64)
    inv = G.formula_inv_freq(16, 1e4, "cpu")
    assert torch.equal(G.rotate(v, 0, 16, inv, 2.0), 2 * v)
