"""The bf16 form of the fused decode-layer GEMVs (csrc/decode_layer_kernels_typed.cuh compiled for bf16_t) bit for bit against
a float64 reference: test_gpu_decode_layer_exact.py over the same case table (tests/_gemv_exact.py), every planner cell and
batch-1 shape, with bf16 tensors.

The inputs are the fp16 suite's numbers -- all of them bf16 numbers too (tests/_gemv_exact_bf16.py) -- so every fp32 partial
sum is exact in every summation order and v_dot2c_f32_bf16, the bf16 4x4x4 MFMA, the reductions and a float64 matmul agree
bit for bit.  About one exact sum in seven needs rounding to 8 bits and one in ten is an exact tie, up and down
(test_gemv_exact_bf16_host.py counts them over 21 cases), so the comparison also catches an output that is truncated or
rounded half away from zero instead of to nearest even.  Outputs lie in buffers pre-filled with a bf16 NaN sentinel, with guard bands.

One family fp16 cannot hold: the inputs (and the residual) times 2 ** 16 -- outputs beyond 65504 for the launches without
a norm, sums of squares beyond fp16's range for the one with a norm; bit-equal again.

Rotation at non-zero positions, per element: one bf16 ulp of the float64 value + (|a| + |b|) * factor * e with the e derived
in test_gpu_bf16_kernels.py::test_rope_all_four_entries_within_one_ulp -- table form e = 2^-21 (the angle is the kernel's
own fp32 product), formula form e = 2^-21 + 2^-22 |angle| at theta = 2^19 (a power of two: the exponent of exp2f is
bit-identical on host and device)."""
import zlib

import pytest
import torch

import _gemv_exact as G
import _gemv_exact_bf16 as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THETA, FACTOR = 1e4, 2.0                      # rotation: the formula's base; the table form's attention factor
THETA_POW2 = 2.0 ** 19                        # the formula form at non-zero positions
POSITIONS = (8191, 131071, 4095, 70000)       # non-zero positions, one per token (t % 4)


def _seed(c):
    return zlib.crc32(G.case_id(c).encode()) & 0x7FFFFFFF


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_same_bits(got, want, what):
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: "
                             f"{float(got[i])!r} != {float(want[i])!r}")


def _out_sizes(c):
    return [c.rows[0]] if len(c.rows) == 1 else [c.rows[0], c.rows[1], c.rows[1]]


def _states(pos):
    st = torch.tensor([[p + 1, 1, 1, 0, 1, 1, 0, 0] for p in pos], dtype=torch.int32, device=DEV)  # seq_len = pos + 1
    return st.contiguous()


def _raw(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def run(c, d, token=None, pos=None, theta=THETA):
    """One launch of the case over the bf16 tensors `d`: the n-token entry, or with `token` the single-token entry on that
    token.  Checks the guard bands, that no sentinel is left inside an output and that the launch left its inputs alone;
    returns the outputs as [tokens, rows_i] bf16 tensors."""
    from quest_amd import _kernels as K

    n_all = d["x"].shape[0]
    n = n_all if token is None else 1
    x = d["x"] if token is None else d["x"][token]
    sizes = _out_sizes(c)
    bufs = [torch.full((n * s + 2 * G.GUARD,), B.SENTINEL, dtype=torch.int16, device=DEV) for s in sizes]
    outs = [b[G.GUARD:G.GUARD + n * s].view(torch.bfloat16) for b, s in zip(bufs, sizes)]
    if c.entry == "residual":
        outs[0].copy_((d["h"] if token is None else d["h"][token]).reshape(-1))
    states = _states(list(pos) if pos is not None else [0] * n_all)
    if token is not None:
        states = states[token]
    inv_freq = G.formula_inv_freq(c.head_dim, THETA, DEV) if c.entry == "rope_table" else None
    inputs = [t for t in [d["x"], d["gamma"], states, inv_freq] + d["w"] if t is not None]
    before = [t.clone() for t in inputs]
    w, gamma = d["w"], d["gamma"]
    if c.entry in ("plain_norm", "plain"):
        (K.decode_norm_gemv_batched if token is None else K.decode_norm_gemv)(x, gamma, G.EPS, w[0], outs[0])
    elif c.entry == "residual":
        (K.decode_gemv_residual_batched if token is None else K.decode_gemv_residual)(x, w[0], outs[0])
    elif c.entry == "gate_up":
        (K.decode_mlp_gate_up_batched if token is None else K.decode_mlp_gate_up)(x, gamma, G.EPS, w[0], w[1], outs[0])
    elif c.entry == "qkv":
        (K.decode_qkv_batched if token is None else K.decode_qkv)(x, gamma, G.EPS, *w, *outs)
    elif c.entry == "rope":
        (K.decode_qkv_rope_batched if token is None else K.decode_qkv_rope)(x, gamma, G.EPS, *w, *outs, c.head_dim, 1.0,
                                                                            theta, states)
    else:
        (K.decode_qkv_rope_batched_freqs if token is None else K.decode_qkv_rope_freqs)(x, gamma, G.EPS, *w, *outs,
                                                                                        c.head_dim, inv_freq, FACTOR, states)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        assert bool((b[:G.GUARD] == B.SENTINEL).all()) and bool((b[-G.GUARD:] == B.SENTINEL).all()), f"guard band of output {i}"
        if c.entry != "residual":   # in place: every element was data before the launch
            left = int((b[G.GUARD:-G.GUARD] == B.SENTINEL).sum())
            assert left == 0, f"{left} elements of output {i} were never written"
    for t, t0 in zip(inputs, before):
        assert torch.equal(_raw(t), _raw(t0)), "a launch wrote to its inputs"
    return [o.clone().view(n, s) for o, s in zip(outs, sizes)]


def _expected(c, d, sums):
    """position-0 expectations: the table form's cos = attention factor, an exact doubling of q and k"""
    ref = B.reference(c, d, sums)
    if c.entry == "rope_table":
        ref = [B.to_bf16(FACTOR * sums[0]), B.to_bf16(FACTOR * sums[1]), ref[2]]
    return ref


def _assert_matches(c, outs, ref, what):
    for i, (o, r) in enumerate(zip(outs, ref)):
        if c.entry == "gate_up":  # correctly rounded or its neighbour (the fp32 epilogue errs by ~2e-6 relative at |g| <= 20)
            dist = G.ulp_distance(o, r)
            print(f"{what}: gate / up worst distance {int(dist.max())} bf16 ulp")
            assert int(dist.max()) <= 1, f"{what}: {int((dist > 1).sum())} elements further than 1 ulp, max {int(dist.max())}"
        else:
            _assert_same_bits(o, r, f"{what} output {i}")


def _assert_rotated(c, outs, sums, pos, tokens, what):
    """non-zero positions: float64 rotation of the exact row sums by the kernel's own fp32 angle, v exact.  Bound: see the
    module docstring."""
    if c.entry == "rope_table":
        inv_freq, factor, freq_rel = G.formula_inv_freq(c.head_dim, THETA, DEV), FACTOR, 0.0
    else:  # the formula at theta = 2^19: exp2 of the exact fp32 argument -19 * 2 i / D, as the kernel forms it
        i2 = (2 * torch.arange(c.head_dim // 2, device=DEV)).float()
        inv_freq, factor, freq_rel = torch.exp2(torch.tensor(-19.0, device=DEV) * i2 / float(c.head_dim)), 1.0, 2.0 ** -22
    worst = 0.0
    for row, t in enumerate(tokens):
        ang = (torch.tensor(float(pos[t]), device=DEV, dtype=torch.float32) * inv_freq).double().abs()
        for i in (0, 1):
            v = sums[i][t].reshape(-1, c.head_dim)
            mag = v[:, : c.head_dim // 2].abs() + v[:, c.head_dim // 2:].abs()
            mag, ang2 = torch.cat([mag, mag], 1).reshape(-1), torch.cat([ang, ang]).repeat(v.shape[0])
            want = G.rotate(sums[i][t], pos[t], c.head_dim, inv_freq, factor)
            bound = B.ulp_bf16(want) + mag * factor * (2.0 ** -21 + freq_rel * ang2)
            err = (outs[i][row].double() - want).abs()
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), f"{what} token {t} output {i}: worst err / bound {float((err / bound).max()):.3f}"
        _assert_same_bits(outs[2][row], B.to_bf16(sums[2][t]), f"{what} token {t} v")
    print(f"{what}: rotation at {[pos[t] for t in tokens]} worst err / bound {worst:.3f}")


def _rotated_positions(c, d, sums, tokens, what, token=None):
    n = d["x"].shape[0]
    pos = [POSITIONS[t % 4] for t in range(n)] if token is None else [POSITIONS[1]] * n
    theta = THETA if c.entry == "rope_table" else THETA_POW2
    _assert_rotated(c, run(c, d, token=token, pos=pos, theta=theta), sums, pos, tokens, what)


def _assert_cell_on_device(c):
    from quest_amd._lib import lib

    cell, info = G.planner_cell(lib, c)
    assert cell == c.cell, f"the planner of this device puts {G.case_id(c)} in {cell} (info {info})"


@pytest.mark.parametrize("c", G.N_TOKEN_CASES, ids=G.case_id)
def test_n_token_launch_is_exact(c):
    _assert_cell_on_device(c)
    G.bit_budget(c)
    d = B.make_inputs(c, DEV, _seed(c))
    sums = B.exact_sums(c, d)
    ref = _expected(c, d, sums)
    outs = run(c, d)
    _assert_matches(c, outs, ref, "n-token launch")
    # a second launch over the same inputs: the same bits
    again = run(c, d)
    for o, a in zip(outs, again):
        _assert_same_bits(a, o, "second launch")
    # the single-token launch on a token = that token's row of the n-token launch
    for t in {0, c.n - 1}:
        one = run(c, d, token=t)
        for o, s in zip(outs, one):
            _assert_same_bits(s[0], o[t], f"single-token launch on token {t}")
    # tokens do not take each other's 1 / rms, position or rows: no token's output is another token's reference
    if G.NORM[c.entry] and c.n > 1 and c.entry != "gate_up":
        same = (_bits(outs[0])[:, None, :] == _bits(ref[0])[None, :, :]).all(-1)
        assert torch.equal(same, torch.eye(c.n, dtype=torch.bool, device=DEV)), same.tolist()
    if c.entry in ("rope", "rope_table"):
        _rotated_positions(c, d, sums, range(c.n), "n-token launch")


@pytest.mark.parametrize("c", G.BATCH1_CASES, ids=G.case_id)
def test_single_token_launch_is_exact(c):
    G.bit_budget(c)
    d = B.make_inputs(c, DEV, _seed(c))
    sums = B.exact_sums(c, d)
    ref = _expected(c, d, sums)
    outs = run(c, d, token=0)
    _assert_matches(c, outs, ref, "single-token launch")
    for o, a in zip(outs, run(c, d, token=0)):
        _assert_same_bits(a, o, "second launch")
    if c.entry in ("rope", "rope_table"):
        _rotated_positions(c, d, sums, [0], "single-token launch", token=0)


# ---------------------------------------------------------------------------------------------------------------------
# Beyond fp16's range: inputs and residual times 2 ** 16
@pytest.mark.parametrize("c", B.scaled_cases(), ids=G.case_id)
def test_launch_is_exact_beyond_fp16_range(c):
    if c.n:
        _assert_cell_on_device(c)
    G.bit_budget(c)   # a power-of-two scale moves no significand
    d = B.make_inputs(c, DEV, _seed(c), scale_exp=B.SCALE_EXP)
    assert float(d["x"].float().abs().min()) > 65504.0 / 2   # s_t >= 1/2: every input element is 2 ** 15 at least
    sums = B.exact_sums(c, d)
    ref = _expected(c, d, sums)
    if G.NORM[c.entry]:   # the sum of squares leaves fp16, the normalised input does not
        assert float(d["x"].float().pow(2).sum(-1).min()) > 65504.0 and float(B.normalised(d["x"], d["gamma"]).abs().max()) <= 2.25
    else:
        assert float(ref[0].float().abs().max()) > 65504.0
    token = None if c.n else 0
    outs = run(c, d, token=token)
    _assert_matches(c, outs, ref, "2 ** 16 launch")
    assert bool(torch.isfinite(outs[0].float()).all())
    if c.n:
        one = run(c, d, token=c.n - 1)
        _assert_same_bits(one[0][0], outs[0][c.n - 1], f"single-token launch on token {c.n - 1}")


# ---------------------------------------------------------------------------------------------------------------------
# Isolation: one case per (entry, n-token kernel, TG).  Small weights; row counts that leave dead rows in the last quad.
ISOLATION_TOKENS = {1: 3, 2: 7, 4: 14}
ISOLATION_CASES = []
for _entry in G.ENTRIES:
    for _tg, _n in ISOLATION_TOKENS.items():
        for _kernel, _in_dim in (("persist", 520), ("fallback", 264)):
            _rows, _hd = G.entry_rows(_entry, 9)
            _cell = ("persist", _tg, 2, 1) if _kernel == "persist" else ("fallback", _tg)
            ISOLATION_CASES.append(G.Case(_entry, _n, _in_dim, _rows, _hd, _cell))


def _pair_rows(c, mat, row):
    """output (matrix, row)s that weight row `row` of matrix `mat` feeds"""
    if c.entry == "gate_up":
        return {(0, row)}
    if c.entry in ("rope", "rope_table") and mat < 2:
        head, j = divmod(row, c.head_dim)
        return {(mat, row), (mat, head * c.head_dim + (j + c.head_dim // 2) % c.head_dim)}
    return {(mat, row)}


def _assert_only(c, base, got, touched, what):
    """`got` equals `base` bit for bit except in the (matrix, row) columns `touched`, which are non-finite for every token"""
    for i, (b, g) in enumerate(zip(base, got)):
        keep = torch.ones(b.shape[1], dtype=torch.bool, device=DEV)
        for m, r in touched:
            if m == i:
                keep[r] = False
        _assert_same_bits(g[:, keep], b[:, keep], f"{what}: untouched rows of output {i}")
        assert not bool(torch.isfinite(g[:, ~keep].float()).any()), f"{what}: a poisoned row of output {i} came out finite"


@pytest.mark.parametrize("c", ISOLATION_CASES, ids=G.case_id)
def test_tokens_and_rows_are_isolated(c):
    _assert_cell_on_device(c)
    d = B.make_inputs(c, DEV, _seed(c))
    assert not bool((d["x"] == 0).any())
    base = run(c, d)
    alternating = torch.where(torch.arange(c.in_dim, device=DEV) % 2 == 0, float("inf"), float("-inf")).bfloat16()
    for victim in (0, c.n // 2):   # token 0 is also what the dead token slots of a ragged group read
        others = torch.ones(c.n, dtype=torch.bool, device=DEV)
        others[victim] = False
        for name, poison in (("nan", torch.full((c.in_dim,), float("nan"), device=DEV, dtype=torch.bfloat16)),
                             ("+-inf", alternating)):
            dp = dict(d, x=d["x"].clone())
            dp["x"][victim] = poison
            got = run(c, dp)
            for i, (b, g) in enumerate(zip(base, got)):
                _assert_same_bits(g[others], b[others], f"token {victim} = {name}: the other tokens' output {i}")
                assert not bool(torch.isfinite(g[victim].float()).any()), f"token {victim} = {name}: output {i} came out finite"
    # one weight row = inf: only its output row (its rotation pair; the gate / up pair's output) changes
    mat = 0 if c.entry in ("rope", "rope_table") else len(d["w"]) - 1
    for row in (5, d["w"][mat].shape[0] - 1):
        dp = dict(d, w=[w.clone() for w in d["w"]])
        dp["w"][mat][row] = float("inf")
        _assert_only(c, base, run(c, dp), _pair_rows(c, mat, row), f"row {row} of matrix {mat} = inf")
    # row 0 of matrix 0 is what dead rows and dead quads read (masked at the store): nothing else may change
    dp = dict(d, w=[w.clone() for w in d["w"]])
    dp["w"][0][0] = float("inf")
    assert c.entry in ("rope", "rope_table") or G.virtual_rows(c) % 4 != 0
    _assert_only(c, base, run(c, dp), _pair_rows(c, 0, 0), "row 0 of matrix 0 = inf")
