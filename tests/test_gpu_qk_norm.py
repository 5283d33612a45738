"""The per-head q/k RMSNorm + RoPE launch (csrc/rope_norm.hip qk_norm_rope_kernel) against transformers' Qwen3RMSNorm +
apply_rotary_pos_emb in fp32 (tests/golden/qk_norm_rope.npz; no transformers at run time), its three row-position forms
against each other, and the unrotated q/k/v projection launches against the rotating ones and fp32.

Measured worst errors are printed (pytest -s) and, when QUEST_QK_NORM_PARITY_FILE names a file, appended to it, as
tests/_bf16.py does for profiles/bf16_parity.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _qk_norm import CASES, CONFIGS, DTYPES, EPS, inputs, quest_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qk_norm_rope.npz")
FORMULA_MAX_POS = 4096  # see test_fixture_fp16


def record(line: str) -> None:
    print(line)
    path = os.environ.get("QUEST_QK_NORM_PARITY_FILE")
    if path:
        new = not os.path.exists(path)
        with open(path, "a") as f:
            if new:
                f.write("# written by tests/test_gpu_qk_norm.py (record()) with\n"
                        "# QUEST_QK_NORM_PARITY_FILE=<this file> pytest tests/test_gpu_qk_norm.py -m gpu\n"
                        "# one line per measurement: <test case> | <figures>; the bars are in the tests' docstrings\n")
            case = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].replace("tests/", "")
            f.write(f"{case} | {line}\n")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _table(name):
    from quest_amd.models import rope

    return rope.device_rope_parameters(quest_config(name), torch.device(DEV))


def _dev(a_f16: np.ndarray, dtype: str) -> torch.Tensor:
    """fp16 data (bf16 variant: of bf16-representable values) as a device tensor of the variant's type (exact)."""
    t = torch.from_numpy(np.ascontiguousarray(a_f16)).to(DEV)
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _launch(q, k, wq, wk, name, past, form="table", states=None):
    from quest_amd import _kernels

    if form == "table":
        inv_freq, factor = _table(name)
        _kernels.apply_qk_norm_rope_in_place(q, k, wq, wk, EPS, past_kv_len=past, inv_freq=inv_freq, attention_factor=factor,
                                             states=states)
    else:
        _kernels.apply_qk_norm_rope_in_place(q, k, wq, wk, EPS, past_kv_len=past, rope_scale=1.0,
                                             rope_theta=CONFIGS[name][4], states=states)


def _run_case(golden, ci, name, i, dtype, form="table"):
    past, n = CASES[i]
    q, k, wq, wk = (_dev(a, dtype) for a in inputs(ci, i, dtype))
    _launch(q, k, wq, wk, name, past, form)
    want_q = torch.from_numpy(golden[f"{name}_{dtype}_q_{past}_{n}"])
    want_k = torch.from_numpy(golden[f"{name}_{dtype}_k_{past}_{n}"])
    return (q.float().cpu(), want_q), (k.float().cpu(), want_k)


@pytest.mark.parametrize("ci,name", list(enumerate(CONFIGS)))
def test_fixture_fp16(golden, ci, name):
    """Every (past, n) of the fixture -- the last row at position 131071 -- at the bar tests/test_gpu_rope_scaling.py uses
    for RoPE: rtol = atol = 5e-3, atol times attention_factor.  Frequencies through the table form, which is how the
    models run them (models/rope.py: also the default RoPE of qwen3 / mistral).  The formula form (no table) is held to
    the same bar on the default-frequency configs at positions up to 4096 only, in addition: its exp2f frequency differs
    from transformers' pow by up to 8e-7 relative (one fp32 ulp of the highest frequencies), which times the position is an
    angle error of 2.4e-4 rad at 4096 but 0.008 rad at 131071 -- 0.03 on an output of magnitude 4, past this bar.  That is
    a property of the formula form, which tests/test_gpu_parity.py's RoPE fixture (positions < 1200) never met."""
    assert golden["cases"].tolist() == [list(c) for c in CASES]
    factor = float(golden[f"{name}_attention_factor"])
    tol = dict(rtol=5e-3, atol=5e-3 * factor)
    worst = 0.0
    for i, (past, n) in enumerate(CASES):
        for got, want in _run_case(golden, ci, name, i, "fp16"):
            err = float(((got - want).abs() / (tol["atol"] + tol["rtol"] * want.abs())).max())
            worst = max(worst, err)
            record(f"fp16 {name} past {past} n {n}: worst |err| / (atol + rtol |ref|) {err:.4f}, worst |err| "
                   f"{float((got - want).abs().max()):.3e}")
            torch.testing.assert_close(got, want, **tol)
        if CONFIGS[name][5] is None and past + n <= FORMULA_MAX_POS:
            for got, want in _run_case(golden, ci, name, i, "fp16", form="formula"):
                record(f"fp16 {name} past {past} n {n} formula form: worst |err| {float((got - want).abs().max()):.3e}")
                torch.testing.assert_close(got, want, **tol)
    record(f"fp16 {name}: WORST |err| / (atol + rtol |ref|) over the fixture {worst:.4f} (bar 1)")


def _norm64(x, w):
    """x * w / rms(x) per head row in fp64: the magnitudes the rotation mixes."""
    x = x.astype(np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + EPS) * w.astype(np.float64)


def _ulp_bf16(x):
    """One bf16 ulp at |x| (8 significant bits), never below the smallest normal's."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 7)


@pytest.mark.parametrize("ci,name", list(enumerate(CONFIGS)))
def test_fixture_bf16(golden, ci, name):
    """bf16 in, bf16 out, against the same fp32 transformers computation on the same real numbers.

    Bound, per element: one bf16 ulp of the reference value + (|n_d| + |n_partner|) * attention_factor * (2^-21 + 2^-19),
    n = x w / rms(x) the normalised pair the rotation mixes (restated in fp64 from the inputs).
      - One ulp: the kernel rounds its fp32 result once (half an ulp) and the reference is itself an fp32 value.
      - 2^-21 (|n_d| + |n_partner|) attention_factor: the rotation, the term of the bf16 RoPE bound in
        tests/test_gpu_bf16_kernels.py (sincosf: a few fp32 ulp of values <= 1; the two products and the sum; the angle is
        the table's single fp32 product, transformers' bit for bit, so there is no frequency term).  It is needed where the
        two products cancel and the ulp of the result is arbitrarily small.
      - 2^-19 (...): the normalisation, which the rotation carries through linearly.  Kernel: sum of squares = an fma
        chain of 8 and a tree of log2(D / 8) <= 5 levels over positive terms, so each term meets at most 13 roundings:
        relative error <= 13 u (u = 2^-24); / D is exact, + eps, sqrtf, the reciprocal: one rounding each, and the square
        root halves what came before: inv within (13 / 2 + 1 / 2 + 1 + 1) u = 9 u; x * inv * w: two more, n within 11 u
        < 2^-20.  The fp32 reference (pow, mean, + eps, rsqrt, two products, in torch's summation order) has the same
        structure: another 2^-20.  Together 2^-19.
    For |n| ~ 1 the fp32 terms are 2.4e-6 against a bf16 ulp of 4e-3 to 8e-3: the bar is one ulp wherever nothing cancels."""
    factor = float(golden[f"{name}_attention_factor"])
    d = CONFIGS[name][0]
    worst_b, worst_u = 0.0, 0.0
    for i, (past, n) in enumerate(CASES):
        q, k, wq, wk = inputs(ci, i, "bf16")
        res = _run_case(golden, ci, name, i, "bf16")
        for (got, want), x, w in zip(res, (q, k), (wq, wk)):
            nrm = _norm64(x.astype(np.float32), w.astype(np.float32))
            mag = np.abs(nrm) + np.abs(np.roll(nrm, d // 2, axis=-1))
            ref = want.numpy().astype(np.float64)
            err = np.abs(got.numpy().astype(np.float64) - ref)
            bound = _ulp_bf16(ref) + mag * factor * (2.0 ** -21 + 2.0 ** -19)
            rb, ru = float((err / bound).max()), float((err / _ulp_bf16(ref)).max())
            worst_b, worst_u = max(worst_b, rb), max(worst_u, ru)
            record(f"bf16 {name} past {past} n {n}: worst err / bound {rb:.3f}, worst err / ulp {ru:.3f}")
            assert (err <= bound).all(), (name, past, n, rb)
    record(f"bf16 {name}: WORST err / bound over the fixture {worst_b:.3f} (bar 1), worst err / ulp {worst_u:.3f}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("form", ["table", "formula"])
def test_state_and_batched_forms_equal_the_eager_form(name, dtype, form):
    """states[i].seq_len - 1 as the position of row i: one state, and a batch of states of different lengths (more rows than
    one workgroup holds), bit for bit the eager launch at the same positions -- i.e. batched == per-sequence."""
    d, hq, hkv = CONFIGS[name][:3]
    g = torch.Generator(device=DEV).manual_seed(11)
    wq = (1 + 0.5 * torch.randn(d, generator=g, device=DEV)).to(dtype)
    wk = (1 + 0.5 * torch.randn(d, generator=g, device=DEV)).to(dtype)
    for lens in ([131072], [1, 4096, 8192, 131072, 77, 32760, 5, 40000, 16, 17, 100000]):
        n = len(lens)
        q = (3 * torch.randn(n, hq, d, generator=g, device=DEV)).to(dtype)
        k = (0.3 * torch.randn(n, hkv, d, generator=g, device=DEV)).to(dtype)
        states = torch.zeros(n, 8, dtype=torch.int32, device=DEV)
        states[:, 0] = torch.tensor(lens, dtype=torch.int32)
        qs, ks = q.clone(), k.clone()
        _launch(qs, ks, wq, wk, name, 0, form, states=states)
        assert not torch.equal(qs, q) and torch.isfinite(qs.float()).all() and torch.isfinite(ks.float()).all()
        for i, L in enumerate(lens):
            qe, ke = q[i:i + 1].clone(), k[i:i + 1].clone()
            _launch(qe, ke, wq, wk, name, L - 1, form)
            assert torch.equal(qs[i:i + 1], qe) and torch.equal(ks[i:i + 1], ke), (name, L)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("d,hq,hkv,n", [(64, 4, 2, 5), (128, 8, 2, 3), (128, 2, 2, 1), (256, 3, 1, 7)])
def test_in_place_touches_only_its_own_rows(d, hq, hkv, n, dtype):
    """q and k sit in ONE allocation between poisoned guard rows: [guard | q | guard | k | guard].  After the launch the
    guards hold their bytes, and rotating q (with a dummy k elsewhere) leaves k's rows alone and vice versa."""
    from quest_amd import _kernels

    g = torch.Generator(device=DEV).manual_seed(d + n)
    guard = 2 * d
    nq, nk = n * hq * d, n * hkv * d
    buf = torch.full((3 * guard + nq + nk,), 777.0, device=DEV, dtype=dtype)
    q = buf[guard:guard + nq].view(n, hq, d)
    k = buf[2 * guard + nq:2 * guard + nq + nk].view(n, hkv, d)
    q.copy_(torch.randn(n, hq, d, generator=g, device=DEV))
    k.copy_(torch.randn(n, hkv, d, generator=g, device=DEV))
    wq = (1 + 0.5 * torch.randn(d, generator=g, device=DEV)).to(dtype)
    wk = (1 + 0.5 * torch.randn(d, generator=g, device=DEV)).to(dtype)
    q0, k0 = q.clone(), k.clone()
    both_q, both_k = q0.clone(), k0.clone()
    _kernels.apply_qk_norm_rope_in_place(both_q, both_k, wq, wk, EPS, past_kv_len=9)
    _kernels.apply_qk_norm_rope_in_place(q, k, wq, wk, EPS, past_kv_len=9)
    assert torch.equal(q, both_q) and torch.equal(k, both_k)
    for lo, hi in ((0, guard), (guard + nq, 2 * guard + nq), (2 * guard + nq + nk, buf.numel())):
        assert bool((buf[lo:hi] == 777.0).all()), (lo, hi)
    assert not torch.equal(q, q0) and not torch.equal(k, k0)
    # one side at a time: a poisoned stand-in takes the other side's place and the real tensor keeps its bytes
    for side in ("q", "k"):
        qq, kk = q0.clone(), k0.clone()
        other = torch.full_like(k0 if side == "q" else q0, 777.0)
        keep = (kk if side == "q" else qq).clone()
        if side == "q":
            _kernels.apply_qk_norm_rope_in_place(qq, other, wq, wk, EPS, past_kv_len=9)
            assert torch.equal(qq, both_q) and torch.equal(kk, keep)
        else:
            _kernels.apply_qk_norm_rope_in_place(other, kk, wq, wk, EPS, past_kv_len=9)
            assert torch.equal(kk, both_k) and torch.equal(qq, keep)


def test_shim_argument_errors():
    from quest_amd import _kernels

    inv_freq, factor = _table("qwen3_default_mha")
    q = torch.zeros(2, 4, 128, device=DEV, dtype=torch.float16)
    k = torch.zeros(2, 2, 128, device=DEV, dtype=torch.float16)
    w = torch.ones(128, device=DEV, dtype=torch.float16)
    for bad in (w.bfloat16(), w.float(), torch.ones(64, device=DEV, dtype=torch.float16), w.cpu(),
                torch.ones(256, device=DEV, dtype=torch.float16)[::2], torch.ones(1, 128, device=DEV, dtype=torch.float16)):
        with pytest.raises(RuntimeError):
            _kernels.apply_qk_norm_rope_in_place(q, k, bad, w, EPS)
        with pytest.raises(RuntimeError):
            _kernels.apply_qk_norm_rope_in_place(q, k, w, bad, EPS)
    with pytest.raises(RuntimeError):  # one element type per call
        _kernels.apply_qk_norm_rope_in_place(q, k.bfloat16(), w, w, EPS)
    with pytest.raises(RuntimeError):
        _kernels.apply_qk_norm_rope_in_place(q.float(), k.float(), w.float(), w.float(), EPS)
    with pytest.raises(RuntimeError):
        _kernels.apply_qk_norm_rope_in_place(q, k, w, w, EPS, inv_freq=inv_freq[:32].clone())
    with pytest.raises(RuntimeError):  # states of the wrong size
        _kernels.apply_qk_norm_rope_in_place(q, k, w, w, EPS, states=torch.ones(1, 8, dtype=torch.int32, device=DEV))
    for kw in (dict(eps=-1.0), dict(eps=float("nan")), dict(eps=EPS, inv_freq=inv_freq, attention_factor=0.0),
               dict(eps=EPS, rope_theta=0.0)):
        eps = kw.pop("eps")
        with pytest.raises(ValueError):  # QUEST_EINVAL from the entry
            _kernels.apply_qk_norm_rope_in_place(q, k, w, w, eps, **kw)
    q96 = torch.zeros(2, 4, 96, device=DEV, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="-2"):  # QUEST_EUNSUPPORTED
        _kernels.apply_qk_norm_rope_in_place(q96, q96.clone(), w[:96].clone(), w[:96].clone(), EPS)
    assert not q.any() and not k.any()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- the unrotated q/k/v projection launches
def _weights(g, hidden, q_rows, kv_rows):
    s = 1.0 / hidden ** 0.5
    gamma = (1 + 0.1 * torch.randn(hidden, generator=g, device=DEV, dtype=torch.float16)).contiguous()
    w = [(torch.randn(r, hidden, generator=g, device=DEV, dtype=torch.float16) * s).contiguous()
         for r in (q_rows, kv_rows, kv_rows)]
    return gamma, w


def _rms_rows(x, g, eps):
    x = x.float()
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g.float()).half().float()


def _outs(n, hq, hkv, d):
    return [torch.full((n, r, d), 777.0, device=DEV, dtype=torch.float16) for r in (hq, hkv, hkv)]


@pytest.mark.parametrize("hidden,hq,hkv,d", [(4096, 32, 8, 128), (2560, 32, 8, 128), (5120, 32, 8, 128), (512, 4, 2, 64),
                                              (640, 4, 2, 128), (1024, 2, 1, 256)])
def test_decode_qkv_vs_rotating_launch_and_fp32(hidden, hq, hkv, d):
    """One token: v == the v of quest_decode_qkv_rope bit for bit; q and k (unrotated) against fp32 at the tolerances of
    tests/test_gpu_decode_layer.py::test_qkv_rope_vs_fp32 (rtol 5e-3, atol 8e-3); q at position 0, where the rotation is
    the identity, also equals the rotating launch's q bit for bit."""
    from quest_amd import _kernels

    g = torch.Generator(device=DEV).manual_seed(hidden + d)
    gamma, (wq, wk, wv) = _weights(g, hidden, hq * d, hkv * d)
    h = torch.randn(hidden, generator=g, device=DEV, dtype=torch.float16)
    q, k, v = _outs(1, hq, hkv, d)
    _kernels.decode_qkv(h, gamma, 1e-5, wq, wk, wv, q, k, v)
    qr, kr, vr = _outs(1, hq, hkv, d)
    state = torch.tensor([1, 1, 1, 0, 1, 1, 0, 0], dtype=torch.int32, device=DEV)  # seq_len 1: position 0
    _kernels.decode_qkv_rope(h, gamma, 1e-5, wq, wk, wv, qr, kr, vr, d, 1.0, 1e4, state)
    assert torch.equal(v, vr)
    assert torch.equal(q, qr) and torch.equal(k, kr)
    nrm = _rms_rows(h, gamma, 1e-5)
    tol = dict(rtol=5e-3, atol=8e-3)
    torch.testing.assert_close(q.float().view(-1), wq.float() @ nrm, **tol)
    torch.testing.assert_close(k.float().view(-1), wk.float() @ nrm, **tol)
    torch.testing.assert_close(v.float().view(-1), wv.float() @ nrm, **tol)


@pytest.mark.parametrize("n", [1, 3, 8, 16])
@pytest.mark.parametrize("hidden,hq,hkv,d,persistent", [
    (4096, 32, 8, 128, 1),    # Qwen3-8B: the persistent kernel
    (2560, 32, 8, 128, 1),    # Qwen3-4B: q rows (4096) != hidden
    (8704, 8, 2, 128, 0),     # inputs too long for its LDS: the inputs-from-L2 kernel
    (512, 4, 2, 64, 1),       # the tiny test model
])
def test_decode_qkv_batched_vs_rotating_launch_and_fp32(n, hidden, hq, hkv, d, persistent):
    """n tokens, both n-token kernels (asserted with quest_decode_batched_plan, for this launch and for the rotating one it
    is compared with): v bit for bit the rotating launch's, q / k / v against fp32 at
    tests/test_gpu_decode_layer.py::test_batched_qkv_rope_vs_fp32's tolerances."""
    from quest_amd import _kernels
    from quest_amd._lib import lib

    rows = (hq + 2 * hkv) * d
    info = (ctypes.c_uint32 * 6)()
    assert lib.quest_decode_batched_plan(hidden, rows, n, 0, info) == persistent
    assert lib.quest_decode_batched_plan(hidden, rows, n, 1, info) == persistent
    g = torch.Generator(device=DEV).manual_seed(hidden + n)
    gamma, (wq, wk, wv) = _weights(g, hidden, hq * d, hkv * d)
    h = torch.randn(n, hidden, generator=g, device=DEV, dtype=torch.float16)
    q, k, v = _outs(n, hq, hkv, d)
    _kernels.decode_qkv_batched(h, gamma, 1e-5, wq, wk, wv, q, k, v)
    qr, kr, vr = _outs(n, hq, hkv, d)
    states = torch.zeros(n, 8, dtype=torch.int32, device=DEV)
    states[:, 0] = 1
    _kernels.decode_qkv_rope_batched(h, gamma, 1e-5, wq, wk, wv, qr, kr, vr, d, 1.0, 1e4, states)
    assert torch.equal(v, vr)
    assert torch.equal(q, qr) and torch.equal(k, kr)  # position 0: the rotation is the identity
    nrm = _rms_rows(h, gamma, 1e-5)
    tol = dict(rtol=5e-3, atol=8e-3)
    torch.testing.assert_close(q.float().view(n, -1), nrm @ wq.float().T, **tol)
    torch.testing.assert_close(k.float().view(n, -1), nrm @ wk.float().T, **tol)
    torch.testing.assert_close(v.float().view(n, -1), nrm @ wv.float().T, **tol)


@pytest.mark.parametrize("n", [1, 3, 8, 16])
def test_batched_launches_with_a_norm_prologue_are_reproducible(n):
    """The n-token launches normalise their inputs in a prologue that every workgroup runs on its own.  Its per-token sum
    of squares is added in a fixed order, so that launching again over the same inputs -- the unrotated launch, the rotating
    one, and one after the other -- gives the same bits every time (Qwen3-8B shapes: the persistent kernel)."""
    from quest_amd import _kernels

    hidden, hq, hkv, d = 4096, 32, 8, 128
    g = torch.Generator(device=DEV).manual_seed(77 + n)
    gamma, (wq, wk, wv) = _weights(g, hidden, hq * d, hkv * d)
    h = torch.randn(n, hidden, generator=g, device=DEV, dtype=torch.float16)
    states = torch.zeros(n, 8, dtype=torch.int32, device=DEV)
    states[:, 0] = 1
    first = None
    for rep in range(12):
        q, k, v = _outs(n, hq, hkv, d)
        if rep % 2:
            _kernels.decode_qkv_rope_batched(h, gamma, 1e-5, wq, wk, wv, q, k, v, d, 1.0, 1e4, states)
        else:
            _kernels.decode_qkv_batched(h, gamma, 1e-5, wq, wk, wv, q, k, v)
        if first is None:
            first = (q, k, v)
        assert torch.equal(q, first[0]) and torch.equal(k, first[1]) and torch.equal(v, first[2]), rep


def test_decode_qkv_shim_refuses_bf16_and_wrong_shapes():
    from quest_amd import _kernels

    g = torch.Generator(device=DEV).manual_seed(2)
    gamma, (wq, wk, wv) = _weights(g, 512, 256, 128)
    h = torch.zeros(512, device=DEV, dtype=torch.float16)
    q, k, v = _outs(1, 4, 2, 64)
    with pytest.raises(RuntimeError):
        _kernels.decode_qkv(h.bfloat16(), gamma, 1e-5, wq, wk, wv, q, k, v)
    with pytest.raises(RuntimeError):
        _kernels.decode_qkv(h, gamma, 1e-5, wq, wk, wv, q, k, v[:, :1])
    with pytest.raises(RuntimeError):
        _kernels.decode_qkv(h, gamma, 1e-5, wq, wk, wv[:64], q, k, v)
    hb = torch.zeros(17, 512, device=DEV, dtype=torch.float16)
    with pytest.raises(RuntimeError):
        _kernels.decode_qkv_batched(hb, gamma, 1e-5, wq, wk, wv, *_outs(17, 4, 2, 64))
    torch.cuda.synchronize()
