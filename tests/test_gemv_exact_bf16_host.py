"""CPU side of the bf16 exact GEMV suite (test_gpu_decode_layer_exact_bf16.py): its premises -- the case table's inputs are
bf16 numbers, the bit budget holds, the reference rounds to nearest even and the cases do exercise the rounding -- the C
ABI's typed entries, and the bf16 kernels as built."""
import ctypes
import os
import re

import pytest
import torch

import _gemv_exact as G
import _gemv_exact_bf16 as B

EINVAL, EUNSUPPORTED = -1, -2
F16, BF16 = 0, 1


def _bits(t):
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


# ---------------------------------------------------------------------------------------------------- premises
def test_every_value_an_input_can_take_is_a_bf16_number():
    """make_inputs draws from small sets whatever the case's shape: x = s m sign (s in 1/2 .. 4, m in 1, 3), gamma = k / 4
    (2 <= k <= 6), weights k / 8 (|k| <= 8) or k / 64 (|k| <= 4), residual k / 64 (|k| <= 256); the whole sets, also times
    2 ** 16 for x and the residual."""
    x = torch.tensor([s * m * sg for s in (0.5, 1.0, 2.0, 4.0) for m in (1.0, 3.0) for sg in (-1.0, 1.0)])
    gamma = torch.arange(2, 7).float() / 4
    w8, w64 = torch.arange(-8, 9).float() / 8, torch.arange(-4, 5).float() / 64
    h = torch.arange(-256, 257).float() / 64
    k = 2.0 ** B.SCALE_EXP
    for name, t in (("x", x), ("gamma", gamma), ("w / 8", w8), ("w / 64", w64), ("h", h), ("x 2^16", x * k), ("h 2^16", h * k)):
        assert B.representable(t), name
        assert torch.equal(t.half().float(), t) or "2^16" in name, name   # (and fp16 numbers: the fp16 suite's premise)
    assert not B.representable(torch.tensor([1.0 + 2.0 ** -8]))            # the check can fail


def _small_cases():
    """the three smallest cases of every entry: 21 cases"""
    out = []
    for e in G.ENTRIES:
        mine = sorted((c for c in G.CASES if c.entry == e), key=lambda c: max(c.n, 1) * c.in_dim + G.virtual_rows(c) * c.in_dim)
        out += mine[:3]
    return out


def test_inputs_of_real_cases_are_bf16_numbers_and_normalise_as_in_fp16():
    cases = _small_cases()
    assert len(cases) == 21
    for c in cases:
        d16 = G.make_inputs(c, "cpu", 7)
        d = B.make_inputs(c, "cpu", 7)            # asserts representability of every tensor
        for name in ("x", "gamma", "h"):
            if d[name] is not None:
                assert torch.equal(d[name].double(), d16[name].double()), (G.case_id(c), name)
        for w, w16 in zip(d["w"], d16["w"]):
            assert torch.equal(w.double(), w16.double()), G.case_id(c)
        # the normalised input rounds to bf16 as it rounds to fp16: one set of exact row sums serves both suites
        assert torch.equal(B.normalised(d["x"], d["gamma"]), G.normalised(d16["x"], d16["gamma"])), G.case_id(c)
        # ... and times 2 ** 16 it normalises to the same numbers
        ds = B.make_inputs(c, "cpu", 7, scale_exp=B.SCALE_EXP)
        if G.NORM[c.entry]:
            assert torch.equal(B.normalised(ds["x"], ds["gamma"]), B.normalised(d["x"], d["gamma"])), G.case_id(c)


def test_bit_budget_of_every_case():
    """24 bits at most for every case of the table; the 2 ** 16 family scales by a power of two and needs no more."""
    assert len(G.CASES) > 100
    for c in G.CASES:
        assert G.bit_budget(c) <= 24
    scaled = B.scaled_cases()
    assert {c.entry for c in scaled} == {"plain", "residual", "plain_norm"}
    assert {c.cell[0] for c in scaled} == {"persist", "fallback", "batch1"}


def test_scaled_family_leaves_fp16_range():
    """the smallest scaled cases on the CPU: outputs of the launches without a norm beyond 65504, finite in bf16"""
    for entry in ("plain", "residual"):
        c = min((c for c in B.scaled_cases() if c.entry == entry), key=lambda c: G.virtual_rows(c) * c.in_dim)
        d = B.make_inputs(c, "cpu", 11, scale_exp=B.SCALE_EXP)
        ref = B.reference(c, d, B.exact_sums(c, d))[0].float()
        assert float(ref.abs().max()) > 65504.0 and bool(torch.isfinite(ref).all())
        assert not bool(torch.isfinite(ref.half()[ref.abs() > 65504.0]).any())   # what fp16 would have made of them


def test_reference_rounds_ties_to_even():
    """a tie that goes down (to the even 1.0), a tie that goes up (to the even 1 + 2^-6), values just off the ties, and a
    negative tie: the patterns of round-to-nearest-even, which truncation and round-half-away each miss somewhere"""
    v = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -8 - 2.0 ** -20,
                      -(1 + 2.0 ** -8), 1 + 2.0 ** -7], dtype=torch.float64)
    got = _bits(B.to_bf16(v)).tolist()
    assert got == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80, 0x3F81], [hex(b) for b in got]
    trunc = [0x3F80, 0x3F81, 0x3F80, 0x3F80, 0xBF80, 0x3F81]
    away = [0x3F81, 0x3F82, 0x3F81, 0x3F80, 0xBF81, 0x3F81]
    assert got != trunc and got != away


def test_cases_exercise_the_rounding():
    """Over the 21 small cases: a good part of the exact sums is no bf16 number, and of those a good part are exact ties, in
    both directions -- a kernel that truncates or rounds half away cannot pass the bit-for-bit comparison."""
    total = inexact = ties = up = down = 0
    for c in _small_cases():
        if c.entry == "gate_up":
            continue
        d = B.make_inputs(c, "cpu", 7)
        for s in B.exact_sums(c, d):
            if c.entry == "residual":
                s = s + d["h"].double()
            r = B.to_bf16(s).double()
            ulp = B.ulp_bf16(s)
            ne = r != s
            tie = ne & ((r - s).abs() * 2 == ulp)
            total, inexact, ties = total + s.numel(), inexact + int(ne.sum()), ties + int(tie.sum())
            up, down = up + int((tie & (r.abs() > s.abs())).sum()), down + int((tie & (r.abs() < s.abs())).sum())
    print(f"{total} sums: {100 * inexact / total:.1f} % need rounding, {100 * ties / total:.1f} % are ties ({up} up, {down} down)")
    assert inexact * 10 > total and ties * 20 > total and up > 100 and down > 100, (total, inexact, ties, up, down)


# ---------------------------------------------------------------------------------------------------- C ABI
ONE = ctypes.c_void_p(4096)   # non-null, aligned; never dereferenced by a call that is refused


def _typed_calls(in_dim=64, dtype=BF16):
    """well-formed argument lists (but for the device pointers) of the ten typed entries, dtype in front of the stream"""
    p = ONE
    rope = (p, p, 1e-5, p, p, p, p, p, p, in_dim, 4, 2, 16, 1.0, 1e4, None, 1.0, p)
    qkv = (p, p, 1e-5, p, p, p, p, p, p, in_dim, 64, 32)
    return {
        "quest_decode_norm_gemv": ((p, p, 1e-5, p, p, in_dim, 32), ()),
        "quest_decode_gemv_residual": ((p, p, p, in_dim, 32), ()),
        "quest_decode_mlp_gate_up": ((p, p, 1e-5, p, p, p, in_dim, 32), ()),
        "quest_decode_qkv_rope": (rope, ()),
        "quest_decode_qkv": (qkv, ()),
        "quest_decode_norm_gemv_batched": ((p, p, 1e-5, p, p, in_dim, 32), (4,)),
        "quest_decode_gemv_residual_batched": ((p, p, p, in_dim, 32), (4,)),
        "quest_decode_mlp_gate_up_batched": ((p, p, 1e-5, p, p, p, in_dim, 32), (4,)),
        "quest_decode_qkv_rope_batched": (rope, (4,)),
        "quest_decode_qkv_batched": (qkv, (4,)),
    }


def test_typed_entries_refuse_an_unknown_dtype_and_shapes_like_fp16():
    from quest_amd._lib import SIGNATURES, lib

    calls = _typed_calls()
    assert len(calls) == 10
    for name, (args, n) in calls.items():
        # one entry per operator and form: no <name>_dtype twin, dtype in front of the stream
        assert not hasattr(lib, name + "_dtype") and name + "_dtype" not in SIGNATURES, name
        assert SIGNATURES[name][1][-2:] == [ctypes.c_uint32, ctypes.c_void_p], name
        entry = getattr(lib, name)
        for bad in (2, 3, 0xFFFFFFFF):
            assert entry(*args, *n, bad, None) == EINVAL, (name, bad)
        # a null operand: EINVAL whatever the type
        null = (None,) + args[1:]
        assert entry(*null, *n, F16, None) == EINVAL and entry(*null, *n, BF16, None) == EINVAL, name
    # shapes fp16 refuses with QUEST_EUNSUPPORTED are refused for bf16: in_dim % 8 != 0
    for name, (args, n) in _typed_calls(in_dim=68).items():
        entry = getattr(lib, name)
        got = (entry(*args, *n, F16, None), entry(*args, *n, BF16, None))
        assert got == (EUNSUPPORTED,) * 2, (name, got)
    # more than 16 tokens: EINVAL from the n-token entries of both types
    for name, (args, n) in _typed_calls().items():
        if n:
            entry = getattr(lib, name)
            assert entry(*args, 17, F16, None) == EINVAL and entry(*args, 17, BF16, None) == EINVAL, name


def test_wrappers_take_one_element_type_per_call(monkeypatch):
    """fp16 or bf16, never mixed, never fp32 -- refused in Python before any pointer reaches the library (the device and
    shape checks switched off: the tensors here live on the CPU, and the dtype check does not depend on them)"""
    from quest_amd import _kernels as K

    monkeypatch.setattr(K, "_CHECKS_ON", False)

    for dt in (torch.float16, torch.bfloat16):
        other = torch.bfloat16 if dt == torch.float16 else torch.float16
        x, w, out = torch.zeros(64, dtype=dt), torch.zeros(32, 64, dtype=dt), torch.zeros(32, dtype=dt)
        with pytest.raises(RuntimeError, match="dispatch with dtype"):
            K.decode_norm_gemv(x, None, 1e-5, w.to(other), out)
        with pytest.raises(RuntimeError, match="dispatch with dtype"):
            K.decode_gemv_residual(x.to(other), w, out)
        with pytest.raises(RuntimeError, match="dispatch with dtype"):
            K.decode_mlp_gate_up_batched(x.view(1, 64), x.to(other), 1e-5, w, w, out.view(1, 32))
    x32 = torch.zeros(64)
    with pytest.raises(RuntimeError, match="dispatch with dtype torch.float32"):
        K.decode_norm_gemv(x32, None, 1e-5, torch.zeros(32, 64), torch.zeros(32))
    with pytest.raises(RuntimeError, match="dispatch with dtype"):   # still defined, still fp16 and nothing else
        K._check_f16(torch.zeros(1, dtype=torch.bfloat16), "op")
    K._check_f16(torch.zeros(1, dtype=torch.float16), "op")


# ---------------------------------------------------------------------------------------------------- the kernels as built
from quest_amd.build import LIB, kernel_metadata  # noqa: E402

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
needs_tools = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")),
                                 reason="needs the built library and the ROCm LLVM tools (llvm-objcopy / llvm-readelf)")


@needs_tools
def test_bf16_gemv_kernels_exist_and_fit_their_launch_bounds():
    """Every instantiation the launchers of csrc/decode_layer.hip can take has its bf16 form (<kernel>_b16) in the library --
    the same template arguments, but for the inputs-from-L2 kernel at 9-16 tokens, which keeps one k step in flight where
    fp16 keeps two -- with no scratch and no spilled register, the LDS of its fp16 twin, and the registers its launch bounds
    leave: gemv_kernel 8 waves x 2 workgroups per CU = 128, skinny_kernel 8 waves x 1 = 256, persist_kernel 16 waves x 1
    (launch bounds 4 waves per SIMD) = 128."""
    meta = kernel_metadata(LIB)
    caps = {"gemv_kernel": 128, "skinny_kernel": 256, "persist_kernel": 128}
    found = {k: 0 for k in caps}
    for name, v in meta.items():
        m = re.match(r"_ZN5quest(\d+)(gemv_kernel|skinny_kernel|persist_kernel)_b16(I.*)", name)
        if not m:
            continue
        kernel = m.group(2)
        found[kernel] += 1
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (name, v)
        assert v["vgpr"] <= caps[kernel], (name, v)
        twin = f"_ZN5quest{int(m.group(1)) - 4}{kernel}{m.group(3)}"
        if kernel == "skinny_kernel" and "ELi8ELi1ELi4E" in name:      # NW 8, U 1, TG 4: fp16 runs U 2
            twin = twin.replace("ELi8ELi1ELi4E", "ELi8ELi2ELi4E")
        assert twin in meta, (name, twin)
        assert v["lds"] == meta[twin]["lds"], (name, v, meta[twin])
    f16 = {k: sum(1 for n in meta if re.match(rf"_ZN5quest\d+{k}I", n)) for k in caps}
    assert found == f16 and found["gemv_kernel"] >= 26 and found["skinny_kernel"] == 12 and found["persist_kernel"] == 12, (found, f16)
