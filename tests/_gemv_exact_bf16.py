"""What the bf16 form of the exact GEMV suite needs besides tests/_gemv_exact.py (whose case table, value ranges, bit budget,
float64 row sums, rotation and ulp distance serve both element types).  Helper of test_gemv_exact_bf16_host.py (CPU) and
test_gpu_decode_layer_exact_bf16.py (GPU); holds no tests.

  - Every input `_gemv_exact.make_inputs` draws is a small integer over a power of two with at most 8 significant bits, so its
    bf16 form is the same number (`make_inputs` here asserts it), and the normalised input -- a multiple of 1/8 up to 2.25 --
    rounds to bf16 as it rounds to fp16: `_gemv_exact.exact_sums` is the bf16 kernels' exact row sums as well.
  - The reference rounds float64 -> fp32 -> bf16, nearest even (`to_bf16`); the first step is exact for every sum the bit
    budget admits.
  - The guard-band sentinel is a bf16 NaN payload: fp16's 0x7E2A read as bf16 is the finite number 2.2e38.
  - `scale_exp`: every token's scale s_t (and the residual) times 2 ** scale_exp.  A power of two moves no significand: the
    bit budget is unchanged, the row sums scale with it, and at 2 ** 16 the inputs, the sums of squares and the outputs of
    the launches without a norm lie beyond fp16's 65504.
"""
import torch

import _gemv_exact as G

SENTINEL = 0x7FA5      # a bf16 NaN payload (exponent all ones, mantissa 0x25) no kernel produces
SCALE_EXP = 16


def to_bf16(v):
    """float64 (or fp32) -> bf16 through fp32, round to nearest even, once"""
    return v.float().bfloat16()


def representable(t):
    """is every element of the fp16 / fp32 tensor `t` a bf16 number?"""
    f = t.float()
    return bool((f.bfloat16().float() == f).all())


def make_inputs(c, device, seed, scale_exp=0):
    """`_gemv_exact.make_inputs` as bf16 tensors (exactly the same numbers), x and the residual times 2 ** scale_exp"""
    d = G.make_inputs(c, device, seed)
    k = 2.0 ** scale_exp
    out = {}
    for name, t in d.items():
        if t is None:
            out[name] = None
            continue
        ts = t if isinstance(t, list) else [t]
        ts = [x.float() * (k if name in ("x", "h") else 1.0) for x in ts]
        assert all(representable(x) for x in ts), (G.case_id(c), name)
        ts = [x.bfloat16().contiguous() for x in ts]
        out[name] = ts if isinstance(t, list) else ts[0]
    return out


def normalised(x, gamma, eps=G.EPS):
    """float64 RMSNorm rounded to bf16 once, as float64 (gamma None: x itself)"""
    x = x.double()
    if gamma is None:
        return x
    return to_bf16(x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gamma.double()).double()


def exact_sums(c, d, eps=G.EPS):
    """float64 row sums of every matrix of the case over the bf16-rounded normalised input: a list of [n, rows_i]"""
    xn = normalised(d["x"], d["gamma"], eps)
    return [G.row_sums(xn, w) for w in d["w"]]


def reference(c, d, sums):
    """Exact float64 results of the case rounded to bf16 once: a list of [n, rows_i] bf16, one per output (rotation at
    position 0 with a factor of one: the row sums themselves)."""
    if c.entry == "residual":
        return [to_bf16(d["h"].double() + sums[0])]
    if c.entry == "gate_up":
        gq, uq = sums
        assert float(gq.abs().max()) <= 20.0, (G.case_id(c), float(gq.abs().max()))  # the premise of the 1-ulp bound
        return [to_bf16(gq / (1 + torch.exp(-gq)) * uq)]
    return [to_bf16(v) for v in sums]


def ulp_bf16(x):
    """One bf16 ulp at |x| (8 significant bits), never below the smallest normal's (float64 tensor)."""
    e = torch.floor(torch.log2(torch.clamp(x.abs(), min=2.0 ** -126)))
    return torch.exp2(e - 7)


def scaled_cases():
    """The cases of the 2 ** 16 family: the launches without a norm (plain, residual), whose outputs scale with the inputs,
    and the plain launch with a norm, whose sums of squares do -- the first case of the table in every (kernel, TG /
    rows-per-wave shape)."""
    seen, out = set(), []
    for c in G.CASES:
        key = (c.entry, c.cell[0], c.cell[1])
        if c.entry in ("plain", "residual", "plain_norm") and key not in seen:
            seen.add(key)
            out.append(c)
    return out
