"""Exact-arithmetic inputs, float64 reference and the case table of the fused decode-layer GEMVs (csrc/decode_layer.hip).
Helper of test_gemv_case_table_host.py (CPU) and test_gpu_decode_layer_exact.py (GPU); holds no tests.

Every GEMV of that file accumulates fp16 x fp16 products in fp32 and rounds to fp16 once; the RMSNorm prologue rounds its
result to fp16 as well.  The inputs below make every fp32 partial sum exact IN EVERY SUMMATION ORDER, so v_dot2 in the
batch-1 kernel, the 4x4x4 MFMA of the n-token kernels, their DPP / LDS reductions and a float64 matmul agree bit for bit:

  x[t, k]   = s_t * m_k * sign[t, k];  m = a shuffle of 3 in_dim / 8 threes and 5 in_dim / 8 ones,  s_t = 2 ** (t % 4 - 1)
              => mean(x_t ** 2) = 4 s_t ** 2 exactly, 1 / rms = 1 / (2 s_t): a different one for every token of a group
  gamma     = multiples of 1/4 in [0.5, 1.5]  => rmsnorm(x) = +-m * gamma / 2 exactly (multiples of 1/8, <= 2.25); eps <= 1e-5
              and a few fp32 ulps of 1 / rms lie far below half an fp16 ulp of a value that is itself representable
  w         = multiples of 1/8 in [-1, 1] (linear launches), multiples of 1/64 in [-4/64, 4/64] (gate / up)
  residual  = multiples of 1/64, |h| <= 4

`bit_budget` derives from these ranges and in_dim how many bits the largest partial sum of a case needs and refuses a case
that leaves fp32's 24.
"""
import math
from collections import namedtuple

import torch

EPS = 1e-5
SENTINEL = 0x7E2A      # an fp16 NaN payload no kernel produces
GUARD = 64             # halves of guard band on both sides of an output: 128 bytes, keeps 16-byte alignment
WORKGROUPS = 256       # compute units of an MI355X = what the planner assumes with no device visible

ENTRIES = ("plain_norm", "plain", "residual", "gate_up", "rope", "rope_table", "qkv")
ROPE_PLAN = {"plain_norm": 0, "plain": 0, "residual": 0, "gate_up": 0, "rope": 1, "rope_table": 1, "qkv": 1}
NORM = {"plain_norm": True, "plain": False, "residual": False, "gate_up": True, "rope": True, "rope_table": True, "qkv": True}
PAIRED = {"gate_up", "rope", "rope_table"}  # batch-1 kernel: row-dots come in pairs, RW even

# entry: one of ENTRIES; rows: (out_dim,) | (intermediate,) | (q_rows, kv_rows); head_dim: 0 unless rotating;
# cell: ("persist", TG, ks, rounds) | ("fallback", TG) | ("batch1", RW, U); batch-1 cases have n == 0 (the single-token
# entry points), n-token cases 1 <= n <= 16
Case = namedtuple("Case", "entry n in_dim rows head_dim cell")


def case_id(c):
    return f"{c.entry}-n{c.n}-{c.in_dim}x{'+'.join(map(str, c.rows))}-d{c.head_dim}-{'_'.join(map(str, c.cell))}"


def virtual_rows(c):
    if c.entry == "gate_up":
        return 2 * c.rows[0]
    if c.entry in ("rope", "rope_table", "qkv"):
        return c.rows[0] + 2 * c.rows[1]
    return c.rows[0]


def token_groups(n):
    return 1 if n <= 4 else (2 if n <= 8 else 4)


def batch1_cell(entry, vrows, in_dim):
    """The dispatch of launch_gemv (csrc/decode_layer.hip:261-290, default build, no QUEST_GEMV_CFG): 8-wave workgroups and
    the largest rows-per-wave RW that still gives 512 workgroups -- RW = 4, U = 2 from 512 * 32 = 16384 virtual rows on;
    below that the plain and residual launches take RW = 2, U = 4 from 512 * 16 = 8192 rows on and RW = 1 otherwise, the
    launches whose row-dots come in pairs (gate / up, rotation) RW = 2, U = 4.  RW = 1 runs with U = 8 up to 7 rounds of
    4096 halves and with U = 4 beyond: the input is staged in whole rounds under a 60 KiB limit (launch_gemv_rw, :244-254).
    The unrotated q-k-v launch is the plain one with three matrices."""
    if vrows // 32 >= 512:
        return ("batch1", 4, 2)
    if entry in PAIRED or vrows // 16 >= 512:
        return ("batch1", 2, 4)
    return ("batch1", 1, 8) if in_dim <= 7 * 4096 else ("batch1", 1, 4)


def batch1_round(cell):
    """halves of a row that one round of the batch-1 kernel covers: U slots x 64 lanes x 8 halves"""
    return cell[2] * 64 * 8


# ---------------------------------------------------------------------------------------------------------------------
# The case table.  A persistent-kernel shape is (in_dim, quads of virtual rows, ks, rounds, last round full, TGs that can
# take it); with 256 workgroups a round holds 256 * 16 / ks quads.  Row counts follow from the quads per entry (below), so
# that the plain launches see every row count % 4, gate / up an odd intermediate and the unrotated q-k-v launch quads that
# straddle two matrices, without leaving the cell: 4 q - 3 .. 4 q virtual rows are the same q quads.
ALL_TG = (1, 2, 4)
PERSIST_SHAPES = {
    1: [(512, 4096, 1, True, ALL_TG), (392, 2052, 1, False, ALL_TG), (392, 6152, 2, False, ALL_TG),
        (392, 12288, 3, True, ALL_TG), (392, 14340, 4, False, ALL_TG), (512, 8192, 2, True, ALL_TG),
        (512, 9, 1, False, ALL_TG)],
    2: [(520, 9, 1, False, ALL_TG), (520, 2048, 1, True, ALL_TG), (520, 4096, 2, True, ALL_TG),
        (520, 6100, 3, False, ALL_TG), (520, 8192, 4, True, ALL_TG), (1024, 4000, 2, False, ALL_TG)],
    4: [(1536, 9, 1, False, ALL_TG), (1536, 1024, 1, True, ALL_TG), (1536, 2048, 2, True, ALL_TG),
        (520, 3072, 3, True, ALL_TG), (1536, 4096, 4, True, ALL_TG), (1160, 2040, 2, False, ALL_TG),
        (1544, 3000, 3, False, ALL_TG)],
    8: [(2056, 9, 1, False, ALL_TG), (2056, 512, 1, True, ALL_TG), (2056, 1024, 2, True, ALL_TG),
        (1536, 1028, 3, False, ALL_TG), (2056, 2048, 4, True, ALL_TG), (4096, 1500, 3, False, ALL_TG),
        (3080, 1536, 3, True, ALL_TG)],
    # rows of 4096 < in_dim <= 8192 fit the persistent kernel at <= 4 tokens only and take ks = 16 by their length; at
    # more tokens ks = 16 is reached from ks = 8 (17 <= spp <= 32) by the fullest-last-round rule, which an even round
    # count can never satisfy (2 m rounds of 256 quads are m rounds of 512): see the host test
    16: [(2056, 64, 1, False, ALL_TG), (2056, 256, 1, True, ALL_TG), (2056, 576, 3, False, ALL_TG),
         (2056, 1028, 5, False, ALL_TG), (2056, 768, 3, True, ALL_TG), (4096, 1280, 5, True, ALL_TG),
         (2184, 200, 1, False, (2, 4)),
         (4104, 512, 2, True, (1,)), (5120, 300, 2, False, (1,)), (8192, 256, 1, True, (1,)), (4104, 1024, 4, True, (1,)),
         (4104, 9, 1, False, (1,))],
}
TOKENS = {1: (1, 3, 4), 2: (5, 8), 4: (9, 13, 16)}
PLAIN_TAIL = {"plain_norm": 1, "plain": 2, "residual": 3}  # virtual rows = 4 quads - tail


def rope_heads(vrows, prefer=(128, 64, 32, 16)):
    """(head_dim, q heads, kv heads) of a rotating launch of `vrows` rows: the largest head_dim of `prefer` that leaves at
    least three heads"""
    for d in prefer:
        if vrows % d == 0 and vrows // d >= 3:
            t = vrows // d
            hkv = max(1, t // 6)
            return d, t - 2 * hkv, hkv
    raise ValueError(f"no head split for {vrows} rows")


def entry_rows(entry, quads, head_dim=None):
    """(rows, head_dim) of `entry` at `quads` quads of virtual rows (rotation: rounded up to whole 16-row blocks)"""
    if entry in PLAIN_TAIL:
        return (4 * quads - PLAIN_TAIL[entry],), 0
    if entry == "gate_up":
        return (2 * quads - 1,), 0           # odd intermediate: the last quad holds one (gate, up) pair
    if entry == "qkv":
        return (4 * quads - 14, 6), 0        # q rows % 4 == 2, kv rows 6: quads straddle q|k, k|v
    vrows = 4 * ((quads + 3) // 4 * 4)
    if head_dim is None:
        head_dim, hq, hkv = rope_heads(vrows)
    else:
        head_dim, hq, hkv = rope_heads(vrows, (head_dim,))
    return (hq * head_dim, hkv * head_dim), head_dim


def _persist_cases():
    out = []
    for ksi, (ks, shapes) in enumerate(sorted(PERSIST_SHAPES.items())):
        for tgi, tg in enumerate(ALL_TG):
            mine = [s for s in shapes if tg in s[4]]
            # every shape of the (TG, ks) and every entry at least once, the pairing rotating with TG and ks
            for i in range(max(len(ENTRIES), len(mine))):
                entry = ENTRIES[i % len(ENTRIES)]
                in_dim, quads, rounds, _full, _tgs = mine[(i + tgi + ksi) % len(mine)]
                n = TOKENS[tg][(i + ksi) % len(TOKENS[tg])]
                rows, hd = entry_rows(entry, quads)
                out.append(Case(entry, n, in_dim, rows, hd, ("persist", tg, ks, rounds)))
    # hidden sizes 5120 (Qwen3-14B / 32B, Llama-2-13B) and 8192 (70B shapes) at both ends of the one token group that fits
    for in_dim, quads, rounds in ((5120, 300, 2), (8192, 256, 1)):
        for n, entry in ((1, "rope"), (4, "gate_up"), (1, "residual"), (4, "qkv")):
            rows, hd = entry_rows(entry, quads)
            out.append(Case(entry, n, in_dim, rows, hd, ("persist", 1, 16, rounds)))
    return out


def _fallback_cases():
    """The inputs-from-L2 kernel: rows shorter than a wave sweep (in_dim <= 384), inputs too large for LDS, head_dim > 256"""
    out = []
    small = (8, 40, 264)
    for tgi, tg in enumerate(ALL_TG):
        for ei, entry in enumerate(ENTRIES):
            in_dim = small[(ei + tgi) % 3]
            quads = (9, 10, 12)[(ei + 2 * tgi) % 3]
            n = TOKENS[tg][(ei + tgi) % len(TOKENS[tg])]
            rows, hd = entry_rows(entry, quads)
            out.append(Case(entry, n, in_dim, rows, hd, ("fallback", tg)))
    # rows above 8192 that are ragged mod 128; down_proj of Llama-2-7B (11008) is the shipped case
    for entry, n, in_dim, quads in (("residual", 3, 8200, 9), ("plain_norm", 4, 8200, 5), ("residual", 16, 11008, 9),
                                    ("plain", 13, 11008, 5), ("qkv", 8, 8200, 9), ("rope", 9, 8200, 12)):
        rows, hd = entry_rows(entry, quads)
        out.append(Case(entry, n, in_dim, rows, hd, ("fallback", token_groups(n))))
    # rotation at head_dim 512: the LDS rotation table of the persistent kernel ends at 256
    for entry, n, in_dim in (("rope", 4, 520), ("rope_table", 8, 1536), ("rope", 13, 520), ("rope_table", 3, 264)):
        rows, hd = entry_rows(entry, 384, 512)
        out.append(Case(entry, n, in_dim, rows, hd, ("fallback", token_groups(n))))
    return out


def _batch1_cases():
    out = []

    def in_dims(cell):  # below one round (full == 0), an exact round, a ragged tail of 33 vectors behind a round, 8
        r = batch1_round(cell)
        return (264, r, r + 264, 8)

    plain_like = {(1, 8): (10, 251), (2, 4): (2051, 2303), (4, 2): (4098, 4101)}
    for (rw, u), quads2 in plain_like.items():
        cell = ("batch1", rw, u)
        for ii, in_dim in enumerate(in_dims(cell)):
            for entry, quads in (("plain_norm" if ii % 2 == 0 else "plain", quads2[0]), ("residual", quads2[1])):
                rows, hd = entry_rows(entry, quads)
                out.append(Case(entry, 0, in_dim, rows, hd, cell))
    paired = {(2, 4): (10, 256), (4, 2): (4098, 4096)}
    for (rw, u), quads2 in paired.items():
        cell = ("batch1", rw, u)
        for ii, in_dim in enumerate(in_dims(cell)):
            rows, hd = entry_rows("gate_up", quads2[0])
            out.append(Case("gate_up", 0, in_dim, rows, hd, cell))
            entry = "rope" if ii % 2 == 0 else "rope_table"
            rows, hd = entry_rows(entry, quads2[1])
            out.append(Case(entry, 0, in_dim, rows, hd, cell))
    for quads, in_dim, cell in ((10, 264, (1, 8)), (2051, 2048, (2, 4)), (4100, 1288, (4, 2))):  # plain, three matrices
        rows, hd = entry_rows("qkv", quads)
        out.append(Case("qkv", 0, in_dim, rows, hd, ("batch1",) + cell))
    # the staging limit, 60 KiB of LDS: every shape serves it (RW = 1 with U = 4: U = 8 pads the stage to 64 KiB)
    out.append(Case("plain_norm", 0, 30720, (37,), 0, ("batch1", 1, 4)))
    out.append(Case("residual", 0, 28672, (37,), 0, ("batch1", 1, 8)))
    out.append(Case("residual", 0, 28680, (37,), 0, ("batch1", 1, 4)))
    out.append(Case("rope", 0, 30720, (16, 16), 16, ("batch1", 2, 4)))
    return out


CASES = _persist_cases() + _fallback_cases() + _batch1_cases()
N_TOKEN_CASES = [c for c in CASES if c.cell[0] != "batch1"]
BATCH1_CASES = [c for c in CASES if c.cell[0] == "batch1"]


def planner_cell(lib, c):
    """The cell quest_decode_batched_plan gives an n-token case (the real planner; needs no GPU)"""
    import ctypes

    info = (ctypes.c_uint32 * 6)()
    rc = lib.quest_decode_batched_plan(c.in_dim, virtual_rows(c), c.n, ROPE_PLAN[c.entry], info)
    assert rc in (0, 1), (case_id(c), rc)
    tg = token_groups(c.n)
    if c.entry in ("rope", "rope_table") and c.head_dim > 256:
        return ("fallback", tg), list(info)   # launch_batched: decided before the planner
    return (("persist", tg, info[0], info[1]) if rc == 1 else ("fallback", tg)), list(info)


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def bit_budget(c):
    """Bits the largest partial sum of the case can need, from the value ranges alone; asserts that fp32 holds them."""
    n = max(c.n, 1)
    s_max = 2.0 ** (min(n - 1, 3) - 1)
    x_max, x_step = (2.25, 1 / 8) if NORM[c.entry] else (3 * s_max, 0.5)
    w_max, w_step = (4 / 64, 1 / 64) if c.entry == "gate_up" else (1.0, 1 / 8)
    step, top = x_step * w_step, c.in_dim * x_max * w_max
    if c.entry == "residual":
        step, top = min(step, 1 / 64), top + 4.0
    bits = math.ceil(math.log2(top / step + 1))
    assert bits <= 24, (case_id(c), bits)
    return bits


def make_inputs(c, device, seed):
    """dict of the case's tensors on `device`: x [n, in_dim], gamma, w (list), h (residual), all fp16"""
    n = max(c.n, 1)
    g = torch.Generator(device=device).manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g, device=device)
    k3 = 3 * c.in_dim // 8
    m = torch.ones(c.in_dim, device=device)
    m[:k3] = 3.0
    m = m[torch.randperm(c.in_dim, generator=g, device=device)]
    sign = (ri(0, 1, n, c.in_dim) * 2 - 1).float()
    s = torch.tensor([2.0 ** (t % 4 - 1) for t in range(n)], device=device)
    d = {"x": (s[:, None] * m[None, :] * sign).half().contiguous()}
    d["gamma"] = (ri(2, 6, c.in_dim).float() / 4).half() if NORM[c.entry] else None
    if c.entry == "gate_up":
        d["w"] = [(ri(-4, 4, c.rows[0], c.in_dim).float() / 64).half() for _ in range(2)]
    elif c.entry in ("rope", "rope_table", "qkv"):
        d["w"] = [(ri(-8, 8, r, c.in_dim).float() / 8).half() for r in (c.rows[0], c.rows[1], c.rows[1])]
    else:
        d["w"] = [(ri(-8, 8, c.rows[0], c.in_dim).float() / 8).half()]
    d["h"] = (ri(-256, 256, n, c.rows[0]).float() / 64).half() if c.entry == "residual" else None
    return d


def normalised(x, gamma, eps=EPS):
    """float64 RMSNorm rounded to fp16 once, as float64 (gamma None: x itself)"""
    x = x.double()
    if gamma is None:
        return x
    return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gamma.double()).float().half().double()


def row_sums(xn, w, chunk=1 << 22):
    """float64 xn [n, in] @ w[rows, in].T in row chunks of <= `chunk` weight elements -> [n, rows] float64"""
    rows, in_dim = w.shape
    step = max(1, chunk // in_dim)
    return torch.cat([xn @ w[r:r + step].double().T for r in range(0, rows, step)], 1)


def to_f16(v):
    return v.float().half()


def exact_sums(c, d, eps=EPS):
    """float64 row sums of every matrix of the case over the fp16-rounded normalised input: a list of [n, rows_i]"""
    xn = normalised(d["x"], d["gamma"], eps)
    return [row_sums(xn, w) for w in d["w"]]


def reference(c, d, eps=EPS, sums=None):
    """Exact float64 results of the case rounded to fp16 once: a list of [n, rows_i] fp16, one per output (rotation at
    position 0 with a factor of one: the row sums themselves)."""
    sums = exact_sums(c, d, eps) if sums is None else sums
    if c.entry == "residual":
        return [to_f16(d["h"].double() + sums[0])]
    if c.entry == "gate_up":
        gq, uq = sums
        assert float(gq.abs().max()) <= 20.0, (case_id(c), float(gq.abs().max()))  # the premise of the 1-ulp bound
        return [to_f16(gq / (1 + torch.exp(-gq)) * uq)]
    return [to_f16(v) for v in sums]


def rotate(v, pos, head_dim, inv_freq, factor):
    """float64 rotate-half of exact row sums v [rows] at `pos`; the angle is the single fp32 product pos * inv_freq[d]"""
    v = v.reshape(-1, head_dim)
    ang = (torch.tensor(float(pos), device=v.device, dtype=torch.float32) * inv_freq).double()
    cs, sn = torch.cos(ang) * factor, torch.sin(ang) * factor
    a, b = v[:, : head_dim // 2], v[:, head_dim // 2:]
    return torch.cat([a * cs - b * sn, b * cs + a * sn], 1).reshape(-1)


def formula_inv_freq(head_dim, theta, device):
    i = torch.arange(head_dim // 2, device=device, dtype=torch.float32)
    return (theta ** (-2 * i / head_dim)).float()


def ulp_distance(a, b):
    """distance of two fp16 tensors in units in the last place, on the ordered bit patterns (-0 == +0)"""
    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()
