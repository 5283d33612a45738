"""Float64 numpy restatement of the sampling contract of include/quest_hip.h ("Token sampling"), the numpy Philox4x32-10
behind it, a decidability report per row, and the inputs the GPU tests use (so that the host test can bound, from the
restatement alone, how many of them are undecided).

Decidability.  The device computes masses and z in fp32; the restatement in float64.  A row is checked strictly only where
fp32 cannot move the answer:
  * top-p boundary: decided when both cumulative masses next to the cut differ from top_p * mass(K1) by more than
    P_MARGIN * mass(K1).  A tree-shaped fp32 sum of at most 2^18 non-negative terms is off by at most 18 * 2^-24 ~ 1.1e-6
    relative, plus a few ulp of expf (the device's integer sum of floor(w * 2^40) is tighter still): two orders of margin.
    Undecided: `kept` may be the neighbouring prefix on the near side.
  * draw: decided when the float64 top-two z differ by more than EPS_Z.  Undecided: the device token must be one of the
    restatement's top two.
EPS_Z = 32 x the largest |z_fp32 - z_fp64| that tests/test_sampling_host.py finds over `gpu_cases()` with numpy float32
(the factor covers a device logf of several ulp and the division by T); that test prints the measured value and holds it
under this constant.
"""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

P_MARGIN = 1e-4
EPS_Z = 4.9e-4   # 32 x 1.53e-5 measured (tests/test_sampling_host.py::test_gpu_inputs_are_decidable prints the figure)
MAX_UNDECIDED = 0.01

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
DRAW_TAG = 0x51554553


# ---------------------------------------------------------------- Philox4x32-10
def philox4x32_10(counter, key):
    """counter ``[..., 4]``, key ``[..., 2]`` (uint32, broadcast against each other) -> ``[..., 4]`` uint32."""
    c = [np.asarray(counter[..., i], np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], np.uint64) for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def draw_words(seed: int, pos: int, vocab: int) -> np.ndarray:
    """word_j for j in [0, vocab): output j & 3 of Philox with key (seed low, seed high), counter (j >> 2, pos, tag, 0)."""
    groups = (vocab + 3) // 4
    counter = np.zeros((groups, 4), np.uint32)
    counter[:, 0] = np.arange(groups, dtype=np.uint32)
    counter[:, 1] = np.uint32(pos & 0xFFFFFFFF)
    counter[:, 2] = np.uint32(DRAW_TAG)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    return philox4x32_10(counter, key).reshape(-1)[:vocab]


def uniforms(words: np.ndarray) -> np.ndarray:
    """((word >> 9) + 0.5) 2^-23 in float32: exact, inside (0, 1)."""
    return ((words >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


# ---------------------------------------------------------------- stored types
def to_bits(values: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values -> the stored 16-bit patterns (round to nearest even)."""
    v = np.asarray(values, np.float32)
    if dtype == "fp16":
        return v.astype(np.float16).view(np.uint16)
    u = v.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def to_f64(bits: np.ndarray, dtype: str) -> np.ndarray:
    b = np.asarray(bits, np.uint16)
    if dtype == "fp16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def half_key(bits: np.ndarray) -> np.ndarray:
    b = np.asarray(bits, np.uint16).astype(np.uint32)
    return np.where(b & 0x8000, (~b) & 0xFFFF, b | 0x8000).astype(np.uint32)


def token_order(bits: np.ndarray) -> np.ndarray:
    """Token indices by (key descending, index ascending)."""
    return np.argsort(-half_key(bits).astype(np.int64), kind="stable")


# ---------------------------------------------------------------- the contract
@dataclass
class Row:
    greedy: bool
    token: int                 # the restatement's token (for its own kept set)
    kept: int
    kept_allowed: dict = field(default_factory=dict)   # kept -> (token, runner-up or None, z gap) for every allowed kept
    boundary_decided: bool = True
    draw_decided: bool = True  # of the restatement's own kept set
    z32_err: float = 0.0       # max |z_fp32 - z_fp64| over the kept set (numpy float32)


def _draw(x, order, n, u):
    """argmax over the first n tokens of `order` of z = x - log(-log u); ties to the earlier token.  -> (token, 2nd, gap)"""
    sel = order[:n]
    with np.errstate(divide="ignore"):
        z = x[sel] - np.log(-np.log(u[sel].astype(np.float64)))
    best = int(np.argmax(z))  # first maximum = the earlier token of the order
    if n == 1:
        return int(sel[best]), None, np.inf
    rest = np.delete(z, best)
    second = int(np.argmax(rest))
    second_tok = int(np.delete(sel, best)[second])
    gap = float(z[best] - rest[second]) if np.isfinite(rest[second]) else np.inf
    return int(sel[best]), second_tok, gap


def sample_row(bits, dtype: str, temperature, top_k: int, top_p, seed: int, pos: int, eps_z: float = EPS_Z) -> Row:
    bits = np.asarray(bits, np.uint16)
    V = bits.size
    s = to_f64(bits, dtype)
    order = token_order(bits)
    T = float(np.float32(temperature))
    p = float(np.float32(top_p))
    if not (T > 0 and np.isfinite(T)) or np.isnan(s).any() or (s == np.inf).any() or s.max() == -np.inf:
        return Row(True, int(order[0]), 1, {1: (int(order[0]), None, np.inf)})
    m = s.max()
    with np.errstate(invalid="ignore"):
        x = (s - m) / T
    k1 = V if top_k <= 0 else min(int(top_k), V)
    cw = np.cumsum(np.exp(x[order[:k1]]))
    total = cw[-1]
    allowed, decided = [], True
    if p >= 1:
        n2 = k1
    elif not p > 0:
        n2 = 1
    else:
        target = p * total
        n2 = int(np.searchsorted(cw, target, side="left")) + 1  # shortest prefix with mass >= target
        n2 = min(n2, k1)
        if abs(cw[n2 - 1] - target) <= P_MARGIN * total and n2 < k1:
            decided = False
            allowed.append(n2 + 1)
        if n2 >= 2 and abs(cw[n2 - 2] - target) <= P_MARGIN * total:
            decided = False
            allowed.append(n2 - 1)
    u = uniforms(draw_words(seed, pos, V))
    out = {}
    for n in [n2] + allowed:
        out[n] = _draw(x, order, n, u)
    # fp32 restatement of z over the kept set, for EPS_Z
    sel = order[:n2]
    s32 = s.astype(np.float32)
    with np.errstate(divide="ignore"):
        z32 = (s32[sel] - np.float32(m)) / np.float32(T) - np.log(-np.log(u[sel]))
        z64 = x[sel] - np.log(-np.log(u[sel].astype(np.float64)))
    fin = np.isfinite(z64)
    err = float(np.abs(z32[fin].astype(np.float64) - z64[fin]).max()) if fin.any() else 0.0
    tok, _, gap = out[n2]
    return Row(False, tok, n2, out, decided, gap > eps_z, err)


def check_row(row: Row, token: int, kept: int) -> str:
    """'' when the device's (token, kept) is what the contract allows for this row, else what is wrong.  Decided rows:
    exactly the restatement's; an undecided boundary: one of the neighbouring kept sets; an undecided draw: one of the
    top two of that set."""
    if kept not in row.kept_allowed:
        return f"kept {kept}, allowed {sorted(row.kept_allowed)} (restatement {row.kept})"
    best, second, gap = row.kept_allowed[kept]
    if token == best or (gap <= EPS_Z and token == second):
        return ""
    return f"token {token}, restatement {best} (runner-up {second}, z gap {gap:.3g}, kept {kept})"


def check_token(row: Row, token: int) -> str:
    """`check_row` where the device's kept count is not at hand (a token read back from a generated sequence): the token
    must be allowed under one of the row's allowed kept sets."""
    msgs = [check_row(row, token, kept) for kept in row.kept_allowed]
    return "" if "" in msgs else msgs[0]


def greedy_token(bits) -> int:
    """The first token of the order: the largest 16-bit key, ties to the lowest index."""
    return int(token_order(np.asarray(bits, np.uint16).reshape(-1))[0])


def is_undecided(row: Row) -> bool:
    return not (row.boundary_decided and row.draw_decided)


# ---------------------------------------------------------------- the GPU tests' inputs
TEMPERATURES = (0.25, 0.7, 1.0, 2.0)
TOP_PS = (0.0, 0.5, 0.9, 1.0)
VOCABS = (1, 4, 63, 64, 65, 1001, 32000)
BATCHES = (1, 3, 16, 65)
BIG_VOCABS = (151936, 1 << 18)


def top_ks(V: int):
    return (0, 1, 5, 50, V, V + 1)


def make_logits(seed: int, n: int, V: int, dtype: str) -> np.ndarray:
    """``[n, V]`` stored bits of normal(0, 10) logits clipped to |s| <= 40."""
    rng = np.random.default_rng(seed)
    return to_bits(np.clip(rng.normal(0.0, 10.0, (n, V)), -40.0, 40.0).astype(np.float32), dtype)


@dataclass
class Case:
    name: str
    dtype: str
    V: int
    n: int
    bits: np.ndarray          # [n, V] uint16 (the device rows are V elements apart: 1001 leaves them misaligned)
    temperature: np.ndarray   # float32 [n]
    top_k: np.ndarray         # int32 [n]
    top_p: np.ndarray         # float32 [n]
    seed: np.ndarray          # uint64 [n]
    pos: np.ndarray           # int32 [n]


def _case(dtype: str, V: int, n: int, salt: int) -> Case:
    rng = np.random.default_rng(1000 * salt + 7)
    combos = [(t, k, p) for t in TEMPERATURES for k in top_ks(V) for p in TOP_PS]
    pick = (np.arange(n) * 37 + 11 * salt) % len(combos)  # 37 is coprime to 96: consecutive rows walk all combinations
    t, k, p = zip(*[combos[i] for i in pick])
    return Case(f"{dtype}-V{V}-n{n}", dtype, V, n, make_logits(salt, n, V, dtype), np.array(t, np.float32),
                np.array(k, np.int32), np.array(p, np.float32), rng.integers(0, 2 ** 63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1),
                rng.integers(1, 40000, n).astype(np.int32))


@lru_cache(maxsize=None)
def gpu_cases():
    cases, salt = [], 0
    for dtype in ("fp16", "bf16"):
        for V in VOCABS:
            for n in BATCHES:
                salt += 1
                cases.append(_case(dtype, V, n, salt))
    cases.append(_case("fp16", BIG_VOCABS[0], 2, 901))
    cases.append(_case("bf16", BIG_VOCABS[1], 2, 902))
    return tuple(cases)


@lru_cache(maxsize=None)
def case_rows(name: str):
    """The restatement's rows of one case (computed once, shared by the tests that need them)."""
    c = {c.name: c for c in gpu_cases()}[name]
    return tuple(sample_row(c.bits[i], c.dtype, c.temperature[i], int(c.top_k[i]), c.top_p[i], int(c.seed[i]), int(c.pos[i]))
                 for i in range(c.n))
