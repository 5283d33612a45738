"""Helpers of tests/test_gpu_high_pages.py: KV pools whose pages lie beyond 4 GiB and 8 GiB of a layer.

A pool layer is indexed in 16-bit elements: page ``p`` starts at element ``p * P`` with ``P = 2 * S * Hkv * D``.  LINE A is
element 2^31 (byte 2^32: a signed element index or an unsigned byte offset wraps), LINE B element 2^32 (8 GiB: an unsigned
element index wraps).  A page is ``low`` / ``mid`` / ``high`` by where it STARTS: below A, from A up to B, at B or above.

Nothing here copies a big pool to the host: a sequence's pages are gathered on the device into a compact pool in logical
order (``compact``), and what else the pool holds is scanned on the device in chunks (``dirty_pages``)."""
import os
from collections import namedtuple

import numpy as np
import torch

import oracle
import _bf16
import _harness as H

DEV = "cuda:0"
LINE_A, LINE_B = 1 << 31, 1 << 32
PATTERN = 0x7FFF          # a NaN in fp16 and in bf16 (``_harness.poison_pools``)
HIGH_PAGES = 128          # pages a big pool holds at or above line B
BANDS = ("low", "mid", "high")
ATOL, BF16_RTOL = 2e-3, 2.0 ** -8   # the suite's bars for o and lse against the oracle


class Geo(namedtuple("Geo", "bf16 layout Hq Hkv D S")):
    """Element type, pool layout and head shape of a case, and where the two lines fall in its pool."""

    @property
    def dtype(self):
        return torch.bfloat16 if self.bf16 else torch.float16

    @property
    def P(self):            # elements per page
        return 2 * self.S * self.Hkv * self.D

    @property
    def pA(self):           # first page that starts at or above line A
        return -(-LINE_A // self.P)

    @property
    def pB(self):           # first page that starts at or above line B
        return -(-LINE_B // self.P)

    @property
    def n_pages(self):      # pages of a single-sequence big pool: a little over 8 GiB per layer
        return self.pB + HIGH_PAGES

    def band(self, page):
        return "low" if page * self.P < LINE_A else "mid" if page * self.P < LINE_B else "high"

    def straddlers(self):
        """Pages that contain a line in their interior (none where P divides the lines)."""
        return [line // self.P for line in (LINE_A, LINE_B) if line % self.P]

    def name(self):
        return f"{'bf16' if self.bf16 else 'fp16'}-layout{self.layout}-Hq{self.Hq}-Hkv{self.Hkv}-D{self.D}-S{self.S}"


def band_counts(geo, pages):
    return {b: sum(1 for p in pages if geo.band(int(p)) == b) for b in BANDS}


# ------------------------------------------------------------------------------------------------ records
_SEEN = {}
_STARTED = set()


def record(family, line):
    """A figure of the run: printed (pytest -s) and, when QUEST_HIGH_PAGES_FILE names a file, appended to it with the test
    case that measured it -- profiles/high_pages.txt is such a file, as the tests wrote it."""
    print(f"[{family}] {line}")
    path = os.environ.get("QUEST_HIGH_PAGES_FILE")
    if path:
        new = path not in _STARTED    # a run's first record starts the file afresh
        _STARTED.add(path)
        with open(path, "w" if new else "a") as f:
            if new:
                f.write("# written by tests/test_gpu_high_pages.py (tests/_high_pages.py record()) with\n"
                        "# QUEST_HIGH_PAGES_FILE=<this file> pytest tests/test_gpu_high_pages.py -m gpu\n"
                        "# one line per case: <family> | <test case> | <figures>; the bars are 2e-3 (fp16), 2e-3 + 2^-8 |x| (bf16)\n")
            case = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].replace("tests/test_gpu_high_pages.py::", "")
            case = "(the module)" if family == "summary" else case
            f.write(f"{family} | {case} | {line}\n")


def note_errors(family, o_err, lse_err):
    worst = _SEEN.setdefault(family, [0.0, 0.0, 0])
    worst[0], worst[1], worst[2] = max(worst[0], o_err), max(worst[1], lse_err), worst[2] + 1


def summary_lines():
    return [f"{fam}: {n} comparisons, largest |o - oracle| {o:.3e}, largest |lse - oracle| {l:.3e}"
            for fam, (o, l, n) in sorted(_SEEN.items())]


# ------------------------------------------------------------------------------------------------ pools and placement
def poison(pool):
    pool.buf.view(torch.int16).fill_(PATTERN)


def big_pool(geo, n_pages=None):
    """A 2-layer KV pool filled with the pattern.  Layer 1 is the one the tests run on; layer 0 is the guard a
    sign-extended negative offset (at most -4 GiB) would land in."""
    from quest_amd.utils.kv_cache import KvPool

    pool = KvPool(2, geo.Hkv, geo.D, n_pages or geo.n_pages, geo.S, geo.dtype, torch.device(DEV), geo.layout)
    assert pool.layer(1).numel() > LINE_B and pool.layer(1).stride(0) == geo.P
    poison(pool)
    return pool


def crafted_order(geo, n, tail_at=(), tail="high", seed=0):
    """``n`` distinct pages in the order a sequence is to receive them: position j takes a page of band low / mid / high for
    j % 3 == 0 / 1 / 2, except the positions ``tail_at`` (the page of the decode append, the page a step opens next), which
    take band ``tail``.  Each band's first picks are its edge pages: (the page just below A or straddling it), (the
    first page at or above A, the page just below B or straddling it), (the first page at or above B, the pool's last)."""
    rng = np.random.default_rng(seed)
    N = geo.n_pages
    edges = {"low": [geo.pA - 1], "mid": [geo.pA, geo.pB - 1], "high": [geo.pB, N - 1]}
    span = {"low": (HIGH_PAGES, geo.pA - 1), "mid": (geo.pA + 1, geo.pB - 1), "high": (geo.pB + 1, N - 1)}
    cand = {}
    for b in BANDS:
        lo, hi = span[b]
        inner = lo + rng.choice(hi - lo, size=min(n, hi - lo), replace=False)
        cand[b] = (edges[b] + [int(p) for p in inner])[::-1]
    order = [cand[tail if j in tail_at else BANDS[j % 3]].pop() for j in range(n)]
    assert len(set(order)) == n and all(0 <= p < N for p in order)
    return order


def drive_free_list(pool, order):
    """Make ``pool`` hand out exactly ``order``, with ``alloc_block`` / ``free_block`` alone: take every page, then give back
    the wanted ones, last first (the free list is LIFO).  The other pages stay taken and are never handed out."""
    for _ in range(pool.capacity):
        pool.alloc_block()
    for p in reversed(order):
        pool.free_block(p)
    assert pool.num_free_blocks == len(order)


def assert_placement(geo, table, tail_idx=(), tail="high"):
    """The placement a single-sequence case relies on, from ``kv_cache.indicies``: at least a quarter of the pages in each
    band, the edge pages of both lines and the pool's last page in the table, the tail pages in their band."""
    counts = band_counts(geo, table)
    assert all(4 * counts[b] >= len(table) for b in BANDS), counts
    for p in (geo.pA - 1, geo.pA, geo.pB - 1, geo.pB, geo.n_pages - 1):
        assert p in table, f"edge page {p} not in the table"
    for s in geo.straddlers():
        assert s in table[:-1], f"straddling page {s} is not an attended page"
    for j in tail_idx:
        assert geo.band(table[j]) == tail, (j, table[j], tail)
    return counts


def dirty_pages(pool, chunk_bytes=1 << 27):
    """Per layer, the pages that hold anything but the pattern: scanned on the device in chunks."""
    out = []
    for l in range(pool.num_layers):
        layer = pool.layer(l).view(torch.int16).view(pool.capacity, -1)
        step = max(1, chunk_bytes // (2 * layer.size(1)))
        hits = [torch.nonzero((layer[a:a + step] != PATTERN).any(dim=1)).flatten() + a for a in range(0, pool.capacity, step)]
        out.append(torch.cat(hits).cpu().tolist())
    return out


def assert_only_owned_written(pool, owned, what):
    """Layer 1 holds something other than the pattern in exactly the owned pages; layer 0 holds the pattern throughout."""
    d0, d1 = dirty_pages(pool)
    assert not d0, f"{what}: layer 0 written, first pages {d0[:8]}"
    owned = sorted(set(int(p) for p in owned))
    stray, missing = sorted(set(d1) - set(owned)), sorted(set(owned) - set(d1))
    assert not stray, f"{what}: {len(stray)} pages nobody owns were written, first {stray[:8]}"
    assert not missing, f"{what}: {len(missing)} owned pages still hold only the pattern, first {missing[:8]}"


def compact(cache, layer=1):
    """A cache's pages gathered on the device in logical order: uint16 bits ``[n_pages, 2, ...]``."""
    idx = torch.tensor(cache.indicies, dtype=torch.long, device=DEV)
    return _bf16.bits(cache.buf_layer(layer)[idx])


# ------------------------------------------------------------------------------------------------ the oracle's side
def dev(a, bf16):
    return _bf16.dev16(a) if bf16 else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f32(bits_, bf16):
    return _bf16.bf16_bits_to_f32(bits_) if bf16 else bits_.view(np.float16).astype(np.float32)


def oracle_compact(geo, k, v, L):
    """The oracle's pools of a sequence of ``L`` tokens over the renumbered table 0 .. n-1."""
    S = geo.S
    n, inner = -(-L // S), ((geo.Hkv, S, geo.D) if geo.layout == 1 else (S, geo.Hkv, geo.D))
    m = -(-n // S)
    kv = oracle.Paged(np.zeros((n, 2) + inner, np.float16), np.arange(n, dtype=np.int32), (L - 1) % S + 1, geo.layout)
    meta = oracle.Paged(np.zeros((m, 2) + inner, np.float16), np.arange(m, dtype=np.int32), (n - 1) % S + 1, geo.layout)
    oracle.append_prefill(kv, meta, k[:L], v[:L])
    return kv, meta


def assert_compact_is_oracle(geo, kv_bits, meta_bits, kv_o, meta_o, L):
    """Compact device pools == the oracle's, bit for bit, on every owned element; every other element of the owned pages
    (the stale slots of the last page, the unused entries of the last metadata page) still holds the pattern."""
    n = -(-L // geo.S)
    for got, o, entries, what in ((kv_bits, kv_o, L, "KV"), (meta_bits, meta_o, n, "metadata")):
        want = _bf16.f16_to_bf16_bits(o.data) if geo.bf16 else o.data.view(np.uint16)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        mask = H.owned_mask(want.shape, geo.layout, range(want.shape[0]), entries)
        want = np.where(mask, want, np.uint16(PATTERN))
        bad = np.argwhere(got != want)
        assert not len(bad), f"{what} pool: {len(bad)} elements differ from the oracle's, first at {bad[0].tolist()}"


def close(o_bits, want, bf16, what):
    """|o - oracle| within 2e-3 (fp16) / 2e-3 + 2^-8 |oracle| (bf16); returns the largest error."""
    got, want = f32(o_bits, bf16).astype(np.float64), np.asarray(want).astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bound = ATOL + (BF16_RTOL * np.abs(want) if bf16 else 0.0)
    assert (err <= bound).all(), (what, float(err.max()), float((err / bound).max()))
    return float(err.max())


def close_lse(lse, want, what):
    err = float(np.abs(np.asarray(lse, np.float64) - np.asarray(want, np.float64)).max())
    assert err <= ATOL, (what, err)
    return err


def check_scores(est_bits, q, meta_o, bf16):
    e = oracle.estimate(q, meta_o)
    if bf16:
        _bf16.check_scores(est_bits, e, max_undecided=1.0)
    else:
        assert np.array_equal(est_bits, e.view(np.uint16)), "estimate differs from the oracle's"


def logical(idx, table):
    """Physical page ids -> positions in ``table``; an id outside the table maps to -1."""
    pos = {int(p): j for j, p in enumerate(table)}
    return np.vectorize(lambda p: pos.get(int(p), -1), otypes=[np.int32])(np.asarray(idx))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_twin_equal(high, twin, what):
    """Two runs that differ in addresses alone: every output bit equal."""
    assert high.keys() == twin.keys(), (sorted(high), sorted(twin))
    bad = [name for name in high if not same_bytes(high[name], twin[name])]
    assert not bad, f"{what}: the run on high pages differs from its low twin in {bad}"


def release():
    import gc

    gc.collect()
    torch.cuda.empty_cache()


class Lse:
    """A NaN-filled float32 buffer handed to a handler; ``take`` returns the values and refills it."""

    def __init__(self, handler, n):
        self.buf = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
        self.handler = handler
        handler.lse_out = self.buf

    def take(self):
        a = self.buf.cpu().numpy().copy()
        self.buf.fill_(float("nan"))
        assert np.isfinite(a).all(), "LSE not written or not finite"
        return a

    def drop(self):
        self.buf.fill_(float("nan"))

    def off(self):
        self.handler.lse_out = None
