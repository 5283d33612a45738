"""The sign-plane estimate (csrc/estimate_planes.hip) without a GPU: its arithmetic restated in numpy equals the CPU oracle
bit for bit, its C entries are exported and declared, and the shapes it does not serve are refused before anything is
launched.

The restatement is what the kernel does: per (page, kv head) ONE value per feature -- max(Kslot, Vslot) where q >= 0,
min(Kslot, Vslot) where q < 0 -- 8 consecutive features accumulated left to right in fp32 from 0 (fp16 x fp16 is exact in
fp32, so ``fma(q, x, acc)`` is ``fp32(acc + q * x)``), the 16 octet sums added in the tree of row_allreduce_sum_fast<16> as
lane 0 sees it, one cast to fp16.  No tolerance: bit patterns."""
import os
import re

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, D, S = 4, 128, 16
EUNSUPPORTED = -2
ENTRIES = [(32, 0), (33, 0), (300, 1), (628, 1)]  # (metadata entries, layout): 2 to 40 metadata pages, NHD and HND


def _tree(p):
    """p: [..., 16] fp32 octet sums -> the row total, (((p0+p8)+(p12+p4)) + ((p14+p6)+(p10+p2))) + (((p15+p7)+(p11+p3)) +
    ((p13+p5)+(p9+p1)))."""
    f = np.float32
    a = lambda i, j: (p[..., i] + p[..., j]).astype(f)
    left = ((a(0, 8) + a(12, 4)).astype(f) + (a(14, 6) + a(10, 2)).astype(f)).astype(f)
    right = ((a(15, 7) + a(11, 3)).astype(f) + (a(13, 5) + a(9, 1)).astype(f)).astype(f)
    return (left + right).astype(f)


def planes_scores(q, kslot, vslot):
    """q [H, D] fp16; kslot / vslot [n, H, D] fp16 in logical entry order -> [H, n] fp16 scores from one plane per feature."""
    hi, lo = np.maximum(kslot, vslot), np.minimum(kslot, vslot)
    neg = np.signbit(q)[None]                                             # the plane a feature reads: sign bit of q
    x = np.where(neg, lo, hi).astype(np.float32)                          # [n, H, D]
    prod = (q.astype(np.float32)[None] * x).reshape(x.shape[0], H, D // 8, 8)  # exact in fp32
    acc = np.zeros(prod.shape[:3], np.float32)
    for i in range(8):
        acc = (acc + prod[..., i]).astype(np.float32)
    return _tree(acc).astype(np.float16).T


def _raw_meta(seed, n_entries, layout):
    """Both slots N(0,1): the K slot is below the V slot about half the time."""
    n_meta = -(-n_entries // S)
    shape = (n_meta + 1, 2, H, S, D) if layout == oracle.HND else (n_meta + 1, 2, S, H, D)
    rng = np.random.default_rng(seed)
    data = rng.standard_normal(shape, dtype=np.float32).astype(np.float16)
    idx = rng.permutation(n_meta + 1)[:n_meta].astype(np.int32)
    return oracle.Paged(data, idx, (n_entries - 1) % S + 1, layout)


def _slots(meta, n):
    pages = meta.data[meta.indices]
    if meta.layout == oracle.HND:
        pages = pages.transpose(0, 1, 3, 2, 4)
    m = pages.shape[0]
    return pages[:, 0].reshape(m * S, H, D)[:n], pages[:, 1].reshape(m * S, H, D)[:n]


@pytest.mark.parametrize("n_entries,layout", ENTRIES)
@pytest.mark.parametrize("zeros", [False, True])
def test_one_plane_per_feature_and_the_row_tree_equal_the_oracle(n_entries, layout, zeros):
    meta = _raw_meta(7 * n_entries + layout, n_entries, layout)
    q = np.random.default_rng(n_entries).standard_normal((1, H, D), dtype=np.float32).astype(np.float16)
    if zeros:
        q[0, 1, 5] = 0.0
        q[0, 3, 77] = 0.0
    want = oracle.estimate(q, meta)
    assert want.shape == (H, n_entries - 1)
    k, v = _slots(meta, n_entries - 1)
    got = planes_scores(q[0], k, v)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint16), np.ascontiguousarray(want).view(np.uint16))


NEW_ENTRIES = ("quest_estimate_planes_bytes", "quest_estimate_planes_build", "quest_append_estimate_planes_batched")


def test_new_entries_are_exported_and_declared():
    from quest_amd import _lib

    header = open(os.path.join(ROOT, "include", "quest_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    # the size of a store: [kv heads][blocks of 256 pages][128 features][2 signs][256 pages] fp16, padded to whole blocks
    assert _lib.lib.quest_estimate_planes_bytes(4, 256) == 4 * 128 * 2 * 256 * 2
    assert _lib.lib.quest_estimate_planes_bytes(32, 257) == 32 * 2 * 128 * 2 * 256 * 2


def _view(heads=4, head_dim=128, page_size=16, dtype=0):
    from quest_amd._lib import PagedKV

    fake = 0x1000  # never dereferenced: every call below is refused before a launch
    return PagedKV(fake, fake, None, heads, page_size, head_dim, 0, 1, 0, 0, dtype)


def _launch(kv=None, meta=None, num_qo_heads=4, n_seqs=1, tile_off=0):
    from quest_amd._lib import Batch, lib

    fake = 0x1000
    return lib.quest_append_estimate_planes_batched(fake, fake, _view(**(kv or {})), fake, fake, num_qo_heads, 512, 300, tile_off,
                                                    _view(**(meta or {})), fake, Batch(n_seqs, 0, 0, 0, None), fake, 512, fake, None)


@pytest.mark.parametrize("what,kwargs", [
    ("two sequences", dict(n_seqs=2)),
    ("GQA", dict(num_qo_heads=8)),
    ("head_dim 64", dict(kv=dict(head_dim=64), meta=dict(head_dim=64))),
    ("metadata page size 8", dict(meta=dict(page_size=8))),
    ("KV page size 32", dict(kv=dict(page_size=32))),
    ("bf16", dict(kv=dict(dtype=1), meta=dict(dtype=1))),
    ("tile maxima", dict(tile_off=304)),
])
def test_unserved_shapes_are_refused_before_any_launch(what, kwargs):
    assert _launch(**kwargs) == EUNSUPPORTED, what


def test_build_refuses_unserved_shapes():
    from quest_amd._lib import lib

    fake = 0x1000
    for meta, kv_page in ((_view(head_dim=64), 16), (_view(page_size=8), 16), (_view(), 32), (_view(dtype=1), 16)):
        assert lib.quest_estimate_planes_build(fake, 512, fake, meta, kv_page, fake, None) == EUNSUPPORTED
    assert lib.quest_estimate_planes_build(fake, 300, fake, _view(), 16, fake, None) == -1  # not whole page blocks
