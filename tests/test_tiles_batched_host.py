"""Host side of the tiles form (tile_max_offset != 0) of quest_append_estimate_batched /
quest_decode_forward_fused_topk_batched: the entries carry the offset, malformed arguments are refused
before anything is launched (no GPU needed), and the row layout arithmetic a batched score scratch relies on."""
import ctypes

import pytest


def test_batched_tiles_symbols_are_exported_and_declared():
    from quest_amd._lib import SIGNATURES, Batch, lib

    for name in ("quest_append_estimate_batched", "quest_decode_forward_fused_topk_batched"):
        assert name in SIGNATURES, name
        assert getattr(lib, name) is not None
        args = SIGNATURES[name][1]
        assert Batch in args  # a quest_batch_t by value
        # tile_max_offset: the u32 behind (stride, max_n), the third of three
        assert args[6:9] == [ctypes.c_uint32] * 3 and args[9] is not ctypes.c_uint32


def test_batched_tiles_entries_validate_arguments_without_gpu():
    from quest_amd._kernels import tile_max_offset, tiles_row_stride
    from quest_amd._lib import Batch, PagedKV, lib

    est = lib.quest_append_estimate_batched
    att = lib.quest_decode_forward_fused_topk_batched
    one = ctypes.c_void_p(16)  # non-null, 16-byte aligned; never dereferenced by the checks
    kv = PagedKV(data=16, indices=16, indptr=16, num_heads=32, page_size=16, head_dim=128, page_budget=0,
                 last_page_len=1, last_page_idx=0, layout=0)
    max_n = 100
    off, stride = tile_max_offset(max_n), tiles_row_stride(max_n)
    b2 = Batch(2, max_n + 4, 8, 0, None)
    EINVAL, ESTATE = -1, -3
    # ---- estimate side
    assert est(one, one, kv, one, one, 32, stride, max_n, off + 8, kv, one, b2, None) == EINVAL      # not max_n rounded up to 8
    assert est(one, one, kv, one, one, 32, off + 8, max_n, off, kv, one, b2, None) == EINVAL         # stride without room
    assert est(one, one, kv, one, one, 32, off, max_n, off, kv, one, b2, None) == EINVAL
    assert est(one, one, kv, one, ctypes.c_void_p(24), 32, stride, max_n, off, kv, one, b2, None) == EINVAL  # misaligned rows
    assert est(one, one, kv, one, one, 32, stride, max_n, off, kv, one, Batch(0, 0, 0, 0, None), None) == EINVAL  # n_seqs == 0
    assert est(one, one, kv, one, one, 32, stride, max_n, off, kv, one, Batch(2, max_n + 4, 6, 0, None), None) == EINVAL  # 6 * 16 < 100
    assert est(one, one, kv, one, one, 32, stride, max_n, off, kv, None, b2, None) == EINVAL         # no state
    # ---- attention side
    h = ctypes.c_void_p()
    assert lib.quest_decode_handler_create(ctypes.byref(h), 0) == 0
    try:
        assert att(h, one, one, kv, 32, one, max_n - 4, max_n, off, one, b2, None, None) == EINVAL  # stride < max_n
        assert att(h, one, one, kv, 32, one, stride, max_n, off, one, Batch(0, 0, 0, 0, None), None, None) == EINVAL
        assert att(h, one, one, kv, 32, one, stride, max_n, off, one, Batch(2, max_n, 8, 0, None), None, None) == EINVAL  # table stride < max_n + 1
        assert att(h, one, one, kv, 32, None, stride, max_n, off, one, b2, None, None) == EINVAL   # no scores
        assert att(h, one, one, kv, 32, one, stride, max_n, off, None, b2, None, None) == EINVAL   # no state
        assert att(h, one, one, kv, 32, one, stride, max_n, off, one, b2, None, None) == ESTATE    # no plan
        info = (ctypes.c_uint32 * 6)()
        assert lib.quest_decode_last_launch_info(h, info) == 0 and list(info) == [0] * 6             # nothing was launched
    finally:
        lib.quest_decode_handler_destroy(h)


@pytest.mark.parametrize("max_n", [1, 7, 8, 9, 63, 64, 100, 2047, 4096, 4097, 8191, 8319, 16383, 16384])
def test_tiles_row_layout_arithmetic(max_n):
    """What a batched score scratch relies on: the maxima start at the scores padded to 8 columns, every row of a
    ``[n_seqs, Hq, stride]`` tensor stays 16-byte aligned, and the stride holds one 16-bit key per run of 8 pages,
    readable in 4-key pieces."""
    from quest_amd._kernels import tile_max_offset, tiles_row_stride

    off, stride = tile_max_offset(max_n), tiles_row_stride(max_n)
    n_tiles = (max_n + 7) // 8
    assert off % 8 == 0 and max_n <= off < max_n + 8
    assert stride % 8 == 0                               # fp16 columns: rows 16 bytes apart modulo 16
    assert stride >= off + (n_tiles + 3) // 4 * 4        # what the C entries check
    assert stride < off + n_tiles + 12                   # and no more than the padding needs


def test_batched_score_scratch_keeps_its_shape_below_the_threshold():
    import torch

    import quest_amd.utils as qu
    from quest_amd import _kernels

    class Ctl(qu.BatchedInferenceController):  # shape logic only: no pools
        def __init__(self, max_pages, **kw):
            self.n_seqs, self.num_heads, self.max_pages, self.device = 3, 4, max_pages, torch.device("cpu")
            self.__dict__.update(kw)

    assert tuple(qu.score_scratch(Ctl(2055)).shape) == (3, 4, 2056)            # as before this feature
    assert tuple(qu.score_scratch(Ctl(4097)).shape) == (3, 4, 4104)            # 4096 columns: below 4097
    long_ = qu.score_scratch(Ctl(8320))
    assert tuple(long_.shape) == (3, 4, _kernels.tiles_row_stride(8319)) and long_.size(2) > 8320
    assert tuple(qu.score_scratch(Ctl(300, tiles_min_pages=64)).shape) == (3, 4, _kernels.tiles_row_stride(299))
    assert tuple(qu.score_scratch(Ctl(8320, tiles_min_pages=1 << 30)).shape) == (3, 4, 8320)
