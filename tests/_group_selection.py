"""The numpy restatement of group-shared page selection (include/quest_hip.h, quest_decode_forward_group_topk), shared
by tests/test_group_selection_host.py and tests/test_gpu_group_selection.py:

  group score of page p for kv head hk = max over g < G of the order-preserving 16-bit key (``oracle.half_key``) of
  score[hk * G + g][p]; selection = ``oracle.topk`` of that row (k = min(budget - 1, pages - 1), keys above the
  threshold plus the lowest columns among ties, ascending column order).
"""
import numpy as np

import oracle


def key_to_half(keys: np.ndarray) -> np.ndarray:
    """Inverse of ``oracle.half_key``: uint16 keys -> the fp16 bit patterns they order."""
    k = np.ascontiguousarray(keys, dtype=np.uint16)
    return np.where(k & 0x8000, k & 0x7FFF, ~k).astype(np.uint16).view(np.float16)


def group_scores(scores: np.ndarray, group: int) -> np.ndarray:
    """``[Hq, n]`` fp16 page scores -> ``[Hq / group, n]`` fp16: per kv head and page the score with the largest key."""
    keys = oracle.half_key(scores)
    hq, n = keys.shape
    return key_to_half(keys.reshape(hq // group, group, n).max(axis=1))


def group_topk(scores: np.ndarray, table, group: int, k: int):
    """(values ``[Hkv, k]`` fp16, physical pages ``[Hkv, k]`` int32) the group-shared selection picks from ``scores``
    ``[Hq, n]`` over the page table ``table`` (its first n entries), k clamped to n."""
    g = group_scores(scores, group)
    hk, n = g.shape
    return oracle.topk(g, np.tile(np.asarray(table, np.int32)[:n], (hk, 1)), k)


def expand(idx: np.ndarray, group: int) -> np.ndarray:
    """``[Hkv, k]`` -> ``[Hq, k]``: every row repeated for the heads of its group."""
    return np.repeat(idx, group, axis=0)
