"""Per-sequence decode state: page tables, budgets, top-k buffers, handler lifecycle.

Mirrors the reference's ``InferenceController`` (quest/utils/controller.py:7-146) attribute for
attribute, because ``quest.utils``' wrappers and ``QuestAttention`` read these fields directly.
Behavioural contract kept: ``prepare_metadata`` -> ``begin_forward`` -> ops -> ``end_forward``;
``page_budget`` is in PAGES and includes the current page (controller.py:14); the first call of a
decode step may pass ``updateTensor=False`` to re-plan with another budget without touching the
index tensors (llama.py:434-439 layer-skip).

What differs is cost, not meaning: index tensors are views/expansions of a device-resident page
table (no Python-list -> tensor rebuild per token), small indptr tensors are cached by value, and
top-k output buffers are reused while the budget is unchanged.  Extension: ``num_kv_heads`` for
GQA pools (per-query-head selection).
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Tuple

import torch

from .decode_wrapper import BatchDecodeWithPagedKVCacheWrapper
from .kv_cache import KvCache
from .utils import TensorLayout


# State-driven sparse layers (``quest_amd.utils.decode_layer_dyn`` / ``decode_layer_batched``): pools from this many pages
# per sequence up take the tiles launches (tile maxima handed from the estimate to the attention launch); below, every
# workgroup of a head selects over the whole row.  A controller's ``tiles_min_pages`` overrides it.
TILES_MIN_PAGES = 4097
QUEST_EUNSUPPORTED = -2  # include/quest_hip.h


def _state_row(c: "InferenceController"):
    """quest_step_state_t (include/quest_hip.h) of one sequence's caches, as its 8 ints."""
    kv, meta = c.kv_cache, c.metadata_cache
    return [kv.seqlen, len(kv.indicies), kv.last_page_len, kv.indicies[-1], len(meta.indicies), meta.last_page_len,
            meta.indicies[-1], 0]


def _check_estimate_shape(num_heads: int, num_kv_heads: int, head_dim: int, layout: int) -> None:
    """Refuse at construction a shape whose page-score estimate the library refuses on THIS pool layout and serves on
    another one (``quest_estimate_plan``, include/quest_hip.h: head_dim 256 with 8 query heads per kv head on the
    row-rotated pool when the kv heads are a multiple of 4) -- such a controller would build its pools and then fail inside
    its first sparse decode step.  The tiles form is refused wherever the whole-row form is, so there is no other route.
    Shapes no layout serves (a group or head_dim outside the built set) are left to the operators, as before: a controller
    may still run full attention over them."""
    from .._lib import lib

    info = (ctypes.c_uint32 * 3)()
    if lib.quest_estimate_plan(head_dim, num_heads, num_kv_heads, layout, 0, info) != QUEST_EUNSUPPORTED:
        return
    serving = [TensorLayout.FORMAT2STR[other] for other in sorted(TensorLayout.FORMAT2STR)
               if other != layout and lib.quest_estimate_plan(head_dim, num_heads, num_kv_heads, other, 0, info) == 0]
    if serving:
        raise ValueError(
            f"the page-score estimate does not serve {num_heads} query heads / {num_kv_heads} kv heads x head_dim {head_dim} "
            f"on kv_layout {TensorLayout.FORMAT2STR[layout]} (whole rows or tiles form: QUEST_EUNSUPPORTED from "
            f"quest_estimate_plan); layouts that serve this shape: {', '.join(serving)}")


# the envelope of the group-selection launch (quest_decode_forward_group_topk, include/quest_hip.h)
GROUP_TOPK_MAX_ROW, GROUP_TOPK_MAX_SELECTED, GROUP_TOPK_MAX_SEQS = 4096, 256, 64


def _check_group_selection(num_heads: int, num_kv_heads: int, head_dim: int, page_size: int, page_budget: int,
                           max_seq_len: int, n_seqs: int = 1) -> None:
    """Refuse at construction a ``group_selection=True`` controller whose shape the group-selection launch does not serve.
    There is no silent fall back to per-head selection: that would change which pages a model attends."""
    group = num_heads // num_kv_heads
    pages = (max_seq_len + page_size - 1) // page_size
    why = None
    if page_size != 16:
        why = f"page_size {page_size} (the launch serves page size 16)"
    elif head_dim not in (64, 128):
        why = f"head_dim {head_dim} (the launch serves head_dim 64 and 128)"
    elif group not in (1, 2, 4, 8):
        why = f"{group} query heads per kv head (the launch serves groups of 1, 2, 4 and 8)"
    elif page_budget - 1 > GROUP_TOPK_MAX_SELECTED:
        why = (f"a budget of {page_budget} pages (the launch selects at most {GROUP_TOPK_MAX_SELECTED} pages besides the "
               "current one)")
    elif pages - 1 > GROUP_TOPK_MAX_ROW:
        why = (f"a pool of {pages} pages per sequence (the launch serves score rows of at most {GROUP_TOPK_MAX_ROW} pages: "
               f"max_seq_len <= {(GROUP_TOPK_MAX_ROW + 1) * page_size} tokens)")
    elif n_seqs > GROUP_TOPK_MAX_SEQS:
        why = f"{n_seqs} sequences (the launch serves at most {GROUP_TOPK_MAX_SEQS})"
    if why:
        raise ValueError(f"group_selection=True does not serve {why}")


def _make_handler(layout: int, dtype):
    """A decode handler for pools of ``layout`` and ``dtype``: built the reference's way (fp16) unless the controller is
    bf16, which is the handler's explicit extension."""
    extra = {} if dtype == torch.float16 else {"dtype": dtype}
    return BatchDecodeWithPagedKVCacheWrapper(kv_layout=TensorLayout.FORMAT2STR[layout], **extra)


def _plan_graph_handlers(ctl, budget: int, dense_layers: bool) -> None:
    """Plan ``ctl``'s sparse handler for ``budget`` pages and, with ``dense_layers``, a second handler for full-KV layers
    over the per-sequence capacity -- once, for launches that will be replayed over many tokens."""
    plans = [(ctl._decode_handler, budget)]
    if dense_layers:
        if ctl._dense_handler is None:
            ctl._dense_handler = _make_handler(ctl.layout, ctl.dtype)
        plans.append((ctl._dense_handler, ctl.max_pages))
    for handler, pages in plans:
        handler.set_batch(ctl.n_seqs)
        handler.begin_forward(torch.tensor([0, pages - 1], dtype=torch.int32), ctl.num_heads, ctl.num_kv_heads,
                              ctl.head_dim, ctl.page_size, ctl.dtype)


class InferenceController:
    # what a state-driven launch reads (quest_amd.utils.decode_layer_*): the sequence is a batch of one, with no
    # per-sequence budgets and no one-launch layers (that form needs a batch that fills the chip)
    n_seqs = 1
    page_budgets = None
    one_launch_layers = False
    tiles_min_pages = TILES_MIN_PAGES
    dtype = torch.float16  # element type of pools, handlers, top-k buffers and score scratch; the constructor's argument
    # sign planes for the sparse layers' estimate where the shape is eligible (estimate_planes_eligible); False = never
    estimate_planes = True
    # opt-in: ONE page selection per kv head (the key-max of its group's scores), attended by all heads of the group
    # (quest_decode_forward_group_topk); the default is the reference's selection per query head
    group_selection = False
    _planes = _planes_covered = None
    _planes_pages = 0
    _planes_registered = False

    def __init__(self, num_layers, num_heads, head_dim, page_size,
                 page_budget,  # pages, including the last (current) page
                 max_seq_len,  # capacity of the KV / metadata pools, in tokens
                 dtype, device, num_kv_heads: Optional[int] = None, layout: int = TensorLayout.NHD,
                 shuffle_seed: Optional[int] = None, kv_pool=None, metadata_pool=None, group_selection: bool = False):
        self.num_heads = num_heads
        self.num_kv_heads = num_heads if num_kv_heads is None else num_kv_heads
        if self.num_heads % self.num_kv_heads != 0:
            raise ValueError(f"num_heads {num_heads} is not a multiple of num_kv_heads {num_kv_heads}")
        self.head_dim = head_dim
        self.page_size = page_size
        self.layout = TensorLayout.parse(layout)
        _check_estimate_shape(self.num_heads, self.num_kv_heads, head_dim, self.layout)
        self.group_selection = bool(group_selection)
        if self.group_selection:
            _check_group_selection(self.num_heads, self.num_kv_heads, head_dim, page_size, page_budget, max_seq_len)
        self.device = device
        self.dtype = dtype

        max_kv_pages = (max_seq_len + page_size - 1) // page_size
        self.kv_cache = KvCache(num_layers, self.num_kv_heads, head_dim, max_seq_len, page_size, dtype, device,
                                self.layout, shuffle_seed, pool=kv_pool)
        # one metadata entry (max in the K slot, min in the V slot) per KV page: controller.py:29-37
        self.metadata_cache = KvCache(num_layers, self.num_kv_heads, head_dim, max_kv_pages, page_size, dtype, device,
                                      self.layout, None if shuffle_seed is None else shuffle_seed + 1,
                                      pool=metadata_pool)

        self._page_budget = page_budget
        # (pools, handlers, top-k buffers and the score scratch all follow `dtype`: float16 or bfloat16)
        self._decode_handler = _make_handler(self.layout, dtype)
        self._dense_handler = None  # planned by begin_graph_decode(dense_layers=True)

        self.kv_indices_with_last = None
        self.kv_indices_without_last = None
        self.metadata_indices = None
        self.kv_last_page_idx = None
        self.metadata_last_page_idx = None
        self.kv_indptr_for_append = None
        self.metadata_indptr_for_append = None
        self.kv_indptr_for_approx_decode = None
        self.inference_page_budget = None
        self.topk_dout_buffer = None
        self.topk_dindices_buffer = None
        self.topk_buf = None

        self._indptr_cache: Dict[Tuple[int, int], torch.Tensor] = {}
        self._without_last_pages = -1
        # top-k output buffers, one pair per distinct width (the model alternates between the full-KV plan of its
        # first layers and the real budget on every token, llama.py:428-439: keyed by width they are allocated once)
        self._topk_buffers: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        # device-resident step state (enable_device_state); state_epoch changes whenever graphs captured over it go stale
        self.kv_table_full = self.meta_table_full = self.step_state = None
        self.kv_tables = self.meta_tables = self.step_states = None  # the same three as the one-row matrices of a batch
        self.state_epoch = 0

    # ------------------------------------------------------------------ budgets
    @property
    def page_budget_pages(self) -> int:
        return self._page_budget

    @property
    def token_budget(self) -> int:
        return self._page_budget * self.page_size

    def set_page_budget(self, page_budget: int) -> None:
        self._page_budget = page_budget

    # ------------------------------------------------------------------ step lifecycle
    def prepare_metadata(self, seq_len: int) -> None:
        """Reserve pages for ``seq_len`` new tokens and metadata entries for the pages they open."""
        new_pages = self.kv_cache.append_seq(seq_len)
        self.metadata_cache.append_seq(new_pages)

    def _indptr(self, n: int) -> torch.Tensor:
        t = self._indptr_cache.get((0, n))
        if t is None:
            if len(self._indptr_cache) > 64:
                self._indptr_cache.clear()
            t = torch.tensor([0, n], dtype=torch.int32, device=self.device)
            self._indptr_cache[(0, n)] = t
        return t

    def begin_forward(self, seq_len: int, updateTensor: bool = True) -> None:
        n_pages = len(self.kv_cache.indicies)
        n_meta = len(self.metadata_cache.indicies)
        if updateTensor:
            self.kv_indptr_for_append = self._indptr(n_pages)
            self.metadata_indptr_for_append = self._indptr(n_meta)
            self.kv_last_page_idx = self.kv_cache.indicies[-1]
            self.metadata_last_page_idx = self.metadata_cache.indicies[-1]
            self.kv_indices_with_last = self.kv_cache.device_table()
            self.metadata_indices = self.metadata_cache.device_table()

        if seq_len > 1:
            return  # prefill: append_kv_cache_prefill + prefill_with_paged_kv_cache need nothing else

        assert n_pages >= 1, "decode needs a non-empty cache"  # one page: attention over the current page only
        if updateTensor and self._without_last_pages != n_pages:
            # input ids of the top-k ([H, n_pages-1], controller.py:106), rebuilt only when a page was added
            self.kv_indices_without_last = self.kv_indices_with_last[:-1].unsqueeze(0).expand(
                self.num_heads, n_pages - 1).contiguous()
            self._without_last_pages = n_pages

        budget = min(self._page_budget, n_pages)
        # keyed on the buffer WIDTH, not on inference_page_budget (begin_graph_decode sets the latter without
        # allocating): a buffer narrower than budget - 1 would be written out of bounds by topk_filtering
        if self.topk_dout_buffer is None or self.topk_dout_buffer.size(1) != budget - 1:
            pair = self._topk_buffers.get(budget - 1)
            if pair is None:
                if len(self._topk_buffers) >= 8:  # a growing dense-regime sequence asks for a new width per page
                    self._topk_buffers.clear()
                pair = (torch.zeros((self.num_heads, budget - 1), dtype=self.dtype, device=self.device),
                        torch.zeros((self.num_heads, budget - 1), dtype=torch.int32, device=self.device))
                self._topk_buffers[budget - 1] = pair
            self.topk_dout_buffer, self.topk_dindices_buffer = pair
            if self.topk_buf is None:  # scratch argument of the reference's RAFT call; unused here
                self.topk_buf = torch.zeros((self.num_heads, 8), dtype=self.dtype, device=self.device)
        self.inference_page_budget = budget
        self.kv_indptr_for_approx_decode = self._indptr(budget - 1)
        # the planner wants the count on the host: hand it a CPU indptr (no device round trip)
        self._decode_handler.begin_forward(torch.tensor([0, budget - 1], dtype=torch.int32), self.num_heads,
                                           self.num_kv_heads, self.head_dim, self.page_size, self.dtype)

    def end_forward(self) -> None:
        self._decode_handler.end_forward()

    # ------------------------------------------------------------------ device-resident step state
    def enable_device_state(self) -> None:
        """Put the sequence's step state (lengths, last-page ids) in device memory so that a decode step
        captured in a hipGraph can be replayed while the sequence grows (EXTENSION).  Call
        after prefill; the state describes the cache BEFORE the next token -- the graph's first node,
        ``_kernels.step_state_advance_batched``, moves it forward by one token on the device."""
        self.kv_table_full = self.kv_cache.full_device_table()
        self.meta_table_full = self.metadata_cache.full_device_table()
        self.max_pages = self.kv_table_full.numel()
        self.step_state = torch.zeros(8, dtype=torch.int32, device=self.device)
        # the same memory as the one-row matrices of a batch (views: a captured graph holds the addresses)
        self.kv_tables, self.meta_tables = self.kv_table_full.view(1, -1), self.meta_table_full.view(1, -1)
        self.step_states = self.step_state.view(1, -1)
        self.state_epoch += 1  # graphs captured before this call are stale
        self.sync_device_state()

    def begin_graph_decode(self, dense_layers: bool = False) -> None:
        """Plan the sparse decode for the configured budget once, for a graph that will be replayed over
        many tokens (the plan depends only on the budget).  With
        ``dense_layers`` a second handler is planned for full-KV layers (the model's first layers,
        llama.py:428-430) over the pool's capacity."""
        # The sequence may still be shorter than the budget: the state-driven attention launch then selects all
        # of its pages (k = n), which is the reference's full-attention branch (QuestAttention.py:123-132), and
        # moves into the sparse regime by itself as the sequence grows -- same graph.
        assert len(self.kv_cache.indicies) >= 1, "prefill first"
        self.inference_page_budget = min(self._page_budget, self.max_pages)
        _plan_graph_handlers(self, self.inference_page_budget, dense_layers)
        self._build_estimate_planes()

    # ------------------------------------------------------------------ sign planes (csrc/estimate_planes.hip)
    def estimate_planes_eligible(self) -> bool:
        """Whether the sparse layers of this controller read their page scores from sign planes: a shadow store of each
        layer's metadata, per (kv head, feature, sign of q) contiguous over logical pages, of which the MHA estimate
        fetches half.  One fp16 MHA sequence, head_dim 128, page size 16, a budget below the pool's
        capacity (else every layer is dense), rows short of the tiles launches; ``estimate_planes = False`` or
        QUEST_ESTIMATE_PLANES=0 switch it off."""
        return bool(self.estimate_planes) and os.environ.get("QUEST_ESTIMATE_PLANES", "1") != "0" \
            and self.n_seqs == 1 and self.num_heads == self.num_kv_heads and self.head_dim == 128 \
            and self.page_size == 16 and self.dtype == torch.float16 and self.step_state is not None \
            and self.inference_page_budget is not None and self.inference_page_budget < self.max_pages \
            and self.max_pages - 1 < self.tiles_min_pages  # (longer rows take the tiles launches, which read the pool)

    def _build_estimate_planes(self) -> None:
        """Allocate the planes once, then per layer: transpose the complete pages' metadata into them (``covered`` = their
        number) and register the store in ``_kernels``, whose append + estimate launch over this layer then takes it.  The
        device state must describe tokens that are in the pools (after the prefill, between decode tokens)."""
        from .. import _kernels

        self._drop_estimate_planes()
        if not self.estimate_planes_eligible():
            return
        layers = self.metadata_cache.pool.num_layers
        pages = _kernels.plane_pages_for(self.max_pages)
        halves = _kernels.estimate_planes_bytes(self.num_kv_heads, pages) // 2
        if self._planes is None or tuple(self._planes.shape) != (layers, halves):
            # ordinary tensors whatever mode the caller is in (a model's prefill runs under inference_mode, resets do not):
            # only the kernels and the two in-place updates below ever write them
            with torch.inference_mode(False):
                self._planes = torch.empty((layers, halves), dtype=torch.float16, device=self.device)
                self._planes_covered = torch.zeros(layers, dtype=torch.int32, device=self.device)
        self._planes_pages = pages
        for l in range(layers):
            meta = self.metadata_layer(l)
            _kernels.estimate_planes_build(self._planes[l], pages, self._planes_covered[l:l + 1], meta, self.meta_table_full,
                                           self.step_state, self.page_size, self.layout)
            _kernels.register_estimate_planes(meta, self.meta_table_full, self.step_state, self._planes[l],
                                              self._planes_covered[l:l + 1], pages)
        self._planes_registered = True

    def _drop_estimate_planes(self) -> None:
        """Zero ``covered`` and drop the registrations: the next launches read the metadata pool."""
        if not self._planes_registered:
            return
        from .. import _kernels

        self._planes_registered = False
        with torch.inference_mode():  # (an in-place update is allowed there for every kind of tensor)
            self._planes_covered.zero_()
        for l in range(self.metadata_cache.pool.num_layers):
            _kernels.unregister_estimate_planes(self.metadata_layer(l), self.step_state)

    def sync_device_state(self) -> None:
        self.step_state.copy_(torch.tensor(_state_row(self), dtype=torch.int32))
        if self._planes_registered:
            # the cache may have been set back: the mirror's last page and everything behind it are no longer vouched for
            # (the mirror may run one reserved token ahead, so a last page that looks full may still lack its token; a
            # planes launch that completes a page writes its entries again and counts on from there)
            with torch.inference_mode():
                self._planes_covered.clamp_(max=len(self.kv_cache.indicies) - 1)

    def kv_layer(self, layer_idx: int) -> torch.Tensor:
        return self.kv_cache.buf_layer(layer_idx)

    def metadata_layer(self, layer_idx: int) -> torch.Tensor:
        return self.metadata_cache.buf_layer(layer_idx)

    def need_estimate(self) -> bool:
        if self.inference_page_budget is None:
            return False
        return len(self.kv_cache.indicies) > self.inference_page_budget

    def clean_states(self) -> None:
        self.kv_cache.release()
        self.metadata_cache.release()
        self._without_last_pages = -1
        self.inference_page_budget = None
        # a captured decode graph holds the page tables / step state of the request that just ended: drop them so
        # that a stale graph cannot be replayed over the next request's pages (callers re-capture after prefill)
        self.invalidate_device_state()

    def invalidate_device_state(self) -> None:
        self._drop_estimate_planes()  # covered = 0, registrations dropped: the store says nothing about the next request
        self.kv_table_full = self.meta_table_full = self.step_state = None
        self.kv_tables = self.meta_tables = self.step_states = None
        self.state_epoch += 1  # graphs captured before this call are stale


class BatchedInferenceController:
    """``n_seqs`` independent sequences decoded with ONE launch per op (EXTENSION; SURVEY 8f-3: the reference
    fixes ``batch_size = 1``, approx_attn.cu:113; BASELINE config 5 decodes 8 sequences per GPU).

    All sequences share one KV pool and one metadata pool (each reserves its ``max_seq_len`` worth of pages up
    front); ``self.seqs[i]`` is an ordinary ``InferenceController`` over those pools, so prefill and the eager
    single-sequence ops work on each sequence exactly as before.  After prefill, ``enable_device_state()``
    stacks the page tables / step states and the ``*_batched`` wrappers of ``quest_amd.utils`` run every
    sequence of a decode step in one grid (grid.z = sequence); results per sequence are bit-identical to the
    single-sequence path."""

    tiles_min_pages = TILES_MIN_PAGES
    dtype = torch.float16  # element type of pools, handlers, top-k buffers and score scratch; the constructor's argument

    def __init__(self, n_seqs, num_layers, num_heads, head_dim, page_size, page_budget, max_seq_len, dtype, device,
                 num_kv_heads: Optional[int] = None, layout: int = TensorLayout.NHD,
                 shuffle_seed: Optional[int] = None, group_selection: bool = False):
        from .kv_cache import KvPool

        if n_seqs <= 0:
            raise ValueError("n_seqs must be positive")
        self.n_seqs = n_seqs
        self.num_heads = num_heads
        self.num_kv_heads = num_heads if num_kv_heads is None else num_kv_heads
        self.head_dim, self.page_size, self.device, self.dtype = head_dim, page_size, device, dtype
        self.layout = TensorLayout.parse(layout)
        if self.num_heads % self.num_kv_heads != 0:
            raise ValueError(f"num_heads {num_heads} is not a multiple of num_kv_heads {num_kv_heads}")
        _check_estimate_shape(self.num_heads, self.num_kv_heads, head_dim, self.layout)  # before the shared pools exist
        self.group_selection = bool(group_selection)  # InferenceController.group_selection, for every sequence
        if self.group_selection:
            _check_group_selection(self.num_heads, self.num_kv_heads, head_dim, page_size, page_budget, max_seq_len, n_seqs)
        self._page_budget = page_budget
        pages = (max_seq_len + page_size - 1) // page_size
        meta_pages = (pages + page_size - 1) // page_size
        self.kv_pool = KvPool(num_layers, self.num_kv_heads, head_dim, n_seqs * pages, page_size, dtype, device,
                              self.layout, shuffle_seed)
        self.metadata_pool = KvPool(num_layers, self.num_kv_heads, head_dim, n_seqs * meta_pages, page_size, dtype,
                                    device, self.layout, None if shuffle_seed is None else shuffle_seed + 1)
        self.seqs = [InferenceController(num_layers, num_heads, head_dim, page_size, page_budget, max_seq_len, dtype,
                                         device, num_kv_heads=num_kv_heads, layout=layout, kv_pool=self.kv_pool,
                                         metadata_pool=self.metadata_pool, group_selection=group_selection)
                     for _ in range(n_seqs)]
        self._decode_handler = _make_handler(self.layout, dtype)
        self._dense_handler = None
        self.kv_tables = self.meta_tables = self.step_states = None
        self.state_epoch = 0
        # per-sequence page budgets: ONE persistent int32 [n_seqs] device buffer (a captured graph holds its address),
        # rewritten in place by set_page_budgets; kNoBudget = "the planned budget" (the kernels clamp to the plan)
        self._budget_buf = None
        self.page_budgets = None      # the buffer once set_page_budgets has been called with a list, else None
        self._host_budgets = None
        self._graph_budget_ptr = 0    # what begin_graph_decode planned with: 0 = no per-sequence budgets
        self.topk_dout_buffer = self.topk_dindices_buffer = None
        self._planned = None
        self._graph_planned = 0       # budget begin_graph_decode planned for (0: no graph plan)
        # decode_layer_batched: one launch per layer (csrc/layer_device.cuh) where the plan allows it AND it pays: its grid
        # is one workgroup per (sequence, head), each bound by what ONE CU moves, so it needs the chip filled in whole
        # rounds -- measured at cfg-3 shapes, us per sequence-layer one / two launches: 5 sequences (160 workgroups on 256
        # CUs) 13.27 / 13.01, 6: 12.03 / 12.47, 7: 11.64 / 11.96, 8: 11.15 / 11.60, 12 (1.5 per CU) 12.10 / 11.86, 16: 11.02 /
        # 11.16 (profiles/r05_sweep_sequences_per_gpu_one_vs_two_launches.txt).  With GQA the query heads of a group would
        # each stream their kv head's metadata (cfg 5: 68.9 vs 58.8 us per layer): two launches.
        # (fp16 only: the one-launch layer has no bf16 form -- quest_decode_layer_fused_batched returns QUEST_EUNSUPPORTED)
        self.one_launch_layers = (dtype == torch.float16 and self.num_heads == self.num_kv_heads
                                  and self._fills_the_chip(n_seqs * num_heads, device))
        self.last_layer_launches = None  # 1 / 2: which form utils.decode_layer_batched ran last (its docstring)

    @staticmethod
    def _fills_the_chip(workgroups: int, device) -> bool:
        """Does a grid of `workgroups` one-per-CU-sized workgroups use the chip's CUs in (nearly) whole rounds?"""
        cus = 256  # MI355X
        try:
            dev = torch.device(device)
            if dev.type == "cuda" and torch.cuda.is_available():
                cus = torch.cuda.get_device_properties(dev).multi_processor_count
        except Exception:  # noqa: BLE001  (CPU-only host logic tests)
            pass
        rounds = -(-workgroups // cus)
        return workgroups / (rounds * cus) >= (0.75 if rounds == 1 else 0.8)

    # ---- per-sequence page budgets + eager (host-planned) batched steps.  The reference keeps one controller and one
    # page budget per request and loops over requests in Python (controller.py:39-41, :80-129: five list -> tensor
    # copies per token per request); here a step of the whole batch is ONE small host -> device copy of the sequences'
    # lengths, and every operator runs once for all sequences (quest_amd.utils.*_batched).
    def set_page_budgets(self, budgets) -> None:
        """Pages each sequence attends per step INCLUDING its current page (None: the constructor's budget for all).
        A sequence with fewer pages than its budget attends all of them."""
        if budgets is None:
            if self._graph_budget_ptr:
                # a captured step reads the buffer: "no per-sequence budget" = the sentinel, in place.  The kernels clamp
                # to the CAPTURED plan, so the constructor's budget can only be honoured if the plan covers it
                if min(self._page_budget, self.max_pages) > self._graph_planned:
                    raise RuntimeError(f"the constructor's budget ({self._page_budget} pages) exceeds the {self._graph_planned} "
                                       "pages the captured plan was made for; call begin_graph_decode() (and re-capture) "
                                       "after dropping the per-sequence budgets")
                self._budget_buf.fill_(self.kNoBudget)
                self._host_budgets = None
                return
            self.page_budgets = self._host_budgets = None
            return
        budgets = [int(x) for x in budgets]
        if len(budgets) != self.n_seqs or min(budgets) < 1:
            raise ValueError("one page budget >= 1 per sequence")
        if self._graph_planned and not self._graph_budget_ptr:
            raise RuntimeError("per-sequence budgets set after begin_graph_decode() planned without them: a captured "
                               "graph would ignore them; call set_page_budgets() before begin_graph_decode()")
        if self._graph_planned and max(budgets) > self._graph_planned:
            raise RuntimeError(f"budget {max(budgets)} exceeds the {self._graph_planned} pages the captured plan was "
                               "made for; call begin_graph_decode() (and re-capture) after raising budgets")
        self._host_budgets = budgets
        if self._budget_buf is None:
            self._budget_buf = torch.empty(self.n_seqs, dtype=torch.int32, device=self.device)
        self._budget_buf.copy_(torch.tensor(budgets, dtype=torch.int32))
        self.page_budgets = self._budget_buf

    kNoBudget = 2 ** 31 - 1

    def max_page_budget(self) -> int:
        return max(self._host_budgets) if self._host_budgets is not None else self._page_budget

    def begin_forward(self) -> None:
        """Plan one eager decode step of the batch after ``prepare_metadata(1)``: upload the sequences' lengths
        (``[n_seqs, 8]`` int32, one copy) and (re)plan the decode handler for the largest budget."""
        if self.step_states is None:
            raise RuntimeError("call enable_device_state() after the prefill")
        self.sync_device_state()
        budget = min(self.max_page_budget(), self.max_pages)
        if self._planned != budget:
            self._decode_handler.set_batch(self.n_seqs)
            self._decode_handler.begin_forward(torch.tensor([0, budget - 1], dtype=torch.int32), self.num_heads,
                                               self.num_kv_heads, self.head_dim, self.page_size, self.dtype)
            self._planned = budget
        # keyed on the buffers' WIDTH, not on _planned: begin_graph_decode plans without allocating them
        k = max(budget - 1, 1)
        if self.topk_dout_buffer is None or self.topk_dout_buffer.size(2) != k:
            self.topk_dout_buffer = torch.zeros(self.n_seqs, self.num_heads, k, dtype=self.dtype, device=self.device)
            self.topk_dindices_buffer = torch.zeros(self.n_seqs, self.num_heads, k, dtype=torch.int32, device=self.device)
        self.inference_page_budget = budget

    def end_forward(self) -> None:
        pass  # nothing to release: tables, states and the handler's workspace persist across steps

    def kv_layer(self, layer_idx: int) -> torch.Tensor:
        return self.kv_pool.layer(layer_idx)

    def metadata_layer(self, layer_idx: int) -> torch.Tensor:
        return self.metadata_pool.layer(layer_idx)

    def prepare_metadata(self, seq_len: int = 1) -> None:
        """Host mirror of the device-side reservation (``step_advance_batched``) for every sequence."""
        for c in self.seqs:
            c.prepare_metadata(seq_len)

    def enable_device_state(self) -> None:
        self.kv_tables = self._stack_tables([c.kv_cache.full_device_table() for c in self.seqs])
        self.meta_tables = self._stack_tables([c.metadata_cache.full_device_table() for c in self.seqs])
        self.max_pages = self.kv_tables.size(1)
        self.step_states = torch.zeros(self.n_seqs, 8, dtype=torch.int32, device=self.device)
        self.state_epoch += 1
        self.sync_device_state()

    @staticmethod
    def _stack_tables(tables) -> torch.Tensor:
        """``[n_seqs, capacity]`` view of a buffer whose rows are padded to a multiple of 4 entries: every sequence's
        table then starts 16-byte aligned, which the fused attention launch needs to fetch 4 page ids with one load
        (a stride of exactly `capacity` entries -- 2055, 2065, 2179 in the bench -- made every batched launch take the
        scalar-load front end).  The pad entries repeat the row's last page and are never indexed."""
        cap = tables[0].numel()
        stride = (cap + 3) // 4 * 4
        buf = torch.empty(len(tables), stride, dtype=torch.int32, device=tables[0].device)
        for row, t in zip(buf, tables):
            row[:cap] = t
            row[cap:] = t[-1]
        return buf[:, :cap]

    def sync_device_state(self) -> None:
        self.step_states.copy_(torch.tensor([_state_row(c) for c in self.seqs], dtype=torch.int32))

    def begin_graph_decode(self, dense_layers: bool = False) -> None:
        """Plan the batched sparse decode once for the configured budget (every sequence must already be in
        the sparse regime), and optionally the batched full-KV decode over the per-sequence capacity."""
        # sequences shorter than the budget attend all of their pages (see InferenceController.begin_graph_decode)
        assert all(len(c.kv_cache.indicies) >= 1 for c in self.seqs), "prefill every sequence first"
        budget = min(self.max_page_budget(), self.max_pages)
        self.inference_page_budget = budget
        self._planned = budget
        # what a graph captured after this call bakes in: the plan's page count and whether the launches read budgets
        self._graph_planned = budget
        self._graph_budget_ptr = self.page_budgets.data_ptr() if self.page_budgets is not None else 0
        _plan_graph_handlers(self, budget, dense_layers)

    def clean_states(self) -> None:
        for c in self.seqs:
            c.clean_states()
        self.kv_tables = self.meta_tables = self.step_states = None
        self._graph_planned, self._graph_budget_ptr = 0, 0  # graphs over the dropped state are stale anyway
        self.state_epoch += 1
