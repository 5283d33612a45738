"""Drop-in for the reference's PyBind module ``quest._kernels`` (quest/ops/csrc/bsk_ops.cu:4-20).

Same 7 free functions + 1 class, same argument order and meaning (bsk_ops.h:23-117); each one
validates its tensors the way the reference's CHECK_* macros do (pytorch_extension_utils.h:52-66)
and then calls the matching C-ABI entry point of libquest_hip.so on torch's current stream.
PyTorch is only the owner of device memory here; all arithmetic is in the HIP library.

``prefill_with_paged_kv_cache`` is a hand-written kernel like the others since round 5: the MFMA
flash kernel of ``csrc/prefill.hip`` over the page table (no gathered K/V copy, no torch attention).
"""
from __future__ import annotations

import ctypes
import os as _os

import torch

from ._lib import Batch, PagedKV, check, lib

_NHD, _HND = 0, 1

STEP_STATE_INTS = 8      # int32 fields of quest_step_state_t
QUEST_EUNSUPPORTED = -2  # include/quest_hip.h: no kernel for this plan / shape, nothing was launched

# The reference compiles its argument validation in or out with -DBSK_TORCH_CHECK
# (quest/ops/CMakeLists.txt:40); here QUEST_TORCH_CHECK=0 turns the same checks off at import time
# (eager decode is host-bound: the checks are ~30 % of an op call's Python time).
_CHECKS_ON = _os.environ.get("QUEST_TORCH_CHECK", "1") != "0"


# ---------------------------------------------------------------- validation (CHECK_* macros)

def _check_input(x: torch.Tensor, name: str) -> None:
    if not _CHECKS_ON:
        return
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not x.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _check_rows(x: torch.Tensor, name: str) -> None:
    """A 2-D CUDA tensor whose rows are contiguous (a padded score buffer's ``[:, :n]`` view qualifies)."""
    if not _CHECKS_ON:
        return
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) < x.size(1):
        raise RuntimeError(f"{name} must be 2-D with contiguous rows")


def _check_dim(d: int, x: torch.Tensor, name: str) -> None:
    if _CHECKS_ON and x.dim() != d:
        raise RuntimeError(f"{name} must be a {d}D tensor")


def _check_eq(a, b, what: str) -> None:
    if _CHECKS_ON and a != b:
        raise RuntimeError(f"CHECK_EQ({what}) failed. {a} vs {b}")


def _check_ge(a, b, what: str) -> None:
    if _CHECKS_ON and not a >= b:
        raise RuntimeError(f"CHECK_GE({what}) failed. {a} vs {b}")


# torch dtype -> QUEST_DTYPE_* (include/quest_hip.h).  The reference's DISPATCH_PYTORCH_DTYPE_TO_CTYPE has only Half;
# bfloat16 is this library's second element type.  Anything else (float32, ...) has no kernel.
_DTYPES = {torch.float16: 0, torch.bfloat16: 1}


def _check_half(x: torch.Tensor, op: str, *same) -> None:
    """``x`` is fp16 or bf16 and every tensor of ``same`` (the other data tensors of the call; None entries skipped) has
    ``x``'s dtype: one call, one element type."""
    if x.dtype not in _DTYPES:
        raise RuntimeError(f"{op} failed to dispatch with dtype {x.dtype}")
    for t in same:
        if t is not None and t.dtype != x.dtype:
            raise RuntimeError(f"{op} failed to dispatch with dtype {t.dtype} (the call's other tensors are {x.dtype})")


def _check_f16(x: torch.Tensor, op: str) -> None:
    """fp16 and nothing else: the check of an fp16-only operator.  (The decode-layer projections of csrc/decode_layer.hip
    used it until they got their bf16 forms; no operator of this module is fp16-only any more, the one-launch layer
    refuses bf16 in the library.)"""
    if x.dtype != torch.float16:
        raise RuntimeError(f"{op} failed to dispatch with dtype {x.dtype}")


def _launched(code: int, what: str) -> bool:
    """False for QUEST_EUNSUPPORTED (nothing was launched: the caller takes its other route), else ``check``."""
    if code == QUEST_EUNSUPPORTED:
        return False
    check(code, what)
    return True


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(x: torch.Tensor) -> int:
    """hipStream_t of torch's current stream on x's device (raw handle: ~0.3 us instead of ~3 us through
    torch.cuda.current_stream(), which matters for the host-bound eager path)."""
    if _raw_stream is not None:
        return _raw_stream(x.device.index)
    return torch.cuda.current_stream(x.device).cuda_stream


def _pool_dims(data: torch.Tensor, layout: int):
    """(page_size, num_heads, head_dim) of a 5-D pool layer view."""
    if layout == _HND:
        return data.size(3), data.size(2), data.size(4)
    return data.size(2), data.size(3), data.size(4)


def _paged(data, indices, indptr, last_page_len, last_page_idx, layout, page_budget=0) -> PagedKV:
    page_size, num_heads, head_dim = _pool_dims(data, layout)
    if data.dtype not in _DTYPES:
        raise RuntimeError(f"paged pool failed to dispatch with dtype {data.dtype}")
    return PagedKV(
        data.data_ptr(),
        indices.data_ptr() if indices is not None else None,
        indptr.data_ptr() if indptr is not None else None,
        num_heads, page_size, head_dim, page_budget, int(last_page_len), int(last_page_idx), int(layout),
        _DTYPES[data.dtype])  # the view carries the element type of the call (quest_paged_kv_t.dtype)


# ---------------------------------------------------------------- free functions

def apply_rope_in_place(q, k, past_kv_len: int, rope_scale: float, rope_theta: float) -> None:
    """page.cu:212-252.  q ``[N, Hq, D]``, k ``[N, Hkv, D]`` rotated in place."""
    _check_input(q, "q")
    _check_input(k, "k")
    _check_dim(3, q, "q")
    _check_dim(3, k, "k")
    _check_eq(q.size(0), k.size(0), "q.size(0), k.size(0)")
    _check_eq(q.size(2), k.size(2), "q.size(2), k.size(2)")
    _check_half(q, "apply_rope_in_place", k)
    _rope_typed(q, k, q.size(0), past_kv_len, rope_scale, rope_theta, None, 1.0, None, "apply_rope_in_place")


def _rope_typed(q, k, n: int, past_kv_len: int, rope_scale: float, rope_theta: float, inv_freq, attention_factor: float,
                states, what: str) -> None:
    """Every RoPE form (formula or frequency table, eager or state-driven positions, fp16 or bf16): the one typed entry of
    the C ABI (quest_apply_rope_in_place_dtype)."""
    check(lib.quest_apply_rope_in_place_dtype(q.data_ptr(), k.data_ptr(), int(n), int(past_kv_len), q.size(1), k.size(1),
                                              q.size(2), float(rope_scale), float(rope_theta),
                                              inv_freq.data_ptr() if inv_freq is not None else None,
                                              float(attention_factor), states.data_ptr() if states is not None else None,
                                              _DTYPES[q.dtype], _stream(q)), what)


def _check_rope_table(inv_freq, head_dim: int) -> None:
    """The frequency table of the RoPE table form: a contiguous fp32 CUDA tensor of head_dim / 2 elements."""
    _check_input(inv_freq, "inv_freq")
    if _CHECKS_ON and inv_freq.dtype != torch.float32:
        raise RuntimeError("inv_freq must be a float32 tensor")
    _check_eq(inv_freq.numel(), head_dim // 2, "inv_freq.numel(), head_dim / 2")


def apply_rope_in_place_freqs(q, k, inv_freq, attention_factor: float, past_kv_len: int = 0, states=None) -> None:
    """RoPE from a frequency table (llama3 / yarn; EXTENSION): pair i of a row at position p rotates by
    ``p * inv_freq[i]``, cos and sin times ``attention_factor``.  q ``[N, Hq, D]``, k ``[N, Hkv, D]`` in place;
    ``states`` None: row i at ``past_kv_len + i``, else ``states`` ``[N, 8]`` int32 step states and row i at
    ``states[i].seq_len - 1``."""
    _check_input(q, "q")
    _check_input(k, "k")
    _check_dim(3, q, "q")
    _check_dim(3, k, "k")
    _check_eq(q.size(0), k.size(0), "q.size(0), k.size(0)")
    _check_eq(q.size(2), k.size(2), "q.size(2), k.size(2)")
    _check_half(q, "apply_rope_in_place", k)
    _check_rope_table(inv_freq, q.size(2))
    if states is not None:
        _check_input(states, "states")
        _check_eq(states.numel(), q.size(0) * STEP_STATE_INTS, "states.numel(), n * 8")
    _rope_typed(q, k, q.size(0), past_kv_len, 1.0, 1.0, inv_freq, attention_factor, states, "apply_rope_in_place_freqs")


def apply_qk_norm_rope_in_place(q, k, q_weight, k_weight, eps: float, past_kv_len: int = 0, rope_scale: float = 1.0,
                                rope_theta: float = 1e4, inv_freq=None, attention_factor: float = 1.0, states=None) -> None:
    """Per-head RMSNorm of q ``[N, Hq, D]`` / k ``[N, Hkv, D]`` (weights ``[D]``, shared by the heads, Qwen3's ``q_norm`` /
    ``k_norm``) fused with RoPE, in place, one launch (EXTENSION).  Frequencies: ``inv_freq`` None = the ``rope_scale`` /
    ``rope_theta`` formula, else the table of ``apply_rope_in_place_freqs``; positions: ``states`` None = row i at
    ``past_kv_len + i``, else ``states`` ``[N, 8]`` int32 step states and row i at ``states[i].seq_len - 1``.  One element
    type per call: q, k and both weights."""
    for t, name in ((q, "q"), (k, "k"), (q_weight, "q_weight"), (k_weight, "k_weight")):
        _check_input(t, name)
    _check_dim(3, q, "q")
    _check_dim(3, k, "k")
    _check_eq(q.size(0), k.size(0), "q.size(0), k.size(0)")
    _check_eq(q.size(2), k.size(2), "q.size(2), k.size(2)")
    _check_half(q, "apply_qk_norm_rope_in_place", k, q_weight, k_weight)
    for w, name in ((q_weight, "q_weight"), (k_weight, "k_weight")):
        _check_eq(tuple(w.shape), (q.size(2),), f"{name}.shape, (head_dim,)")
    if inv_freq is not None:
        _check_rope_table(inv_freq, q.size(2))
    if states is not None:
        _check_input(states, "states")
        _check_eq(states.dtype, torch.int32, "states.scalar_type(), torch::kInt32")
        _check_eq(states.numel(), q.size(0) * STEP_STATE_INTS, "states.numel(), n * 8")
    check(lib.quest_apply_qk_norm_rope_in_place_dtype(
        q.data_ptr(), k.data_ptr(), q.size(0), int(past_kv_len), q.size(1), k.size(1), q.size(2), q_weight.data_ptr(),
        k_weight.data_ptr(), float(eps), float(rope_scale), float(rope_theta),
        inv_freq.data_ptr() if inv_freq is not None else None, float(attention_factor),
        states.data_ptr() if states is not None else None, _DTYPES[q.dtype], _stream(q)), "apply_qk_norm_rope_in_place")


def rms_norm_forward(input, weight, output, epsilon: float) -> None:
    """rms_norm.cu:183-212.  input/output ``[1, N, C]``, weight ``[C]``."""
    _check_input(input, "input")
    _check_input(weight, "weight")
    _check_input(output, "output")
    _check_eq(input.dim(), 3, "input.dim(), 3")
    _check_half(input, "rms_norm_forward", weight, output)
    if input.dtype != torch.float16:
        return check(lib.quest_rms_norm_forward_dtype(input.data_ptr(), weight.data_ptr(), output.data_ptr(),
                                                      input.size(0) * input.size(1), input.size(2), float(epsilon),
                                                      _DTYPES[input.dtype], _stream(input)), "rms_norm")
    check(lib.quest_rms_norm_forward(input.data_ptr(), weight.data_ptr(), output.data_ptr(),
                                     input.size(0) * input.size(1), input.size(2), float(epsilon), _stream(input)),
          "rms_norm")


def topk_filtering(estimated_value, estimated_indices, d_out, indices_out, buf, page_budget: int) -> None:
    """topk.cu:7-46.  Rows = heads; selects ``page_budget`` largest of each row.  ``estimated_value`` may be a
    ``[:, :n]`` view of a buffer with padded rows (``decode_append_estimate``'s output): the row stride is passed on."""
    _check_rows(estimated_value, "estimated_value")
    _check_input(estimated_indices, "estimated_indices")
    _check_input(d_out, "d_out")
    _check_input(indices_out, "indices_out")
    _check_dim(2, estimated_value, "estimated_value")
    _check_dim(2, estimated_indices, "estimated_indices")
    num_heads, num_pages = estimated_value.size(0), estimated_value.size(1)
    _check_eq(num_pages, estimated_indices.size(1), "num_pages, estimated_indices.size(1)")
    _check_eq(num_heads, estimated_indices.size(0), "num_heads, estimated_indices.size(0)")
    _check_ge(num_pages, page_budget, "num_pages, page_budget")
    _check_eq(estimated_indices.dtype, torch.int32, "estimated_indices.scalar_type(), torch::kInt32")
    _check_eq(indices_out.dtype, torch.int32, "indices_out.scalar_type(), torch::kInt32")
    _check_eq(page_budget, d_out.size(1), "page_budget, d_out.size(1)")
    _check_eq(page_budget, indices_out.size(1), "page_budget, indices_out.size(1)")
    _check_half(estimated_value, "Top-k filtering", d_out)  # (the selection orders 16-bit patterns: one code for both types)
    check(lib.quest_topk_filtering(estimated_value.data_ptr(), estimated_value.stride(0), estimated_indices.data_ptr(),
                                   d_out.data_ptr(), indices_out.data_ptr(), buf.data_ptr() if buf is not None else None,
                                   num_heads, num_pages, int(page_budget), _stream(estimated_value)), "Top-k filtering")


def estimate_attn_score(q, o, metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len: int,
                        metadata_last_page_idx: int, layout: int) -> None:
    """estimate.cu:6-84.  q ``[1, Hq, D]``; o ``[Hq, n_pages-1]`` written in place."""
    _check_input(q, "q")
    _check_input(o, "o")
    _check_input(metadata_data, "metadata_data")
    _check_input(metadata_indices, "metadata_indices")
    _check_dim(3, q, "q")
    _check_dim(2, o, "o")
    _check_dim(5, metadata_data, "metadata_data")
    _check_dim(1, metadata_indices, "metadata_indices")
    _check_eq(q.size(0), 1, "q.size(0), 1")
    _check_eq(metadata_indices.dtype, torch.int32, "metadata_indices.scalar_type(), torch::kInt32")
    _check_half(q, "Estimate_attn_score", o, metadata_data)
    page_size, num_kv_heads, head_dim = _pool_dims(metadata_data, layout)
    _check_eq(metadata_data.size(4), q.size(2), "metadata_data.size(4), head_dim")
    _check_eq(o.size(0), q.size(1), "o.size(0), num_heads")
    meta = _paged(metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len, metadata_last_page_idx,
                  layout)
    check(lib.quest_estimate_attn_score(q.data_ptr(), o.data_ptr(), q.size(1), o.size(1), meta, _stream(q)),
          "Estimate_attn_score")


def _check_append(k, v, kv_data, kv_indices, kv_indptr, metadata_data, metadata_indices, metadata_indptr, layout):
    for t, n in ((k, "k"), (v, "v"), (kv_data, "kv_data"), (kv_indices, "kv_indices"),
                 (metadata_data, "metadata_data"), (metadata_indices, "metadata_indices")):
        _check_input(t, n)
    _check_dim(1, kv_indices, "kv_indices")
    _check_dim(1, metadata_indices, "metadata_indices")
    _check_dim(3, k, "k")
    _check_dim(3, v, "v")
    _check_dim(5, kv_data, "kv_data")
    _check_dim(5, metadata_data, "metadata_data")
    for t, n in ((kv_indices, "kv_indices"), (metadata_indices, "metadata_indices"), (kv_indptr, "kv_indptr"),
                 (metadata_indptr, "metadata_indptr")):
        _check_eq(t.dtype, torch.int32, f"{n}.scalar_type(), torch::kInt32")
    page_size, num_heads, head_dim = _pool_dims(kv_data, layout)
    _check_eq(num_heads, k.size(1), "kv_data heads, num_heads")
    _check_eq(head_dim, k.size(2), "kv_data.size(4), head_dim")
    _check_eq(v.size(0), k.size(0), "seq_len, v.size(0)")


def append_kv_cache_prefill(k, v, kv_data, kv_indices, kv_indptr, kv_last_page_len: int, kv_last_page_idx: int,
                            metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len: int,
                            metadata_last_page_idx: int, layout: int) -> None:
    """page.cu:101-210.  k, v ``[N>=2, H, D]`` appended; per-page min/max metadata rebuilt."""
    _check_append(k, v, kv_data, kv_indices, kv_indptr, metadata_data, metadata_indices, metadata_indptr, layout)
    _check_ge(k.size(0), 2, "k.size(0), 2")
    _check_half(k, "Append_kv_cache_prefill", v, kv_data, metadata_data)
    kv = _paged(kv_data, kv_indices, kv_indptr, kv_last_page_len, kv_last_page_idx, layout)
    meta = _paged(metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len, metadata_last_page_idx,
                  layout)
    check(lib.quest_append_kv_cache_prefill(k.data_ptr(), v.data_ptr(), k.size(0), kv_indices.size(0), kv, meta,
                                            _stream(k)), "Append_kv_cache_prefill")


def append_kv_cache_decode(k, v, kv_data, kv_indices, kv_indptr, kv_last_page_len: int, kv_last_page_idx: int,
                           metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len: int,
                           metadata_last_page_idx: int, layout: int) -> None:
    """page.cu:6-99.  k, v ``[1, H, D]``."""
    _check_append(k, v, kv_data, kv_indices, kv_indptr, metadata_data, metadata_indices, metadata_indptr, layout)
    _check_eq(k.size(0), 1, "k.size(0), 1")
    _check_half(k, "Append_kv_cache_decode", v, kv_data, metadata_data)
    kv = _paged(kv_data, kv_indices, kv_indptr, kv_last_page_len, kv_last_page_idx, layout)
    meta = _paged(metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len, metadata_last_page_idx,
                  layout)
    check(lib.quest_append_kv_cache_decode(k.data_ptr(), v.data_ptr(), kv, meta, _stream(k)),
          "Append_kv_cache_decode")


def append_estimate(k, v, kv_data, kv_indices, kv_indptr, kv_last_page_len: int, kv_last_page_idx: int, q, o,
                    metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len: int,
                    metadata_last_page_idx: int, layout: int) -> None:
    """EXTENSION (not in the reference surface): append_kv_cache_decode + estimate_attn_score in one
    launch; results identical to the two separate ops."""
    _check_append(k, v, kv_data, kv_indices, kv_indptr, metadata_data, metadata_indices, metadata_indptr, layout)
    _check_eq(k.size(0), 1, "k.size(0), 1")
    _check_input(q, "q")
    _check_rows(o, "o")  # [Hq, n_out], rows possibly padded (a view of a wider buffer)
    _check_dim(3, q, "q")
    _check_eq(q.size(0), 1, "q.size(0), 1")
    _check_eq(o.size(0), q.size(1), "o.size(0), num_heads")
    _check_half(k, "Append_kv_cache_decode", v, kv_data, metadata_data)
    _check_half(q, "Estimate_attn_score", o, k)
    kv = _paged(kv_data, kv_indices, kv_indptr, kv_last_page_len, kv_last_page_idx, layout)
    meta = _paged(metadata_data, metadata_indices, metadata_indptr, metadata_last_page_len, metadata_last_page_idx,
                  layout)
    check(lib.quest_append_estimate(k.data_ptr(), v.data_ptr(), kv, q.data_ptr(), o.data_ptr(), q.size(1), o.size(1),
                                    o.stride(0), meta, _stream(k)), "append_estimate")


# ---- decode-token projections of a decoder layer, fused (EXTENSION: csrc/decode_layer.hip)

# ``like``: the call's first data tensor -- fp16 or bf16, and every tensor of the call has its dtype (``_check_half``)
def _check_vec(x, n: int, name: str, like) -> None:
    _check_input(x, name)
    _check_eq(x.numel(), n, f"{name}.numel(), {n}")
    _check_half(like, name, x)


def _check_mat(x, n: int, cols: int, name: str, like) -> None:
    _check_input(x, name)
    _check_eq(x.numel(), n * cols, f"{name}.numel(), {n} * {cols}")
    _check_half(like, name, x)


def _check_weight(w, out_dim: int, in_dim: int, name: str, like) -> None:
    _check_input(w, name)
    _check_dim(2, w, name)
    _check_eq(tuple(w.shape), (out_dim, in_dim), f"{name}.shape, (out, in)")
    _check_half(like, name, w)


# One private body per operator: validation and the call.  ``n`` None: the one-token entry (vectors); else the n-token
# entry (``[n, dim]`` matrices), after ``_check_tokens``.  The twelve public names below are thin calls of the five bodies.
MAX_BATCHED_TOKENS = 16


def _check_tokens(n: int) -> None:
    if not 1 <= n <= MAX_BATCHED_TOKENS:
        raise RuntimeError(f"batched decode-layer launches take 1..{MAX_BATCHED_TOKENS} tokens, got {n}")


def _check_act(x, n, dim: int, name: str, like) -> None:
    """An activation of the one-token (``n`` None: ``[dim]``) or the n-token (``[n, dim]``) entry."""
    if n is None:
        _check_vec(x, dim, name, like)
    else:
        _check_mat(x, n, dim, name, like)


def _entry(name: str, n):
    """(C entry, tail of its argument list before dtype, name for error messages) of operator ``name``'s form for ``n``."""
    if n is None:
        return getattr(lib, f"quest_decode_{name}"), (), f"decode_{name}"
    return getattr(lib, f"quest_decode_{name}_batched"), (n,), f"decode_{name}_batched"


def _norm_gemv(x, gamma, eps, w, out, n) -> None:
    out_dim, in_dim = w.shape
    _check_act(x, n, in_dim, "x", x)
    _check_act(out, n, out_dim, "out", x)
    _check_weight(w, out_dim, in_dim, "w", x)
    if gamma is not None:
        _check_vec(gamma, in_dim, "gamma", x)
    fn, tokens, what = _entry("norm_gemv", n)
    check(fn(x.data_ptr(), gamma.data_ptr() if gamma is not None else None, float(eps), w.data_ptr(), out.data_ptr(), in_dim,
             out_dim, *tokens, _DTYPES[x.dtype], _stream(x)), what)


def _gemv_residual(x, w, h, n) -> None:
    out_dim, in_dim = w.shape
    _check_act(x, n, in_dim, "x", x)
    _check_act(h, n, out_dim, "h", x)
    _check_weight(w, out_dim, in_dim, "w", x)
    fn, tokens, what = _entry("gemv_residual", n)
    check(fn(x.data_ptr(), w.data_ptr(), h.data_ptr(), in_dim, out_dim, *tokens, _DTYPES[x.dtype], _stream(x)), what)


def _mlp_gate_up(h, gamma, eps, w_gate, w_up, act, n) -> None:
    inter, hidden = w_gate.shape
    _check_act(h, n, hidden, "h", h)
    _check_vec(gamma, hidden, "gamma", h)
    _check_act(act, n, inter, "act", h)
    _check_weight(w_gate, inter, hidden, "w_gate", h)
    _check_weight(w_up, inter, hidden, "w_up", h)
    fn, tokens, what = _entry("mlp_gate_up", n)
    check(fn(h.data_ptr(), gamma.data_ptr(), float(eps), w_gate.data_ptr(), w_up.data_ptr(), act.data_ptr(), hidden, inter,
             *tokens, _DTYPES[h.dtype], _stream(h)), what)


def _qkv_args(h, gamma, eps, wq, wk, wv, q, k, v, n):
    """Validation and leading C arguments shared by the two q/k/v projection operators; ``n`` tokens (None: one)."""
    n = 1 if n is None else n
    hidden = wq.size(1)
    _check_mat(h, n, hidden, "h", h)
    _check_vec(gamma, hidden, "gamma", h)
    _check_weight(wq, wq.size(0), hidden, "wq", h)
    _check_weight(wk, wk.size(0), hidden, "wk", h)
    _check_weight(wv, wk.size(0), hidden, "wv", h)
    _check_mat(q, n, wq.size(0), "q", h)
    _check_mat(k, n, wk.size(0), "k", h)
    _check_mat(v, n, wk.size(0), "v", h)
    return (h.data_ptr(), gamma.data_ptr(), float(eps), wq.data_ptr(), wk.data_ptr(), wv.data_ptr(), q.data_ptr(),
            k.data_ptr(), v.data_ptr(), hidden)


def _qkv_rope(h, gamma, eps, wq, wk, wv, q, k, v, head_dim: int, rope_scale, rope_theta, inv_freq, attention_factor, state,
              n) -> None:
    """The rotating q/k/v launch: ``state`` = the tokens' step state(s) ``[n, 8]`` int32, heads counted in ``head_dim``;
    ``inv_freq`` None: the closed form (``rope_scale``, ``rope_theta``), else the frequency table (the ``_freqs`` names)."""
    args = _qkv_args(h, gamma, eps, wq, wk, wv, q, k, v, n)
    _check_input(state, "state")
    _check_eq(state.numel(), (1 if n is None else n) * STEP_STATE_INTS, "states.numel(), n * 8")
    _check_eq(wq.size(0) % head_dim, 0, "wq.size(0) % head_dim, 0")
    fn, tokens, what = _entry("qkv_rope", n)
    if inv_freq is not None:
        _check_rope_table(inv_freq, head_dim)
        what += "_freqs"
    check(fn(*args, wq.size(0) // head_dim, wk.size(0) // head_dim, int(head_dim), float(rope_scale), float(rope_theta),
             inv_freq.data_ptr() if inv_freq is not None else None, float(attention_factor), state.data_ptr(), *tokens,
             _DTYPES[h.dtype], _stream(h)), what)


def _qkv(h, gamma, eps, wq, wk, wv, q, k, v, n) -> None:
    fn, tokens, what = _entry("qkv", n)
    check(fn(*_qkv_args(h, gamma, eps, wq, wk, wv, q, k, v, n), wq.size(0), wk.size(0), *tokens, _DTYPES[h.dtype], _stream(h)),
          what)


def decode_norm_gemv(x, gamma, eps: float, w, out) -> None:
    """``out = w @ rmsnorm(x; gamma, eps)`` (``gamma`` None: ``out = w @ x``); x ``[in]``, w ``[out, in]``, out ``[out]``."""
    _norm_gemv(x, gamma, eps, w, out, None)


def decode_gemv_residual(x, w, h) -> None:
    """``h += w @ x`` in place; x ``[in]``, w ``[out, in]``, h ``[out]``."""
    _gemv_residual(x, w, h, None)


def decode_mlp_gate_up(h, gamma, eps: float, w_gate, w_up, act) -> None:
    """``act = silu(w_gate @ n) * (w_up @ n)`` with ``n = rmsnorm(h; gamma, eps)``."""
    _mlp_gate_up(h, gamma, eps, w_gate, w_up, act, None)


def decode_qkv_rope(h, gamma, eps: float, wq, wk, wv, q, k, v, head_dim: int, rope_scale: float, rope_theta: float,
                    state) -> None:
    """q ``[1, Hq, D]``, k / v ``[1, Hkv, D]`` = projections of ``rmsnorm(h; gamma, eps)`` with RoPE on q and k at the
    position ``state.seq_len - 1`` (the device-resident step state, after ``step_state_advance_batched``)."""
    _qkv_rope(h, gamma, eps, wq, wk, wv, q, k, v, head_dim, rope_scale, rope_theta, None, 1.0, state, None)


def decode_qkv_rope_freqs(h, gamma, eps: float, wq, wk, wv, q, k, v, head_dim: int, inv_freq, attention_factor: float,
                          state) -> None:
    """``decode_qkv_rope`` with the RoPE frequency table of ``apply_rope_in_place_freqs`` (llama3 / yarn)."""
    _qkv_rope(h, gamma, eps, wq, wk, wv, q, k, v, head_dim, 1.0, 1.0, inv_freq, attention_factor, state, None)


def decode_qkv(h, gamma, eps: float, wq, wk, wv, q, k, v) -> None:
    """q ``[1, Hq, D]``, k / v ``[1, Hkv, D]`` = projections of ``rmsnorm(h; gamma, eps)``, NOT rotated: the q-k-v launch of
    models with a per-head q/k norm, which ``apply_qk_norm_rope_in_place`` follows."""
    _qkv(h, gamma, eps, wq, wk, wv, q, k, v, None)


# ---- the same for n <= 16 tokens (one per sequence of a batch)

def _tokens(x, in_dim: int) -> int:
    n = x.numel() // in_dim
    _check_tokens(n)
    return n


def decode_norm_gemv_batched(x, gamma, eps: float, w, out) -> None:
    """``out[i] = w @ rmsnorm(x[i]; gamma, eps)`` (``gamma`` None: no norm); x ``[n, in]``, out ``[n, out]``."""
    _norm_gemv(x, gamma, eps, w, out, _tokens(x, w.size(1)))


def decode_gemv_residual_batched(x, w, h) -> None:
    """``h[i] += w @ x[i]`` in place; x ``[n, in]``, h ``[n, out]``."""
    _gemv_residual(x, w, h, _tokens(x, w.size(1)))


def decode_mlp_gate_up_batched(h, gamma, eps: float, w_gate, w_up, act) -> None:
    """``act[i] = silu(w_gate @ n_i) * (w_up @ n_i)``, ``n_i = rmsnorm(h[i]; gamma, eps)``; h ``[n, hidden]``."""
    _mlp_gate_up(h, gamma, eps, w_gate, w_up, act, _tokens(h, w_gate.size(1)))


def decode_qkv_rope_batched(h, gamma, eps: float, wq, wk, wv, q, k, v, head_dim: int, rope_scale: float,
                            rope_theta: float, states) -> None:
    """q ``[n, Hq, D]``, k / v ``[n, Hkv, D]`` = projections of ``rmsnorm(h[i]; gamma, eps)``, RoPE on q and k at
    ``states[i].seq_len - 1`` (``states``: the batched step state ``[n, 8]`` int32)."""
    _qkv_rope(h, gamma, eps, wq, wk, wv, q, k, v, head_dim, rope_scale, rope_theta, None, 1.0, states, _tokens(h, wq.size(1)))


def decode_qkv_rope_batched_freqs(h, gamma, eps: float, wq, wk, wv, q, k, v, head_dim: int, inv_freq,
                                  attention_factor: float, states) -> None:
    """``decode_qkv_rope_batched`` with the RoPE frequency table of ``apply_rope_in_place_freqs`` (llama3 / yarn)."""
    _qkv_rope(h, gamma, eps, wq, wk, wv, q, k, v, head_dim, 1.0, 1.0, inv_freq, attention_factor, states,
              _tokens(h, wq.size(1)))


def decode_qkv_batched(h, gamma, eps: float, wq, wk, wv, q, k, v) -> None:
    """``decode_qkv`` for n <= 16 tokens: h ``[n, hidden]``, q ``[n, Hq, D]``, k / v ``[n, Hkv, D]``."""
    _qkv(h, gamma, eps, wq, wk, wv, q, k, v, _tokens(h, wq.size(1)))


# ---- state-driven (graph-replayable) forms: EXTENSIONS, see include/quest_hip.h quest_step_state_t.  One launch serves
# the n sequences of a batch (BASELINE config 5): the pools are shared, page tables are rows of ``[n, stride]``
# int32 matrices, ``state`` is ``[n, 8]`` int32, q/k/v/o are ``[n, heads, dim]``, scores ``[n, Hq, stride]``.  A single
# sequence is the batch of one and may come in its own shapes -- state ``[8]``, tables ``[capacity]``, scores
# ``[Hq, stride]`` -- which reach the library as ``[1, ...]`` views of the same memory (a captured graph holds the addresses).

def _lead(t, dims: int):
    """``t`` as a ``dims``-D tensor: a view with a leading dimension of one where ``t`` has the single-sequence rank."""
    return t.unsqueeze(0) if t is not None and t.dim() == dims - 1 else t


def _batch(state, kv_tables, meta_tables, budgets=None) -> Batch:
    """quest_batch_t of ``state`` ``[n, 8]`` (or ``[8]``: one sequence, tables ``[capacity]``).  ``budgets``: optional int32
    ``[n]`` device tensor of per-sequence page budgets (pages a sequence attends INCLUDING its current one); None = the
    budget the handler was planned with, for every sequence."""
    state, kv_tables, meta_tables = _lead(state, 2), _lead(kv_tables, 2), _lead(meta_tables, 2)
    _check_dim(2, state, "state")
    _check_eq(state.size(1), STEP_STATE_INTS, "state.size(-1), 8")
    n = state.size(0)
    if budgets is not None:
        _check_input(budgets, "page_budgets")
        _check_dim(1, budgets, "page_budgets")
        _check_eq(budgets.size(0), n, "page_budgets.size(0), n_seqs")
        if budgets.dtype != torch.int32:
            raise RuntimeError("page_budgets must be an int32 tensor")
    for t, name in ((kv_tables, "kv_tables"), (meta_tables, "meta_tables")):
        if t is not None:
            # rows of `capacity` entries at a stride >= capacity: BatchedInferenceController pads the stride to a multiple
            # of 4 entries so that every sequence's table is 16-byte aligned (vector loads of page ids)
            _check_rows(t, name)
            _check_eq(t.size(0), n, f"{name}.size(0), n_seqs")
            if t.dtype != torch.int32:
                raise RuntimeError(f"{name} must be an int32 tensor")
    return Batch(n, 0 if kv_tables is None else kv_tables.stride(0), 0 if meta_tables is None else meta_tables.stride(0), 0,
                 None if budgets is None else budgets.data_ptr())


def step_state_advance_batched(state, kv_tables, meta_tables, page_size: int) -> None:
    """Device-side prepare_metadata(1) of every sequence: ``state`` int32 ``[n, 8]`` (quest_step_state_t), tables int32
    ``[n, capacity]``."""
    _check_input(state, "state")
    _check_eq(state.dtype, torch.int32, "state.scalar_type(), torch::kInt32")
    b = _batch(state, kv_tables, meta_tables)
    check(lib.quest_step_state_advance_batched(state.data_ptr(), kv_tables.data_ptr(), meta_tables.data_ptr(),
                                               int(page_size), kv_tables.size(-1), meta_tables.size(-1), b,
                                               _stream(state)), "step_state_advance_batched")


def tile_max_offset(max_n: int) -> int:
    """Column offset of the tile maxima in a score row of the tiles launches: the scores padded to 8 columns."""
    return (int(max_n) + 7) // 8 * 8


def tiles_row_stride(max_n: int) -> int:
    """Smallest row stride (fp16 columns, a multiple of 8) of a score scratch that also holds the tile maxima."""
    return (tile_max_offset(max_n) + ((int(max_n) + 7) // 8 + 3) // 4 * 4 + 7) // 8 * 8


# ---- sign planes (csrc/estimate_planes.hip, include/quest_hip.h SIGN PLANES): a single-sequence MHA controller registers
# each layer's shadow store under the metadata layer's data pointer; ``append_estimate_batched(..., tiles=False)`` over that
# layer, page table and step state then takes the planes launch -- whoever calls it (``decode_layer_dyn``, a benchmark that
# times the launch on its own).  A registration is used only while the tensors it was made for are alive (weak references:
# the allocator hands a dead controller's addresses to the next one), and only for the same table and state.

PLANE_BLOCK = 256  # pages per workgroup of the planes launch: the page capacity of a store is a multiple of it
_PLANES: dict = {}


class _Planes:
    __slots__ = ("meta_ref", "state_ref", "state_ptr", "table_ptr", "planes", "covered", "plane_pages")


def plane_pages_for(max_pages: int) -> int:
    """Page capacity of a planes store that serves a pool of ``max_pages`` pages: padded to whole page blocks."""
    return (int(max_pages) + PLANE_BLOCK - 1) // PLANE_BLOCK * PLANE_BLOCK


def estimate_planes_bytes(num_kv_heads: int, plane_pages: int) -> int:
    return int(lib.quest_estimate_planes_bytes(int(num_kv_heads), int(plane_pages)))


def estimate_planes_build(planes, plane_pages: int, covered, metadata_data, meta_table, state, kv_page_size: int,
                          layout: int) -> None:
    """Transpose the complete pages of one layer's metadata pool into ``planes`` (fp16, ``estimate_planes_bytes`` bytes)
    and set ``covered`` (int32, one element) to their number, both read from ``state`` (``[8]`` or ``[1, 8]`` int32)."""
    for t, n in ((planes, "planes"), (covered, "covered"), (metadata_data, "metadata_data"), (state, "state")):
        _check_input(t, n)
    _check_eq(covered.dtype, torch.int32, "covered.scalar_type(), torch::kInt32")
    _check_eq(planes.dtype, torch.float16, "planes.scalar_type(), torch::kHalf")
    meta = _paged(metadata_data, meta_table, None, 1, 0, layout)
    _check_ge(planes.numel() * 2, estimate_planes_bytes(meta.num_heads, plane_pages), "planes bytes")
    check(lib.quest_estimate_planes_build(planes.data_ptr(), int(plane_pages), covered.data_ptr(), meta, int(kv_page_size),
                                          state.data_ptr(), _stream(planes)), "estimate_planes_build")


def register_estimate_planes(metadata_data, meta_table, state, planes, covered, plane_pages: int) -> None:
    """Route ``append_estimate_batched(..., tiles=False)`` over (``metadata_data``, ``meta_table``, ``state``) to the planes
    launch with this store.  The caller keeps ``metadata_data`` and ``state`` alive for as long as it wants the route."""
    import weakref

    e = _Planes()
    e.meta_ref, e.state_ref = weakref.ref(metadata_data), weakref.ref(state)
    e.state_ptr, e.table_ptr = state.data_ptr(), meta_table.data_ptr()
    e.planes, e.covered, e.plane_pages = planes, covered, int(plane_pages)
    entries = [x for x in _PLANES.get(metadata_data.data_ptr(), ()) if _planes_alive(x) and x.state_ptr != e.state_ptr]
    _PLANES[metadata_data.data_ptr()] = entries + [e]


def unregister_estimate_planes(metadata_data, state=None) -> None:
    """Drop the registration(s) under ``metadata_data`` (of ``state`` only, where given)."""
    key = metadata_data.data_ptr()
    left = [x for x in _PLANES.get(key, ()) if state is not None and x.state_ptr != state.data_ptr() and _planes_alive(x)]
    if left:
        _PLANES[key] = left
    else:
        _PLANES.pop(key, None)


def _planes_alive(e) -> bool:
    return e.meta_ref() is not None and e.state_ref() is not None


def estimate_planes_for(metadata_data, meta_table, state):
    """The registered store that serves this (metadata layer, page table, step state), or None."""
    entries = _PLANES.get(metadata_data.data_ptr())
    if not entries:
        return None
    for e in entries:
        if e.state_ptr == state.data_ptr() and e.table_ptr == meta_table.data_ptr() and _planes_alive(e) \
                and e.meta_ref().data_ptr() == metadata_data.data_ptr():
            return e
    return None


def append_estimate_batched(k, v, kv_data, kv_tables, q, o, metadata_data, meta_tables, state, max_n_out: int,
                            layout: int, tiles: bool = False) -> bool:
    """append_estimate for ``n`` sequences in one launch, lengths / last-page ids / n_out read from ``state``: k/v
    ``[n, Hkv, D]``, q ``[n, Hq, D]``, o ``[n, Hq, stride]``.
    ``tiles``: every row also gets its tile maxima (per 8 pages the largest score, as a 16-bit key) at column
    ``tile_max_offset(max_n_out)`` -- ``o.size(-1)`` must be at least ``tiles_row_stride(max_n_out)``; returns False
    (nothing launched) for QUEST_EUNSUPPORTED: no estimate tile of this shape is a multiple of 8 pages wide (checked before
    the launch, ``csrc/estimate.hip`` ``launch_estimate``), or the group size / head_dim has no instantiation at all -- the
    caller's whole-row launch (``tiles=False``) then raises for the latter."""
    for t, n in ((k, "k"), (v, "v"), (kv_data, "kv_data"), (q, "q"), (o, "o"), (metadata_data, "metadata_data"),
                 (state, "state")):
        _check_input(t, n)
    b = _batch(state, kv_tables, meta_tables)
    o = _lead(o, 3)
    _check_dim(3, k, "k")
    _check_dim(3, q, "q")
    _check_dim(3, o, "o")
    _check_eq(k.size(0), b.n_seqs, "k.size(0), n_seqs")
    _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
    _check_eq(o.size(0), b.n_seqs, "o.size(0), n_seqs")
    _check_eq(o.size(1), q.size(1), "o.size(1), num_heads")
    _check_ge(o.size(2), max_n_out, "o.size(2), max_n_out")
    _check_half(k, "Append_kv_cache_decode", v, kv_data, metadata_data)
    _check_half(q, "Estimate_attn_score", o, k)
    kv = _paged(kv_data, kv_tables, None, 1, 0, layout)
    meta = _paged(metadata_data, meta_tables, None, 1, 0, layout)
    if tiles:
        _check_ge(o.size(2), tiles_row_stride(max_n_out), "o.size(2), tiles_row_stride(max_n_out)")
    planes = None if tiles or not _PLANES or b.n_seqs != 1 else estimate_planes_for(metadata_data, meta_tables, state)
    if planes is not None and planes.plane_pages >= max_n_out:
        # a registered shadow store of this layer (sign planes): same rows, same bits, half the metadata bytes
        check(lib.quest_append_estimate_planes_batched(k.data_ptr(), v.data_ptr(), kv, q.data_ptr(), o.data_ptr(), q.size(1),
                                                       o.size(2), int(max_n_out), 0, meta, state.data_ptr(), b,
                                                       planes.planes.data_ptr(), planes.plane_pages,
                                                       planes.covered.data_ptr(), _stream(k)),
              "append_estimate_planes_batched")
        return True
    code = lib.quest_append_estimate_batched(k.data_ptr(), v.data_ptr(), kv, q.data_ptr(), o.data_ptr(), q.size(1), o.size(2),
                                             int(max_n_out), tile_max_offset(max_n_out) if tiles else 0, meta,
                                             state.data_ptr(), b, _stream(k))
    if not tiles:  # whole rows are the caller's last route: QUEST_EUNSUPPORTED raises
        check(code, "append_estimate_batched")
    return _launched(code, "append_estimate_batched")


def append_estimate_dyn(k, v, kv_data, kv_table, q, o, metadata_data, meta_table, state, max_n_out: int,
                        layout: int, tiles: bool = False) -> bool:
    """``append_estimate_batched`` under its single-sequence name: k/v/q ``[1, H, D]``, ``o`` ``[Hq, stride]``, state ``[8]``."""
    return append_estimate_batched(k, v, kv_data, kv_table, q, o, metadata_data, meta_table, state, max_n_out, layout, tiles)


def estimate_attn_score_batched(q, o, metadata_data, meta_tables, state, max_n_out: int, layout: int) -> None:
    """estimate_attn_score (estimate.cu:6-84) for ``n`` sequences in one launch: q ``[n, Hq, D]``, o ``[n, Hq, stride]``;
    row i is scored over ``state[i].n_pages - 1`` pages."""
    for t, n in ((q, "q"), (o, "o"), (metadata_data, "metadata_data"), (state, "state")):
        _check_input(t, n)
    b = _batch(state, None, meta_tables)
    _check_dim(3, q, "q")
    _check_dim(3, o, "o")
    _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
    _check_eq(o.size(0), b.n_seqs, "o.size(0), n_seqs")
    _check_eq(o.size(1), q.size(1), "o.size(1), num_heads")
    _check_ge(o.size(2), max_n_out, "o.size(2), max_n_out")
    _check_half(q, "Estimate_attn_score", o, metadata_data)
    meta = _paged(metadata_data, meta_tables, None, 1, 0, layout)
    check(lib.quest_estimate_attn_score_batched(q.data_ptr(), o.data_ptr(), q.size(1), o.size(2), int(max_n_out), meta,
                                                state.data_ptr(), b, _stream(q)), "Estimate_attn_score")


def topk_filtering_batched(scores, kv_tables, d_out, indices_out, state, max_num_pages: int, page_budget: int,
                           budgets=None) -> None:
    """topk_filtering (topk.cu:7-46) for ``n`` sequences in one launch: scores ``[n, H, stride]``, page ids = each
    sequence's own page table ``kv_tables[i]``, outputs ``[n, H, k_max]`` of which row (i, h) gets its first
    ``min(budget_i - 1, n_pages_i - 1)`` entries written (``budget_i`` from ``budgets`` or ``page_budget``)."""
    for t, n in ((scores, "scores"), (d_out, "d_out"), (indices_out, "indices_out"), (state, "state")):
        _check_input(t, n)
    b = _batch(state, kv_tables, None, budgets)
    _check_dim(3, scores, "scores")
    _check_dim(3, d_out, "d_out")
    _check_dim(3, indices_out, "indices_out")
    _check_eq(scores.size(0), b.n_seqs, "scores.size(0), n_seqs")
    _check_eq(d_out.size(0), b.n_seqs, "d_out.size(0), n_seqs")
    _check_eq(d_out.size(1), scores.size(1), "d_out.size(1), num_heads")
    _check_eq(tuple(indices_out.shape), tuple(d_out.shape), "indices_out.shape, d_out.shape")
    _check_eq(indices_out.dtype, torch.int32, "indices_out.scalar_type(), torch::kInt32")
    _check_ge(scores.size(2), max_num_pages, "scores.size(2), max_num_pages")
    _check_half(scores, "Top-k filtering", d_out)
    check(lib.quest_topk_filtering_batched(scores.data_ptr(), scores.size(2), int(max_num_pages), kv_tables.data_ptr(),
                                           d_out.data_ptr(), indices_out.data_ptr(), d_out.size(2), scores.size(1),
                                           int(page_budget), state.data_ptr(), b, _stream(scores)), "Top-k filtering")


def append_kv_cache_decode_batched(k, v, kv_data, kv_tables, metadata_data, meta_tables, state, layout: int) -> None:
    """append_kv_cache_decode of one token per sequence, lengths / last-page ids from ``state``: k, v ``[n, Hkv, D]``."""
    for t, n in ((k, "k"), (v, "v"), (kv_data, "kv_data"), (metadata_data, "metadata_data"), (state, "state")):
        _check_input(t, n)
    b = _batch(state, kv_tables, meta_tables)
    _check_eq(k.size(0), b.n_seqs, "k.size(0), n_seqs")
    _check_half(k, "Append_kv_cache_decode", v, kv_data, metadata_data)
    kv = _paged(kv_data, kv_tables, None, 1, 0, layout)
    meta = _paged(metadata_data, meta_tables, None, 1, 0, layout)
    check(lib.quest_append_kv_cache_decode_batched(k.data_ptr(), v.data_ptr(), kv, meta, state.data_ptr(), b,
                                                   _stream(k)), "Append_kv_cache_decode")


def apply_rope_in_place_batched(q, k, rope_scale: float, rope_theta: float, state) -> None:
    """apply_rope_in_place with row i of q ``[n, Hq, D]`` / k ``[n, Hkv, D]`` at position ``state[i].seq_len - 1``."""
    _check_input(q, "q")
    _check_input(k, "k")
    _check_input(state, "state")
    b = _batch(state, None, None)
    _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
    _check_eq(k.size(0), b.n_seqs, "k.size(0), n_seqs")
    _check_half(q, "apply_rope_in_place", k)
    _rope_typed(q, k, b.n_seqs, 0, rope_scale, rope_theta, None, 1.0, state, "apply_rope_in_place_batched")


def prefill_with_paged_kv_cache(q, kv_data, kv_indices, kv_last_page_len: int, causal: bool, layout: int,
                                allow_fp16_qk_reduction: bool, rope_scale: float, rope_theta: float):
    """batch_prefill.cu:27-117 -> BatchPrefillWithPagedKVCache (prefill.cuh:1008-1119): attention of the ``n`` new rows
    of ``q`` over the sequence's pages, the new tokens included (row i sees keys 0 .. kv_len - n + i when ``causal``).
    One launch of the MFMA flash kernel of csrc/prefill.hip straight over the page table: no gathered K/V copy, no mask
    tensor, whole prompt and chunked prefill alike, GQA by head index.  ``allow_fp16_qk_reduction`` asks the reference
    for fp16 score accumulation on RTX 4090 (utils/__init__.py:165); scores accumulate in fp32 here either way.  The
    rotary arguments are unused, as in the reference (RotaryMode::kNone, batch_prefill.cu:102).  Returns a new tensor
    (batch_prefill.cu:73)."""
    _check_input(q, "q")
    _check_input(kv_data, "kv_data")
    _check_input(kv_indices, "kv_indices")
    _check_dim(3, q, "q")
    _check_dim(5, kv_data, "kv_data")
    _check_dim(1, kv_indices, "kv_indices")
    _check_eq(kv_indices.dtype, torch.int32, "kv_indices.scalar_type(), torch::kInt32")
    _check_eq(q.size(2), kv_data.size(4), "q.size(2), kv_data.size(4)")
    _check_half(q, "BatchPrefillWithPagedKVCache", kv_data)
    o = torch.empty_like(q)
    if q.size(0) == 0:  # nothing to attend from (the reference launches an empty grid)
        return o
    kv = _paged(kv_data, kv_indices, None, kv_last_page_len, 0, layout)
    check(lib.quest_prefill_with_paged_kv_cache(q.data_ptr(), o.data_ptr(), q.size(0), q.size(1), kv, kv_indices.size(0),
                                                1 if causal else 0, _stream(q)), "BatchPrefillWithPagedKVCache")
    return o


# ---------------------------------------------------------------- handler class

SAMPLE_MAX_VOCAB = 1 << 18  # quest_sample_tokens: QUEST_EUNSUPPORTED beyond
SAMPLE_MAX_EOS = 8


def sample_tokens(logits, temperature, top_k, top_p, seed, tokens, *, states=None, positions=None, kept=None,
                  eos_ids=None, pad_id: int = 0, finished=None, history=None, history_len=None, embed=None,
                  next_input=None) -> None:
    """One token per row of ``logits`` ``[n, vocab]`` (fp16 / bf16, contiguous rows ``logits.stride(0)`` apart, any
    2-byte alignment) under the sampling contract of include/quest_hip.h ("Token sampling"; EXTENSION): temperature, then
    top-k, then top-p, a Gumbel-max draw from Philox4x32-10 of (seed, position, token index); greedy for temperature 0.
    ``temperature`` / ``top_p`` fp32 ``[n]``, ``top_k`` int32 ``[n]``, ``seed`` int64 ``[n]`` (the uint64's bits), ``tokens``
    int32 ``[n]`` (written); exactly one of ``states`` (``[n, 8]`` int32 step states: position = ``seq_len``) /
    ``positions`` (int32 ``[n]``).  Optional: ``kept`` int32 ``[n]``; ``finished`` int32 ``[n]`` in/out with ``eos_ids``
    (int32, at most 8) and ``pad_id``; ``history`` int32 ``[n, stride]`` with ``history_len`` int32 ``[n]``; ``embed``
    ``[vocab, hidden]`` with ``next_input`` ``[n, hidden]`` (the launch copies the chosen token's embedding row there)."""
    _check_rows(logits, "logits")
    n, vocab = logits.size(0), logits.size(1)
    _check_half(logits, "sample_tokens", embed, next_input)
    i32, f32 = torch.int32, torch.float32
    for t, name, dt, numel in ((temperature, "temperature", f32, n), (top_k, "top_k", i32, n), (top_p, "top_p", f32, n),
                               (seed, "seed", torch.int64, n), (tokens, "tokens", i32, n), (kept, "kept", i32, n),
                               (positions, "positions", i32, n), (states, "states", i32, n * STEP_STATE_INTS),
                               (finished, "finished", i32, n), (history_len, "history_len", i32, n),
                               (eos_ids, "eos_ids", i32, None), (history, "history", i32, None)):
        if t is None:
            continue
        _check_input(t, name)
        _check_eq(t.dtype, dt, f"{name}.scalar_type()")
        if numel is not None:
            _check_eq(t.numel(), numel, f"{name}.numel()")
    if history is not None:
        _check_dim(2, history, "history")
        _check_eq(history.size(0), n, "history.size(0), n")
    hidden = 0
    if embed is not None:
        _check_input(embed, "embed")
        _check_dim(2, embed, "embed")
        _check_eq(embed.size(0), vocab, "embed.size(0), vocab")
        hidden = embed.size(1)
        if next_input is not None:
            _check_input(next_input, "next_input")
            _check_eq(next_input.numel(), n * hidden, "next_input.numel(), n * hidden")
    ptr = lambda t: t.data_ptr() if t is not None else None
    check(lib.quest_sample_tokens(
        logits.data_ptr(), logits.stride(0), vocab, n, _DTYPES[logits.dtype], ptr(temperature), ptr(top_k), ptr(top_p),
        ptr(seed), ptr(states), ptr(positions), ptr(tokens), ptr(kept), ptr(eos_ids),
        eos_ids.numel() if eos_ids is not None else 0, int(pad_id), ptr(finished), ptr(history),
        history.size(1) if history is not None else 0, ptr(history_len), ptr(embed), hidden, ptr(next_input),
        _stream(logits)), "sample_tokens")


class BatchDecodeWithPagedKVCachePyTorchWrapper:
    """bsk_ops.h:88-117 / approx_attn.cu:27-150: begin_forward plans, forward launches."""

    # EXTENSION: where every attention launch of this handler also writes the log-sum-exp (natural log) of its softmax
    # denominators -- a float32 contiguous device tensor of at least ``n_seqs * num_qo_heads`` elements, row (sequence, head)
    # at ``seq * num_qo_heads + head`` (the ``lse`` argument of include/quest_hip.h); None: no LSE is written.  What an
    # integrator needs to merge the attention over two page sets.  The caller keeps the tensor alive while set.
    lse_out = None

    def __init__(self, layout: int, *, dtype: torch.dtype = torch.float16):
        """``dtype`` (EXTENSION, keyword only): the element type this handler serves.  Constructed the reference's way it
        is fp16 and refuses everything else, like the reference's dispatch; ``dtype=torch.bfloat16`` makes a bf16 handler
        (which refuses fp16).  float32 has no kernels."""
        self._layout = int(layout)
        if dtype not in _DTYPES:
            raise RuntimeError(f"BatchDecodeWithPagedKVCache failed to dispatch with dtype {dtype}")
        self._dtype = dtype
        h = ctypes.c_void_p()
        check(lib.quest_decode_handler_create(ctypes.byref(h), self._layout), "BatchDecodeWithPagedKVCache")
        self._h = h
        if dtype != torch.float16:
            check(lib.quest_decode_set_dtype(h, _DTYPES[dtype]), "BatchDecodeWithPagedKVCache")
        self._destroy = lib.quest_decode_handler_destroy  # keep alive for __del__ at interpreter exit

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._destroy(h)

    def begin_forward(self, indptr, num_qo_heads: int, num_kv_heads: int, head_dim: int, page_size: int,
                      empty_data) -> None:
        _check_dim(1, indptr, "indptr")
        _check_eq(indptr.dtype, torch.int32, "indptr.scalar_type(), torch::kInt32")
        if empty_data.dtype != self._dtype:
            raise RuntimeError(f"BatchDecodeWithPagedKVCache failed to dispatch with dtype {empty_data.dtype}")
        # the planner needs the selected-page count on the host; the reference copies indptr back
        # too (decode_attn.cuh:866-873).  A CPU indptr skips the device sync.
        host = indptr if not indptr.is_cuda else indptr.cpu()
        n_sel = int(host[-1]) - int(host[0])
        stream = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None
        check(lib.quest_decode_begin_forward(self._h, n_sel, int(num_qo_heads), int(num_kv_heads), int(head_dim),
                                             int(page_size), stream), "BatchDecodeWithPagedKVCache")

    def _lse(self, q):
        """Pointer of ``lse_out`` for a launch over q ``[n_seqs, Hq, D]`` (None: the launch writes no LSE)."""
        t = self.lse_out
        if t is None:
            return None
        _check_input(t, "lse_out")
        if t.dtype != torch.float32:
            raise RuntimeError("lse_out must be a float32 tensor")
        _check_ge(t.numel(), q.size(0) * q.size(1), "lse_out.numel(), n_seqs * num_qo_heads")
        return t.data_ptr()

    def _check_dtype(self, q, *same) -> None:
        """q has the handler's element type and so have the call's other data tensors."""
        if q.dtype != self._dtype:
            raise RuntimeError(f"BatchDecodeWithPagedKVCache failed to dispatch with dtype {q.dtype} "
                               f"(the handler was made for {self._dtype})")
        _check_half(q, "BatchDecodeWithPagedKVCache", *same)

    def end_forward(self) -> None:
        check(lib.quest_decode_end_forward(self._h), "BatchDecodeWithPagedKVCache")

    def forward(self, q, o, paged_kv_data, paged_kv_indices, paged_kv_indptr, paged_kv_last_page_len: int,
                paged_kv_last_page_idx: int, rope_scale: float, rope_theta: float) -> None:
        _check_input(q, "q")
        _check_input(o, "o")
        _check_input(paged_kv_data, "paged_kv_data")
        _check_input(paged_kv_indices, "paged_kv_indices")
        _check_dim(3, q, "q")
        _check_dim(2, paged_kv_indices, "paged_kv_indices")
        _check_dim(5, paged_kv_data, "paged_kv_data")
        _check_eq(paged_kv_indices.size(0), q.size(1), "paged_kv_indices.size(0), num_qo_heads")
        _check_eq(paged_kv_data.size(1), 2, "paged_kv_data.size(1), 2")
        _check_eq(paged_kv_data.size(4), q.size(2), "paged_kv_data.size(4), head_dim")
        _check_eq(paged_kv_indices.dtype, torch.int32, "paged_kv_indices.scalar_type(), torch::kInt32")
        self._check_dtype(q, o, paged_kv_data)
        kv = _paged(paged_kv_data, paged_kv_indices, paged_kv_indptr, paged_kv_last_page_len,
                    paged_kv_last_page_idx, self._layout, page_budget=paged_kv_indices.size(1))
        check(lib.quest_decode_forward(self._h, q.data_ptr(), o.data_ptr(), kv, q.size(1), self._lse(q), _stream(q)),
              "BatchDecodeWithPagedKVCache")

    def forward_shared(self, q, o, paged_kv_data, page_list, paged_kv_last_page_len: int,
                       paged_kv_last_page_idx: int) -> bool:
        """EXTENSION: forward when all query heads share ONE page list ``[n_selected]`` (full-KV decode).  With
        GQA each K/V tile is fetched once per kv head.  False (nothing launched) if the shape is outside the
        shared kernel's set (page_size 16, head_dim 64/128)."""
        _check_input(q, "q")
        _check_input(o, "o")
        _check_input(paged_kv_data, "paged_kv_data")
        _check_input(page_list, "page_list")
        _check_dim(1, page_list, "page_list")
        _check_eq(page_list.dtype, torch.int32, "page_list.scalar_type(), torch::kInt32")
        self._check_dtype(q, o, paged_kv_data)
        kv = _paged(paged_kv_data, page_list, None, paged_kv_last_page_len, paged_kv_last_page_idx, self._layout)
        return _launched(lib.quest_decode_forward_shared(self._h, q.data_ptr(), o.data_ptr(), kv, q.size(1), self._lse(q),
                                                         _stream(q)), "BatchDecodeWithPagedKVCache")

    def forward_fused_topk(self, q, o, paged_kv_data, page_table, scores, topk_val_out, topk_idx_out,
                           paged_kv_last_page_len: int, paged_kv_last_page_idx: int) -> bool:
        """EXTENSION: topk_filtering + forward in one launch.  ``page_table`` is the sequence's page table
        ``[n_pages]`` (kv_indices_with_last), ``scores`` the estimate output ``[Hq, n_pages-1]``.  Returns
        False (nothing launched) when the current plan's chunks are too large for the fused front end."""
        _check_input(q, "q")
        _check_input(o, "o")
        _check_input(paged_kv_data, "paged_kv_data")
        _check_input(page_table, "page_table")
        _check_rows(scores, "scores")  # [Hq, n_scores], rows possibly padded (decode_append_estimate's output)
        _check_dim(3, q, "q")
        _check_dim(1, page_table, "page_table")
        _check_dim(5, paged_kv_data, "paged_kv_data")
        _check_eq(scores.size(0), q.size(1), "scores.size(0), num_qo_heads")
        _check_eq(page_table.size(0), scores.size(1) + 1, "page_table.size(0), n_scores + 1")
        _check_eq(page_table.dtype, torch.int32, "page_table.scalar_type(), torch::kInt32")
        self._check_dtype(q, o, paged_kv_data, scores)
        kv = _paged(paged_kv_data, page_table, None, paged_kv_last_page_len, paged_kv_last_page_idx, self._layout)
        # (QUEST_EUNSUPPORTED: chunk larger than the fused front end stages)
        return _launched(lib.quest_decode_forward_fused_topk(
            self._h, q.data_ptr(), o.data_ptr(), kv, q.size(1), scores.data_ptr(), scores.size(1), scores.stride(0),
            topk_val_out.data_ptr() if topk_val_out is not None else None,
            topk_idx_out.data_ptr() if topk_idx_out is not None else None, self._lse(q), _stream(q)), "BatchDecodeWithPagedKVCache")

    # ---- state-driven launches (see the free functions above): n sequences per launch, one sequence = the batch of one in
    # its own shapes (state ``[8]``, tables ``[capacity]``, scores ``[Hq, stride]``)
    def set_batch(self, n_seqs: int) -> None:
        """Sequences per launch the NEXT begin_forward plans for (workspace, work split)."""
        check(lib.quest_decode_set_batch(self._h, int(n_seqs)), "set_batch")

    def forward_shared_batched(self, q, o, paged_kv_data, kv_tables, state) -> None:
        """forward_shared over all pages of every sequence, live lengths from ``state`` (graph replay): q/o ``[n, Hq, D]``."""
        for t, n in ((q, "q"), (o, "o"), (paged_kv_data, "paged_kv_data"), (state, "state")):
            _check_input(t, n)
        b = _batch(state, kv_tables, None)
        _check_dim(3, q, "q")
        _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
        self._check_dtype(q, o, paged_kv_data)
        kv = _paged(paged_kv_data, kv_tables, None, 1, 0, self._layout)
        check(lib.quest_decode_forward_shared_batched(self._h, q.data_ptr(), o.data_ptr(), kv, q.size(1),
                                                      state.data_ptr(), b, self._lse(q), _stream(q)),
              "BatchDecodeWithPagedKVCache")

    def forward_shared_dyn(self, q, o, paged_kv_data, page_table, state) -> None:
        """``forward_shared_batched`` under its single-sequence name."""
        self.forward_shared_batched(q, o, paged_kv_data, page_table, state)

    def append_forward_shared_batched(self, k, v, metadata_data, meta_tables, q, o, paged_kv_data, kv_tables, state) -> bool:
        """``append_kv_cache_decode_batched`` + ``forward_shared_batched`` in ONE launch (k, v ``[n, Hkv, D]``; the new
        token's row is taken from k / v by the workgroup that attends the current page, written to the pool and folded into
        the metadata there).  False when the shape is outside the group-shared kernel: the caller issues the two launches."""
        for t, n in ((k, "k"), (v, "v"), (metadata_data, "metadata_data"), (q, "q"), (o, "o"),
                     (paged_kv_data, "paged_kv_data"), (state, "state")):
            _check_input(t, n)
        b = _batch(state, kv_tables, meta_tables)
        _check_dim(3, q, "q")
        _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
        _check_eq(k.size(0), b.n_seqs, "k.size(0), n_seqs")
        self._check_dtype(q, o, paged_kv_data, k, v, metadata_data)
        _check_eq(tuple(k.shape), tuple(v.shape), "k.shape, v.shape")
        kv = _paged(paged_kv_data, kv_tables, None, 1, 0, self._layout)
        _check_eq(tuple(k.shape[-2:]), (kv.num_heads, kv.head_dim), "k.shape[-2:], (kv heads, head_dim)")
        meta = _paged(metadata_data, meta_tables, None, 1, 0, self._layout)
        return _launched(lib.quest_decode_append_forward_shared_batched(
            self._h, k.data_ptr(), v.data_ptr(), meta, q.data_ptr(), o.data_ptr(), kv, q.size(1), state.data_ptr(), b, self._lse(q),
            _stream(q)), "BatchDecodeWithPagedKVCache")

    def append_forward_shared_dyn(self, k, v, metadata_data, meta_table, q, o, paged_kv_data, page_table, state) -> bool:
        """``append_forward_shared_batched`` under its single-sequence name."""
        return self.append_forward_shared_batched(k, v, metadata_data, meta_table, q, o, paged_kv_data, page_table, state)

    def forward_batched(self, q, o, paged_kv_data, indices, state, budgets=None) -> None:
        """forward for ``n`` sequences in one launch: q/o ``[n, Hq, D]``, indices ``[n, Hq, k_max]`` (int32) of which
        row (i, h) is read up to ``min(budget_i - 1, n_pages_i - 1)`` entries; the current page comes from ``state``."""
        for t, n in ((q, "q"), (o, "o"), (paged_kv_data, "paged_kv_data"), (indices, "indices"), (state, "state")):
            _check_input(t, n)
        b = _batch(state, None, None, budgets)
        _check_dim(3, q, "q")
        _check_dim(3, indices, "indices")
        _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
        _check_eq(indices.size(0), b.n_seqs, "indices.size(0), n_seqs")
        _check_eq(indices.size(1), q.size(1), "indices.size(1), num_qo_heads")
        _check_eq(indices.dtype, torch.int32, "indices.scalar_type(), torch::kInt32")
        self._check_dtype(q, o, paged_kv_data)
        kv = _paged(paged_kv_data, None, None, 1, 0, self._layout)
        check(lib.quest_decode_forward_batched(self._h, q.data_ptr(), o.data_ptr(), kv, q.size(1), indices.data_ptr(),
                                               indices.size(2), state.data_ptr(), b, self._lse(q), _stream(q)),
              "BatchDecodeWithPagedKVCache")

    def forward_fused_topk_batched(self, q, o, paged_kv_data, kv_tables, scores, state, max_n_scores: int,
                                   budgets=None, tiles: bool = False) -> bool:
        """forward_fused_topk for ``n`` sequences in one launch, row lengths and current pages from ``state`` (graph
        replay): q/o ``[n, Hq, D]``, scores ``[n, Hq, stride]``.
        ``tiles``: the rows carry their tile maxima (``append_estimate_batched(..., tiles=True)`` wrote them): two short
        selection passes instead of passes over the whole row; returns False (nothing launched) where the plan is
        outside what the tiles launch serves (more than 256 selected pages, page size != 16)."""
        for t, n in ((q, "q"), (o, "o"), (paged_kv_data, "paged_kv_data"), (scores, "scores"), (state, "state")):
            _check_input(t, n)
        b = _batch(state, kv_tables, None, budgets)
        scores = _lead(scores, 3)
        _check_dim(3, q, "q")
        _check_dim(3, scores, "scores")
        _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
        _check_eq(scores.size(0), b.n_seqs, "scores.size(0), n_seqs")
        _check_eq(scores.size(1), q.size(1), "scores.size(1), num_qo_heads")
        _check_ge(scores.size(2), max_n_scores, "scores.size(2), max_n_scores")
        self._check_dtype(q, o, paged_kv_data, scores)  # (the score rows are read as 16-bit keys of the handler's type)
        kv = _paged(paged_kv_data, kv_tables, None, 1, 0, self._layout)
        if tiles:
            _check_ge(scores.size(2), tiles_row_stride(max_n_scores), "scores.size(2), tiles_row_stride(max_n_scores)")
        code = lib.quest_decode_forward_fused_topk_batched(
            self._h, q.data_ptr(), o.data_ptr(), kv, q.size(1), scores.data_ptr(), scores.size(2), int(max_n_scores),
            tile_max_offset(max_n_scores) if tiles else 0, state.data_ptr(), b, self._lse(q), _stream(q))
        if not tiles:  # whole rows are the caller's last route: QUEST_EUNSUPPORTED raises
            check(code, "BatchDecodeWithPagedKVCache")
        return _launched(code, "BatchDecodeWithPagedKVCache")

    def forward_fused_topk_dyn(self, q, o, paged_kv_data, page_table, scores, state, max_n_scores: int,
                               tiles: bool = False) -> bool:
        """``forward_fused_topk_batched`` under its single-sequence name: ``scores`` ``[Hq, stride]``, state ``[8]``."""
        return self.forward_fused_topk_batched(q, o, paged_kv_data, page_table, scores, state, max_n_scores, tiles=tiles)

    def forward_group_topk(self, q, o, paged_kv_data, kv_tables, scores, state, max_n_scores: int, budgets=None,
                           paged_kv_last_page_len: int = 1, paged_kv_last_page_idx: int = 0) -> bool:
        """EXTENSION, opt-in: group-shared page selection for GQA -- ONE selection per kv head (the key-max of its group's
        score rows, then the top-k contract), attended by all query heads of the group: each selected K/V tile is fetched
        once per kv head.  Arguments as ``forward_fused_topk_batched``; ``state=None`` is the eager single-sequence form
        (q/o ``[1, Hq, D]``, scores ``[Hq, stride]`` with ``max_n_scores`` live columns, ``kv_tables`` the page table
        ``[max_n_scores + 1]``, the current page from ``paged_kv_last_page_len`` / ``paged_kv_last_page_idx``).
        ``set_selection_out`` rows are ``[n_seqs, Hkv, n_selected]``.  Returns False (nothing launched, ``o`` untouched) where
        the shape is outside the launch's envelope (page size 16, head_dim 64 / 128, group 1 / 2 / 4 / 8, <= 256 selected
        pages, rows <= 4096 pages, <= 64 sequences)."""
        for t, n in ((q, "q"), (o, "o"), (paged_kv_data, "paged_kv_data")):
            _check_input(t, n)
        if scores.dim() == 2:  # one sequence: rows possibly padded (decode_append_estimate's output)
            _check_rows(scores, "scores")
        else:
            _check_input(scores, "scores")
        scores = _lead(scores, 3)
        _check_dim(3, q, "q")
        _check_dim(3, scores, "scores")
        if state is None:
            _check_input(kv_tables, "kv_tables")
            _check_eq(q.size(0), 1, "q.size(0), 1")
            _check_ge(kv_tables.numel(), max_n_scores + 1, "kv_tables.numel(), max_n_scores + 1")
            _check_eq(kv_tables.dtype, torch.int32, "kv_tables.scalar_type(), torch::kInt32")
            b = Batch(1, 0, 0, 0, None)
        else:
            _check_input(state, "state")
            b = _batch(state, kv_tables, None, budgets)
        _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
        _check_eq(scores.size(0), b.n_seqs, "scores.size(0), n_seqs")
        _check_eq(scores.size(1), q.size(1), "scores.size(1), num_qo_heads")
        _check_ge(scores.stride(1), max_n_scores, "scores.stride(1), max_n_scores")
        self._check_dtype(q, o, paged_kv_data, scores)
        kv = _paged(paged_kv_data, kv_tables, None, paged_kv_last_page_len, paged_kv_last_page_idx, self._layout)
        return _launched(lib.quest_decode_forward_group_topk(
            self._h, q.data_ptr(), o.data_ptr(), kv, q.size(1), scores.data_ptr(), scores.stride(1), int(max_n_scores),
            state.data_ptr() if state is not None else None, b, self._lse(q), _stream(q)), "BatchDecodeWithPagedKVCache")

    def layer_fused_batched(self, k, v, metadata_data, meta_tables, q, o, paged_kv_data, kv_tables, state,
                            max_n_scores: int, budgets=None, scores_out=None) -> bool:
        """One launch per layer of a batched step: ``append_estimate_batched`` + ``forward_fused_topk_batched`` as one
        grid of (sequence, head) workgroups that keep the page scores in LDS (csrc/layer_device.cuh).  Same pool bytes,
        selections and outputs.  ``scores_out``: optional ``[n, Hq, >= max_n_scores]`` fp16 inspection copy of the
        scores.  Returns False (nothing launched) when the plan / shape is outside what the launch serves."""
        for t, n in ((k, "k"), (v, "v"), (metadata_data, "metadata_data"), (q, "q"), (o, "o"),
                     (paged_kv_data, "paged_kv_data"), (state, "state")):
            _check_input(t, n)
        b = _batch(state, kv_tables, meta_tables, budgets)
        _check_dim(3, q, "q")
        _check_dim(3, k, "k")
        _check_eq(q.size(0), b.n_seqs, "q.size(0), n_seqs")
        _check_eq(k.size(0), b.n_seqs, "k.size(0), n_seqs")
        _check_eq(tuple(o.shape), tuple(q.shape), "o.shape, q.shape")
        _check_eq(tuple(k.shape), tuple(v.shape), "k.shape, v.shape")
        self._check_dtype(q, o, paged_kv_data, k, v, metadata_data)
        kv = _paged(paged_kv_data, kv_tables, None, 1, 0, self._layout)
        _check_eq(tuple(k.shape[-2:]), (kv.num_heads, kv.head_dim), "k.shape[-2:], (kv heads, head_dim)")
        meta = _paged(metadata_data, meta_tables, None, 1, 0, self._layout)
        sc_ptr, sc_stride = None, 0
        if scores_out is not None:
            scores_out = _lead(scores_out, 3)
            _check_input(scores_out, "scores_out")
            _check_dim(3, scores_out, "scores_out")
            _check_eq(tuple(scores_out.shape[:2]), tuple(q.shape[:2]), "scores_out.shape[:2], (n_seqs, num_qo_heads)")
            _check_ge(scores_out.size(2), max_n_scores, "scores_out.size(2), max_n_scores")
            self._check_dtype(q, scores_out)
            sc_ptr, sc_stride = scores_out.data_ptr(), scores_out.size(2)
        return _launched(lib.quest_decode_layer_fused_batched(
            self._h, k.data_ptr(), v.data_ptr(), meta, q.data_ptr(), o.data_ptr(), kv, q.size(1), int(max_n_scores),
            state.data_ptr(), b, sc_ptr, sc_stride, self._lse(q), _stream(q)), "BatchDecodeWithPagedKVCache")

    # introspection used by the bench / tuning sweeps (not part of the reference surface)
    def plan_info(self):
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib.quest_decode_plan_info(self._h, ctypes.byref(a), ctypes.byref(b)), "plan_info")
        return a.value, b.value

    def last_launch_info(self) -> dict:
        """Which kernel instantiation the handler's most recent per-head-list launch took: keys per thread of the fused
        front end (0 = index-tensor launch), waves per workgroup, front-end variant (DecodeParams.vec_front: 0 / 1 / 3
        first generation staged / vector-staged / direct, 2 second generation, 8 tiles, 7 the one-launch layer, 9 the
        group-selection launch, whose workgroups are counted per kv head), whether
        the one-variant instantiation was launched, workgroups per head, sequences.  So that tests and benches can assert
        they run the same kernel."""
        info = (ctypes.c_uint32 * 6)()
        check(lib.quest_decode_last_launch_info(self._h, info), "last_launch_info")
        return {"keys_per_thread": info[0], "waves": info[1], "front_end_variant": info[2], "specialised": bool(info[3]),
                "workgroups_per_head": info[4], "n_seqs": info[5]}

    def set_pages_per_chunk(self, ppc: int) -> None:
        check(lib.quest_decode_set_pages_per_chunk(self._h, int(ppc)), "set_pages_per_chunk")

    def set_front_end(self, generation: int) -> None:
        """Tuning / test aid: force the fused launches' top-k front end (0 = automatic; 1 = first generation, 2 / 3 =
        second generation without / with its histogram pre-filter)."""
        check(lib.quest_decode_set_front_end(self._h, int(generation)), "set_front_end")

    def set_selection_out(self, val_out, idx_out) -> None:
        """Inspection aid: the state-driven / batched fused launches also write their selection into
        ``val_out`` fp16 / ``idx_out`` int32, both ``[n_seqs, Hq, n_selected]`` (None, None: off).  The caller keeps
        the tensors alive while set."""
        if idx_out is not None:
            _check_input(idx_out, "idx_out")
            _check_eq(idx_out.dtype, torch.int32, "idx_out.scalar_type(), torch::kInt32")
        if val_out is not None:
            _check_input(val_out, "val_out")
            if val_out.dtype != self._dtype:
                raise RuntimeError(f"set_selection_out failed to dispatch with dtype {val_out.dtype} "
                                   f"(the handler was made for {self._dtype})")
        self._sel_keepalive = (val_out, idx_out)
        check(lib.quest_decode_set_selection_out(self._h, val_out.data_ptr() if val_out is not None else None,
                                                 idx_out.data_ptr() if idx_out is not None else None),
              "set_selection_out")

    def arm_step_advance(self, state, kv_tables, meta_tables, page_size: int) -> None:
        """The NEXT token's reservation (``step_state_advance_batched``) rides in this handler's next forward call: in its merge
        launch where the plan has one, as its own launch behind the attention kernel otherwise.  ``state`` is the step state
        ``[8]`` (one sequence, tables ``[capacity]``) or ``[n, 8]`` (tables ``[n, capacity]``).  Call right before the LAST
        layer's forward of a step whose first token was reserved by ``step_state_advance_batched`` (quest_hip.h)."""
        _check_input(state, "state")
        _check_eq(state.dtype, torch.int32, "state.scalar_type(), torch::kInt32")
        b = _batch(state, kv_tables, meta_tables)
        check(lib.quest_decode_arm_step_advance(self._h, state.data_ptr(), kv_tables.data_ptr(), meta_tables.data_ptr(),
                                                int(page_size), kv_tables.size(-1), meta_tables.size(-1), b),
              "arm_step_advance")

    def set_skip_merge(self, skip: bool) -> None:
        """Measurement aid: launch only the attention kernel (partial states stay unmerged, ``o`` unwritten)."""
        check(lib.quest_decode_set_skip_merge(self._h, int(bool(skip))), "set_skip_merge")
