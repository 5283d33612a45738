"""The element type at the C ABI and in the Python layers, without a GPU: every call below is refused before a launch (or,
where it is well formed and no device is visible, gets as far as the launch and comes back with a HIP error), and the
resources of the bf16 kernels are read from the built library's code-object metadata.

The entry table, the fake operands and the planned handler are tests/test_return_codes.py's."""
import ctypes
import os

import pytest
import torch

from test_return_codes import EINVAL, EUNSUPPORTED, PLAN, _device_visible, _entries, _kv
from test_return_codes import _call as _entry_call

F16, BF16 = 0, 1


def _handler(lib, dtype=F16):
    h = ctypes.c_void_p()
    assert lib.quest_decode_handler_create(ctypes.byref(h), 0) == 0
    assert lib.quest_decode_set_dtype(h, dtype) == 0
    assert lib.quest_decode_set_batch(h, PLAN["batch"]) == 0
    assert lib.quest_decode_begin_forward(h, PLAN["n_sel"], PLAN["hq"], PLAN["hkv"], PLAN["d"], PLAN["ps"], None) == 0
    return h


def _call(lib, name, h, **rep):
    """`name`: an entry in one of its forms, as tests/test_return_codes.py lists them."""
    entry, args = _entry_call(_entries(), name, rep)
    if "h" in args:
        args["h"] = h
    return getattr(lib, entry)(*args.values())


def test_unknown_dtype_is_einval_before_any_launch():
    """dtype = 7 in a pool view: QUEST_EINVAL from every entry that takes a view, whichever view carries it -- on operands
    that are otherwise well formed, so a launch would have followed."""
    from quest_amd._lib import lib

    h = _handler(lib)
    try:
        n = 0
        for name, args in _entries().items():
            for pool in ("kv", "metadata"):
                if pool in dict(args):
                    assert _call(lib, name, h, **{pool: _kv(dtype=7)}) == EINVAL, (name, pool)
                    n += 1
        assert n >= 35
        assert lib.quest_prefill_with_paged_kv_cache(16, 16, 4, 32, _kv(dtype=7), 4, 1, None) == EINVAL
        assert lib.quest_decode_set_dtype(h, 7) == EINVAL
        assert lib.quest_apply_rope_in_place_dtype(16, 16, 1, 0, 4, 4, 128, 1.0, 1e4, None, 1.0, None, 7, None) == EINVAL
        assert lib.quest_rms_norm_forward_dtype(16, 16, 16, 1, 128, 1e-5, 7, None) == EINVAL
    finally:
        lib.quest_decode_handler_destroy(h)


def test_mismatched_views_and_handlers_are_einval_before_any_launch():
    """Two views of one call with different element types, or a view of another type than the handler's: QUEST_EINVAL.
    The same calls with matching types are well formed (where no device is visible they reach the launch: > 0)."""
    from quest_amd._lib import lib

    h16, hbf = _handler(lib, F16), _handler(lib, BF16)
    try:
        both = [name for name, args in _entries().items() if "kv" in dict(args) and "metadata" in dict(args)]
        assert len(both) >= 12
        for name in both:
            for h in (h16, hbf):
                assert _call(lib, name, h, kv=_kv(dtype=BF16), metadata=_kv(dtype=F16)) == EINVAL, name
                assert _call(lib, name, h, kv=_kv(dtype=F16), metadata=_kv(dtype=BF16)) == EINVAL, name
        with_h = [name for name, args in _entries().items() if "h" in dict(args)]
        assert len(with_h) >= 13
        for name in with_h:
            views = {p: _kv(dtype=BF16) for p in ("kv", "metadata") if p in dict(_entries()[name])}
            assert _call(lib, name, h16, **views) == EINVAL, name                      # bf16 views, fp16 handler
            assert _call(lib, name, hbf) == EINVAL, name                               # fp16 views, bf16 handler
        # the one-launch layer has no bf16 form: QUEST_EUNSUPPORTED (nothing launched), and the controller never asks for it
        views = dict(kv=_kv(dtype=BF16), metadata=_kv(dtype=BF16))
        assert _call(lib, "quest_decode_layer_fused_batched", hbf, **views) == EUNSUPPORTED
        if not _device_visible():  # (a device would run these on the fake operands)
            for name in with_h:
                if name == "quest_decode_layer_fused_batched":
                    continue
                views = {p: _kv(dtype=BF16) for p in ("kv", "metadata") if p in dict(_entries()[name])}
                assert _call(lib, name, hbf, **views) > 0, name
            for name in ("quest_append_kv_cache_decode", "quest_append_kv_cache_prefill", "quest_estimate_attn_score",
                         "quest_append_estimate, contiguous rows"):
                views = {p: _kv(dtype=BF16) for p in ("kv", "metadata") if p in dict(_entries()[name])}
                assert _call(lib, name, None, **views) > 0, name
    finally:
        lib.quest_decode_handler_destroy(h16)
        lib.quest_decode_handler_destroy(hbf)


def test_one_launch_layers_are_fp16_only():
    import quest_amd.utils as qu

    kw = dict(num_kv_heads=32)
    b16 = qu.BatchedInferenceController(8, 1, 32, 128, 16, 8, 64, torch.float16, "cpu", **kw)
    bbf = qu.BatchedInferenceController(8, 1, 32, 128, 16, 8, 64, torch.bfloat16, "cpu", **kw)
    assert b16.one_launch_layers is True and bbf.one_launch_layers is False
    assert bbf.kv_pool.layer(0).dtype == torch.bfloat16 and bbf.metadata_pool.layer(0).dtype == torch.bfloat16


def test_drop_in_wrapper_refuses_bf16_by_default_and_fp32_always():
    from quest_amd import _kernels

    indptr = torch.tensor([0, 3], dtype=torch.int32)
    w = _kernels.BatchDecodeWithPagedKVCachePyTorchWrapper(0)  # constructed the reference's way
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        w.begin_forward(indptr, 32, 32, 128, 16, torch.empty(0, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        w.begin_forward(indptr, 32, 32, 128, 16, torch.empty(0, dtype=torch.float32))
    wb = _kernels.BatchDecodeWithPagedKVCachePyTorchWrapper(0, dtype=torch.bfloat16)  # the explicit extension
    wb.set_batch(64)  # one workgroup per head: a plan that allocates nothing, so it can be made without a device
    wb.begin_forward(indptr, 32, 32, 128, 16, torch.empty(0, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        wb.begin_forward(indptr, 32, 32, 128, 16, torch.empty(0, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        _kernels.BatchDecodeWithPagedKVCachePyTorchWrapper(0, dtype=torch.float32)
    with pytest.raises(TypeError):  # keyword only: the reference's positional signature is (layout)
        _kernels.BatchDecodeWithPagedKVCachePyTorchWrapper(0, torch.bfloat16)
    # the free functions: fp32 has no kernel, and one call has one element type
    x32 = torch.zeros(1, 2, 128)
    with pytest.raises(RuntimeError, match="dispatch with dtype torch.float32"):
        _kernels._check_half(x32, "op")
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        _kernels._check_half(x32.half(), "op", x32.bfloat16())
    _kernels._check_half(x32.bfloat16(), "op", x32.bfloat16(), None)
    with pytest.raises(RuntimeError, match="dispatch with dtype"):  # the fused projections stay fp16-only
        _kernels._check_f16(x32.bfloat16(), "decode_norm_gemv")
    # a pool view carries its tensor's type
    pool = torch.zeros(2, 2, 16, 4, 128, dtype=torch.bfloat16)
    assert _kernels._paged(pool, None, None, 1, 0, 0).dtype == BF16
    assert _kernels._paged(pool.half(), None, None, 1, 0, 0).dtype == F16
    with pytest.raises(RuntimeError, match="dispatch with dtype"):
        _kernels._paged(pool.float(), None, None, 1, 0, 0)


# ---- resources of the bf16 kernels as built: the instantiations tests/test_build_metadata.py names, in their _bf16 form
from quest_amd.build import LIB, kernel_metadata  # noqa: E402

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
needs_tools = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")),
                                 reason="needs the built library and the ROCm LLVM tools (llvm-objcopy / llvm-readelf)")


@pytest.fixture(scope="module")
def meta():
    return kernel_metadata(LIB)


def _pair(meta, fragment):
    """(fp16 kernel, its bf16 twin) of a mangled-name fragment that starts at the kernel's name."""
    name = fragment[:fragment.index("ILi")]
    f16 = [v for k, v in meta.items() if f"{len(name)}{fragment}" in k]
    bf = [v for k, v in meta.items() if f"{len(name) + 5}{name}_bf16{fragment[len(name):]}" in k]
    assert len(f16) == 1 and len(bf) == 1, (fragment, len(f16), len(bf))
    return f16[0], bf[0]


@needs_tools
@pytest.mark.parametrize("fragment", [
    "sparse_decode_kernelILi128ELi16ELi8ELi8ELi3E", "sparse_decode_kernelILi128ELi16ELi8ELi8ELi1E",
    "sparse_decode_kernelILi128ELi16ELi8ELi8ELi8E", "sparse_decode_kernelILi128ELi16ELi24ELi8ELi2E",
    "sparse_decode_kernelILi128ELi16ELi0ELi4ELin1E", "sparse_decode_kernelILi128ELi16ELi0ELi8ELin1E",
])
def test_bf16_attention_kernels_fit_two_workgroups_per_cu(meta, fragment):
    """No scratch, no spills, at most 128 VGPRs -- and the fp16 kernel's static LDS, byte for byte: the partial states
    were fp32 before (workspace records and the per-wave LDS accumulators alike), so bf16 needs nothing more.  Figure
    found: + 0 bytes for every instantiation below."""
    f16, bf = _pair(meta, fragment)
    assert bf["scratch"] == 0 and bf["vgpr_spill"] == 0, bf
    assert bf["vgpr"] <= 128, bf
    assert bf["lds"] == f16["lds"], (bf, f16)


@needs_tools
def test_bf16_instantiations_exist_and_do_not_spill(meta):
    """One bf16 kernel per fp16 kernel of the attention path (the fp16-only ones: the one-launch layer, the decode-layer
    projections); none of the bf16 head_dim 64 / 128 attention kernels, estimate, merge, shared-list, append, RoPE, norm or
    prefill kernels uses scratch where its fp16 twin does not."""
    import re

    twins = 0
    for name, v in meta.items():
        if "_bf16" not in name:
            continue
        twins += 1
        # _ZN5quest25sparse_decode_kernel_bf16ILi... -> _ZN5quest20sparse_decode_kernelILi...
        f16_name = re.sub(r"(\d+)([a-z_]+kernel)_bf16", lambda m: f"{int(m.group(1)) - 5}{m.group(2)}", name, count=1)
        assert f16_name in meta, (name, f16_name)
        f16 = meta[f16_name]
        assert v["lds"] <= f16["lds"], (name, v, f16)
        if not (f16["scratch"] or f16["vgpr_spill"]):
            assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (name, v)
    f16_typed = [k for k in meta if "_bf16" not in k and any(s in k for s in (
        "sparse_decode_kernel", "shared_decode_kernel", "merge_states_kernel", "estimate_kernel", "append_decode_kernel",
        "append_prefill_kernel", "rope_kernel", "rms_norm_kernel", "14prefill_kernel"))]
    assert twins == len(f16_typed) and twins > 100, (twins, len(f16_typed))
    hits = {k: v for k, v in meta.items() if "19prefill_kernel_bf16ILi" in k}
    assert len(hits) == 6, list(hits)
    for k, v in hits.items():
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["lds"] <= 80 * 1024, (k, v)
        if "ILi256E" not in k:
            assert v["vgpr"] <= 256, (k, v)
