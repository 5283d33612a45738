"""Resources of the sign-plane kernels as BUILT (code-object metadata of libquest_hip.so; no GPU), like
tests/test_build_metadata.py: no scratch, no spills; the estimate kernel stays within 128 VGPRs (four waves per SIMD) and
holds the octet partials of its 128 pages in 8 KiB of LDS."""
import os

import pytest

from quest_amd.build import LIB, kernel_metadata

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")),
                                reason="needs the built library and the ROCm LLVM tools (llvm-objcopy / llvm-readelf)")


def test_planes_kernels_have_no_scratch_and_no_spills():
    meta = kernel_metadata(LIB)
    for fragment, max_vgpr, lds in (("22estimate_planes_kernel", 128, 8 * 1024), ("28estimate_planes_build_kernel", 128, 0)):
        hits = [v for k, v in meta.items() if fragment in k]
        assert len(hits) == 1, (fragment, [k for k in meta if "planes" in k])
        k = hits[0]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgpr"] <= max_vgpr and k["lds"] == lds, k
