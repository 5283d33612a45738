// The sign-plane estimate: append + estimate of ONE MHA sequence (head_dim 128, page size 16, fp16) with the scores read
// from a shadow store of the layer's metadata pool that keeps, per (kv head, feature, sign of q), the one value the score
// uses -- contiguous over logical pages.  With one query head per kv head the estimate needs, per (page, feature), either
// max(Kslot, Vslot) or min(Kslot, Vslot), never both: this launch fetches half of what the pool launch (estimate.hip)
// fetches, and follows no page table.
//
// Same arguments, same score rows and the same bits as quest_append_estimate_batched (whole rows): the per-lane octet sums
// and the row tree of estimate_tile are restated (estimate_planes_device.cuh), not approximated.
//
// Safety: a device word per layer, `covered`, counts the leading logical pages whose plane entries equal the pool's.  The
// build kernel sets it, the append role of this launch moves it on when a token completes a page, and a workgroup whose
// scored range is not entirely below it reads the pool instead (same arithmetic, same bits).  Appends that do not maintain
// the planes therefore only leave `covered` behind; nothing stale is read.  Bound: HBM.
#include "estimate_planes_device.cuh"
#include "pool_check.h"

namespace quest {

__global__ __launch_bounds__(kPlaneBlock) void estimate_planes_build_kernel(half_t* planes, uint32_t blocks, int32_t* covered,
                                                                            quest_paged_kv_t meta,
                                                                            const quest_step_state_t* state) {
    planes_build_body(planes, blocks, covered, meta, state);
}

// Blocks [0, est_blocks): estimate workgroups, head fastest; the blocks behind them run the decode append.  The leading
// arguments are what a workgroup's first loads need (preloaded into SGPRs at wave launch, build.py).
__global__ __launch_bounds__(kPlaneThreads) void estimate_planes_kernel(const half_t* __restrict__ q, half_t* planes,
                                                                        int32_t* covered, const quest_step_state_t* state,
                                                                        uint32_t blocks, uint32_t est_blocks, uint32_t n_cap,
                                                                        uint32_t o_stride, half_t* __restrict__ o,
                                                                        quest_paged_kv_t meta, quest_paged_kv_t kv,
                                                                        const uint16_t* key, const uint16_t* value) {
    if (QUEST_UNLIKELY(blockIdx.x >= est_blocks)) {
        planes_append_body(planes, blocks, covered, kv, meta, key, value, state, (blockIdx.x - est_blocks) * kPlaneThreads + threadIdx.x);
        return;
    }
    __shared__ __attribute__((aligned(16))) float part[kPlaneDim / kVec][kPlaneWgPages];
    planes_estimate_body(q, planes, blocks, covered, meta, state, n_cap, o_stride, o, blockIdx.x % meta.num_heads,
                         blockIdx.x / meta.num_heads, part);
}

// What the planes serve: one fp16 MHA sequence, head_dim 128, page size 16 on both pools.  QUEST_EUNSUPPORTED otherwise,
// before any other check and before anything is launched.
static int planes_supported(uint32_t n_seqs, uint32_t num_qo_heads, const quest_paged_kv_t& metadata, uint32_t kv_page_size,
                            uint32_t kv_dtype) {
    if (n_seqs != 1) return QUEST_EUNSUPPORTED;
    if (metadata.num_heads == 0 || num_qo_heads != metadata.num_heads) return QUEST_EUNSUPPORTED;
    if (metadata.head_dim != kPlaneDim) return QUEST_EUNSUPPORTED;
    if (metadata.page_size != kPlanePageSize || kv_page_size != kPlanePageSize) return QUEST_EUNSUPPORTED;
    if (metadata.dtype == QUEST_DTYPE_BF16 || kv_dtype == QUEST_DTYPE_BF16) return QUEST_EUNSUPPORTED;
    return 0;
}

}  // namespace quest

using namespace quest;

extern "C" uint64_t quest_estimate_planes_bytes(uint32_t num_kv_heads, uint32_t plane_pages) {
    return (uint64_t)plane_halves(num_kv_heads, (plane_pages + kPlaneBlock - 1) / kPlaneBlock) * sizeof(half_t);
}

extern "C" int quest_estimate_planes_build(void* planes, uint32_t plane_pages, int32_t* covered, quest_paged_kv_t metadata,
                                           uint32_t kv_page_size, const quest_step_state_t* state, quest_stream_t stream) {
    if (int e = planes_supported(1, metadata.num_heads, metadata, kv_page_size, QUEST_DTYPE_F16)) return e;
    if (!planes || !covered || !state || plane_pages == 0 || plane_pages % kPlaneBlock != 0) return QUEST_EINVAL;
    if (((uintptr_t)planes & 15u) != 0) return QUEST_EINVAL;
    metadata.last_page_len = 1;  // placeholder; the kernel reads the live lengths from `state`
    if (int e = check_pool(metadata)) return e;
    const uint32_t blocks = plane_pages / kPlaneBlock;
    hipLaunchKernelGGL(estimate_planes_build_kernel, dim3(blocks, metadata.num_heads), dim3(kPlaneBlock), 0, (hipStream_t)stream,
                       (half_t*)planes, blocks, covered, metadata, state);
    QUEST_LAUNCH_CHECK();
    return 0;
}

extern "C" int quest_append_estimate_planes_batched(const void* k, const void* v, quest_paged_kv_t kv, const void* q, void* o,
                                                    uint32_t num_qo_heads, uint32_t o_stride, uint32_t max_n_out,
                                                    uint32_t tile_max_offset, quest_paged_kv_t metadata,
                                                    const quest_step_state_t* state, quest_batch_t batch, void* planes,
                                                    uint32_t plane_pages, int32_t* covered, quest_stream_t stream) {
    if (int e = planes_supported(batch.n_seqs, num_qo_heads, metadata, kv.page_size, kv.dtype)) return e;
    if (tile_max_offset) return QUEST_EUNSUPPORTED;
    if (int e = check_dtype_pair(kv, metadata)) return e;
    if (!k || !v || !q || !o || !state || max_n_out == 0 || o_stride < max_n_out) return QUEST_EINVAL;
    if (!planes || !covered || ((uintptr_t)planes & 15u) != 0) return QUEST_EINVAL;
    // the store is padded to whole page blocks and covers every page the grid is sized for
    if (plane_pages % kPlaneBlock != 0 || plane_pages < max_n_out) return QUEST_EINVAL;
    if (int e = check_pool_pair(kv, metadata, true, false)) return e;
    const uint32_t blocks = plane_pages / kPlaneBlock;
    const uint32_t est_blocks = ((max_n_out + kPlaneWgPages - 1) / kPlaneWgPages) * metadata.num_heads;
    const uint32_t append_blocks = (metadata.num_heads * (kPlaneDim / kVec) + kPlaneThreads - 1) / kPlaneThreads;
    hipLaunchKernelGGL(estimate_planes_kernel, dim3(est_blocks + append_blocks), dim3(kPlaneThreads), 0, (hipStream_t)stream,
                       (const half_t*)q, (half_t*)planes, covered, state, blocks, est_blocks, max_n_out, o_stride, (half_t*)o,
                       metadata, kv, (const uint16_t*)k, (const uint16_t*)v);
    QUEST_LAUNCH_CHECK();
    return 0;
}
