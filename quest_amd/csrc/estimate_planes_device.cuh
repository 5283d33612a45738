// Device code of the sign-plane estimate (estimate_planes.hip): the MHA page-criticality estimate of ONE sequence read from
// a per-layer shadow store of the metadata pool that holds, per (kv head, feature, sign of q), the one fp16 value the
// score needs, contiguous over LOGICAL pages -- half the bytes of the pool's (max row, min row) pair, and no page table.
// See estimate.hip / estimate_device.cuh for the arithmetic this restates bit for bit.
#pragma once
#include "estimate_device.cuh"

namespace quest {

constexpr uint32_t kPlaneBlock = 256;  // pages of one page block = length of one contiguous (feature, sign) run
constexpr uint32_t kPlaneDim = 128;    // head_dim served
#ifndef QUEST_PLANES_WG_PAGES
// Pages one estimate workgroup scores: 128 (half a block, 4 waves, 256-byte pieces of the runs) or 256 (a whole block, 8
// waves).  Measured on one box, alternating, cfg 3 (profiles/estimate_planes_ab.txt): 128 -> 1596 tokens/s, 256 -> 1509
// (parent 1435): twice the workgroups, half as wide, start and retire in finer steps.  -DQUEST_PLANES_WG_PAGES=256: A/B.
#define QUEST_PLANES_WG_PAGES 128
#endif
constexpr uint32_t kPlaneWgPages = QUEST_PLANES_WG_PAGES;
static_assert(kPlaneWgPages == 256 || kPlaneWgPages == 128, "a workgroup scores a whole page block or half of one");
constexpr uint32_t kPlaneThreads = 2 * kPlaneWgPages;  // (pages / 8) groups of 8 pages x 16 feature octets
constexpr uint32_t kPlanePageSize = 16;  // page size served (KV pool and metadata pool)

// THE layout of the store, in halves: [kv head][block of 256 pages][feature][sign][256 pages].  A workgroup's region
// (head, block) is 128 KiB contiguous; for each feature it reads the 512-byte run of ONE sign.  sign 0 = hi (q >= 0),
// sign 1 = lo (q < 0).  `blocks` = page blocks per head (the padded page capacity / 256).
__host__ __device__ inline size_t plane_off(uint32_t h, uint32_t e, uint32_t d, uint32_t s, uint32_t blocks) {
    return ((((size_t)h * blocks + e / kPlaneBlock) * kPlaneDim + d) * 2u + s) * kPlaneBlock + e % kPlaneBlock;
}
__host__ __device__ inline size_t plane_halves(uint32_t num_heads, uint32_t blocks) {
    return (size_t)num_heads * blocks * kPlaneDim * 2u * kPlaneBlock;
}

// Address of the metadata pool's K-slot (max) row of (logical page e, kv head h), and the halves from it to the V-slot row.
__device__ __forceinline__ const half_t* plane_pool_row(const quest_paged_kv_t& meta, const PoolStrides& ms, uint32_t e,
                                                        uint32_t h, uint32_t& v_off) {
    const uint32_t e_in = e % kPlanePageSize, slot = pool_slot(ms, h, e_in);
    const size_t pg = (size_t)meta.indices[e / kPlanePageSize];
    v_off = pool_v_off(ms, slot);
    return reinterpret_cast<const half_t*>(meta.data) + pg * ms.page + (size_t)slot * ms.head + (size_t)e_in * ms.entry;
}

// hi / lo of a (max row, min row) piece with the packed fp16 max / min of the estimate's fast form (estimate_device.cuh):
// whatever the pool holds -- reversed slots, +-inf, NaN -- the planes hold what that kernel would select from.
__device__ __forceinline__ void plane_hi_lo(half8 mx, half8 mn, half8& hi, half8& lo) {
    hi = __builtin_elementwise_max(mx, mn);
    lo = __builtin_elementwise_min(mx, mn);
}

// Build: pages [0, n_full) of one layer's metadata pool -> planes; covered = n_full.  n_full = the sequence's complete
// pages (n_pages - 1, + 1 when the last page is full), read from the step state.  One thread = one (head, page): 16 pairs
// of 16-byte row pieces in, 2 x 128 two-byte stores out, coalesced over the pages of a wave.  grid (page blocks, heads).
__device__ __forceinline__ void planes_build_body(half_t* planes, uint32_t blocks, int32_t* covered, quest_paged_kv_t meta,
                                                  const quest_step_state_t* state) {
    const quest_step_state_t st = *state;
    uint32_t n_full = (uint32_t)(st.n_pages > 0 ? st.n_pages - 1 : 0) + (st.kv_last_page_len == (int32_t)kPlanePageSize ? 1u : 0u);
    if (st.n_pages <= 0) n_full = 0;
    if (n_full > blocks * kPlaneBlock) n_full = blocks * kPlaneBlock;
    const uint32_t h = blockIdx.y, e = blockIdx.x * kPlaneBlock + threadIdx.x;
    if (blockIdx.x == 0 && h == 0 && threadIdx.x == 0) *covered = (int32_t)n_full;
    if (e >= n_full) return;
    const PoolStrides ms = pool_strides(meta);
    uint32_t v_off;
    const half_t* row = plane_pool_row(meta, ms, e, h, v_off);
    uint16_t* out = reinterpret_cast<uint16_t*>(planes);
#pragma unroll 4
    for (uint32_t c = 0; c < kPlaneDim / kVec; ++c) {
        half8 hi, lo;
        plane_hi_lo(ld8(row + c * kVec), ld8(row + v_off + c * kVec), hi, lo);
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)kVec; ++i) {
            out[plane_off(h, e, c * kVec + i, 0, blocks)] = half_bits(hi[i]);
            out[plane_off(h, e, c * kVec + i, 1, blocks)] = half_bits(lo[i]);
        }
    }
}

// The append role of the planes launch, global thread `gtid` of the append blocks: today's decode append, then -- when this
// token completes its page -- the page's folded (max, min) entry goes into the planes at logical page n_pages - 1 and
// `covered` moves from n_pages - 1 to n_pages.  The scatter is unconditional on completion (idempotent; a page completed
// again after the state was set back is simply rewritten), the counter never jumps over a gap.  The page is not scored in
// this launch (the estimate stops at n_pages - 1), so the estimate workgroups never read what is written here; they may
// read either value of `covered`, and both give the same decision (both are >= the last scored page + 1).
__device__ __forceinline__ void planes_append_body(half_t* planes, uint32_t blocks, int32_t* covered, quest_paged_kv_t kv,
                                                   quest_paged_kv_t meta, const uint16_t* key, const uint16_t* value,
                                                   const quest_step_state_t* state, uint32_t gtid) {
    const quest_step_state_t st = *state;
    meta.last_page_len = (uint32_t)st.meta_last_page_len;
    meta.last_page_idx = st.meta_last_page_idx;
    kv.last_page_len = (uint32_t)st.kv_last_page_len;
    kv.last_page_idx = st.kv_last_page_idx;
    append_decode_body<half_t>(kv, meta, key, value, gtid);
    if (QUEST_LIKELY(st.kv_last_page_len != (int32_t)kPlanePageSize) || st.n_pages <= 0) return;
    const uint32_t e = (uint32_t)st.n_pages - 1u;
    if (e >= blocks * kPlaneBlock) return;
    constexpr uint32_t lpr = kPlaneDim / kVec;
    if (gtid < meta.num_heads * lpr) {
        // the entry this thread has just folded and stored (its own stores: program order)
        const uint32_t h = gtid / lpr, f = (gtid % lpr) * kVec;
        const PoolStrides ms = pool_strides(meta);
        const uint32_t mentry = meta.last_page_len - 1, mslot = pool_slot(ms, h, mentry);
        const half_t* row = reinterpret_cast<const half_t*>(meta.data) + (size_t)meta.last_page_idx * ms.page +
                            (size_t)mslot * ms.head + (size_t)mentry * ms.entry + f;
        half8 hi, lo;
        plane_hi_lo(ld8(row), ld8(row + pool_v_off(ms, mslot)), hi, lo);
        uint16_t* out = reinterpret_cast<uint16_t*>(planes);
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)kVec; ++i) {
            out[plane_off(h, e, f + i, 0, blocks)] = half_bits(hi[i]);
            out[plane_off(h, e, f + i, 1, blocks)] = half_bits(lo[i]);
        }
    }
    if (gtid == 0 && *covered == (int32_t)e) *covered = (int32_t)e + 1;
}

// Sum of a page's 16 octet partials p[c] in the association order of row_allreduce_sum_fast<16> as lane 0 sees it
// (row_ror 8, 4, 2, 1; each step adds the rotated-in value to the lane's own): the tree oracle/quest_oracle.c restates.
__device__ __forceinline__ float plane_row_tree(const float (&p)[16]) {
    float a[16], b[16], c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = p[i] + p[(i + 8) & 15];
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = a[i] + a[(i + 12) & 15];
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = b[i] + b[(i + 14) & 15];
    return c[0] + c[15];
}

// One estimate workgroup = (kv head h, kPlaneWgPages pages of one block): thread (pg = tid % groups, c = tid / groups) owns the 8 consecutive
// pages e0 + 8 pg .. + 7 and the feature octet c, accumulates the octet's 8 products per page left to right in fp32 from
// 0.f (one lane of a row of estimate_tile), the 16 octet partials of a page meet in LDS and are summed in the row tree,
// cast once to fp16.
//   planes path: eight 16-byte loads, one per feature, from the plane the sign of q[8c + i] chooses -- the lanes of an octet
//     cover the workgroup's piece of one 512-byte run; all issued up front, unconditional (the store is padded to whole blocks; entries past `covered` are
//     loaded and never used);
//   pool path (the whole workgroup: it spans the block's page range, and the head's q is its own): where the block's scored
//     range is not entirely below `covered`, or the head's q holds a zero or non-finite element -- the same 8 x 8 block from
//     the metadata pool (table lookup, K-slot and V-slot row pieces) and estimate_tile's fast or literal arithmetic.
__device__ __forceinline__ void planes_estimate_body(const half_t* __restrict__ q, const half_t* planes, uint32_t blocks,
                                                     const int32_t* covered, const quest_paged_kv_t& meta,
                                                     const quest_step_state_t* state, uint32_t n_cap, uint32_t o_stride,
                                                     half_t* __restrict__ o, uint32_t h, uint32_t b, float (*part)[kPlaneWgPages]) {
    constexpr uint32_t kGroups = kPlaneWgPages / kVec;  // groups of 8 pages per workgroup
    const uint32_t tid = threadIdx.x, pg = tid % kGroups, c = tid / kGroups;
    const uint32_t e0 = b * kPlaneWgPages;
    // q: the thread's octet, and -- every wave for itself, so no barrier stands before the loads -- the whole row's test
    const half_t* qh = q + (size_t)h * kPlaneDim;
    const half8 q8 = ld8(qh + c * kVec);
    const uint32_t qw = reinterpret_cast<const uint32_t*>(qh)[tid & 63u];
    const int32_t live_pages = ld_uniform_i32(&state->n_pages);
    const int32_t cov = __atomic_load_n(covered, __ATOMIC_RELAXED);
    uint32_t n_out = live_pages > 0 ? (uint32_t)(live_pages - 1) : 0u;
    if (n_out > n_cap) n_out = n_cap;
    if (e0 >= n_out) return;
    // (|x| bits) - 1 >= 0x7bff  <=>  x is +-0, +-inf or NaN (fp16 encoding)
    const bool odd_q = ((qw & 0x7fffu) - 1u >= 0x7bffu) | (((qw >> 16) & 0x7fffu) - 1u >= 0x7bffu);
    const bool literal = __ballot(odd_q) != 0ull;
    const uint32_t end = e0 + kPlaneWgPages < n_out ? e0 + kPlaneWgPages : n_out;
    const bool from_pool = literal || cov < 0 || end > (uint32_t)cov;
    const uint4 qb = __builtin_bit_cast(uint4, q8);
    const uint32_t qbw[4] = {qb.x, qb.y, qb.z, qb.w};
    const float8 qf = to_f32<half_t>(q8);
    float p[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) p[j] = 0.f;
    if (QUEST_LIKELY(!from_pool)) {
        const half_t* base = planes + plane_off(h, e0 + pg * kVec, c * kVec, 0, blocks);
        half8 x[kVec];
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const uint32_t s = (qbw[i >> 1] >> ((i & 1) ? 31 : 15)) & 1u;
            x[i] = ld8_stream(base + ((size_t)i * 2u + s) * kPlaneBlock);
        }
#pragma unroll
        for (int i = 0; i < kVec; ++i) {
            const float8 xf = to_f32<half_t>(x[i]);
#pragma unroll
            for (int j = 0; j < kVec; ++j) p[j] = __builtin_fmaf(qf[i], xf[j], p[j]);
        }
    } else {
        const PoolStrides ms = pool_strides(meta);
        half8 mx[kVec], mn[kVec];
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            uint32_t e = e0 + pg * kVec + j;  // clamped like estimate_tile's rows: the table and the pool cover n_cap entries
            e = e < n_cap ? e : n_cap - 1;
            uint32_t v_off;
            const half_t* row = plane_pool_row(meta, ms, e, h, v_off) + c * kVec;
            mx[j] = ld8_stream(row);
            mn[j] = ld8_stream(row + v_off);
        }
        if (!literal) {
            uint4 nm;  // per 16-bit feature: q < 0 ? 0xffff : 0
            nm.x = ((qb.x >> 15) & 0x00010001u) * 0xffffu;
            nm.y = ((qb.y >> 15) & 0x00010001u) * 0xffffu;
            nm.z = ((qb.z >> 15) & 0x00010001u) * 0xffffu;
            nm.w = ((qb.w >> 15) & 0x00010001u) * 0xffffu;
#pragma unroll
            for (int j = 0; j < kVec; ++j) {
                half8 hi, lo;
                plane_hi_lo(mx[j], mn[j], hi, lo);
                const uint4 hb = __builtin_bit_cast(uint4, hi), lb = __builtin_bit_cast(uint4, lo);
                uint4 sb;
                sb.x = (lb.x & nm.x) | (hb.x & ~nm.x);
                sb.y = (lb.y & nm.y) | (hb.y & ~nm.y);
                sb.z = (lb.z & nm.z) | (hb.z & ~nm.z);
                sb.w = (lb.w & nm.w) | (hb.w & ~nm.w);
                const float8 x = to_f32<half_t>(__builtin_bit_cast(half8, sb));
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < kVec; ++i) acc = __builtin_fmaf(qf[i], x[i], acc);
                p[j] = acc;
            }
        } else {  // literal form of decode_attn.cuh:152-156
#pragma unroll
            for (int j = 0; j < kVec; ++j) {
                const float8 a = to_f32<half_t>(mx[j]), bb = to_f32<half_t>(mn[j]);
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < kVec; ++i) acc += __builtin_fmaxf(qf[i] * a[i], qf[i] * bb[i]);
                p[j] = acc;
            }
        }
    }
    float4* dst = reinterpret_cast<float4*>(&part[c][pg * kVec]);
    dst[0] = make_float4(p[0], p[1], p[2], p[3]);
    dst[1] = make_float4(p[4], p[5], p[6], p[7]);
    __syncthreads();
    if (tid < kPlaneWgPages) {
        float pc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) pc[k] = part[k][tid];
        const float total = plane_row_tree(pc);
        const uint32_t e = e0 + tid;
        if (e < n_out) o[(size_t)h * o_stride + e] = (half_t)total;
    }
}

}  // namespace quest
