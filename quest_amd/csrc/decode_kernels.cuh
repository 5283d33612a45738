// The four attention kernels of sparse_attn.hip: sparse_decode_kernel (per-head page lists, every fused top-k front end),
// layer_decode_kernel (the one-launch layer), shared_decode_kernel (one page list per KV-head group) and merge_states_kernel
// (partials of the chunks of a head -> output).  Bodies: decode_device.cuh, layer_device.cuh; launchers: sparse_attn.hip.
#pragma once
#include "append_device.cuh"
#include "decode_device.cuh"
#include "layer_device.cuh"

namespace quest {

// Workgroups go to the 8 XCDs round-robin by linear workgroup id, and each XCD has its own L2.  With GQA the query
// heads of a kv-head group select overlapping page sets (measured: 21 % of their pages are shared, scripts/gqa_overlap.py),
// so their workgroups should sit on the SAME XCD, at the same time: the host picks `xcd_period` such that grid rows
// y, y + period, y + 2 period, ... (same XCD for every chunk index) serve a run of consecutive query heads.
// (head_dim 256 keeps twice the K/V registers in flight per lane: its 8-wave instantiations are built for 2 waves per SIMD
// -- up to 256 VGPRs, one workgroup per CU -- instead of spilling 41-46 registers to scratch at the 128 of 4 waves per SIMD)
// (every kernel below exists once per element type -- fp16 under its name, bf16 as <name>_bf16 -- over one body templated
// on the type: the element type is not a template parameter of the kernels themselves)
#define QUEST_DECODE_HEAD_FORWARD a_q, a_indices, a_scores, a_state, a_n_scores, a_score_stride, a_table_stride, a_pack, a_num_qo_heads
template <typename T, int D, int S_T, int FC, int NW, int VF>
__device__ __forceinline__ void sparse_decode_kernel_body(QUEST_DECODE_HEAD_PARAMS, DecodeParams p) {
    QUEST_DECODE_HEAD_TAKE(p);
    uint32_t hq = blockIdx.y;
    const uint32_t period = p.xcd_period & 255u, slow = (p.xcd_period >> 8) & 15u, group_l2 = p.xcd_period >> 12;
    if (period > 1) {
        hq = (hq % period) * (a_num_qo_heads / period) + hq / period;
    } else if (slow) {
        // slow-class kv heads first (grid_row_order): the first quarter of the rows serves the kv heads = slow - 1 mod 4 (with
        // all query heads of their groups), the rest follow in order
        const uint32_t sr = slow - 1u, unit = hq >> group_l2, quarter = a_num_qo_heads >> (2u + group_l2);
        uint32_t hk;
        if (unit < quarter) {
            hk = 4u * unit + sr;
        } else {
            const uint32_t r = unit - quarter;
            hk = 4u * (r / 3u) + ((sr + 1u + r % 3u) & 3u);
        }
        hq = (hk << group_l2) + (hq & ((1u << group_l2) - 1u));
    }
    p.xcd_period = period;
    if constexpr (VF == 8) sparse_decode_tiles_body<T, D, NW>(p, blockIdx.x, hq, blockIdx.z, a_num_qo_heads);
    else sparse_decode_body<T, D, S_T, FC, NW, VF>(p, blockIdx.x, hq, blockIdx.z, a_num_qo_heads);
}
template <int D, int S_T, int FC, int NW, int VF = -1>
__global__ __launch_bounds__(NW* kWave, (D >= 256 && NW >= 8) ? NW / 4 : NW / 2) void sparse_decode_kernel(QUEST_DECODE_HEAD_PARAMS, DecodeParams p) {
    sparse_decode_kernel_body<half_t, D, S_T, FC, NW, VF>(QUEST_DECODE_HEAD_FORWARD, p);
}
template <int D, int S_T, int FC, int NW, int VF = -1>
__global__ __launch_bounds__(NW* kWave, (D >= 256 && NW >= 8) ? NW / 4 : NW / 2) void sparse_decode_kernel_bf16(QUEST_DECODE_HEAD_PARAMS, DecodeParams p) {
    sparse_decode_kernel_body<bf16_t, D, S_T, FC, NW, VF>(QUEST_DECODE_HEAD_FORWARD, p);
}

// One launch per layer of a batched step: the workgroup of a (sequence, query head) appends, scores its head's pages into
// LDS, selects from LDS and gathers (layer_device.cuh).  grid (1, Hq, n_seqs) -- the per-head-list kernel's, so the same
// XCD-aware row order applies.
template <int D, int FC, int NW>
__global__ __launch_bounds__(NW* kWave, NW / 2) void layer_decode_kernel(QUEST_LAYER_HEAD_PARAMS, LayerParams p) {
    layer_decode_body<D, FC, NW>(a_q, a_state, a_meta, a_meta_tables, a_kv_tables, a_n_cap, a_meta_table_stride,
                                 a_kv_table_stride, a_pack, a_num_qo_heads, p);
}

}  // namespace quest

// shared_decode_kernel / merge_states_kernel (+ their _bf16 twins): decode_kernels_typed.cuh, once per element type
#define QUEST_ELEM half_t
#define QUEST_KNAME(n) n
#include "decode_kernels_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME
#define QUEST_ELEM bf16_t
#define QUEST_KNAME(n) n##_bf16
#include "decode_kernels_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME
