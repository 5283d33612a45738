// Prefill attention over the paged KV cache: prefill_with_paged_kv_cache (bsk_ops.h:78-86, batch_prefill.cu:27-117 ->
// BatchPrefillWithPagedKVCache, kernels/include/prefill/prefill.cuh:1008-1119, kernel :688-882) -- SURVEY 8(f)-4's
// "HIP flash-prefill", the one GEMM-shaped operator of the `_kernels` surface and so the one that belongs on MFMA.
//
// What the reference computes (restated, not translated): o[i] = softmax_j(q[i] . k[j] / sqrt(D)) v[j] over the keys
// j <= kv_len - n + i (causal; every key otherwise) of the sequence whose pages `indices` lists; the new tokens' K/V are
// already in the cache (utils/__init__.py:127-170), no rotary (RotaryMode::kNone, batch_prefill.cu:102), fp16 in/out.
//
// Shape of the kernel (gfx950; head_dim 64 / 128 / 256, the set of the reference's SWITCH_HEAD_DIM_PREFILL,
// prefill.cuh:1073 -- the macro itself lives in the absent flashinfer submodule; the text below is for 128): a
// workgroup = 4 waves = 128 query rows of one query head; a wave owns 32 of them.  Per
// 64-key tile a wave computes the TRANSPOSED scores S^T = K Q^T with v_mfma_f32_32x32x16_f16 (K rows from LDS as the A
// operand, its Q rows -- loaded once, 32 registers -- as B): a 32x32 result has its column, i.e. the QUERY, on the lane
// and 16 keys in the lane's registers, so the row maximum and sum of the online softmax are per-lane loops plus one
// exchange with lane ^ 32, the rescale factor of the output is one scalar per lane, and the fp16 probabilities are,
// register for register, the B operand of O^T += V^T P^T (guide: "an accumulator tile as the next MFMA's operand") --
// no LDS round trip for P.  V^T fragments come out of the row-major V tile with ds_read_b64_tr_b16.  K and V tiles are
// staged global -> registers -> LDS one tile ahead (two LDS buffers, one barrier per tile) in the guide's dual-use
// image (8-row x 32-column subtiles, the chunks of a subtile row XOR-swizzled by the row), conflict-free for both kinds
// of read and for the staging writes (SQ_LDS_BANK_CONFLICT = 0 measured).  The tile loop is unrolled by the two buffers so that every LDS address is a
// loop-invariant register plus an immediate, and the softmax keeps a deferred reference maximum (guide T13): in the
// steady state a tile costs a wave 32 MFMAs, 48 LDS reads and ~150 vector instructions (32 v_exp, 32 v_fma, 32 v_add,
// 16 v_max3, 16 v_cvt_pk) -- the first version's 220 bought 7 %.
// Measured (profiles/r05_prefill_*): 0.74-0.98 PFLOP/s at 4K-32K tokens, 32 query heads (1.7-2.6x torch's fused
// attention on contiguous K/V, 3.0-4.3x its masked path on a chunk, 20x with GQA); MFMA pipe busy 48 % of the cycles at
// the ~1.6 GHz the chip holds under this load, LDS port active 38 %, no bank conflicts.  head_dim 64: 0.56-0.82, head_dim
// 256: 0.58-0.73 PFLOP/s (1.2-2.5x torch's).
#include "quest_common.cuh"

namespace quest {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short short4v __attribute__((__vector_size__(4 * sizeof(short))));

constexpr uint32_t kPfRows = 128;  // query rows per workgroup
constexpr int kPfKeys = 64;        // keys per tile

struct PrefillParams {
    const half_t* q;
    half_t* o;
    const half_t* kv;
    const int32_t* table;
    uint32_t n_q, kv_len, num_qo_heads, group, page_size, q_blocks, causal;
    PoolStrides st;
    float scale_log2;  // log2(e) / sqrt(D)
};

// Byte offset of 16-byte chunk `ch` of row `row` in a [rows][D halves] tile image: the guide's dual-use image (a) (T10) --
// 8-row x 32-column subtiles of 512 B, the four chunks of a subtile row XOR-swizzled by the row -- which serves the K row
// reads (ds_read_b128) and the V transposed reads (ds_read_b64_tr_b16) of the 32x32x16 operands without bank conflicts and
// with two address registers each for any D (every other term is an immediate).
template <int D>
__device__ __forceinline__ constexpr uint32_t img_off(uint32_t row, uint32_t ch) {
    return 16u * D * (row >> 3) + 512u * (ch >> 2) + 64u * (row & 7u) + 16u * ((ch & 3u) ^ ((row >> 2) & 3u));
}

#define QUEST_LDS __attribute__((address_space(3)))

__device__ __forceinline__ half8 lds_read16(uint32_t addr) {
    return *reinterpret_cast<const QUEST_LDS half8*>((uintptr_t)addr);
}
__device__ __forceinline__ void lds_write16(uint32_t addr, half8 v) {
    *reinterpret_cast<QUEST_LDS half8*>((uintptr_t)addr) = v;
}
// ds_read_b64_tr_b16: the 16 lanes of a group read a 4-row x 16-column block and each receives one COLUMN of it
__device__ __forceinline__ half4 lds_read_tr(uint32_t addr) {
    return __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                         reinterpret_cast<QUEST_LDS short4v*>((uintptr_t)addr)));
}

constexpr float kPfDefer = 8.0f;  // log2 units a row maximum may run ahead of the exponent's reference before a rescale

// Element type T (bf16_t: Q K^T and P V through v_mfma_f32_32x32x16_bf16; the softmax statistics are fp32 as for fp16 and
// the probabilities are rounded to bf16 on their way into the second MFMA).  Staging, LDS image and the transposed reads move
// 16-bit lanes and do not depend on T.
template <typename T>
__device__ __forceinline__ f32x16 mfma_32x32x16(half8 a, half8 b, f32x16 c) {
    if constexpr (kIsBf16<T>)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

}  // namespace quest

// prefill_kernel / prefill_kernel_bf16: prefill_kernel_typed.cuh, once per element type
#define QUEST_ELEM half_t
#define QUEST_KNAME(n) n
#include "prefill_kernel_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME
#define QUEST_ELEM bf16_t
#define QUEST_KNAME(n) n##_bf16
#include "prefill_kernel_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME

namespace quest {

template <int D>
static void launch_prefill(const PrefillParams& p, uint32_t grid, bool s16, bool bf, hipStream_t s) {
    if (s16)
        hipLaunchKernelGGL((bf ? prefill_kernel_bf16<D, true> : prefill_kernel<D, true>), dim3(grid), dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((bf ? prefill_kernel_bf16<D, false> : prefill_kernel<D, false>), dim3(grid), dim3(256), 0, s, p);
}

}  // namespace quest

using namespace quest;

extern "C" int quest_prefill_with_paged_kv_cache(const void* q, void* o, uint32_t n_q, uint32_t num_qo_heads,
                                                 quest_paged_kv_t kv, uint32_t n_pages_host, int causal,
                                                 quest_stream_t stream) {
    if (kv.dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;  // element type of q, o and the pool
    if (!q || !o || !kv.data || !kv.indices) return QUEST_EINVAL;
    if (n_q == 0 || num_qo_heads == 0 || kv.num_heads == 0 || kv.page_size == 0 || n_pages_host == 0) return QUEST_EINVAL;
    if (kv.layout > QUEST_LAYOUT_NHD_ROT) return QUEST_EINVAL;
    if (kv.last_page_len == 0 || kv.last_page_len > kv.page_size) return QUEST_EINVAL;
    if (num_qo_heads % kv.num_heads != 0) return QUEST_EINVAL;
    if (kv.head_dim != 64 && kv.head_dim != 128 && kv.head_dim != 256) return QUEST_EUNSUPPORTED;
    const uint64_t kv_len = (uint64_t)(n_pages_host - 1) * kv.page_size + kv.last_page_len;
    // causal rows are the LAST n_q tokens of the sequence: the reference assumes kv_len >= qo_len (test_prefill_attention.py:50)
    if (kv_len > 0x7fffffffull || (causal && n_q > kv_len)) return QUEST_EINVAL;
    PrefillParams p;
    p.q = static_cast<const half_t*>(q);
    p.o = static_cast<half_t*>(o);
    p.kv = static_cast<const half_t*>(kv.data);
    p.table = kv.indices;
    p.n_q = n_q;
    p.kv_len = (uint32_t)kv_len;
    p.num_qo_heads = num_qo_heads;
    p.group = num_qo_heads / kv.num_heads;
    p.page_size = kv.page_size;
    p.causal = causal ? 1u : 0u;
    p.st = pool_strides(kv);
    p.scale_log2 = 1.4426950408889634f / sqrtf((float)kv.head_dim);
    p.q_blocks = (n_q + kPfRows - 1) / kPfRows;
    const uint64_t grid = (uint64_t)p.q_blocks * num_qo_heads;
    if (grid > 0x7fffffffull) return QUEST_ETOOLARGE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool bf = kv.dtype == QUEST_DTYPE_BF16;
    switch (kv.head_dim) {
        case 64: launch_prefill<64>(p, (uint32_t)grid, kv.page_size == 16, bf, s); break;
        case 128: launch_prefill<128>(p, (uint32_t)grid, kv.page_size == 16, bf, s); break;
        default: launch_prefill<256>(p, (uint32_t)grid, kv.page_size == 16, bf, s); break;
    }
    QUEST_LAUNCH_CHECK();
    return 0;
}
