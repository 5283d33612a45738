// Page-criticality estimate: o[h][p] = fp16( sum_d max(q[h][d]*Kmax[p][h][d], q[h][d]*Kmin[p][h][d]) )
// for every KV page p except the current (last) one.
//
// Reference behaviour restated (not translated): MaxPossibleSampleWithPagedKVCacheKernel,
// kernels/include/decode/decode_attn.cuh:245-401, arithmetic compute_max_possible :137-168.
// The reference launches one block per kv head (grid (1, H), :1131) which starves a 256-CU
// part; here the (entry, head) rows are tiled: one workgroup = 8 entries x 8 heads = 64 rows
// (1024 workgroups at cfg 3), each streaming 32 KiB with all of its loads in flight at once
// (8 x 16 B per lane); LDS holds the tile's query vectors and the score transpose.
//
// Semantics: the reference's per-feature max of the two fp32 products (decode_attn.cuh:152-156), for ANY
// caller-supplied metadata -- the K slot need not be >= the V slot (the reference's own gtest fills both with
// N(0,1), test_max_possible.cu:50-51), entries may be +-inf or NaN.  See the kernel comment for how.
//
// Bit-exactness: per lane 8 consecutive features are accumulated left to right in fp32 (as the
// reference kernel does, decode_attn.cuh:152-156); the 16 lanes of a row are then reduced with the
// DPP rotation tree of row_allreduce_sum_fast (row_ror 8,4,2,1 -- one VALU op per step instead of an
// LDS-crossbar ds_bpermute round trip per step of the reference's xor butterfly, which cost 0.6 us at
// MHA and 2.3 us at GQA-4 here), lane 0's value is cast once to fp16 (RNE).  The oracle (qo_estimate)
// restates exactly this tree, so HIP == oracle bit for bit.  Bound: HBM.
#include "estimate_device.cuh"
#include "pool_check.h"

namespace quest {

// One tile per workgroup (device body: estimate_device.cuh); blocks >= tail.est_blocks run the decode append.
// The leading scalar arguments are the fields the first loads of a workgroup need (role, page-table entry, metadata
// rows, live length): scalar kernel arguments are preloaded into SGPRs at wave launch (14 dwords beside the kernarg
// pointer, build.py), a struct passed by value is not -- its remaining fields arrive by s_load while those loads fly.
#define QUEST_ESTIMATE_PARAMS                                                                                            \
    const half_t *__restrict__ q, void *a_meta_data, const int32_t *a_meta_indices, const quest_step_state_t *a_state,   \
        uint32_t n_out, uint32_t a_num_heads, uint32_t a_page_size, uint32_t a_tile_log2, uint32_t a_append_from,        \
        uint32_t a_meta_table_stride, half_t *__restrict__ o, quest_paged_kv_t meta, AppendTail tail
#define QUEST_ESTIMATE_ARGS \
    q, a_meta_data, a_meta_indices, a_state, n_out, a_num_heads, a_page_size, a_tile_log2, a_append_from, a_meta_table_stride, o, meta, tail
template <typename T, int D, int G, bool HND, int EWV>
__device__ __forceinline__ void estimate_kernel_body(QUEST_ESTIMATE_PARAMS) {
    // a_append_from: first append block (= est_blocks), 0xffffffff when no append rides in this launch
    meta.data = a_meta_data, meta.indices = a_meta_indices, meta.num_heads = a_num_heads, meta.page_size = a_page_size;
    // a_tile_log2: log2(tile heads) | row-rotated pool << 8 (the layout decides the first loads' addresses, so it travels in
    // the preloaded block, not in the struct; NHD and NHD_ROT share the HND = false instantiation)
    meta.head_dim = D, meta.layout = HND ? QUEST_LAYOUT_HND : (a_tile_log2 >> 8) ? QUEST_LAYOUT_NHD_ROT : QUEST_LAYOUT_NHD;
    a_tile_log2 &= 255u;
    tail.state = a_state, tail.tile_log2 = a_tile_log2, tail.tile_heads = 1u << a_tile_log2, tail.est_blocks = a_append_from, tail.enabled = 1u;
    tail.meta_table_stride = a_meta_table_stride;
    uint32_t seq = 0;
    if (tail.state) {  // state-driven launches may be batched: blockIdx.y = sequence (0 for a single one)
        seq = blockIdx.y;
        tail.state += seq;
        q += (size_t)seq * meta.num_heads * G * D;
        meta.indices += (size_t)seq * tail.meta_table_stride;
    }
    if (QUEST_UNLIKELY(blockIdx.x >= tail.est_blocks)) {  // the few append blocks at the end of the grid
        tail.key += (size_t)seq * meta.num_heads * D;
        tail.value += (size_t)seq * meta.num_heads * D;
        if (tail.state) {
            const quest_step_state_t st = *tail.state;
            meta.last_page_len = (uint32_t)st.meta_last_page_len;
            meta.last_page_idx = st.meta_last_page_idx;
            tail.kv.last_page_len = (uint32_t)st.kv_last_page_len;
            tail.kv.last_page_idx = st.kv_last_page_idx;
        }
        // The appended token only touches the CURRENT page's KV entry and metadata entry (index n_out),
        // which the estimate excludes (e < n_out), so the two halves of the launch share no byte.
        append_decode_body<T>(tail.kv, meta, tail.key, tail.value, (blockIdx.x - tail.est_blocks) * (EWV * kWave) + threadIdx.x);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char est_smem[];
    __shared__ uint32_t s_literal[EWV];
    const uint32_t head_tiles = meta.num_heads >> tail.tile_log2;
    estimate_tile<T, D, G, HND, EWV, 1>(q, o, meta, n_out, tail, blockIdx.x / head_tiles, blockIdx.x % head_tiles,
                                        threadIdx.x, est_smem, s_literal, seq * meta.num_heads * G);
}
// fp16 pools and bf16 pools (quest_paged_kv_t.dtype): separately named kernels over the one body
template <int D, int G, bool HND, int EWV>
__global__ __launch_bounds__(EWV* kWave, QUEST_EST_MIN_WAVES) void estimate_kernel(QUEST_ESTIMATE_PARAMS) {
    estimate_kernel_body<half_t, D, G, HND, EWV>(QUEST_ESTIMATE_ARGS);
}
template <int D, int G, bool HND, int EWV>
__global__ __launch_bounds__(EWV* kWave, QUEST_EST_MIN_WAVES) void estimate_kernel_bf16(QUEST_ESTIMATE_PARAMS) {
    estimate_kernel_body<bf16_t, D, G, HND, EWV>(QUEST_ESTIMATE_ARGS);
}

// The launch planner: which kernel instantiation and tile a shape takes.  ONE function for the launch (launch_estimate) and
// for quest_estimate_plan, which tests and the controllers ask without a GPU.
struct EstimatePlan {
    uint32_t waves;  // waves per workgroup (EWV): 2 or 4
    uint32_t hw;     // kv heads per tile: 1, 2, 4 or 8
    uint32_t ew;     // entries (pages) per tile = tile rows / hw
};

// Tile shape of a launch with `ewv`-wave workgroups: kv heads per tile (`hw`) and whether the shape can be served.
static bool estimate_tile_shape(uint32_t D, uint32_t G, uint32_t ewv, uint32_t num_heads, uint32_t rot, bool tiles, uint32_t& hw) {
    const uint32_t lpr = D / kVec, R = kWave / lpr;
    const uint32_t rows = ewv * (uint32_t)(G >= 2 ? QUEST_EST_ITER_GQA : kEstIter) * R;  // est_iter<G>()
    hw = pick_tile_heads(num_heads, G, lpr, ewv);
    // Tile maxima are one key per run of 8 consecutive columns of ONE query head, taken from 8 consecutive lanes of the
    // score store loop: a tile must be a multiple of 8 entries wide.  Narrow the tile's head range where it is not (head_dim
    // 256, two-wave workgroups), and refuse what still does not fit -- before anything is launched.
    while (tiles && hw > 1 && (rows / hw) % 8u != 0) hw >>= 1;
    if (tiles && (rows / hw) % 8u != 0) return false;
    // row-rotated pool: the heads of a tile's rows (slot ^ (entry & rot)) must be heads of the same tile
    if (rot >= hw) return false;
    return hw * G * lpr <= 2u * ewv * kWave;  // q staging capacity
}

// Workgroup width: TWO waves (32-row tiles) where the tile shape allows -- smaller workgroups start and retire in finer
// steps, measured A B A B on one box (profiles/r06_ab_estimate_tile_shapes.txt, r06_ab_estimate_waves.txt): cfg 4 A+E 9.16 ->
// 8.73 us (layer 28.9 -> 28.4), cfg 3 7.97 -> 7.83 (21.82 -> 21.72), 8 x cfg 3 two-launch form 11.20 -> 11.11, cfg 5 no
// change; 8 waves and 8 load rounds per wave are slower -- else the four-wave tile of rounds 1-5 (it stages twice the query
// vectors: GQA shapes whose group does not fit two waves' staging, row-rotated pools whose rotation needs >= 4 heads).
// -DQUEST_EST_WAVES=4 forces the four-wave form (A/B).
// QUEST_EUNSUPPORTED: a head_dim / group without an instantiation, or a shape neither width serves (the refused shapes
// listed at quest_estimate_attn_score in include/quest_hip.h).
static int estimate_plan(uint32_t D, uint32_t G, uint32_t num_heads, uint32_t layout, bool tiles, EstimatePlan& plan) {
    if (D != 64 && D != 128 && D != 256) return QUEST_EUNSUPPORTED;
    if (G != 1 && G != 2 && G != 4 && G != 8) return QUEST_EUNSUPPORTED;
    quest_paged_kv_t shape{};
    shape.num_heads = num_heads, shape.head_dim = D, shape.page_size = 1, shape.layout = layout;
    const uint32_t rot = pool_strides(shape).rot;
    for (uint32_t ewv = (kEstWaves == 2 ? 2u : 4u); ewv <= 4u; ewv += 2u) {
        uint32_t hw = 0;
        if (!estimate_tile_shape(D, G, ewv, num_heads, rot, tiles, hw)) continue;
        const uint32_t rows = ewv * (uint32_t)(G >= 2 ? QUEST_EST_ITER_GQA : kEstIter) * (kWave / (D / kVec));
        plan.waves = ewv, plan.hw = hw, plan.ew = rows / hw;
        return 0;
    }
    return QUEST_EUNSUPPORTED;
}

// argument checks on the head counts and the layout, shared by every estimate entry and quest_estimate_plan
static int estimate_check_heads(uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t layout) {
    if (layout > QUEST_LAYOUT_NHD_ROT || num_kv_heads == 0) return QUEST_EINVAL;
    if (num_qo_heads == 0 || num_qo_heads % num_kv_heads != 0) return QUEST_EINVAL;
    return 0;
}

template <int D, int G, int EWV>
static int launch_estimate_w(const void* q, void* o, uint32_t n_out, const quest_paged_kv_t& meta, AppendTail tail,
                             hipStream_t s, uint32_t n_seqs, uint32_t hw) {
    constexpr int R = kWave / (D / kVec);
    constexpr uint32_t ROWS = EWV * est_iter<G>() * R;
    const bool hnd = meta.layout == QUEST_LAYOUT_HND;
    if (!tail.state && tail.o_stride == 0) tail.o_stride = n_out;  // contiguous rows unless the caller pads them
    const uint32_t ew = ROWS / hw;
    tail.tile_heads = hw;
    tail.tile_log2 = (uint32_t)__builtin_ctz(hw);
    tail.est_blocks = ((n_out + ew - 1) / ew) * (meta.num_heads / hw);
    uint32_t blocks = tail.est_blocks;
    if (tail.enabled) blocks += (meta.num_heads * (D / kVec) + EWV * kWave - 1) / (EWV * kWave);
    if (blocks == 0) return 0;
    dim3 grid(blocks, n_seqs);
    const bool bf = meta.dtype == QUEST_DTYPE_BF16;
    const size_t lds = est_tile_lds_bytes(hw, G, D, ew, bf);
    const uint32_t append_from = tail.enabled ? tail.est_blocks : 0xffffffffu;
    if (hnd)
        hipLaunchKernelGGL((bf ? estimate_kernel_bf16<D, G, true, EWV> : estimate_kernel<D, G, true, EWV>), grid, dim3(EWV * kWave), lds, s, (const half_t*)q, meta.data,
                           meta.indices, tail.state, n_out, meta.num_heads, meta.page_size, tail.tile_log2, append_from,
                           tail.meta_table_stride, (half_t*)o, meta, tail);
    else
        hipLaunchKernelGGL((bf ? estimate_kernel_bf16<D, G, false, EWV> : estimate_kernel<D, G, false, EWV>), grid, dim3(EWV * kWave), lds, s, (const half_t*)q, meta.data,
                           meta.indices, tail.state, n_out, meta.num_heads, meta.page_size,
                           tail.tile_log2 | (meta.layout == QUEST_LAYOUT_NHD_ROT ? 1u << 8 : 0u), append_from,
                           tail.meta_table_stride, (half_t*)o, meta, tail);
    QUEST_LAUNCH_CHECK();
    return 0;
}

// the planner's choice (estimate_plan above) -> the instantiation
template <int D, int G>
static int launch_estimate(const void* q, void* o, uint32_t n_out, const quest_paged_kv_t& meta, const AppendTail& tail,
                           hipStream_t s, uint32_t n_seqs) {
    EstimatePlan plan{};
    if (int e = estimate_plan(D, G, meta.num_heads, meta.layout, tail.tile_off != 0, plan)) return e;
    if (plan.waves == 2) return launch_estimate_w<D, G, 2>(q, o, n_out, meta, tail, s, n_seqs, plan.hw);
    return launch_estimate_w<D, G, 4>(q, o, n_out, meta, tail, s, n_seqs, plan.hw);
}

template <int D>
static int dispatch_group(uint32_t G, const void* q, void* o, uint32_t n_out, const quest_paged_kv_t& meta,
                          const AppendTail& tail, hipStream_t s, uint32_t n_seqs) {
    switch (G) {
        case 1: return launch_estimate<D, 1>(q, o, n_out, meta, tail, s, n_seqs);
        case 2: return launch_estimate<D, 2>(q, o, n_out, meta, tail, s, n_seqs);
        case 4: return launch_estimate<D, 4>(q, o, n_out, meta, tail, s, n_seqs);
        case 8: return launch_estimate<D, 8>(q, o, n_out, meta, tail, s, n_seqs);
        default: return QUEST_EUNSUPPORTED;
    }
}

}  // namespace quest

using namespace quest;

static int estimate_entry(const void* q, void* o, uint32_t num_qo_heads, uint32_t n_out, const quest_paged_kv_t& metadata,
                          const AppendTail& tail, hipStream_t s, uint32_t n_seqs) {
    // element type: the metadata view's, and the KV view's of a launch that also appends must agree with it
    if (int e = tail.enabled ? check_dtype_pair(tail.kv, metadata) : check_dtype(metadata)) return e;
    if (!q || !metadata.data || !metadata.indices) return QUEST_EINVAL;
    if (metadata.page_size == 0) return QUEST_EINVAL;
    if (int e = estimate_check_heads(num_qo_heads, metadata.num_heads, metadata.layout)) return e;
    if (n_out > 0 && !o) return QUEST_EINVAL;
    if (n_out == 0 && !tail.enabled) return 0;  // nothing to score (single page)
    const uint32_t G = num_qo_heads / metadata.num_heads;
    switch (metadata.head_dim) {
        case 64: return dispatch_group<64>(G, q, o, n_out, metadata, tail, s, n_seqs);
        case 128: return dispatch_group<128>(G, q, o, n_out, metadata, tail, s, n_seqs);
        case 256: return dispatch_group<256>(G, q, o, n_out, metadata, tail, s, n_seqs);
        default: return QUEST_EUNSUPPORTED;
    }
}

extern "C" int quest_estimate_plan(uint32_t head_dim, uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t layout, int tiles,
                                   uint32_t info[3]) {
    if (!info) return QUEST_EINVAL;
    if (int e = estimate_check_heads(num_qo_heads, num_kv_heads, layout)) return e;
    EstimatePlan plan{};
    if (int e = estimate_plan(head_dim, num_qo_heads / num_kv_heads, num_kv_heads, layout, tiles != 0, plan)) return e;
    info[0] = plan.waves, info[1] = plan.hw, info[2] = plan.ew;
    return 0;
}

extern "C" int quest_estimate_attn_score(const void* q, void* o, uint32_t num_qo_heads, uint32_t n_out,
                                         quest_paged_kv_t metadata, quest_stream_t stream) {
    AppendTail tail{};
    return estimate_entry(q, o, num_qo_heads, n_out, metadata, tail, (hipStream_t)stream, 1);
}

// the append role of an estimate launch: this token's K / V into `kv` (the blocks behind the estimate's)
static AppendTail append_tail(const void* k, const void* v, const quest_paged_kv_t& kv, uint32_t o_stride) {
    AppendTail tail{};
    tail.kv = kv, tail.key = (const uint16_t*)k, tail.value = (const uint16_t*)v;
    tail.enabled = 1, tail.o_stride = o_stride;
    return tail;
}

extern "C" int quest_estimate_attn_score_batched(const void* q, void* o, uint32_t num_qo_heads, uint32_t o_stride,
                                                 uint32_t max_n_out, quest_paged_kv_t metadata,
                                                 const quest_step_state_t* state, quest_batch_t batch, quest_stream_t stream) {
    if (int e = check_dtype(metadata)) return e;
    if (!state || max_n_out == 0 || o_stride < max_n_out || batch.n_seqs == 0) return QUEST_EINVAL;
    if (batch.n_seqs > 1 && (uint64_t)batch.meta_table_stride * metadata.page_size < max_n_out) return QUEST_EINVAL;
    metadata.last_page_len = 1;  // placeholder; the kernel reads the live length from `state`
    if (int e = check_pool(metadata)) return e;
    AppendTail tail{};
    tail.state = state;
    tail.o_stride = o_stride;
    tail.meta_table_stride = batch.meta_table_stride;
    return estimate_entry(q, o, num_qo_heads, max_n_out, metadata, tail, (hipStream_t)stream, batch.n_seqs);
}

// The state-driven append + estimate: whole rows (tile_max_offset 0), or every row of `o` ([n_seqs][num_qo_heads][o_stride])
// also carries its own tile maxima at `tile_max_offset`.  The grid is sized for the shared capacity; a shorter sequence writes
// the maxima of its live runs only, and the attention launch masks the tile keys beyond them.
extern "C" int quest_append_estimate_batched(const void* k, const void* v, quest_paged_kv_t kv, const void* q, void* o,
                                             uint32_t num_qo_heads, uint32_t o_stride, uint32_t max_n_out,
                                             uint32_t tile_max_offset, quest_paged_kv_t metadata,
                                             const quest_step_state_t* state, quest_batch_t batch, quest_stream_t stream) {
    if (tile_max_offset) {
        if (tile_max_offset != ((max_n_out + 7u) & ~7u)) return QUEST_EINVAL;
        // rows 16-byte aligned: what the attention launch's 8-byte score loads and 4-byte tile-key loads are checked against
        if (((uintptr_t)o & 15u) != 0 || o_stride % 8u != 0) return QUEST_EINVAL;
    }
    // every sequence's metadata table must cover the entries the grid is sized for
    if (batch.n_seqs > 1 && (uint64_t)batch.meta_table_stride * metadata.page_size < max_n_out) return QUEST_EINVAL;
    if (int e = check_dtype_pair(kv, metadata)) return e;
    if (!k || !v || !state || max_n_out == 0 || o_stride < max_n_out || batch.n_seqs == 0) return QUEST_EINVAL;
    // the maxima live behind the scores of the same row, readable in 8-byte pieces
    if (tile_max_offset && o_stride < tile_max_offset + ((((max_n_out + 7u) / 8u) + 3u) & ~3u)) return QUEST_EINVAL;
    if (int e = check_pool_pair(kv, metadata, true, false)) return e;
    AppendTail tail = append_tail(k, v, kv, o_stride);
    tail.state = state;
    tail.meta_table_stride = batch.meta_table_stride;
    tail.tile_off = tile_max_offset;
    return estimate_entry(q, o, num_qo_heads, max_n_out, metadata, tail, (hipStream_t)stream, batch.n_seqs);
}

extern "C" int quest_append_estimate(const void* k, const void* v, quest_paged_kv_t kv, const void* q, void* o,
                                     uint32_t num_qo_heads, uint32_t n_out, uint32_t o_stride, quest_paged_kv_t metadata,
                                     quest_stream_t stream) {
    if (int e = check_dtype_pair(kv, metadata)) return e;
    if (!k || !v || (o_stride != 0 && o_stride < n_out)) return QUEST_EINVAL;
    if (int e = check_pool_pair(kv, metadata, false, false)) return e;
    AppendTail tail = append_tail(k, v, kv, o_stride);
    return estimate_entry(q, o, num_qo_heads, n_out, metadata, tail, (hipStream_t)stream, 1);
}
