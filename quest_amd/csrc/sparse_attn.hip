// Sparse paged single-token decode attention over the top-K selected pages + the current page,
// and the handler that plans its split over the chip.
//
// Reference behaviour restated (not translated):
//   kernel   BatchDecodeWithPagedKVCacheKernel        kernels/include/decode/decode_attn.cuh:440-646
//   indexing protective_get_k_ptr_heads              kernels/include/decode/decode_page.cuh:325-351
//   planner  BatchDecodeWithPagedKVCacheWorkEstimation / PartitionPagedKVCacheComputeAuxiliaryInfo
//                                                      decode_attn.cuh:675-893
//   merge    VariableLengthMergeStates (flashinfer cascade.cuh, un-vendored) call :992-1001
//   handler  BatchDecodeHandler                        kernels/include/decode/decode_handler.cuh:39-244
//
// gfx950 design.  The op is a gather of (page, head) K/V tiles -- 16 rows x 256 B each for
// D=128 -- and a batch-1 vector-matrix product: HBM-bound, no MFMA.  Per head the page list
// (n_sel selected pages + the current page as one extra slot, so no pseudo-batch) is cut into
// chunks of `pages_per_chunk`; one 4-wave workgroup per (chunk, head).  A wave owns one page at a
// time: each 16 B-per-lane load instruction fetches 4 token rows (1 KiB), all 8 loads of a page
// (4 K + 4 V) are issued before any is consumed and the next page's loads are issued before the
// current page is reduced (register double buffer, no LDS round trip -- K/V are used once).
// The 16 lanes of a row reduce q.k with a DPP rotation tree (row_allreduce_sum_fast); every row keeps its own online-softmax
// state (m, d, acc[8]/lane), rows merge by shuffles, waves through LDS, chunks by a small second
// kernel that also normalises and casts (VariableLengthMergeStates' job).
#include <cstdlib>
#include <new>
#include <vector>

#include "decode_kernels.cuh"
#include "group_topk_kernels.cuh"
#include "pool_check.h"

using namespace quest;

struct quest_decode_handler {
    uint32_t layout = 0;
    uint32_t dtype = QUEST_DTYPE_F16;  // element type of the pools / q / o this handler serves (quest_decode_set_dtype)
    bool started = false;
    uint32_t n_sel = 0, num_qo_heads = 0, num_kv_heads = 0, head_dim = 0, page_size = 0;
    uint32_t pages_per_chunk = 0, n_chunks = 0;
    uint32_t forced_ppc = 0;
    float* ws = nullptr;
    size_t ws_bytes = 0;
    uint32_t ws_stride = 0;
    // Workspaces outgrown by a later plan.  Launches captured in a hipGraph hold the workspace pointer BY VALUE
    // (DecodeParams.ws), so a buffer that any launch was issued on may still be written by a replay: it is
    // retired, never freed before the handler itself is destroyed.  (A few hundred KiB each.)
    std::vector<float*> retired_ws;
    uint32_t dec_waves = 4;
    uint32_t shared_ppc = 0, shared_chunks = 0;  // plan of the group-shared kernel (grid.y = kv heads)
    uint32_t group_ppc = 0, group_chunks = 0;    // plan of the group-selection launch (grid.y = kv heads, fused front end)
    uint32_t batch = 1;                          // sequences per launch the plan / workspace are made for
    uint32_t num_cus = 256;                      // compute units of the current device (MI355X: 256)
    bool skip_merge = false;                     // measurement aid: leave the partial states unmerged
    int front_end = 0;                           // fused top-k front end: 0 = by row length, 1 / 2 = forced generation, 3 = 2 + pre-filter
    uint32_t last_launch[6] = {0, 0, 0, 0, 0, 0};  // quest_decode_last_launch_info
    void* sel_val_out = nullptr;                 // inspection aid (quest_decode_set_selection_out)
    int32_t* sel_idx_out = nullptr;
    StepAdvance armed_advance = {};              // quest_decode_arm_step_advance: rides in the next merge launch, once
};

// the armed reservation, handed to the merge launch that is about to be issued (and disarmed)
static StepAdvance take_armed_advance(quest_decode_handler* h) {
    const StepAdvance adv = h->armed_advance;
    h->armed_advance = StepAdvance{};
    return adv;
}
// a launch that turned out to have no merge launch (one workgroup per head, merge skipped): the reservation still happens
// behind this layer's kernels, as its own launch
static int flush_armed_advance(quest_decode_handler* h, hipStream_t s) {
    if (!h->armed_advance.st) return 0;
    StepAdvance a = take_armed_advance(h);
    if (a.batch.n_seqs == 1)  // (one sequence: its tables are plain arrays whose strides nobody reads; the entry checks them)
        a.batch.kv_table_stride = a.max_kv_pages, a.batch.meta_table_stride = a.max_meta_pages;
    return quest_step_state_advance_batched(a.st, a.kv_table, a.meta_table, a.page_size, a.max_kv_pages, a.max_meta_pages,
                                            a.batch, (quest_stream_t)s);
}

// Workgroups the planner aims for.  One sequence: the kernel is built for 2 workgroups (8 waves) per CU,
// so 2 x CUs workgroups (512) are one fully resident round, each wave with 16 x 1 KiB loads in flight.
// A batch: ONE workgroup per CU (256) -- measured at cfg-3 shapes for 2/4/8/16 sequences:
// every extra workgroup of a head repeats the fused selection and adds a partial record to merge, and
// with 8 x 32 (sequence, head) pairs the split disappears altogether (one workgroup per head, no merge
// launch).
static uint32_t target_workgroups(const quest_decode_handler* h) { return h->batch > 1 ? h->num_cus : 2 * h->num_cus; }
static constexpr uint32_t kMaxChunks = 1024;  // merge kernel's LDS weight table
// Pages per workgroup when the `n_slots` pages of a head are cut for `workgroups` workgroups (at most `cap` pages each,
// unless the split is forced: quest_decode_set_pages_per_chunk), in no more than kMaxChunks pieces.
static uint32_t split_pages(uint32_t n_slots, uint32_t workgroups, uint32_t forced_ppc, uint32_t cap) {
    uint32_t chunks = workgroups < 1 ? 1 : workgroups;
    if (chunks > n_slots) chunks = n_slots;
    if (chunks > kMaxChunks) chunks = kMaxChunks;
    uint32_t ppc = forced_ppc ? forced_ppc : (n_slots + chunks - 1) / chunks;
    if (!forced_ppc && ppc > cap) ppc = cap;
    if ((n_slots + ppc - 1) / ppc > kMaxChunks) ppc = (n_slots + kMaxChunks - 1) / kMaxChunks;
    return ppc;
}
extern "C" int quest_decode_arm_step_advance(quest_decode_handler_t* h, quest_step_state_t* state, const int32_t* kv_tables,
                                             const int32_t* meta_tables, uint32_t page_size, uint32_t max_kv_pages,
                                             uint32_t max_meta_pages, quest_batch_t batch) {
    if (!h) return QUEST_EINVAL;
    if (!state) {  // disarm
        h->armed_advance = StepAdvance{};
        return 0;
    }
    if (!kv_tables || !meta_tables || page_size == 0 || max_kv_pages == 0 || max_meta_pages == 0 || batch.n_seqs == 0)
        return QUEST_EINVAL;
    if (batch.n_seqs > 1 && (batch.kv_table_stride < max_kv_pages || batch.meta_table_stride < max_meta_pages)) return QUEST_EINVAL;
    if (!h->started) return QUEST_ESTATE;
    // the reservation rides in the next MERGE launch (one thread per sequence of its first workgroup); a forward whose plan
    // has no merge launch issues it as its own launch behind the attention kernel instead (correct, nothing saved)
    if (batch.n_seqs > 64) return QUEST_EUNSUPPORTED;
    h->armed_advance = StepAdvance{state, kv_tables, meta_tables, page_size, max_kv_pages, max_meta_pages, batch};
    return 0;
}

extern "C" int quest_decode_handler_create(quest_decode_handler_t** out, uint32_t layout) {
    if (!out || layout > QUEST_LAYOUT_NHD_ROT) return QUEST_EINVAL;
    quest_decode_handler* h = new (std::nothrow) quest_decode_handler();
    if (!h) return (int)hipErrorOutOfMemory;
    h->layout = layout;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        h->num_cus = (uint32_t)cus;
    else
        (void)hipGetLastError();  // no device (CPU-only import): keep the MI355X default
    h->dec_waves = quest_tuning_int("QUEST_DEC_WAVES", 4) == 8 ? 8 : 4;  // tuning knob, read per handler
    *out = h;
    return 0;
}

extern "C" void quest_decode_handler_destroy(quest_decode_handler_t* h) {
    if (!h) return;
    if (h->ws) (void)hipFree(h->ws);
    for (float* w : h->retired_ws) (void)hipFree(w);
    delete h;
}

extern "C" int quest_decode_set_pages_per_chunk(quest_decode_handler_t* h, uint32_t ppc) {
    if (!h) return QUEST_EINVAL;
    h->forced_ppc = ppc;
    return 0;
}

extern "C" int quest_decode_set_skip_merge(quest_decode_handler_t* h, int skip) {
    if (!h) return QUEST_EINVAL;
    h->skip_merge = skip != 0;
    return 0;
}

extern "C" int quest_decode_set_front_end(quest_decode_handler_t* h, int generation) {
    if (!h || generation < 0 || generation > 3) return QUEST_EINVAL;
    h->front_end = generation;
    return 0;
}

extern "C" int quest_decode_set_selection_out(quest_decode_handler_t* h, void* val_out, int32_t* idx_out) {
    if (!h) return QUEST_EINVAL;
    h->sel_val_out = val_out;
    h->sel_idx_out = idx_out;
    return 0;
}

extern "C" int quest_decode_set_dtype(quest_decode_handler_t* h, uint32_t dtype) {
    if (!h || dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    h->dtype = dtype;
    return 0;
}

extern "C" int quest_decode_set_batch(quest_decode_handler_t* h, uint32_t n_seqs) {
    if (!h || n_seqs == 0 || n_seqs > 65535u) return QUEST_EINVAL;  // grid.z limit
    h->batch = n_seqs;
    return 0;
}

extern "C" int quest_decode_begin_forward(quest_decode_handler_t* h, uint32_t n_selected_pages, uint32_t num_qo_heads,
                                          uint32_t num_kv_heads, uint32_t head_dim, uint32_t page_size,
                                          quest_stream_t stream) {
    (void)stream;
    if (!h || num_qo_heads == 0 || num_kv_heads == 0 || page_size == 0) return QUEST_EINVAL;
    if (num_qo_heads % num_kv_heads != 0) return QUEST_EINVAL;  // decode_attn.cuh:1045-1050
    if (head_dim != 64 && head_dim != 128 && head_dim != 256) return QUEST_EUNSUPPORTED;
    h->n_sel = n_selected_pages;
    h->num_qo_heads = num_qo_heads;
    h->num_kv_heads = num_kv_heads;
    h->head_dim = head_dim;
    h->page_size = page_size;
    const uint32_t n_slots = n_selected_pages + 1;
    // a batch brings its own parallelism: the workgroups are spread over the sequences (fewer, longer chunks per head ->
    // fewer partials and fewer repeats of the fused selection).  The cap keeps the fused front end usable for every plan
    // (it stages one chunk's page ids in LDS): eager callers can fall back to two launches, the state-driven / batched
    // entries cannot
    h->pages_per_chunk = split_pages(n_slots, target_workgroups(h) / (num_qo_heads * h->batch), h->forced_ppc, kFusedMaxPpc);
    h->n_chunks = (n_slots + h->pages_per_chunk - 1) / h->pages_per_chunk;
    // the group-shared kernel runs one workgroup per (chunk, KV head): plan it for the same 512 workgroups
    h->shared_ppc = split_pages(n_slots, 2 * h->num_cus / (num_kv_heads * h->batch), h->forced_ppc, n_slots);
    h->shared_chunks = (n_slots + h->shared_ppc - 1) / h->shared_ppc;
    // the group-selection launch (quest_decode_forward_group_topk): (chunk, kv head) workgroups for the same target as the
    // per-head plan, each staging its chunk's page ids in LDS like the fused front end
    h->group_ppc = split_pages(n_slots, target_workgroups(h) / (num_kv_heads * h->batch), h->forced_ppc, kFusedMaxPpc);
    h->group_chunks = (n_slots + h->group_ppc - 1) / h->group_ppc;
    h->ws_stride = (head_dim + 2 + 31) / 32 * 32;
    uint32_t max_chunks = h->n_chunks > h->shared_chunks ? h->n_chunks : h->shared_chunks;
    if (h->group_chunks > max_chunks) max_chunks = h->group_chunks;
    const size_t need = (size_t)h->batch * num_qo_heads * max_chunks * h->ws_stride * sizeof(float);
#ifdef QUEST_WALLSTAMPS
    const bool want_ws = true;  // one-chunk plans leave their per-workgroup stamps in the workspace as well
#else
    const bool want_ws = max_chunks > 1;
#endif
    if (want_ws && need > h->ws_bytes) {  // grow-only; reused across begin/end cycles
        float* bigger = nullptr;
        hipError_t e = hipMalloc((void**)&bigger, need);
        if (e != hipSuccess) return (int)e;
        if (h->ws) {
            try {
                h->retired_ws.push_back(h->ws);  // a captured graph may still reference it (see retired_ws)
            } catch (...) {
                (void)hipFree(bigger);
                return (int)hipErrorOutOfMemory;
            }
        }
        h->ws = bigger;
        h->ws_bytes = need;
    }
    h->started = true;
    return 0;
}

extern "C" int quest_decode_end_forward(quest_decode_handler_t* h) {
    if (!h) return QUEST_EINVAL;
    h->started = false;  // workspace is kept for the next begin_forward (freed in destroy)
    return 0;
}

extern "C" int quest_decode_plan_info(const quest_decode_handler_t* h, uint32_t* pages_per_chunk,
                                      uint32_t* chunks_per_head) {
    if (!h || !h->started) return QUEST_ESTATE;
    if (pages_per_chunk) *pages_per_chunk = h->pages_per_chunk;
    if (chunks_per_head) *chunks_per_head = h->n_chunks;
    return 0;
}

extern "C" int quest_decode_debug_workspace(const quest_decode_handler_t* h, void** ptr, uint64_t* bytes, uint32_t* record_floats) {
    if (!h || !ptr || !bytes) return QUEST_EINVAL;
    *ptr = h->ws;
    *bytes = h->ws_bytes;
    if (record_floats) *record_floats = h->ws_stride;
    return 0;
}

extern "C" int quest_decode_last_launch_info(const quest_decode_handler_t* h, uint32_t info[6]) {
    if (!h || !info) return QUEST_EINVAL;
    for (int i = 0; i < 6; ++i) info[i] = h->last_launch[i];
    return 0;
}

// One attention launch as the entries hand it to decode_entry / shared_entry / the one-launch layer: every operand by name.
struct DecodeRequest {
    const void* q = nullptr;
    void* o = nullptr;
    quest_paged_kv_t kv = {};
    uint32_t num_qo_heads = 0;
    float* lse = nullptr;
    const void* scores = nullptr;  // fused top-k front end: the score rows (else the page ids come from kv.indices)
    uint32_t n_scores = 0, score_stride = 0, tile_off = 0;
    void* topk_val_out = nullptr;
    int32_t* topk_idx_out = nullptr;
    const quest_step_state_t* state = nullptr;
    quest_batch_t batch = {1, 0, 0, 0};
    const void *app_k = nullptr, *app_v = nullptr;  // optional decode append riding in the launch, with its metadata pool
    quest_paged_kv_t metadata = {};
};

static DecodeRequest attention_request(const void* q, void* o, const quest_paged_kv_t& kv, uint32_t num_qo_heads, float* lse) {
    DecodeRequest r;
    r.q = q, r.o = o, r.kv = kv, r.num_qo_heads = num_qo_heads, r.lse = lse;
    return r;
}

// ---- the request checks
enum class Route { kHeadLists, kSharedList, kLayer };  // which page lists the launch reads: per query head / one / the tables

// A request against the handler's plan, in the order the entries' return codes promise: no plan or a plan for fewer
// sequences (ESTATE) before the operands, the operands before the geometry.  Puts the placeholders of a state-driven
// launch into the pools.
static int check_request(const quest_decode_handler* h, DecodeRequest& r, Route route) {
    quest_paged_kv_t& kv = r.kv;
    // element type first: an unknown value, a view that disagrees with the handler's type (quest_decode_set_dtype) or with the
    // metadata view travelling in the same call
    if (kv.dtype > QUEST_DTYPE_BF16 || (h && kv.dtype != h->dtype)) return QUEST_EINVAL;
    if ((r.app_k || route == Route::kLayer) && r.metadata.dtype != kv.dtype) return QUEST_EINVAL;
    if (!h || r.batch.n_seqs == 0) return QUEST_EINVAL;
    if (r.state) kv.last_page_len = 1;  // placeholder; the kernel reads the real one from `state`
    if (!h->started) return QUEST_ESTATE;
    if (r.batch.n_seqs > h->batch) return QUEST_ESTATE;  // workspace / plan were made for fewer sequences
    if (!r.q || !r.o || !kv.data) return QUEST_EINVAL;
    if (route == Route::kLayer) {
        // the append and the estimate address the metadata pool with the KV pool's strides: same geometry required
        if (int e = check_pool_pair(kv, r.metadata, true, true)) return e;
    } else if (r.scores) {
        if (!kv.indices || h->n_sel == 0 || h->n_sel > r.n_scores) return QUEST_EINVAL;
        if (r.n_scores > QUEST_TOPK_MAX_ROW) return QUEST_ETOOLARGE;
        if (h->pages_per_chunk > (uint32_t)kFusedMaxPpc) return QUEST_EUNSUPPORTED;
        // (rows beyond 4096 columns need the second-generation front end, i.e. aligned score rows: choose_front_end)
    } else if (h->n_sel > 0 && (!kv.indices || (route == Route::kHeadLists && !r.state && kv.page_budget < h->n_sel))) {
        return QUEST_EINVAL;  // (state-driven: one shared list, row stride kv.page_budget == 0)
    }
    if (kv.layout != h->layout || kv.head_dim != h->head_dim || kv.page_size != h->page_size ||
        kv.num_heads != h->num_kv_heads || r.num_qo_heads != h->num_qo_heads)
        return QUEST_EINVAL;
    if (kv.last_page_len == 0 || kv.last_page_len > kv.page_size) return QUEST_EINVAL;
    return 0;
}

static float softmax_scale_log2(uint32_t head_dim) { return (float)(1.4426950408889634 / sqrt((double)head_dim)); }

// What every attention launch passes to its kernel, whichever split of the plan (pages per chunk, chunks) it runs.
static DecodeParams base_params(const quest_decode_handler* h, const DecodeRequest& r, uint32_t pages_per_chunk, uint32_t n_chunks) {
    const quest_paged_kv_t& kv = r.kv;
    DecodeParams p{};
    p.q = (const half_t*)r.q, p.o = (half_t*)r.o, p.lse = r.lse;
    p.kv = (const half_t*)kv.data, p.indices = kv.indices, p.st = pool_strides(kv);
    p.last_page_len = kv.last_page_len, p.last_page_idx = kv.last_page_idx, p.page_size = kv.page_size;
    p.group = r.num_qo_heads / kv.num_heads, p.scale_log2 = softmax_scale_log2(kv.head_dim);
    p.n_sel = h->n_sel, p.pages_per_chunk = pages_per_chunk, p.n_chunks = n_chunks;
    p.ws = h->ws, p.ws_stride = h->ws_stride, p.state = r.state, p.table_stride = r.batch.kv_table_stride;
    return p;
}

// ---- the front-end choice
// Everything the choice depends on, as values: no handler, no HIP.
struct FrontEndInputs {
    uintptr_t scores = 0, table = 0;   // addresses of the score rows (0: no fused front end) and of the page table(s)
    uint32_t n_scores = 0, score_stride = 0, table_stride = 0, n_seqs = 1, page_size = 0, n_sel = 0, tile_off = 0;
    uint32_t waves = 4;                // the handler's workgroup size (QUEST_DEC_WAVES)
    int forced = 0;                    // quest_decode_set_front_end (0: by row length)
};
// fc: keys per thread of the fused front end's instantiation (0 = page ids come from an index tensor), waves = workgroup
// size; the rest are the DecodeParams fields of the same names.
struct FrontEnd {
    int fc = 0;
    uint32_t waves = 4, vec_front = 0, cpt = 0, stage_ids = 0, ids_lds_offset = 0, row_lead = 0, fe2_prefilter = 0, table_vec = 0;
};

static int choose_front_end(const FrontEndInputs& in, FrontEnd& fe) {
    const uint32_t n_scores = in.n_scores, stride = in.score_stride;
    const bool fused = in.scores != 0;
    fe = FrontEnd{};
    fe.waves = in.waves;
    fe.stage_ids = n_scores <= 4096 ? 1u : 0u;  // keys always staged (2 B each); ids (4 B each) up to 16 KiB
    fe.ids_lds_offset = (uint32_t)((((size_t)n_scores * 2) + 15) & ~(size_t)15);
    int forced = 0;
    bool aligned = false, table_aligned = false;  // score rows / page tables that vector loads can read
    if (fused) {
        // second-generation front end (topk_bitmap.cuh): 8-byte loads of 4 scores straight from the row -> the rows
        // must be 8-byte aligned and readable up to the next multiple of 4 columns (the row stride covers it)
        // Measured on MI355X (state-driven launches, us per launch gen 1 -> gen 2): cfg 3 (2047 columns, 16 workgroups
        // per head) 12.7 -> 13.6, 8 x cfg 3 batched 47.9 -> 50.1, cfg 4 (8191 columns) 28.6 -> 21.9.  The second
        // generation has fewer barriers but its per-wave scans are redundant work on an issue-bound CU (4 waves per
        // SIMD), which costs more than it saves on short rows -> gen 2 from 4097 columns up (gen 1 spills there).
        // quest_decode_set_front_end / QUEST_FRONT_END=1 / 2 force a generation where it is applicable (tuning, tests).
        static const int env_forced = quest_tuning_int("QUEST_FRONT_END", 0);
        forced = in.forced ? in.forced : env_forced;
        aligned = (in.scores & 7u) == 0 && stride % 4u == 0 && stride >= ((n_scores + 3u) & ~3u);
        table_aligned = (in.table & 15u) == 0 && (in.n_seqs == 1 || in.table_stride % 4u == 0);
        fe.table_vec = table_aligned ? 1u : 0u;
        int gen = 1;
        bool lead_rows = false;
        if (aligned) {
            if (forced == 2 || forced == 3 || (forced == 0 && n_scores > 4096u)) gen = 2;
        } else if (n_scores > 4096u && n_scores + 3u <= QUEST_TOPK_MAX_ROW && forced != 1) {  // (the bitmaps cover positions)
            // the reference's own score layout beyond 4096 pages (contiguous [Hq][pages - 1] rows: 2-byte aligned,
            // quest/utils/__init__.py:194): the second generation on the aligned stream BELOW each row (row_lead) -- one
            // fused launch where rounds 2-4 needed topk_filtering + forward
            gen = 2;
            lead_rows = true;
        }
        if (gen != 1) {
            fe.vec_front = 2;
            fe.ids_lds_offset = 0;  // no key staging
            fe.row_lead = lead_rows ? 1u : 0u;
            // page ids are staged with 16-byte loads: the table(s) must be 16-byte aligned (and columns = positions)
            if (!table_aligned || lead_rows) fe.stage_ids = 0;
            // (gen 2 stages ids only in the instantiations with <= 16 keys per thread: rows <= 4096 columns)
            // pre-filter of the histogram: pays where a thread holds many keys (rows beyond 4096 columns); QUEST_FE2_PREFILTER=0
            // turns it off, =2 turns it on for every second-generation launch (tuning, tests)
            static const int pre_env = quest_tuning_int("QUEST_FE2_PREFILTER", 1);
            fe.fe2_prefilter = forced == 3 || pre_env == 2 || (pre_env == 1 && forced != 2 && n_scores > 4096u) ? 1u : 0u;
        } else if (aligned && table_aligned && fe.stage_ids && forced != 1) {
            fe.vec_front = 1;  // generation 1 with its staging arrays filled by the granule loads (8 / 16 bytes per lane)
        }
    }
    // rows beyond 4096 columns are served by the second-generation front end only (the first one spills there):
    // state-driven callers own the score scratch and give it an 8-byte aligned row stride (a multiple of 4 columns)
    if (fused && !fe.vec_front && n_scores > 4096u && !in.tile_off) return QUEST_EUNSUPPORTED;
    if (in.tile_off) {  // tiles front end (sparse_decode_tiles_body): the rows carry their tile maxima behind the scores
        const uint32_t tiles_cap = (n_scores + 7u) / 8u;
        if (!fused || in.tile_off != ((n_scores + 7u) & ~7u) || (in.scores & 15u) != 0 || stride % 8u != 0 ||
            stride < in.tile_off + ((tiles_cap + 3u) & ~3u))
            return QUEST_EINVAL;
        if (in.page_size != 16 || in.n_sel > 256u || tiles_cap > 4u * 512u) return QUEST_EUNSUPPORTED;
        fe.vec_front = 8;
        fe.stage_ids = 0;
        fe.ids_lds_offset = 0;
    }
    if (fused && fe.vec_front == 8u) {
        fe.waves = 8;
        fe.fc = 8;
        fe.cpt = (n_scores + 7u) / 8u <= 2u * 512u ? 2u : 4u;  // tile keys per thread
    } else if (fused) {
        // the selection is VALU-issue bound (~1000 instructions per wave at 8 keys per thread), so rows
        // beyond 1024 pages get 8 waves (<= 4 keys per thread up to 2048 pages, <= 8 up to 4096); the
        // attention part runs the same with 4 or 8 waves.  Measured at cfg 3: 15.2 vs 15.8 us.
        if (in.page_size == 16 && n_scores > 4u * 4u * kWave) fe.waves = 8;
        const uint32_t nt = (in.page_size == 16 ? fe.waves : 4u) * kWave;
        const uint32_t per_thread = (n_scores + (fe.row_lead ? 3u : 0u) + nt - 1) / nt;  // (+ the skipped leading columns)
        // (24: rows of 8193-12288 columns at 512 threads -- cfg 4's capacity of ~8320 pages needs 17 keys per thread; the
        // 32-key instantiation carries two more dead load / histogram / bitmap rounds in every unrolled phase.
        // QUEST_FC24=0 takes the 32-key instantiation instead: A/B)
        static const bool fc24 = quest_tuning_int("QUEST_FC24", 1) != 0;
        fe.fc = per_thread <= 8 ? 8 : per_thread <= 16 ? 16 : (per_thread <= 24 && fc24) ? 24 : per_thread <= 32 ? 32 : 64;
        // ownership chunk: a multiple of 4 columns when the register capacity allows, so a thread's keys are one
        // 8/16-byte LDS read (topk_load_keys)
        const uint32_t r4 = (per_thread + 3) / 4 * 4;
        fe.cpt = r4 <= (uint32_t)fe.fc ? r4 : per_thread;
        // rows of <= 8 columns per thread with vector-loadable chunks: each thread takes its own columns and page ids
        // straight into registers (no staging arrays).  Measured (us per launch, staged -> direct): cfg 3 12.79 ->
        // 12.38; 8 sequences batched 48.6 -> 48.85, cfg 5 51.2 -> 51.2 -> single-sequence launches only.
        // QUEST_FE1_DIRECT=0 keeps the staged variant, =2 takes the direct one for batches too (tuning, tests).
        static const int direct_env = quest_tuning_int("QUEST_FE1_DIRECT", 1);
        const bool direct_ok = direct_env == 2 || (direct_env == 1 && in.n_seqs == 1);
        const bool direct_possible = aligned && fe.vec_front != 2 && forced != 1 && fe.fc == 8 &&
            (fe.cpt == 4 || (fe.cpt == 8 && (in.scores & 15u) == 0 && stride % 8u == 0 && stride >= ((n_scores + 7u) & ~7u)));
        if (direct_possible && direct_ok && fe.vec_front == 1) fe.vec_front = 3;
        // (Round 4 built two more front ends and measured both slower: column-range ownership -- a workgroup gathers the
        // selected pages of ITS range of columns, no rank scan, no page-list hand-off: cfg 3 13.27 vs 12.07 us, cfg 4 20.34
        // vs 19.54, the per-CU page imbalance costs more than the earlier page list returns -- and a third generation for
        // long rows, pre-filter -> compact -> short-row select: 22.4 vs 19.6 us at cfg 4.  Removed from the tree in round 5,
        // DESIGN.md 3.5; history: git log -S sparse_decode_colrange_body, -S fe3_select.)
    }
    return 0;
}

// ---- the grid row order
// DecodeParams::xcd_period of a launch with `chunks_per_head` workgroups per query head.  slow_first_pool: the KV pool of
// a single-sequence sparse_decode_kernel launch, the one kernel that honours the slow-class-first packing (else NULL).
static uint32_t grid_row_order(uint32_t chunks_per_head, uint32_t num_qo_heads, uint32_t group, const quest_paged_kv_t* slow_first_pool) {
    // XCD-aware row order for GQA (see sparse_decode_kernel); QUEST_XCD_GROUP=0 keeps the plain order (tuning)
    static const bool xcd_group = quest_tuning_int("QUEST_XCD_GROUP", 1) != 0;
    uint32_t gcd = 8, c = chunks_per_head % 8u;
    while (c) { const uint32_t t = gcd % c; gcd = c; c = t; }
    const uint32_t period = 8u / gcd;
    uint32_t order = (xcd_group && group > 1 && period > 1 && num_qo_heads % period == 0 &&
                      (num_qo_heads / period) % group == 0) ? period : 1u;
    // Dispatch order by address class (round 5, scripts/probe/addr_class_probe.hip): on the NHD pool a head's K/V rows
    // are 256-byte pieces at one offset inside every 1 KiB, and pieces whose address bits 8-9 are 01 are served ~20 %
    // slower than the others under mixed traffic -- heads 1, 5, 9, ... of a 128-wide MHA pool.  A single sequence's
    // launch is two workgroups per CU, dispatched rows-first: the first 16 rows' workgroups get ahead of the second
    // 16 (they start their gather ~1 us earlier and finish ~2 us earlier), so the slow heads go FIRST, where they
    // have that slack, instead of deciding the end of the launch from the second half.
    // Measured at cfg 3, same box, us per launch: 12.04 -> 11.82 (profiles/r05_ab_slow_class_heads_first.txt);
    // QUEST_SLOW_FIRST=0 keeps the plain order (A/B).  Same work per head, same bits.
    static const int slow_env = quest_tuning_int("QUEST_SLOW_FIRST", 1);
    if (const quest_paged_kv_t* kv = slow_first_pool)
        if (slow_env && order == 1 && (group & (group - 1u)) == 0 && kv->layout == QUEST_LAYOUT_NHD && kv->head_dim == 128 &&
            kv->num_heads % 4u == 0) {
            const uint32_t c0 = (uint32_t)(((uintptr_t)kv->data >> 8) & 3u);  // class of kv head 0
            order |= (1u + ((1u - c0) & 3u)) << 8 | (uint32_t)__builtin_ctz(group) << 12;
        }
    return order;
}

// ---- the launchers
// Behind every attention launch: the merge of a head's partials (it carries the armed step advance) or, for a plan
// without a merge launch, the advance as a launch of its own.
template <int D>
static int merge_and_advance(quest_decode_handler* h, const DecodeParams& p, uint32_t heads_x_seqs, float* lse, hipStream_t s,
                             bool bf16) {
    if (p.n_chunks > 1 && !h->skip_merge) {  // o / lse / partials of a batch are contiguous over (sequence, head): one grid
        hipLaunchKernelGGL((bf16 ? merge_states_kernel_bf16<D> : merge_states_kernel<D>), dim3(heads_x_seqs), dim3(D * kMergeGroups), 0, s, (const float*)p.ws, p.o,
                           lse, p.n_chunks, p.ws_stride, take_armed_advance(h));
        QUEST_LAUNCH_CHECK();
    }
    return flush_armed_advance(h, s);
}

template <int D, int FC>
static int launch_decode_fc(quest_decode_handler* h, const DecodeParams& p, uint32_t num_qo_heads, uint32_t waves,
                            hipStream_t s, uint32_t n_seqs, bool bf16) {  // bf16: the *_bf16 kernels (the handler's element type)
    dim3 grid(h->n_chunks, num_qo_heads, n_seqs);
    const size_t lds = FC > 0 ? (size_t)p.ids_lds_offset + (p.stage_ids ? (size_t)((p.n_scores + 4u) & ~3u) * 4 : 0) : 0;  // the table has n_scores + 1 entries, staged in granules of 4
    // what this launch is (quest_decode_last_launch_info): keys per thread, waves, front-end variant, one-variant
    // instantiation or the generic kernel, workgroups per head, sequences
    uint32_t* info = h->last_launch;
    info[0] = (uint32_t)FC, info[1] = waves, info[2] = FC > 0 ? p.vec_front : 0u, info[3] = 0u, info[4] = h->n_chunks, info[5] = n_seqs;
    // The common (keys per thread, front-end variant) pairs of 8-wave page-16 launches as their own compact
    // instantiations -- the generic kernel carries every front-end variant (27 KiB of code in round 3; the one-variant
    // kernels are 10-14 KiB) and measured 0.57 us per launch slower at the headline shape:
    //   FC 8,  variant 3: single-sequence rows <= 4096 pages, keys and page ids straight into registers (cfg 3)
    //   FC 8,  variant 1: the same rows in batched launches, staging arrays fed by vector loads (cfg 5)
    //   FC 8,  variant 8: tiles front end, rows that carry their tile maxima (cfg 4)
    //   FC 16 / 24 / 32, variant 2: second-generation front end of long rows without tile maxima
    // QUEST_FE_SPECIALIZE=0 launches the generic kernel instead (A/B).
    static const bool specialize = quest_tuning_int("QUEST_FE_SPECIALIZE", 1) != 0;
    float* const lse = QUEST_LSE_ENABLED ? p.lse : nullptr;
    if (p.vec_front == 8u) {  // tiles front end (choose_front_end: page size 16, 8 waves)
        if constexpr (FC == 8) {
            info[3] = 1u;
            hipLaunchKernelGGL((bf16 ? sparse_decode_kernel_bf16<D, 16, 8, 8, 8> : sparse_decode_kernel<D, 16, 8, 8, 8>), grid, dim3(8 * kWave), 0, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p);
            QUEST_LAUNCH_CHECK();
            return merge_and_advance<D>(h, p, num_qo_heads * n_seqs, lse, s, bf16);
        } else {
            return QUEST_EUNSUPPORTED;
        }
    }
    if (specialize && p.page_size == 16 && waves == 8) {
        constexpr int VFA = FC == 8 ? 3 : 2, VFB = FC == 8 ? 1 : 2;
        if constexpr (FC == 8 || FC == 16 || FC == 24 || FC == 32) {
            info[3] = 1u;
            if (p.vec_front == (uint32_t)VFA) {
                hipLaunchKernelGGL((bf16 ? sparse_decode_kernel_bf16<D, 16, FC, 8, VFA> : sparse_decode_kernel<D, 16, FC, 8, VFA>), grid, dim3(8 * kWave), lds, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p);
                QUEST_LAUNCH_CHECK();
                return merge_and_advance<D>(h, p, num_qo_heads * n_seqs, lse, s, bf16);
            }
            if (VFB != VFA && p.vec_front == (uint32_t)VFB) {
                hipLaunchKernelGGL((bf16 ? sparse_decode_kernel_bf16<D, 16, FC, 8, VFB> : sparse_decode_kernel<D, 16, FC, 8, VFB>), grid, dim3(8 * kWave), lds, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p);
                QUEST_LAUNCH_CHECK();
                return merge_and_advance<D>(h, p, num_qo_heads * n_seqs, lse, s, bf16);
            }
            info[3] = 0u;
        }
    }
    if (p.page_size == 16 && waves == 8)
        hipLaunchKernelGGL((bf16 ? sparse_decode_kernel_bf16<D, 16, FC, 8> : sparse_decode_kernel<D, 16, FC, 8>), grid, dim3(8 * kWave), lds, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p);
    else if (p.page_size == 16)
        hipLaunchKernelGGL((bf16 ? sparse_decode_kernel_bf16<D, 16, FC, 4> : sparse_decode_kernel<D, 16, FC, 4>), grid, dim3(4 * kWave), lds, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p);
    else
        hipLaunchKernelGGL((bf16 ? sparse_decode_kernel_bf16<D, 0, FC, 4> : sparse_decode_kernel<D, 0, FC, 4>), grid, dim3(4 * kWave), lds, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p);
    QUEST_LAUNCH_CHECK();
    return merge_and_advance<D>(h, p, num_qo_heads * n_seqs, lse, s, bf16);
}

// fc: fused top-k front end variant (0 = page ids come from an index tensor)
template <int D>
static int launch_decode(quest_decode_handler* h, const DecodeParams& p, uint32_t num_qo_heads, int fc,
                         uint32_t waves, hipStream_t s, uint32_t n_seqs, bool bf16) {
    switch (fc) {
        case 0: return launch_decode_fc<D, 0>(h, p, num_qo_heads, waves, s, n_seqs, bf16);
        case 8: return launch_decode_fc<D, 8>(h, p, num_qo_heads, waves, s, n_seqs, bf16);
        case 16: return launch_decode_fc<D, 16>(h, p, num_qo_heads, waves, s, n_seqs, bf16);
        case 24: return launch_decode_fc<D, 24>(h, p, num_qo_heads, waves, s, n_seqs, bf16);
        case 32: return launch_decode_fc<D, 32>(h, p, num_qo_heads, waves, s, n_seqs, bf16);
        case 64: return launch_decode_fc<D, 64>(h, p, num_qo_heads, waves, s, n_seqs, bf16);
        default: return QUEST_EUNSUPPORTED;
    }
}

// A per-head-list decode launch: checks, kernel parameters, front end, row order, launch.
static int decode_entry(quest_decode_handler* h, DecodeRequest r, hipStream_t s) {
    if (int e = check_request(h, r, Route::kHeadLists)) return e;
    const quest_paged_kv_t& kv = r.kv;
    const bool fused = r.scores != nullptr;
    DecodeParams p = base_params(h, r, h->pages_per_chunk, h->n_chunks);
    p.idx_stride = fused ? 0 : kv.page_budget;
    p.scores = (const uint16_t*)r.scores;
    p.n_scores = r.n_scores;
    p.sel_val_out = (uint16_t*)r.topk_val_out;
    p.sel_idx_out = r.topk_idx_out;
    if (fused && r.state && !r.topk_idx_out) {  // state-driven launches have no output arguments: handler-level aid
        p.sel_val_out = (uint16_t*)h->sel_val_out;
        p.sel_idx_out = h->sel_idx_out;
    }
    p.sel_stride = h->n_sel;
    p.score_stride = r.score_stride ? r.score_stride : r.n_scores;
    FrontEndInputs in;
    in.scores = (uintptr_t)r.scores, in.table = (uintptr_t)kv.indices;
    in.n_scores = r.n_scores, in.score_stride = p.score_stride, in.table_stride = r.batch.kv_table_stride;
    in.n_seqs = r.batch.n_seqs, in.page_size = kv.page_size, in.n_sel = h->n_sel, in.tile_off = r.tile_off;
    in.waves = h->dec_waves, in.forced = h->front_end;
    FrontEnd fe;
    if (int e = choose_front_end(in, fe)) return e;
    p.vec_front = fe.vec_front, p.cpt = fe.cpt, p.stage_ids = fe.stage_ids, p.ids_lds_offset = fe.ids_lds_offset;
    p.row_lead = fe.row_lead, p.fe2_prefilter = fe.fe2_prefilter, p.table_vec = fe.table_vec;
    p.budgets = r.state ? r.batch.page_budgets : nullptr;
    p.xcd_period = grid_row_order(h->n_chunks, r.num_qo_heads, p.group, r.batch.n_seqs == 1 ? &kv : nullptr);
    const bool bf16 = h->dtype == QUEST_DTYPE_BF16;  // (check_request: the view's type is the handler's)
    switch (kv.head_dim) {
        case 64: return launch_decode<64>(h, p, r.num_qo_heads, fe.fc, fe.waves, s, r.batch.n_seqs, bf16);
        case 128: return launch_decode<128>(h, p, r.num_qo_heads, fe.fc, fe.waves, s, r.batch.n_seqs, bf16);
        case 256: return launch_decode<256>(h, p, r.num_qo_heads, fe.fc, fe.waves, s, r.batch.n_seqs, bf16);
        default: return QUEST_EUNSUPPORTED;
    }
}

template <int D>
static int launch_shared(quest_decode_handler* h, DecodeParams p, uint32_t num_qo_heads, uint32_t gs, hipStream_t s,
                         uint32_t n_seqs) {
    const bool bf16 = h->dtype == QUEST_DTYPE_BF16;  // (check_request: the view's type is the handler's)
    // (8-wave workgroups for group sizes 1 / 2 -- 16 waves per CU instead of 8, each with one page in flight -- measured
    // slower in round 4: cfg 2 18.4 vs 17.8 us per layer, the 32K dense kernel 94.4 vs 92.4 us)
    static const char* order_env = quest_tuning_env("QUEST_SHARED_HEADS_FIRST");  // unset: by layout
    const bool nhd = p.st.head < p.st.entry;
    const bool heads_first = order_env ? atoi(order_env) != 0 : nhd && num_qo_heads / gs > 1;
    p.xcd_period = heads_first ? 1u : 0u;
    dim3 grid(p.n_chunks, num_qo_heads / gs, n_seqs), block(4 * kWave);
    if (heads_first) grid = dim3(num_qo_heads / gs, p.n_chunks, n_seqs);
#define QUEST_SHARED_CASE(GS)                                                                                                  \
    case GS:                                                                                                                   \
        if (p.app_k)                                                                                                           \
            hipLaunchKernelGGL((bf16 ? shared_decode_kernel_bf16<D, GS, 4, true> : shared_decode_kernel<D, GS, 4, true>), grid, block, 0, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p); \
        else                                                                                                                   \
            hipLaunchKernelGGL((bf16 ? shared_decode_kernel_bf16<D, GS, 4, false> : shared_decode_kernel<D, GS, 4, false>), grid, block, 0, s, QUEST_DECODE_HEAD_ARGS(p, num_qo_heads), p); \
        break;
    switch (gs) {
        QUEST_SHARED_CASE(1)
        QUEST_SHARED_CASE(2)
        QUEST_SHARED_CASE(4)
        QUEST_SHARED_CASE(8)
        default: return QUEST_EUNSUPPORTED;
    }
#undef QUEST_SHARED_CASE
    QUEST_LAUNCH_CHECK();
    return merge_and_advance<D>(h, p, num_qo_heads * n_seqs, p.lse, s, bf16);
}

static int shared_entry(quest_decode_handler* h, DecodeRequest r, hipStream_t s) {
    if (int e = check_request(h, r, Route::kSharedList)) return e;
    const quest_paged_kv_t& kv = r.kv;
    if (kv.page_size != 16 || (kv.head_dim != 64 && kv.head_dim != 128)) {
        // outside the group-shared kernel's set.  Eager callers get EUNSUPPORTED and pass the per-head index
        // tensor to quest_decode_forward; a state-driven launch has no such tensor, so it runs the per-head-list
        // kernel with every head reading the ONE page table (row stride 0) and the live length from `state`.
        if (!r.state || r.app_k) return QUEST_EUNSUPPORTED;  // (with an append: the caller issues it as its own launch)
        r.kv.page_budget = 0;
        return decode_entry(h, r, s);
    }
    DecodeParams p = base_params(h, r, h->shared_ppc, h->shared_chunks);
    if (r.app_k) {
        const quest_paged_kv_t& m = r.metadata;
        if (!r.app_v || !m.data) return QUEST_EINVAL;
        // the append addresses the metadata pool with the KV pool's strides: same geometry required (it is: the
        // controller builds both from one KvCache class with the same page size, heads, dim and layout)
        if (!same_pool_geometry(m, kv)) return QUEST_EINVAL;
        if (!r.state && (m.last_page_len == 0 || m.last_page_len > m.page_size)) return QUEST_EINVAL;
        p.app_k = (const half_t*)r.app_k, p.app_v = (const half_t*)r.app_v, p.app_meta = (half_t*)m.data;
        p.meta_last_page_len = m.last_page_len, p.meta_last_page_idx = m.last_page_idx;
    }
    return kv.head_dim == 64 ? launch_shared<64>(h, p, r.num_qo_heads, p.group, s, r.batch.n_seqs)
                             : launch_shared<128>(h, p, r.num_qo_heads, p.group, s, r.batch.n_seqs);
}

// ---- the entries: fill the request, call

extern "C" int quest_decode_forward(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t kv,
                                    uint32_t num_qo_heads, float* lse, quest_stream_t stream) {
    return decode_entry(h, attention_request(q, o, kv, num_qo_heads, lse), (hipStream_t)stream);
}

extern "C" int quest_decode_forward_shared(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t kv,
                                           uint32_t num_qo_heads, float* lse, quest_stream_t stream) {
    return shared_entry(h, attention_request(q, o, kv, num_qo_heads, lse), (hipStream_t)stream);
}

extern "C" int quest_decode_forward_shared_batched(quest_decode_handler_t* h, const void* q, void* o,
                                                   quest_paged_kv_t kv, uint32_t num_qo_heads,
                                                   const quest_step_state_t* state, quest_batch_t batch, float* lse,
                                                   quest_stream_t stream) {
    if (!state) return QUEST_EINVAL;
    if (h && batch.n_seqs > 1 && batch.kv_table_stride < h->n_sel + 1) return QUEST_EINVAL;
    DecodeRequest r = attention_request(q, o, kv, num_qo_heads, lse);
    r.state = state, r.batch = batch;
    return shared_entry(h, r, (hipStream_t)stream);
}

extern "C" int quest_decode_append_forward_shared_batched(quest_decode_handler_t* h, const void* k, const void* v,
                                                          quest_paged_kv_t metadata, const void* q, void* o,
                                                          quest_paged_kv_t kv, uint32_t num_qo_heads,
                                                          const quest_step_state_t* state, quest_batch_t batch, float* lse,
                                                          quest_stream_t stream) {
    if (!state || !k || !v) return QUEST_EINVAL;
    if (h && batch.n_seqs > 1 && batch.kv_table_stride < h->n_sel + 1) return QUEST_EINVAL;
    DecodeRequest r = attention_request(q, o, kv, num_qo_heads, lse);
    r.state = state, r.batch = batch;
    r.app_k = k, r.app_v = v, r.metadata = metadata;
    return shared_entry(h, r, (hipStream_t)stream);
}

extern "C" int quest_decode_forward_fused_topk(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t kv,
                                               uint32_t num_qo_heads, const void* scores, uint32_t n_scores,
                                               uint32_t score_stride, void* topk_val_out, int32_t* topk_idx_out, float* lse,
                                               quest_stream_t stream) {
    if (!scores || (score_stride != 0 && score_stride < n_scores)) return QUEST_EINVAL;
    DecodeRequest r = attention_request(q, o, kv, num_qo_heads, lse);
    r.scores = scores, r.n_scores = n_scores, r.score_stride = score_stride;
    r.topk_val_out = topk_val_out, r.topk_idx_out = topk_idx_out;
    return decode_entry(h, r, (hipStream_t)stream);
}

// The state-driven fused launch: whole rows (tile_max_offset 0) or rows that carry their tile maxima at
// `tile_max_offset`, one sequence or a batch (blockIdx.z = sequence; live lengths and budgets per sequence).  Dispatch
// (keys per thread) is chosen for the longest row the graph will see.
extern "C" int quest_decode_forward_fused_topk_batched(quest_decode_handler_t* h, const void* q, void* o,
                                                       quest_paged_kv_t kv, uint32_t num_qo_heads, const void* scores,
                                                       uint32_t score_stride, uint32_t max_n_scores,
                                                       uint32_t tile_max_offset, const quest_step_state_t* state,
                                                       quest_batch_t batch, float* lse, quest_stream_t stream) {
    if (!scores || !state || score_stride < max_n_scores) return QUEST_EINVAL;
    if (batch.n_seqs > 1 && batch.kv_table_stride < max_n_scores + 1) return QUEST_EINVAL;
    DecodeRequest r = attention_request(q, o, kv, num_qo_heads, lse);
    r.state = state, r.batch = batch;
    r.scores = scores, r.n_scores = max_n_scores, r.score_stride = score_stride, r.tile_off = tile_max_offset;
    return decode_entry(h, r, (hipStream_t)stream);
}

// ---- group-shared page selection (opt-in): one selection per kv head, attended by all heads of its group
template <int D>
static int launch_group_topk(quest_decode_handler* h, const GroupTopkParams& p, uint32_t gs, uint32_t n_seqs, hipStream_t s) {
    const bool bf16 = h->dtype == QUEST_DTYPE_BF16;
    constexpr int NW = kGroupTopkWaves;
    dim3 grid(p.n_chunks, p.num_kv_heads, n_seqs), block(NW * kWave);
#define QUEST_GROUP_CASE(GS)                                                                                                    \
    case GS:                                                                                                                    \
        hipLaunchKernelGGL((bf16 ? group_topk_attend_kernel_bfloat16<D, GS, NW> : group_topk_attend_kernel<D, GS, NW>), grid, block, 0, s, p); \
        break;
    switch (gs) {
        QUEST_GROUP_CASE(1)
        QUEST_GROUP_CASE(2)
        QUEST_GROUP_CASE(4)
        QUEST_GROUP_CASE(8)
        default: return QUEST_EUNSUPPORTED;
    }
#undef QUEST_GROUP_CASE
    QUEST_LAUNCH_CHECK();
    uint32_t* info = h->last_launch;  // front-end variant 9 = the group-selection launch
    info[0] = (uint32_t)kGroupTopkKeys, info[1] = (uint32_t)NW, info[2] = 9u, info[3] = 1u, info[4] = p.n_chunks, info[5] = n_seqs;
    DecodeParams m{};  // what the merge launch reads
    m.o = p.o, m.ws = p.ws, m.n_chunks = p.n_chunks, m.ws_stride = p.ws_stride;
    return merge_and_advance<D>(h, m, p.num_kv_heads * gs * n_seqs, p.lse, s, bf16);
}

extern "C" int quest_decode_forward_group_topk(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t kv,
                                               uint32_t num_qo_heads, const void* scores, uint32_t score_stride,
                                               uint32_t max_n_scores, const quest_step_state_t* state, quest_batch_t batch,
                                               float* lse, quest_stream_t stream) {
    if (!scores || score_stride < max_n_scores) return QUEST_EINVAL;
    if (!state && batch.n_seqs != 1) return QUEST_EINVAL;  // the eager form is one sequence: lengths come from the view
    if (batch.n_seqs > 1 && batch.kv_table_stride < max_n_scores + 1) return QUEST_EINVAL;
    DecodeRequest r = attention_request(q, o, kv, num_qo_heads, lse);
    r.state = state, r.batch = batch;
    r.scores = scores, r.n_scores = max_n_scores, r.score_stride = score_stride;
    if (int e = check_request(h, r, Route::kHeadLists)) return e;
    // the envelope (include/quest_hip.h), before anything is launched
    const uint32_t group = num_qo_heads / kv.num_heads;
    if (kv.page_size != 16 || (kv.head_dim != 64 && kv.head_dim != 128)) return QUEST_EUNSUPPORTED;
    if (group != 1 && group != 2 && group != 4 && group != 8) return QUEST_EUNSUPPORTED;
    if (h->n_sel > QUEST_GROUP_TOPK_MAX_SELECTED || max_n_scores > QUEST_GROUP_TOPK_MAX_ROW ||
        batch.n_seqs > QUEST_GROUP_TOPK_MAX_SEQS || h->group_ppc > (uint32_t)kFusedMaxPpc)
        return QUEST_EUNSUPPORTED;
    GroupTopkParams p{};
    p.q = (const half_t*)q, p.kv = (const half_t*)kv.data, p.tables = kv.indices, p.scores = (const uint16_t*)scores;
    p.state = state, p.budgets = state ? batch.page_budgets : nullptr;
    p.o = (half_t*)o, p.ws = h->ws, p.lse = lse;
    p.sel_val_out = (uint16_t*)h->sel_val_out, p.sel_idx_out = h->sel_idx_out, p.sel_stride = h->n_sel;
    p.st = pool_strides(kv), p.num_kv_heads = kv.num_heads;
    p.n_cap = max_n_scores, p.score_stride = score_stride, p.table_stride = batch.kv_table_stride;
    const uint32_t nt = kGroupTopkWaves * kWave, per_thread = (max_n_scores + nt - 1) / nt;
    p.cpt = (per_thread + 3) / 4 * 4;  // 4 or 8: a thread's columns are one or two 8-byte loads per score row
    p.vec_scores = ((uintptr_t)scores & 7u) == 0 && score_stride % 4u == 0 && score_stride >= ((max_n_scores + 3u) & ~3u) ? 1u : 0u;
    p.table_vec = ((uintptr_t)kv.indices & 15u) == 0 && (batch.n_seqs == 1 || batch.kv_table_stride % 4u == 0) ? 1u : 0u;
    p.n_sel = h->n_sel, p.n_scores = max_n_scores;
    p.last_page_len = r.kv.last_page_len, p.last_page_idx = kv.last_page_idx;
    p.pages_per_chunk = h->group_ppc, p.n_chunks = h->group_chunks, p.ws_stride = h->ws_stride;
    p.scale_log2 = softmax_scale_log2(kv.head_dim);
    return kv.head_dim == 64 ? launch_group_topk<64>(h, p, group, batch.n_seqs, (hipStream_t)stream)
                             : launch_group_topk<128>(h, p, group, batch.n_seqs, (hipStream_t)stream);
}

// append + estimate + top-k + sparse attention of one layer for a whole batch in ONE launch (layer_device.cuh).
// QUEST_EUNSUPPORTED when the plan or the shape is outside what the launch serves: the caller then issues
// quest_append_estimate_batched + quest_decode_forward_fused_topk_batched (same bits).
extern "C" int quest_decode_layer_fused_batched(quest_decode_handler_t* h, const void* k, const void* v,
                                                quest_paged_kv_t metadata, const void* q, void* o, quest_paged_kv_t kv,
                                                uint32_t num_qo_heads, uint32_t max_n_scores,
                                                const quest_step_state_t* state, quest_batch_t batch, void* scores_out,
                                                uint32_t score_stride, float* lse, quest_stream_t stream) {
    if (!h || !k || !v || !q || !o || !state || batch.n_seqs == 0 || max_n_scores == 0) return QUEST_EINVAL;
    DecodeRequest r = attention_request(q, o, kv, num_qo_heads, lse);
    r.state = state, r.batch = batch;
    r.app_k = k, r.app_v = v, r.metadata = metadata;
    if (int e = check_request(h, r, Route::kLayer)) return e;
    if (kv.dtype != QUEST_DTYPE_F16) return QUEST_EUNSUPPORTED;  // the one-launch layer has no bf16 form: the caller's two launches
    if (scores_out && score_stride < max_n_scores) return QUEST_EINVAL;
    if (batch.n_seqs > 1 && (batch.kv_table_stride < max_n_scores + 1 ||
                             (uint64_t)batch.meta_table_stride * metadata.page_size < max_n_scores))
        return QUEST_EINVAL;
    // served: one workgroup per head (the planner's split for a batch that fills the chip), the whole selection in one
    // workgroup's LDS list, page size 16, head_dim 128 / 64, rows the 8-keys-per-thread selection covers
    constexpr uint32_t NW = 8, NT = NW * kWave, FC = 8;
    if (h->n_chunks != 1 || h->n_sel + 1 > (uint32_t)kFusedMaxPpc || h->n_sel == 0) return QUEST_EUNSUPPORTED;
    if (kv.page_size != 16 || (kv.head_dim != 128 && kv.head_dim != 64)) return QUEST_EUNSUPPORTED;
    if (max_n_scores > FC * NT) return QUEST_EUNSUPPORTED;
    LayerParams p{};
    p.q = (const half_t*)q, p.k_new = (const half_t*)k, p.v_new = (const half_t*)v, p.o = (half_t*)o, p.lse = lse;
    p.state = state, p.budgets = batch.page_budgets;
    p.meta = (const half_t*)metadata.data, p.meta_tables = metadata.indices, p.meta_table_stride = batch.meta_table_stride;
    p.kv = (half_t*)kv.data, p.kv_tables = kv.indices, p.kv_table_stride = batch.kv_table_stride;
    p.st = pool_strides(kv), p.num_kv_heads = kv.num_heads;
    p.n_cap = max_n_scores;
    const uint32_t per_thread = (max_n_scores + NT - 1) / NT, r4 = (per_thread + 3) / 4 * 4;
    p.cpt = r4 <= FC ? r4 : per_thread;
    p.group = num_qo_heads / kv.num_heads;
    p.xcd_period = grid_row_order(1, num_qo_heads, p.group, nullptr);  // one workgroup per head
#ifdef QUEST_WALLSTAMPS
    p.ws = h->ws;
#endif
    p.scores_out = (uint16_t*)scores_out, p.score_stride = score_stride;
    p.sel_val_out = (uint16_t*)h->sel_val_out, p.sel_idx_out = h->sel_idx_out, p.sel_stride = h->n_sel;
    p.n_sel = h->n_sel;
    p.ids_lds_offset = (uint32_t)((((size_t)max_n_scores * 2) + 15) & ~(size_t)15);
    p.ws_stride = h->ws_stride;
    p.scale_log2 = softmax_scale_log2(kv.head_dim);
    const size_t lds = (size_t)p.ids_lds_offset + (size_t)(max_n_scores + 1u) * 4u;
    dim3 grid(1, num_qo_heads, batch.n_seqs), block(NT);
    hipStream_t s = (hipStream_t)stream;
    if (kv.head_dim == 128)
        hipLaunchKernelGGL((layer_decode_kernel<128, FC, NW>), grid, block, lds, s, QUEST_LAYER_HEAD_ARGS(p, num_qo_heads), p);
    else
        hipLaunchKernelGGL((layer_decode_kernel<64, FC, NW>), grid, block, lds, s, QUEST_LAYER_HEAD_ARGS(p, num_qo_heads), p);
    QUEST_LAUNCH_CHECK();
    uint32_t* info = h->last_launch;  // front-end variant 7 = the one-launch layer (keys from LDS)
    info[0] = FC, info[1] = NW, info[2] = 7u, info[3] = 1u, info[4] = 1u, info[5] = batch.n_seqs;
    return flush_armed_advance(h, s);  // (no merge launch to ride in: the armed reservation follows as its own launch)
}

extern "C" int quest_decode_forward_batched(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t kv,
                                            uint32_t num_qo_heads, const int32_t* indices, uint32_t idx_stride,
                                            const quest_step_state_t* state, quest_batch_t batch, float* lse,
                                            quest_stream_t stream) {
    if (!h || !state || !indices) return QUEST_EINVAL;
    if (idx_stride < h->n_sel) return QUEST_EINVAL;  // rows must hold the plan's selected-page count
    DecodeRequest r = attention_request(q, o, kv, num_qo_heads, lse);
    r.kv.indices = indices;        // [n_seqs][num_qo_heads][idx_stride]
    r.kv.page_budget = idx_stride;  // row stride of a head's list
    r.state = state, r.batch = batch;
    r.batch.kv_table_stride = num_qo_heads * idx_stride;  // entries between the sequences' index blocks
    return decode_entry(h, r, (hipStream_t)stream);
}

extern "C" const char* quest_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case QUEST_EINVAL: return "quest: invalid argument";
        case QUEST_EUNSUPPORTED: return "quest: unsupported head_dim/page_size/group size";
        case QUEST_ESTATE: return "quest: begin_forward() must be called before forward()";
        case QUEST_ETOOLARGE: return "quest: top-k row exceeds QUEST_TOPK_MAX_ROW";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "quest: unknown error";
    }
}

// "quest_hip gfx950 src=<16 hex digits> r4": the digits are build.py's hash of csrc/*, include/quest_hip.h and the compiler
// flags; quest_amd/_lib.py recomputes it from the sources at import and refuses a library built from anything else.
#ifndef QUEST_SRC_HASH
#define QUEST_SRC_HASH "unhashed-build!!"
#endif
extern "C" const char* quest_build_info(void) { return "quest_hip gfx950 src=" QUEST_SRC_HASH " r4"; }
