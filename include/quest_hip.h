/*
 * quest_hip.h -- C ABI of libquest_hip.so, the MI355X (gfx950) implementation of Quest's
 * query-aware sparse decode path.
 *
 * This is the drop-in boundary: every entry point takes plain device pointers, sizes and a
 * HIP stream -- no torch types -- and corresponds one-to-one to an operator the reference
 * exposes through its PyBind module `quest._kernels` (quest/ops/csrc/bsk_ops.cu:4-20,
 * declarations bsk_ops.h:23-117).  INTEGRATION.md shows the binding a maintainer adds on
 * the reference side.
 *
 * Conventions
 *   - Tensors are contiguous and resident in device memory.  Index tensors are int32.
 *   - Element type: fp16 (QUEST_DTYPE_F16 = 0, the default; the reference dispatches only Half:
 *     pytorch_extension_utils.h:25-36) or bfloat16 (QUEST_DTYPE_BF16 = 1, EXTENSION).  Where this file says "fp16" of a
 *     q / k / v / o / score tensor or a pool, read "the call's element type".  A call's element type is the `dtype` field
 *     of the pool view(s) it is given (quest_paged_kv_t; the field was `reserved`, so a zero-initialised view still means
 *     fp16): q, k, v, o and the score rows of that call have that type.  An unknown value, or two views of one call with
 *     different values, is QUEST_EINVAL before anything is launched.  A decode handler has a type of its own
 *     (quest_decode_set_dtype, default fp16) and refuses views of the other one with QUEST_EINVAL.  The two operators
 *     that take neither a view nor a handler have one typed entry each: quest_apply_rope_in_place_dtype (every RoPE
 *     form) and quest_rms_norm_forward_dtype; every other symbol means fp16 when given zeroed views.  Top-k (quest_topk_filtering*) orders 16-bit sign-magnitude bit patterns and is the same code for both.
 *     bf16 differences: metadata max / min treat patterns above 0x7f80 as NaN, a new page's entry starts from -/+ the
 *     largest finite bf16 (0xff7f / 0x7f7f) instead of -/+65504, scores are bf16_rne of the same fp32 sum, partial
 *     attention states stay fp32.  The decode-layer projections (quest_decode_norm_gemv, _gemv_residual, _mlp_gate_up,
 *     _qkv_rope, _qkv and their _batched forms) take neither a view nor a handler either: each is one entry with
 *     `uint32_t dtype` in front of `stream`.
 *     fp16 only: quest_decode_layer_fused_batched, which returns QUEST_EUNSUPPORTED for bf16 views
 *     (the caller issues quest_append_estimate_batched + quest_decode_forward_fused_topk_batched).
 *   - One entry per operator.  An operator that reads lengths and last pages from device-resident step state
 *     (quest_step_state_t) has the suffix _batched and takes a quest_batch_t; one sequence is the batch of one.  Row strides
 *     and tile offsets are arguments of the one entry, 0 = contiguous rows / whole rows.
 *   - Return value: 0 on success; a positive value is a hipError_t from a launch; a negative
 *     value is one of the QUEST_E* argument errors below.  quest_error_string() names both.
 *     Nothing throws; nothing allocates except quest_decode_begin_forward (workspace, like
 *     BatchDecodeHandler::BeginForward, decode_handler.cuh:73-121).
 *   - Every launch is asynchronous on `stream` (the reference launches on the NULL stream,
 *     page.cu:89 / approx_attn.cu:141; here the caller passes torch's current stream).
 *   - layout: 0 = NHD pool [pages][2][page_size][heads][dim], 1 = HND [pages][2][heads][page_size][dim]
 *     (quest/utils/utils.py:1-5, kernels/include/decode/decode_page.cuh:196-239).
 */
#ifndef QUEST_HIP_H_
#define QUEST_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* quest_stream_t; /* hipStream_t */

#define QUEST_LAYOUT_NHD 0u
#define QUEST_LAYOUT_HND 1u
/*
 * EXTENSION (round 6): NHD with the heads of an entry ROTATED by the entry.  A pool layer has the NHD shape
 * [pages][2][page_size][num_heads][head_dim], but inside entry e's row of heads the K (metadata pool: max) vector of
 * head h sits in head slot   h ^ (e & rot),   rot   = min(num_heads & -num_heads, 4) - 1        (0, 1 or 3)
 * and its V (min) vector in   that slot ^ flip,  flip  = (min(num_heads & -num_heads, 32) - 1) & ~3  (0, 4, 12 or 28).
 * Why: on the plain NHD pool all 256-byte pieces of a head share address bits 8-12, and MI355X serves pieces whose
 * address bits 8-9 are 01 ~20 % slower than the others under mixed traffic (scripts/probe/addr_class_probe.hip), so a
 * launch with one workgroup per head ends with its "slow" heads while most CUs idle.  Rotated, every head's pieces
 * cycle through all values of those bits: every workgroup sees the mix's mean.  Same bytes, same arithmetic, same fold
 * order as NHD -> the same scores, selections and outputs bit for bit; only WHERE a vector lives differs
 * (quest_pool_slot, declared with the pool view below, is the whole definition).  Not a layout the reference has (quest/utils/utils.py:1-5 knows NHD and
 * HND; decode_page.cuh:196-239 are their offsets): a pool in this layout must be written and read through this library.
 */
#define QUEST_LAYOUT_NHD_ROT 2u

/* Element type of a pool and of the q / k / v / o / score tensors that travel with it (quest_paged_kv_t.dtype). */
#define QUEST_DTYPE_F16 0u
#define QUEST_DTYPE_BF16 1u

#define QUEST_EINVAL (-1)      /* malformed argument (null pointer, zero size, bad layout) */
#define QUEST_EUNSUPPORTED (-2) /* head_dim / page_size / group size outside the built set */
#define QUEST_ESTATE (-3)      /* forward without begin_forward (decode_handler.cuh:226-231) */
#define QUEST_ETOOLARGE (-4)   /* top-k row longer than QUEST_TOPK_MAX_ROW */

#define QUEST_TOPK_MAX_ROW 16384u

/*
 * View of one layer of a paged pool plus one sequence's page table.  Replaces
 * paged_kv_t<kIndices, layout, half, int32_t> (decode_page.cuh:79-110), which the reference
 * passes to its kernels by value; so is this.
 */
typedef struct quest_paged_kv {
    void* data;             /* pool base of this layer, elements of type `dtype` (kv_cache.py:111-113 buf_layer) */
    const int32_t* indices; /* page table; for quest_decode_forward: [num_qo_heads][page_budget] */
    const int32_t* indptr;  /* device int32[2] = {0, n_pages} */
    uint32_t num_heads;     /* heads stored in the pool (kv heads) */
    uint32_t page_size;
    uint32_t head_dim;
    uint32_t page_budget;   /* row stride of `indices` in quest_decode_forward, else 0 */
    uint32_t last_page_len; /* 1..page_size */
    int32_t last_page_idx;  /* physical id of the sequence's last page */
    uint32_t layout;
    uint32_t dtype;         /* QUEST_DTYPE_F16 (0: what a zero-initialised view means) or QUEST_DTYPE_BF16 */
} quest_paged_kv_t;

/* Where a vector lives inside an entry's row of heads (host function, no GPU): the head SLOT of head `head`'s K / max vector
 * (v_slot == 0) or V / min vector (v_slot != 0) of entry `entry` (its index inside the page) in a pool of `num_heads` heads.
 * NHD and HND: the head itself; NHD_ROT: head ^ (entry & rot) [^ flip for V], the definition in the comment of
 * QUEST_LAYOUT_NHD_ROT above.  The address of the vector is then, in halves from the layer's base,
 * page * 2*S*H*D + v * S*H*D + entry * H*D + slot * D (NHD family).  0xffffffff for a malformed layout / head. */
uint32_t quest_pool_slot(uint32_t layout, uint32_t num_heads, uint32_t head, uint32_t entry, int v_slot);

const char* quest_error_string(int code);

/* Build identification: "gfx950" and the kernel generation, for logs. */
const char* quest_build_info(void);

/*
 * append_kv_cache_decode (bsk_ops.h:64-76, page.cu:6-99 -> AppendPagedKVCacheDecode,
 * decode_page.cuh:577-597, kernel :398-449).
 * k, v: [1][num_heads][head_dim].  Writes the token into the last page and folds k into the
 * page's (max -> K slot, min -> V slot) metadata entry, re-initialising it to -/+65504 when the
 * token opens a new page.
 */
int quest_append_kv_cache_decode(const void* k, const void* v, quest_paged_kv_t kv,
                                 quest_paged_kv_t metadata, quest_stream_t stream);

/*
 * append_kv_cache_prefill (bsk_ops.h:50-62, page.cu:101-210 -> AppendPagedKVCachePrefill,
 * decode_page.cuh:613-642, kernel :471-562).  k, v: [append_len][num_heads][head_dim];
 * n_pages_host = number of pages of the sequence (the host knows it: len(kv_indices)).
 */
int quest_append_kv_cache_prefill(const void* k, const void* v, uint32_t append_len,
                                  uint32_t n_pages_host, quest_paged_kv_t kv,
                                  quest_paged_kv_t metadata, quest_stream_t stream);

/*
 * estimate_attn_score (bsk_ops.h:41-48, estimate.cu:6-84 -> MaxPossibleSampleWithPagedKVCache,
 * decode_attn.cuh:1092-1149, kernel :245-401).
 * q: [1][num_qo_heads][head_dim]; o: [num_qo_heads][n_out] fp16 with n_out = (number of KV
 * pages) - 1; o[h][p] = fp16( sum_d max(q*Kmax, q*Kmin) ).
 * Shapes: head_dim 64 / 128 / 256, group (num_qo_heads / kv heads) 1 / 2 / 4 / 8, any page size, the three layouts;
 * QUEST_EUNSUPPORTED otherwise, before anything is launched and with `o` untouched.  REFUSED within that set, by every
 * estimate entry (this one, quest_append_estimate, quest_estimate_attn_score_batched, quest_append_estimate_batched in
 * both forms): head_dim 256 with group 8 on QUEST_LAYOUT_NHD_ROT when the number of kv heads is a multiple of 4 -- the
 * rotation of such a pool (rot = 3) needs 4 kv heads in one workgroup tile, whose 32 query vectors of 256 elements do not
 * fit the tile's staging pass.  The same shapes on QUEST_LAYOUT_NHD and QUEST_LAYOUT_HND are served (same scores bit for
 * bit).  quest_estimate_plan (below, no GPU needed) answers for a shape what the launch would; the Python controllers ask
 * it at construction.
 */
int quest_estimate_attn_score(const void* q, void* o, uint32_t num_qo_heads, uint32_t n_out,
                              quest_paged_kv_t metadata, quest_stream_t stream);

/*
 * Fused form of the two calls QuestAttention.forward makes back to back for a decode token
 * (QuestAttention.py:106 append_kv, :136 decode_estimate): ONE launch writes the new token (k, v) into
 * the cache + folds it into its page's metadata, and scores all pages but the current one.  The two
 * halves touch disjoint bytes (the estimate excludes the current page's entry), so the result is
 * identical to calling quest_append_kv_cache_decode then quest_estimate_attn_score.
 * o_stride: elements between the rows of consecutive query heads (0 = n_out, contiguous rows).
 */
int quest_append_estimate(const void* k, const void* v, quest_paged_kv_t kv, const void* q, void* o,
                          uint32_t num_qo_heads, uint32_t n_out, uint32_t o_stride, quest_paged_kv_t metadata,
                          quest_stream_t stream);

/*
 * topk_filtering (bsk_ops.h:34-39, topk.cu:7-46 -> decode_select_k, decode_select_k.cuh:25-62,
 * which calls RAFT's radix_topk_one_block_kernel; re-implemented here).
 * estimated_value/indices: [num_heads][num_pages]; d_out/indices_out: [num_heads][page_budget].
 * Deterministic: ties at the k-th value go to the lowest column; output in ascending column order.
 * `buf` is the reference's scratch argument; unused (may be NULL).
 * value_stride: elements between consecutive heads' rows of `estimated_value` (0 = num_pages, contiguous rows): serves the
 * padded score rows quest_append_estimate writes without a compacting copy.
 */
int quest_topk_filtering(const void* estimated_value, uint32_t value_stride, const int32_t* estimated_indices, void* d_out,
                         int32_t* indices_out, void* buf, uint32_t num_heads, uint32_t num_pages, uint32_t page_budget,
                         quest_stream_t stream);

/*
 * BatchDecodeWithPagedKVCachePyTorchWrapper (bsk_ops.h:88-117, approx_attn.cu:27-150 ->
 * BatchDecodeHandler, decode_handler.cuh:39-244).
 */
typedef struct quest_decode_handler quest_decode_handler_t;

int quest_decode_handler_create(quest_decode_handler_t** out, uint32_t layout);
void quest_decode_handler_destroy(quest_decode_handler_t* h);

/* begin_forward: n_selected_pages = indptr[1] - indptr[0] = page budget - 1 (the caller has it on
 * the host; the reference copies it back from the device, decode_attn.cuh:866-873).  Plans the
 * split of each head's page list over workgroups and sizes the partial-state workspace. */
int quest_decode_begin_forward(quest_decode_handler_t* h, uint32_t n_selected_pages,
                               uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t head_dim,
                               uint32_t page_size, quest_stream_t stream);
int quest_decode_end_forward(quest_decode_handler_t* h);

/* forward: q, o: [1][num_qo_heads][head_dim]; paged_kv.indices = [num_qo_heads][page_budget]
 * selected physical pages (row stride paged_kv.page_budget), to which the sequence's last page
 * (last_page_idx, last_page_len tokens) is always added (decode_page.cuh:325-351).
 * lse: optional float[num_qo_heads] (natural log), may be NULL; every entry below that takes `lse` writes the same quantity,
 * the batched / state-driven ones as float[n_seqs][num_qo_heads] (row of sequence i at i * num_qo_heads). */
int quest_decode_forward(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t paged_kv,
                         uint32_t num_qo_heads, float* lse, quest_stream_t stream);

/*
 * forward for the case where every query head attends the SAME page list (what the reference passes as
 * kv_indices_without_last.repeat(num_heads, 1) when the budget covers the cache, controller.py:106,
 * QuestAttention.py:125-132): paged_kv.indices = ONE row [n_selected_pages].  With GQA the K/V tiles of
 * a kv head are then fetched once for its whole query group.  page_size 16, head_dim 64/128.
 */
int quest_decode_forward_shared(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t paged_kv,
                                uint32_t num_qo_heads, float* lse, quest_stream_t stream);

/*
 * Fused form of decode_topk + decode_sparse_attn (QuestAttention.py:144-157): the top-k selection of
 * quest_topk_filtering runs at the head of the attention kernel (every workgroup of a head recomputes
 * it from the head's score row -- a 4 KiB L2-resident read -- so no second launch and no cross-workgroup
 * hand-off), then the selected pages are gathered exactly as in quest_decode_forward.
 *   scores      [num_qo_heads][n_scores] fp16, the estimate output (n_scores = pages - 1)
 *   page_table  paged_kv.indices = the sequence's page table [n_scores + 1] (kv_indices_with_last)
 *   topk_val_out / topk_idx_out  optional [num_qo_heads][n_selected_pages]: the selection, bit-identical
 *                to quest_topk_filtering's outputs (same routine), for callers that inspect it.
 *   score_stride  elements between the rows of `scores` (0 = n_scores).  The reference's score tensor is a contiguous
 *                [num_qo_heads][pages - 1] (quest/utils/__init__.py:171-205), whose rows are only 2-byte aligned; rows padded
 *                to a multiple of 8 columns (16 bytes: quest_append_estimate writes them) let the front end fetch a thread's
 *                scores with one vector load.  Both layouts are served in ONE launch (also the reference's layout beyond 4096
 *                pages: every workgroup reads the 8-byte aligned stream below its row and skips the 0-3 leading columns of
 *                the previous row; up to QUEST_TOPK_MAX_ROW - 3 pages -- QUEST_EUNSUPPORTED beyond: callers then issue
 *                quest_topk_filtering + quest_decode_forward).
 */
int quest_decode_forward_fused_topk(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t paged_kv,
                                    uint32_t num_qo_heads, const void* scores, uint32_t n_scores, uint32_t score_stride,
                                    void* topk_val_out, int32_t* topk_idx_out, float* lse, quest_stream_t stream);

/*
 * Device-resident step state (host planning rewrite).  The reference rebuilds page-table
 * tensors and re-plans on the host for every token (quest/utils/controller.py:80-129); with the sequence
 * state in device memory a decode step captured ONCE in a hipGraph can be replayed token after token while
 * the sequence grows: quest_step_state_advance_batched is prepare_metadata(1) on the device, and the STATE-DRIVEN entries
 * (the *_batched ones below) read lengths / last-page ids from the state instead of from the by-value fields of their views.
 * The page tables must be materialised up to the pool capacity (page i of the sequence = kv_table[i]).
 */
typedef struct quest_step_state {
    int32_t seq_len;            /* tokens in the cache, including the one being decoded */
    int32_t n_pages;            /* KV pages in use */
    int32_t kv_last_page_len;   /* 1..page_size */
    int32_t kv_last_page_idx;   /* physical id */
    int32_t n_meta_pages;
    int32_t meta_last_page_len;
    int32_t meta_last_page_idx;
    int32_t reserved;           /* set to 1 by quest_step_state_advance_batched when the pool is exhausted */
} quest_step_state_t;

/*
 * The sequences a state-driven launch serves (SURVEY.md 8f-3 second half: the reference fixes `constexpr batch_size = 1`,
 * approx_attn.cu:113 / estimate.cu:14; BASELINE config 5 decodes 8 sequences per GPU).  One launch serves
 * n_seqs independent sequences (grid.z / grid.y = sequence), no data is shared between them:
 *   - ONE KV pool and ONE metadata pool hold every sequence's pages (`data` of the views below);
 *   - page tables are rows of one int32 matrix: sequence i's table = indices + i * *_table_stride,
 *     each materialised up to its capacity;
 *   - `state` is an array of n_seqs step states; q / o / k / v are [n_seqs][heads][dim], scores
 *     [n_seqs][num_qo_heads][score_stride], lse [n_seqs][num_qo_heads].
 * A SINGLE SEQUENCE is the batch {1, 0, 0, 0, NULL}: its tables are plain arrays, and with n_seqs == 1 no entry reads the
 * strides -- except quest_step_state_advance_batched, which checks them against the capacities for every n_seqs (pass the
 * capacities there).  It runs the same device code as sequence 0 of a larger batch.
 * Per sequence, pools, estimates and page selections do not depend on n_seqs, bit for bit; attention outputs neither when
 * the work split (pages per workgroup) is the same, otherwise they differ by the fp32 rounding of a different
 * partial-state merge order (tests: <= 2e-3).
 */
typedef struct quest_batch {
    uint32_t n_seqs;
    uint32_t kv_table_stride;   /* int32 entries between consecutive sequences' KV page tables */
    uint32_t meta_table_stride; /* ... metadata page tables */
    uint32_t reserved;
    /* Optional per-sequence page budgets, device int32[n_seqs]: pages sequence i attends INCLUDING its current page
     * (the reference's per-request page budget: InferenceController.set_page_budget, quest/utils/controller.py:66-68,
     * one controller per request).  NULL: every sequence takes the budget the handler was planned with.  With
     * budgets, plan the handler (begin_forward) with the LARGEST one; sequence i then selects
     * min(budget[i] - 1, its pages - 1) pages. */
    const int32_t* page_budgets;
} quest_batch_t;

/* Reserve room for one more token of every sequence: the device-side prepare_metadata(1) (controller.py:72-76).  The tables
 * ([n_seqs][*_table_stride]) hold max_kv_pages / max_meta_pages valid entries per row (the pools' capacities); when the
 * next token would not fit the state is left unchanged and `reserved` is set, so a replayed graph can never index past a
 * table. */
int quest_step_state_advance_batched(quest_step_state_t* state, const int32_t* kv_tables, const int32_t* meta_tables,
                                     uint32_t page_size, uint32_t max_kv_pages, uint32_t max_meta_pages,
                                     quest_batch_t batch, quest_stream_t stream);

/* The same reservation RIDING IN A STEP'S LAST LAUNCH (round 6): quest_step_state_advance_batched at the head of a captured
 * step is a 1-thread launch of dependent loads -- 4.7 us per token.  Nothing after a layer's merge launch reads the step state, so the
 * reservation for the NEXT token can be made there: arm it on the handler right before the last layer's forward call of a
 * step; the merge launch of that call carries it (one thread per sequence of its first workgroup) and the handler disarms.
 * A forward whose plan has no merge launch issues it as its own launch behind the attention kernel (correct, nothing saved).
 * The caller reserves the FIRST token with quest_step_state_advance_batched before the first step; from then on the device
 * state (and its host mirror, InferenceController.prepare_metadata(1) after every step) runs one reserved token ahead of the
 * tokens appended.  state == NULL disarms.  At most 64 sequences. */
int quest_decode_arm_step_advance(quest_decode_handler_t* h, quest_step_state_t* state, const int32_t* kv_tables,
                                  const int32_t* meta_tables, uint32_t page_size, uint32_t max_kv_pages,
                                  uint32_t max_meta_pages, quest_batch_t batch);

/* quest_append_estimate with lengths / last-page ids / n_out (= state[i].n_pages - 1) taken from `state`.
 * o is [n_seqs][num_qo_heads][o_stride] with o_stride >= max_n_out, the largest n_out the graph will ever see
 * (the grid is sized for it; surplus workgroups exit).  tile_max_offset: 0, or the tiles form described below. */
int quest_append_estimate_batched(const void* k, const void* v, quest_paged_kv_t kv, const void* q, void* o,
                                  uint32_t num_qo_heads, uint32_t o_stride, uint32_t max_n_out, uint32_t tile_max_offset,
                                  quest_paged_kv_t metadata, const quest_step_state_t* state, quest_batch_t batch,
                                  quest_stream_t stream);
/* quest_decode_forward_fused_topk with the row length (state[i].n_pages - 1) and the current page taken
 * from `state`; scores is [n_seqs][num_qo_heads][score_stride].  The plan (selected-page count) is the one of
 * begin_forward and must not exceed state[i].n_pages - 1 for the life of the graph; the handler must have been planned for
 * the batch: quest_decode_set_batch(h, n_seqs) before begin_forward.  tile_max_offset: 0, or the tiles form. */
int quest_decode_forward_fused_topk_batched(quest_decode_handler_t* h, const void* q, void* o,
                                            quest_paged_kv_t paged_kv, uint32_t num_qo_heads, const void* scores,
                                            uint32_t score_stride, uint32_t max_n_scores, uint32_t tile_max_offset,
                                            const quest_step_state_t* state, quest_batch_t batch, float* lse,
                                            quest_stream_t stream);
/*
 * THE TILES FORM of the pair above (tile_max_offset != 0), for LONG score rows (round 5; cfg 4: 8191 pages), with TILE
 * MAXIMA handed across the kernel boundary: the estimate workgroup that holds the scores of 8 consecutive pages also stores
 * the largest of them (as an order-preserving 16-bit key) at o[i][h][tile_max_offset + page / 8], and the attention launch
 * selects in two short passes -- the top-k TILES by maximum (a sufficient candidate set under the declared tie rule:
 * csrc/decode_device.cuh sparse_decode_tiles_body), then the exact top-k over those tiles' 8 k scores -- instead of passes
 * over the whole row in every workgroup of a head.  Selections and outputs are those of the whole-row form
 * (tile_max_offset 0) under the same plan, bit for bit.
 * Row layout: every row carries its own tile maxima at tile_max_offset = max_n rounded up to 8; rows 16-byte aligned (base
 * 16-byte aligned and stride a multiple of 8) with stride >= tile_max_offset + ceil(max_n / 8) rounded up to 4.  All
 * sequences share the capacity max_n; sequence i's live row (state[i].n_pages - 1 columns) may be shorter, down to empty:
 * only the maxima of its live runs of 8 pages are written and read, whatever lies behind them in the row is never looked
 * at.  Per-sequence budgets (batch.page_budgets), a sequence shorter than its budget (it attends all of its pages) and
 * quest_decode_set_selection_out work as in the whole-row form.
 * QUEST_EINVAL: tile_max_offset not max_n rounded up to 8, a stride without room for the maxima, misaligned rows,
 * n_seqs == 0, a KV table stride shorter than max_n + 1 or a metadata table that does not cover max_n (n_seqs > 1).
 * QUEST_ESTATE: no plan, or a plan for fewer sequences.  QUEST_EUNSUPPORTED, before anything is launched: page size other
 * than 16, more than 256 selected pages, rows beyond 16384 pages, an estimate shape with no tile 8 pages wide (the
 * estimate side needs its workgroup tile to be a multiple of 8 pages wide; head_dim 256: the tile covers 4 kv heads instead
 * of 8) -- the caller then issues the whole-row form.  quest_decode_last_launch_info reports front-end variant 8 and n_seqs.
 */

/*
 * GROUP-SHARED PAGE SELECTION for GQA (EXTENSION, opt-in): ONE selection per KV HEAD, attended by all query heads of its
 * group, in place of quest_decode_forward_fused_topk_batched's one selection per query head.  The attention launch then
 * fetches each selected K/V tile once per kv head instead of once per query head (group x fewer K/V bytes).  This is NOT the
 * reference's algorithm -- evaluation/quest_attention.py:139-140 repeats K/V and selects per query head -- so nothing takes
 * it by default, and its effect on a real checkpoint's accuracy has not been measured.
 *
 * Semantics, for sequence i and kv head hk, G = num_qo_heads / num_kv_heads:
 *   1. group score of page p = the maximum over g < G of scores[i][hk * G + g][p] (the rows quest_append_estimate_batched
 *      writes), taken on the 16-bit order-preserving keys the top-k uses: exact and total, also for +-0 and NaN patterns;
 *   2. selection = the contract of the top-k operator on that row: k = min(budget_i - 1, n_pages_i - 1) columns, every key
 *      above the threshold plus the lowest columns among ties, in ascending column order;
 *   3. every head of the group attends those k pages + the current page; partial records, merge and lse as in the other
 *      launches.
 * For G = 1 the selection is quest_decode_forward_fused_topk_batched's, bit for bit.
 *
 * Arguments as quest_decode_forward_fused_topk_batched, without the tiles form.  state == NULL: the eager single-sequence
 * form -- batch.n_seqs must be 1, the row length is max_n_scores, the current page comes from the view (last_page_len /
 * last_page_idx) and the plan's selected-page count must not exceed max_n_scores.  begin_forward plans this launch's own
 * work split of (kv head, chunk) workgroups next to the per-head one (at most 256 pages per workgroup) and sizes the
 * workspace for both.  quest_decode_set_selection_out is served with rows [n_seqs][num_kv_heads][n_selected_pages of the
 * plan]; quest_decode_last_launch_info reports front-end variant 9; an armed step advance rides in the merge launch.
 * Return codes, all before anything is launched (o untouched): QUEST_EINVAL / QUEST_ESTATE as the sibling entry, and
 * QUEST_EINVAL for state == NULL with n_seqs != 1; QUEST_ETOOLARGE for rows beyond QUEST_TOPK_MAX_ROW;
 * QUEST_EUNSUPPORTED outside the envelope: page size 16, head_dim 64 / 128, group 1 / 2 / 4 / 8, at most
 * QUEST_GROUP_TOPK_MAX_SELECTED selected pages, score rows of at most QUEST_GROUP_TOPK_MAX_ROW pages (each thread of the
 * 512 keeps its 8 columns' keys and page ids in registers; longer rows would need the tiles form, not built for this
 * launch), at most QUEST_GROUP_TOPK_MAX_SEQS sequences.
 */
#define QUEST_GROUP_TOPK_MAX_ROW 4096u
#define QUEST_GROUP_TOPK_MAX_SELECTED 256u
#define QUEST_GROUP_TOPK_MAX_SEQS 64u
int quest_decode_forward_group_topk(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t paged_kv,
                                    uint32_t num_qo_heads, const void* scores, uint32_t score_stride,
                                    uint32_t max_n_scores, const quest_step_state_t* state, quest_batch_t batch, float* lse,
                                    quest_stream_t stream);

/* quest_append_kv_cache_decode with lengths / last-page ids from `state` (dense layers of a replayed step). */
int quest_append_kv_cache_decode_batched(const void* k, const void* v, quest_paged_kv_t kv, quest_paged_kv_t metadata,
                                         const quest_step_state_t* state, quest_batch_t batch, quest_stream_t stream);
/* quest_decode_forward_shared over ALL pages of every sequence (state[i].n_pages - 1 listed pages + the current
 * one): paged_kv.indices = the full page tables.  Plan with begin_forward(n_selected_pages = pool capacity - 1);
 * workgroups past the live length contribute empty partial states. */
int quest_decode_forward_shared_batched(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t paged_kv,
                                        uint32_t num_qo_heads, const quest_step_state_t* state, quest_batch_t batch,
                                        float* lse, quest_stream_t stream);
/* quest_append_kv_cache_decode_batched + quest_decode_forward_shared_batched in ONE launch (round 4: a full-KV layer of a
 * captured step = attention + merge instead of append + attention + merge; the reference's pair of calls is
 * QuestAttention.py:106 and :125-132 / page.cu:6-99).  k, v: the new tokens [n_seqs][kv heads][head_dim], not yet in the
 * pool: the one workgroup per kv head that attends the current page takes the row from k / v, writes it to the pool and
 * folds k into the page's (max, min) metadata entry -- same pool bytes as the separate append.  metadata: the layer's
 * metadata pool (same geometry as the KV pool; lengths from `state`).  QUEST_EUNSUPPORTED for shapes outside the
 * group-shared kernel (page_size 16, head_dim 64 / 128): issue the two launches then. */
int quest_decode_append_forward_shared_batched(quest_decode_handler_t* h, const void* k, const void* v,
                                               quest_paged_kv_t metadata, const void* q, void* o,
                                               quest_paged_kv_t paged_kv, uint32_t num_qo_heads,
                                               const quest_step_state_t* state, quest_batch_t batch, float* lse,
                                               quest_stream_t stream);
/*
 * One launch per layer of a batched decode step (round 5): quest_append_estimate_batched +
 * quest_decode_forward_fused_topk_batched as ONE grid of (sequence, query head) workgroups, each of which owns its head
 * end to end -- appends its kv head's new token (QuestAttention.py:106, page.cu:6-99), scores its head's pages into LDS
 * (:136, estimate.cu:6-84), selects from LDS (:144, topk.cu:7-46) and gathers the selected pages + the current one
 * (:147-157, approx_attn.cu:68-151).  No score scratch, no cross-workgroup hand-off, the same pool bytes, selections and
 * outputs as the two launches.  k, v: [n_seqs][kv heads][head_dim] (not yet in the pool); metadata / paged_kv: the
 * layer's pools (same geometry) with indices = the stacked page tables; max_n_scores = page capacity - 1.
 * scores_out: optional inspection copy of the page scores, [n_seqs][num_qo_heads][score_stride] fp16 (NULL: they stay
 * in LDS); the selection can be inspected with quest_decode_set_selection_out.
 * Serves plans with ONE workgroup per head (quest_decode_set_batch + begin_forward on a batch that fills the chip),
 * page_size 16, head_dim 64 / 128, at most 255 selected pages (token budget 4096), rows up to 4096 pages; QUEST_EUNSUPPORTED otherwise
 * (issue the two launches then).
 */
int quest_decode_layer_fused_batched(quest_decode_handler_t* h, const void* k, const void* v, quest_paged_kv_t metadata,
                                     const void* q, void* o, quest_paged_kv_t paged_kv, uint32_t num_qo_heads,
                                     uint32_t max_n_scores, const quest_step_state_t* state, quest_batch_t batch,
                                     void* scores_out, uint32_t score_stride, float* lse, quest_stream_t stream);
/*
 * The four operators of a decode step one by one for a whole batch (the state-driven counterparts of
 * append_kv_cache_decode / estimate_attn_score / topk_filtering / BatchDecodeWithPagedKVCache.forward, bsk_ops.h:34-117,
 * as quest/utils/__init__.py:141-276 calls them per request): quest_append_kv_cache_decode_batched above, and
 *   estimate : o[n_seqs][num_qo_heads][o_stride], row i scored over state[i].n_pages - 1 pages;
 *   top-k    : per (sequence, head) the k_i = min(budget_i - 1, n_pages_i - 1) largest scores of the row and the
 *              physical pages they belong to (kv_tables[i][column]), written to the first k_i entries of rows of
 *              out_stride entries; page_budget = the launch-wide budget (pages incl. the current one) used where
 *              batch.page_budgets is NULL;
 *   attention: per (sequence, head) over indices[i][h][0 .. k_i) + the current page; plan the handler with
 *              begin_forward(n_selected_pages = max_i budget_i - 1) after quest_decode_set_batch.
 * Same bits as the eager operators on each sequence.
 */
int quest_estimate_attn_score_batched(const void* q, void* o, uint32_t num_qo_heads, uint32_t o_stride, uint32_t max_n_out,
                                      quest_paged_kv_t metadata, const quest_step_state_t* state, quest_batch_t batch,
                                      quest_stream_t stream);
int quest_topk_filtering_batched(const void* scores, uint32_t score_stride, uint32_t max_num_pages, const int32_t* kv_tables,
                                 void* d_out, int32_t* indices_out, uint32_t out_stride, uint32_t num_heads,
                                 uint32_t page_budget, const quest_step_state_t* state, quest_batch_t batch,
                                 quest_stream_t stream);
int quest_decode_forward_batched(quest_decode_handler_t* h, const void* q, void* o, quest_paged_kv_t paged_kv,
                                 uint32_t num_qo_heads, const int32_t* indices, uint32_t idx_stride,
                                 const quest_step_state_t* state, quest_batch_t batch, float* lse, quest_stream_t stream);
/* Element type of the pools / q / o this handler's forwards serve (QUEST_DTYPE_*; default QUEST_DTYPE_F16).  Every forward
 * checks its view's dtype against it (QUEST_EINVAL).  May be called at any time between forwards; the plan and the fp32
 * workspace do not depend on it.  QUEST_EINVAL for an unknown value. */
int quest_decode_set_dtype(quest_decode_handler_t* h, uint32_t dtype);
/* Sequences per launch the next begin_forward plans (workspace, work split) for; default 1. */
int quest_decode_set_batch(quest_decode_handler_t* h, uint32_t n_seqs);

/*
 * apply_rope_in_place (bsk_ops.h:23-27, page.cu:212-252 -> QKApplyRotaryInPlace,
 * decode_page.cuh:695-728).  q: [n][num_qo_heads][dim], k: [n][num_kv_heads][dim], in place.
 */
int quest_apply_rope_in_place(void* q, void* k, uint32_t n, uint32_t past_kv_len,
                              uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t head_dim,
                              float rope_scale, float rope_theta, quest_stream_t stream);

/*
 * RoPE for q / k of element type `dtype` (QUEST_DTYPE_*), every form in one entry (EXTENSION).
 * Frequencies: inv_freq NULL = the rope_scale / rope_theta formula of quest_apply_rope_in_place (attention_factor unused;
 * default and linear scaling); else a frequency table (the llama3 and yarn scalings of Hugging Face's modeling_rope_utils,
 * whose frequencies no closed formula in the kernel reproduces bit for bit): pair i (features i, i + head_dim/2) at position
 * p rotates by p * inv_freq[i]; cos and sin are multiplied by attention_factor; inv_freq: device, head_dim/2 fp32
 * (rope_scale / rope_theta unused).  QUEST_EINVAL for an attention_factor that is not finite and > 0.
 * Positions: states NULL = row i at past_kv_len + i; else row i at states[i].seq_len - 1 (n = sequences, one row per
 * sequence; past_kv_len unused), so one entry serves the eager and the state-driven forms.
 * head_dim 64 / 128 / 256.  fp32 arithmetic, one rounding to the element type.
 */
int quest_apply_rope_in_place_dtype(void* q, void* k, uint32_t n, uint32_t past_kv_len, uint32_t num_qo_heads,
                                    uint32_t num_kv_heads, uint32_t head_dim, float rope_scale, float rope_theta,
                                    const float* inv_freq, float attention_factor, const quest_step_state_t* states,
                                    uint32_t dtype, quest_stream_t stream);

/* Per-head RMSNorm of q and k fused with RoPE, in place, one launch (EXTENSION: Qwen3's q_norm / k_norm; the reference has
 * no counterpart).  Rows, position sources, frequency sources and `dtype` as for quest_apply_rope_in_place_dtype;
 * q_norm_weight / k_norm_weight: [head_dim] of the element type, shared by the heads.  Per head row, in fp32:
 * inv = 1 / sqrtf(sum x^2 / head_dim + eps), n_d = x_d * inv * w_d, rotate-half RoPE on n, one round-to-nearest-even to
 * the element type (transformers rounds after the normalisation, after the weight, and rounds cos / sin).
 * QUEST_EINVAL before any launch for a NULL operand, an eps that is negative or not finite, an unknown dtype or a bad
 * table / rope_scale / rope_theta; QUEST_EUNSUPPORTED for a head_dim other than 64 / 128 / 256. */
int quest_apply_qk_norm_rope_in_place_dtype(void* q, void* k, uint32_t n, uint32_t past_kv_len, uint32_t num_qo_heads,
                                            uint32_t num_kv_heads, uint32_t head_dim, const void* q_norm_weight,
                                            const void* k_norm_weight, float eps, float rope_scale, float rope_theta,
                                            const float* inv_freq, float attention_factor,
                                            const quest_step_state_t* states, uint32_t dtype, quest_stream_t stream);

/* rms_norm_forward (bsk_ops.h:29-32, rms_norm.cu:160-212). input/output: [rows][cols], weight [cols]. */
int quest_rms_norm_forward(const void* input, const void* weight, void* output, uint32_t rows,
                           uint32_t cols, float epsilon, quest_stream_t stream);
/* The same for input / weight / output of element type `dtype` (QUEST_DTYPE_*). */
int quest_rms_norm_forward_dtype(const void* input, const void* weight, void* output, uint32_t rows, uint32_t cols,
                                 float epsilon, uint32_t dtype, quest_stream_t stream);

/*
 * prefill_with_paged_kv_cache (bsk_ops.h:78-86, batch_prefill.cu:27-117 -> BatchPrefillWithPagedKVCache,
 * kernels/include/prefill/prefill.cuh:1008-1119, kernel :688-882).  q, o: [n_q][num_qo_heads][head_dim] fp16; the
 * sequence's K/V (the n_q new tokens included: append_kv_cache_prefill ran before, utils/__init__.py:127-170) are the
 * n_pages_host pages kv.indices lists, the last one holding kv.last_page_len tokens.  Row i attends the keys
 * 0 .. kv_len - n_q + i when `causal`, every key otherwise; no rotary (RotaryMode::kNone, batch_prefill.cu:102),
 * softmax scale 1/sqrt(head_dim).  GQA: num_qo_heads a multiple of kv.num_heads, query head h reads kv head
 * h / (num_qo_heads / kv.num_heads).  head_dim 64 / 128 / 256 (the set of the reference's SWITCH_HEAD_DIM_PREFILL,
 * prefill.cuh:1073), any page_size, both layouts; QUEST_EUNSUPPORTED otherwise;
 * causal with n_q > kv_len is QUEST_EINVAL (the reference assumes kv_len >= qo_len, test_prefill_attention.py:50-51).
 * MFMA flash kernel (csrc/prefill.hip): 128 query rows per workgroup, 64-key tiles, nothing but o is written.
 */
int quest_prefill_with_paged_kv_cache(const void* q, void* o, uint32_t n_q, uint32_t num_qo_heads,
                                      quest_paged_kv_t kv, uint32_t n_pages_host, int causal,
                                      quest_stream_t stream);

/*
 * Decode-token projections of a Llama decoder layer around the attention path, fused (EXTENSION; csrc/decode_layer.hip).
 * The reference leaves them to cuBLAS + PyTorch kernels: RMSNorm (quest/ops/csrc/rms_norm.cu:82-213 via
 * quest/models/llama.py:72), q/k/v projections (QuestAttention.py:88-90) + RoPE (:99, decode_page.cuh:644-728), o_proj
 * (QuestAttention.py:175), residual adds and the SwiGLU MLP (llama.py LlamaMLP).  Row-major weights [out][in]
 * (torch.nn.Linear.weight).
 *
 * Operators (n = rmsnorm(x or h; gamma, eps)):
 *   norm_gemv      out[out_dim] = W . n                                       (gamma NULL: out = W . x)
 *   gemv_residual  h[out_dim]  += W . x                                       (in place on the residual stream)
 *   mlp_gate_up    act[intermediate] = silu(Wg . n) * (Wu . n)
 *   qkv_rope       q, k, v = Wq . n, Wk . n, Wv . n with rotate-half RoPE on q and k at position state->seq_len - 1
 *                  (call after quest_step_state_advance_batched).  inv_freq NULL: default / linear RoPE, frequency
 *                  (1 / rope_scale) * rope_theta^(-2i / head_dim); else the frequency table and attention_factor of
 *                  quest_apply_rope_in_place_dtype (QUEST_EINVAL like there)
 *   qkv            q = Wq . n [q_rows], k = Wk . n, v = Wv . n [kv_rows], stored unrotated, for models whose q and k pass
 *                  a per-head norm before RoPE; quest_apply_qk_norm_rope_in_place_dtype follows
 *
 * Forms: one entry per operator and form.  quest_decode_<operator> is one decode token; quest_decode_<operator>_batched
 * is n_tokens <= 16 tokens at once -- one per sequence of a batch (the reference asserts batch size 1;
 * BatchedInferenceController): x / h `[n_tokens][in]`, outputs `[n_tokens][out]` (q / k / v
 * `[n_tokens][heads][head_dim]`), all contiguous; `states` = n_tokens consecutive quest_step_state_t records (the batched
 * step state), token i rotated at states[i].seq_len - 1.  The weights are read once for the whole batch (MFMA row-dots:
 * weights = A operand, tokens = the 16 columns of B); head_dim % 16 == 0 for the rotating launch.  The two forms launch
 * different kernels, and one token through the batched form differs from the one-token form in the last bits.
 *
 * Element type: `dtype` (QUEST_DTYPE_F16 / QUEST_DTYPE_BF16), in front of `stream`, is the type of every vector and matrix
 * of the call; anything else is QUEST_EINVAL before any launch.  Both types run the same kernels compiled once per type
 * (bf16: <kernel>_b16; v_dot2c_f32_bf16 / v_mfma_f32_4x4x4_16b_bf16), with the same planner cells, grids, row orders and
 * shape limits (what fp16 refuses with QUEST_EUNSUPPORTED, bf16 refuses too).
 *
 * Numeric contract: products accumulate in fp32, the RMSNorm prologue rounds x * inv_rms * gamma to the element type
 * once (as quest_rms_norm_forward_dtype), SiLU * up and the rotation are computed in fp32, the residual add is
 * round(float(h) + acc), every output is rounded once, to nearest even.  qkv adds the same row-dots in the same order as
 * qkv_rope at head_dim <= 256: a lane of the one-token kernel adds a row's products in the same order whatever the
 * workgroup shape, and the batched form is planned with the rotating launch's LDS budget, so both take the same n-token
 * kernel -- the one quest_decode_batched_plan(hidden, q_rows + 2 kv_rows, n_tokens, 1, ...) names -- and v is
 * bit-identical.  (Beyond head_dim 256 the rotating launch always takes the inputs-from-L2 kernel.)
 */
int quest_decode_norm_gemv(const void* x, const void* gamma, float eps, const void* w, void* out, uint32_t in_dim,
                           uint32_t out_dim, uint32_t dtype, quest_stream_t stream);
int quest_decode_norm_gemv_batched(const void* x, const void* gamma, float eps, const void* w, void* out, uint32_t in_dim,
                                   uint32_t out_dim, uint32_t n_tokens, uint32_t dtype, quest_stream_t stream);
int quest_decode_gemv_residual(const void* x, const void* w, void* h, uint32_t in_dim, uint32_t out_dim, uint32_t dtype,
                               quest_stream_t stream);
int quest_decode_gemv_residual_batched(const void* x, const void* w, void* h, uint32_t in_dim, uint32_t out_dim,
                                       uint32_t n_tokens, uint32_t dtype, quest_stream_t stream);
int quest_decode_mlp_gate_up(const void* h, const void* gamma, float eps, const void* w_gate, const void* w_up, void* act,
                             uint32_t hidden, uint32_t intermediate, uint32_t dtype, quest_stream_t stream);
int quest_decode_mlp_gate_up_batched(const void* h, const void* gamma, float eps, const void* w_gate, const void* w_up,
                                     void* act, uint32_t hidden, uint32_t intermediate, uint32_t n_tokens, uint32_t dtype,
                                     quest_stream_t stream);
int quest_decode_qkv_rope(const void* h, const void* gamma, float eps, const void* wq, const void* wk, const void* wv,
                          void* q, void* k, void* v, uint32_t hidden, uint32_t num_qo_heads, uint32_t num_kv_heads,
                          uint32_t head_dim, float rope_scale, float rope_theta, const float* inv_freq,
                          float attention_factor, const quest_step_state_t* state, uint32_t dtype, quest_stream_t stream);
int quest_decode_qkv_rope_batched(const void* h, const void* gamma, float eps, const void* wq, const void* wk,
                                  const void* wv, void* q, void* k, void* v, uint32_t hidden, uint32_t num_qo_heads,
                                  uint32_t num_kv_heads, uint32_t head_dim, float rope_scale, float rope_theta,
                                  const float* inv_freq, float attention_factor, const quest_step_state_t* states,
                                  uint32_t n_tokens, uint32_t dtype, quest_stream_t stream);
int quest_decode_qkv(const void* h, const void* gamma, float eps, const void* wq, const void* wk, const void* wv, void* q,
                     void* k, void* v, uint32_t hidden, uint32_t q_rows, uint32_t kv_rows, uint32_t dtype,
                     quest_stream_t stream);
int quest_decode_qkv_batched(const void* h, const void* gamma, float eps, const void* wq, const void* wk, const void* wv,
                             void* q, void* k, void* v, uint32_t hidden, uint32_t q_rows, uint32_t kv_rows,
                             uint32_t n_tokens, uint32_t dtype, quest_stream_t stream);

/*
 * ---- NOT PART OF THE STABLE SURFACE: introspection and overrides for benches, tests and tuning sweeps.  They may change
 * with the kernels they look into; an integration calls none of them.
 */

/* Introspection of the current plan (for benches/tests): pages per workgroup, workgroups per head. */
int quest_decode_plan_info(const quest_decode_handler_t* h, uint32_t* pages_per_chunk,
                           uint32_t* chunks_per_head);
/* Which kernel instantiation the handler's most recent per-head-list launch (quest_decode_forward*, fused or not) took:
 * info = {keys per thread of the fused top-k front end (0: index-tensor launch), waves per workgroup, front-end variant
 * (0 / 1 / 3: first generation with scalar / vector-fed staging arrays / keys straight into registers; 2: second
 * generation; 8: tiles -- the rows carry tile maxima; 7: the one-launch layer, quest_decode_layer_fused_batched), 1 if the
 * one-variant instantiation was launched (0: the generic kernel), workgroups per head, sequences}.  Tests and benches
 * assert with it that they run the kernel they mean to. */
int quest_decode_last_launch_info(const quest_decode_handler_t* h, uint32_t info[6]);
/* Developer aid: the handler's partial-state workspace ([sequences][heads][workgroups per head][record_floats] fp32:
 * acc[head_dim], m, d, spare).  Builds with -DQUEST_WALLSTAMPS leave per-workgroup wall-clock stamps in the spare words
 * (scripts/wallstamps.py). */
int quest_decode_debug_workspace(const quest_decode_handler_t* h, void** ptr, uint64_t* bytes, uint32_t* record_floats);
/* Measurement aid: with skip != 0, quest_decode_forward* launch only the attention kernel and leave the
 * per-workgroup partial states in the handler's workspace (the output tensor is NOT written when the plan has
 * more than one workgroup per head).  Lets a bench time the dominant kernel by itself. */
int quest_decode_set_skip_merge(quest_decode_handler_t* h, int skip);
/* Inspection aid for the state-driven / batched fused launches (quest_decode_forward_fused_topk_batched), which
 * otherwise keep the selected pages inside the kernel: while set, every such launch also writes its selection --
 * values (fp16 scores) to val_out and physical page ids to idx_out, both [n_seqs][num_qo_heads][n_selected_pages of
 * the plan] (rows of a sequence still shorter than the budget are filled up to its live page count).  NULL
 * pointers turn it off.  Not an entry the reference has: its top-k output lives in topk_filtering's tensors. */
int quest_decode_set_selection_out(quest_decode_handler_t* h, void* val_out, int32_t* idx_out);
/* Which top-k front end the fused launches use: 0 = automatic (by row length and alignment), 1 = first generation
 * (csrc/topk_select.cuh; rows up to 4096 pages), 2 = second generation (csrc/topk_bitmap.cuh; needs 8-byte aligned
 * score rows) without its histogram pre-filter, 3 = second generation with the pre-filter.  All are slot ownership and
 * implement the same selection: bit-identical page lists and outputs.  Tuning / test aid.  (The tiles front end is chosen
 * by the launch's tile_max_offset.  Round 4's column-range ownership and third generation measured
 * slower and were removed in round 5.) */
int quest_decode_set_front_end(quest_decode_handler_t* h, int generation);
/* Override the planner (0 = automatic).  Used by tuning sweeps. */
int quest_decode_set_pages_per_chunk(quest_decode_handler_t* h, uint32_t pages_per_chunk);

/* Which kernel an n-token launch of this shape takes (tests / tuning; nothing is launched): 1 and info = {k slices per
 * quad of rows, rounds, dynamic LDS bytes, workgroups, 128-wide k steps per row, weight fragments per set} for the persistent
 * kernel (inputs resident in LDS), 0 for the inputs-from-L2 kernel, < 0 for argument errors.  virtual_rows = output rows
 * of the launch (q + k + v rows; 2 x intermediate for the gate/up launch).  The plan does not depend on the element
 * type: fp16 and bf16 are both 16 bits wide, so a launch of either type takes the kernel named here. */
int quest_decode_batched_plan(uint32_t in_dim, uint32_t virtual_rows, uint32_t n_tokens, int rope, uint32_t info[6]);

/* Which workgroup tile an estimate launch of this shape takes (tests / tuning / the controllers' early check; host function,
 * no GPU, nothing is launched): 0 and info = {waves per workgroup (2 or 4), kv heads per tile (1, 2, 4 or 8), entries
 * (pages) per tile}, or the code every estimate entry returns for the shape -- QUEST_EINVAL (unknown layout, zero heads,
 * num_qo_heads not a multiple of num_kv_heads, info NULL), QUEST_EUNSUPPORTED (head_dim / group outside the built set, or a
 * refused shape: see quest_estimate_attn_score).  tiles != 0: the tiles form of quest_append_estimate_batched
 * (tile_max_offset != 0), whose tile must be a multiple of 8 entries wide.  It is the function the launch itself plans
 * with.  A tile scores `entries` consecutive pages of `kv heads` heads; its page-table entry is one scalar load when the
 * page size is a multiple of `entries`, else one load per row.  The plan does not depend on the element type. */
int quest_estimate_plan(uint32_t head_dim, uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t layout, int tiles,
                        uint32_t info[3]);

/*
 * SIGN PLANES: a shadow store of ONE layer's metadata pool for ONE single-sequence MHA cache (EXTENSION).  With one query
 * head per kv head the estimate needs, per (page, feature), max(Kslot, Vslot) where q >= 0 and min(Kslot, Vslot) where
 * q < 0 -- one of the pool's two fp16 values.  The planes hold both, taken with the estimate kernel's packed fp16 max / min
 * (so reversed slots, +-inf and NaN entries select what the pool launch selects), laid out
 *     [kv head][block of 256 logical pages][feature][sign: 0 = max, 1 = min][256 pages]     (fp16)
 * so that the pages of one (head, feature, sign) are contiguous in 512-byte runs and indexed by LOGICAL page: a launch reads
 * the run of the sign it needs -- half the bytes, no page table.  plane_pages = the page capacity of the store, a multiple
 * of 256 and >= every max_n_out it is used with; the buffer (16-byte aligned, caller-owned, contents arbitrary before the
 * build) has quest_estimate_planes_bytes bytes.
 * `covered` (one device int32 per layer, caller-owned, 0 = nothing) counts the leading logical pages whose plane entries
 * equal the pool's.  Only the two launches below write it.  Whoever changes the metadata of a page below `covered` by other
 * means (a cache set back to fewer pages, pool bytes rewritten) must lower it or build again.
 * Shapes served: n_seqs 1, num_qo_heads == num_kv_heads, head_dim 128, page size 16 on the KV and the metadata pool, fp16,
 * whole score rows (tile_max_offset 0) -- QUEST_EUNSUPPORTED otherwise, checked first and before anything is launched.
 */
uint64_t quest_estimate_planes_bytes(uint32_t num_kv_heads, uint32_t plane_pages);

/* Transpose the metadata of the sequence's complete pages -- state->n_pages - 1, plus the last page when
 * state->kv_last_page_len == kv_page_size; `state` must describe tokens that are in the pool -- into the planes and set
 * *covered to their number.  About one pass over the layer's metadata; run it once per request after the prefill. */
int quest_estimate_planes_build(void* planes, uint32_t plane_pages, int32_t* covered, quest_paged_kv_t metadata,
                                uint32_t kv_page_size, const quest_step_state_t* state, quest_stream_t stream);

/* quest_append_estimate_batched (whole rows) for the shapes above: same arguments, same score rows, same bits.  The append
 * blocks run the same append; when the token completes its page they also write the page's entry into the planes at logical
 * page n_pages - 1 and move *covered from n_pages - 1 to n_pages (never over a gap).  An estimate workgroup (kv head, 128
 * pages) reads the planes when its scored pages all lie below *covered and its head's q has no zero or non-finite element,
 * else the metadata pool -- so appends that do not maintain the planes (every other append entry) only leave *covered
 * behind, and every sequence of calls gives the pool launch's scores. */
int quest_append_estimate_planes_batched(const void* k, const void* v, quest_paged_kv_t kv, const void* q, void* o,
                                         uint32_t num_qo_heads, uint32_t o_stride, uint32_t max_n_out,
                                         uint32_t tile_max_offset, quest_paged_kv_t metadata,
                                         const quest_step_state_t* state, quest_batch_t batch, void* planes,
                                         uint32_t plane_pages, int32_t* covered, quest_stream_t stream);

/*
 * Token sampling on the device (EXTENSION; opt-in): the token choice that follows the lm_head launch, so that a captured
 * decode step needs no host round trip per token.  The reference samples on the host (the temperature / top-p / top-k
 * sampler with a stop token of its scripts/example_demo.py, model.generate of transformers elsewhere).
 *
 * THE CONTRACT, per row i (one row = one sequence); tests/_sampling_ref.py restates it in float64.
 *   Inputs: logits s[0..vocab) in the stored type (fp16 / bf16, converted exactly), temperature[i] (fp32), top_k[i] (int32),
 *   top_p[i] (fp32), seed[i] (uint64) and the position pos_i = the index the sampled token will occupy: states[i].seq_len
 *   (at the end of a state-driven step the state counts the token being decoded) or positions[i].
 *   Order: tokens are ordered by (16-bit key descending, token index ascending); the key is the monotone key of the page
 *   selection (sign-magnitude bits twiddled into an unsigned order; the same bit trick for bf16), so -0 < +0.
 *   Greedy rows: temperature == 0 (and any temperature that is not a positive finite number), a row that holds a NaN or
 *   +inf, a row whose maximum is -inf.  The token is the first in the order: ties go to the lowest index, a row of -inf
 *   gives token 0, among NaNs the largest key wins.  kept = 1.
 *   Sampled rows: with m = max s the mass of token j is w_j = exp((s_j - m) / T).  K1 = the first min(top_k, vocab) tokens
 *   of the order (top_k <= 0: all).  K2 = the shortest prefix of K1 whose mass is >= top_p * mass(K1) (top_p >= 1: K2 = K1;
 *   top_p <= 0 or NaN: the first token only).  kept = |K2|.  This is the order of transformers' warpers: temperature, then
 *   top-k, then top-p.  The reference's demo sampler filters top-p before top-k; the two differ only when both filters
 *   are active.
 *   Draw (Gumbel-max): token = argmax over j in K2 of z_j = (s_j - m) / T - log(-log(u_j)), ties to the earlier token of
 *   the order.  u_j = ((word >> 9) + 0.5) * 2^-23 (exact in fp32, never 0 or 1), word = output j & 3 of Philox4x32-10 with
 *   key (seed low, seed high) and counter (j >> 2, pos_i, 0x51554553, 0); multipliers 0xD2511F53 / 0xCD9E8D57, key bumps
 *   0x9E3779B9 / 0xBB67AE85 (Random123's philox4x32).
 *   Invariance: the draw depends on (seed, pos_i, j) only -- a sequence samples the same token alone, at any row of any
 *   batch, eagerly or from a replayed graph, bit for bit.  The top-k / top-p boundary is deterministic too: counts are
 *   integers, and a token's mass enters as the integer floor(expf((s_j - m) / T) * 2^40), a function of its key alone, so
 *   sums do not depend on their order.  Against the exact real-number boundary that is a relative error around 1e-6 of
 *   mass(K1); rows whose cut lies closer to top_p * mass(K1) than that may keep one token more or fewer than float64 says.
 *
 * ARGUMENTS.  logits: n_rows rows of `vocab` elements, logits_stride elements apart (>= vocab; rows need 2-byte alignment
 * only).  temperature / top_k / top_p / seed: device arrays of n_rows.  Exactly one of states (n_rows consecutive step
 * states) / positions (int32[n_rows]) is non-NULL.  tokens (int32[n_rows]) is written for every row and always lies in
 * [0, vocab); kept (int32[n_rows], may be NULL) receives |K2| (0 for a finished row).
 * Stop handling: finished (int32[n_rows], in/out, may be NULL), eos_ids (device int32[n_eos], n_eos <= 8), pad_id.  A row
 * whose flag is set emits pad_id, draws nothing and changes neither its flag nor its history; a row that samples an eos id
 * emits it and sets its flag.
 * History (optional, both or neither): history int32[n_rows][history_stride], history_len int32[n_rows] in/out -- the token
 * of an unfinished row is stored at history_len[i] when that is < history_stride and the length incremented; nothing is
 * written past a row.
 * Closing the loop (optional, both or neither): embed [vocab][hidden] and next_input [n_rows][hidden] in the stored type --
 * the row's workgroup copies embed[token] to next_input[i], so the launch feeds the next step's input.
 *
 * REFUSALS, before anything is launched and with every output untouched.  QUEST_EINVAL: a NULL required pointer, both or
 * neither of states / positions, vocab or n_rows 0, logits_stride < vocab, an odd logits address, pad_id or an eos id outside
 * [0, vocab), n_eos > 8, one of a pair (history / history_len, embed / next_input) without the other, an unknown dtype.
 * QUEST_EUNSUPPORTED: vocab > 2^18.  The eos ids are device memory: outside a stream capture the entry reads them back (one
 * wait on `stream`); while `stream` is capturing they cannot be read, and an id outside the vocabulary then simply matches
 * no token.
 * Not part of this entry: repetition penalty (it reorders the row, so the 16-bit key order no longer decides), min-p and
 * typical sampling, beam search, log-prob outputs, logits processors, tokenizers.
 */
int quest_sample_tokens(const void* logits, uint32_t logits_stride, uint32_t vocab, uint32_t n_rows, uint32_t dtype,
                        const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seed,
                        const quest_step_state_t* states, const int32_t* positions, int32_t* tokens, int32_t* kept,
                        const int32_t* eos_ids, uint32_t n_eos, int32_t pad_id, int32_t* finished, int32_t* history,
                        uint32_t history_stride, int32_t* history_len, const void* embed, uint32_t hidden, void* next_input,
                        quest_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* QUEST_HIP_H_ */
