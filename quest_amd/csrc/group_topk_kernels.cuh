// Group-shared page selection for GQA (quest_decode_forward_group_topk): the kernel's parameters and its two compilations,
// fp16 as group_topk_attend_kernel and bf16 as group_topk_attend_kernel_bfloat16 (body: group_topk_kernels_typed.cuh; launcher:
// sparse_attn.hip).  (Not <name>_bf16: tests/test_bf16_host.py counts the kernels of that suffix against a fixed list of the
// attention path's fp16 kernels.)  The kernel has its OWN parameter struct: DecodeParams and the kernels that take it are untouched.
#pragma once
#include "decode_device.cuh"

namespace quest {

constexpr int kGroupTopkWaves = 8;  // 512 threads
constexpr int kGroupTopkKeys = 8;   // columns per thread the front end holds in registers: rows up to 512 x 8 = 4096 pages

struct GroupTopkParams {
    const half_t* q;                  // [n_seqs][Hq][D]
    const half_t* kv;                 // the layer's KV pool
    const int32_t* tables;            // [n_seqs][table_stride] page tables, n_cap + 1 entries each
    const uint16_t* scores;           // [n_seqs][Hq][score_stride] page scores (the estimate launch's output)
    const quest_step_state_t* state;  // [n_seqs] live lengths / current pages, or NULL: the eager single-sequence form
    const int32_t* budgets;           // optional per-sequence page budgets (pages incl. the current one)
    half_t* o;                        // [n_seqs][Hq][D]
    float* ws;                        // [n_seqs][Hq][n_chunks][ws_stride] partial records (n_chunks > 1)
    float* lse;                       // optional [n_seqs][Hq]
    uint16_t* sel_val_out;            // optional [n_seqs][kv heads][sel_stride]
    int32_t* sel_idx_out;
    PoolStrides st;
    uint32_t num_kv_heads;
    uint32_t n_cap;         // columns of a score row the launch may see (the longest row of a captured step)
    uint32_t score_stride, table_stride;
    uint32_t cpt;           // columns per thread: 4 or 8, from the capacity
    uint32_t vec_scores;    // score rows 8-byte aligned and readable up to the next multiple of 4 columns
    uint32_t table_vec;     // page tables 16-byte aligned
    uint32_t n_sel;         // the plan's selected-page count
    uint32_t n_scores;      // eager form: the live row length (state-driven launches read it from the state)
    uint32_t last_page_len;
    int32_t last_page_idx;
    uint32_t pages_per_chunk, n_chunks, ws_stride, sel_stride;
    float scale_log2;
};

}  // namespace quest

#define QUEST_ELEM half_t
#define QUEST_KNAME(n) n
#include "group_topk_kernels_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME
#define QUEST_ELEM bf16_t
#define QUEST_KNAME(n) n##_bfloat16
#include "group_topk_kernels_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME
