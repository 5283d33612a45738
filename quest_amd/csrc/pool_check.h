// Host-side checks of the paged pools a launch is given (append.hip, estimate.hip, sparse_attn.hip).
#pragma once
#include "../../include/quest_hip.h"

namespace quest {

int check_pool(const quest_paged_kv_t& p);  // append.hip

// Element type of a launch (quest_paged_kv_t.dtype: QUEST_DTYPE_F16 / QUEST_DTYPE_BF16): q, k, v, o and the scores have the
// type of the pool view(s) they come with.  An unknown value, or two views of one call that disagree, is QUEST_EINVAL --
// checked first, before any other argument and before any launch.
inline int check_dtype(const quest_paged_kv_t& p) { return p.dtype <= QUEST_DTYPE_BF16 ? 0 : QUEST_EINVAL; }
inline int check_dtype_pair(const quest_paged_kv_t& a, const quest_paged_kv_t& b) {
    return a.dtype <= QUEST_DTYPE_BF16 && a.dtype == b.dtype ? 0 : QUEST_EINVAL;
}

inline bool same_pool_geometry(const quest_paged_kv_t& a, const quest_paged_kv_t& b) {
    return a.layout == b.layout && a.head_dim == b.head_dim && a.page_size == b.page_size && a.num_heads == b.num_heads;
}

// The KV pool and the metadata pool of one launch.  state_driven: the kernel reads the live page lengths from the step
// state, the fields get placeholders.  shared_strides: the launch addresses the metadata pool with the KV pool's strides
// (same layout and page size required, not only the same heads and head_dim).
inline int check_pool_pair(quest_paged_kv_t& kv, quest_paged_kv_t& metadata, bool state_driven, bool shared_strides) {
    if (state_driven) kv.last_page_len = metadata.last_page_len = 1;
    if (int e = check_pool(kv)) return e;
    if (int e = check_pool(metadata)) return e;
    if (kv.dtype != metadata.dtype) return QUEST_EINVAL;
    if (kv.num_heads != metadata.num_heads || kv.head_dim != metadata.head_dim) return QUEST_EINVAL;
    if (shared_strides && !same_pool_geometry(kv, metadata)) return QUEST_EINVAL;
    return 0;
}

}  // namespace quest
