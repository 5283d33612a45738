// group_topk_attend_kernel, written ONCE and compiled once per element type: group_topk_kernels.cuh includes this file twice,
// with QUEST_ELEM = half_t / QUEST_KNAME(n) = n and with QUEST_ELEM = bf16_t / QUEST_KNAME(n) = n_bfloat16 (no include guard on
// purpose), the way decode_kernels_typed.cuh is compiled.
namespace quest {

// ------------------------------------------------------------------------------------------------
// Group-shared page selection (opt-in; NOT the reference's algorithm, which selects per query head:
// evaluation/quest_attention.py:139-140): ONE selection per kv head, attended by all GS query heads of its group.
//   group score of page p = max over the group's heads of the 16-bit order-preserving keys of score[hk * GS + g][p]
//   selection            = the contract of topk_select.cuh on that row (k = min(budget - 1, pages - 1), keys above the
//                          threshold plus the lowest columns among ties, ascending column order)
//   attention            = every head of the group over those pages + the current page
// One workgroup per (chunk, kv head, sequence).  Front end: thread t owns the contiguous columns [t cpt, t cpt + cpt) of
// the GS score rows (L2-resident), folds them to one key per column and runs the shared selection routine; columns whose
// output slot falls in the workgroup's chunk drop their physical page id into an LDS list.  All workgroups of a kv head
// repeat the selection instead of waiting for one another.  Gather: the issue / fold structure of the
// group-shared full-KV kernel (decode_kernels_typed.cuh) -- each K/V tile is fetched once and folded into GS
// online-softmax states -- with the page taken from the LDS list, or the current page for the last slot.
// Same partial records and merge launch as the other attention kernels.
template <int D, int GS, int NW>
__global__ __launch_bounds__(NW* kWave, 2) void QUEST_KNAME(group_topk_attend_kernel)(GroupTopkParams p) {
    using T = QUEST_ELEM;
    constexpr int NT = NW * kWave, FC = kGroupTopkKeys;
    constexpr int LPR = D / kVec, R = kWave / LPR, S_T = 16, T_ = (S_T + R - 1) / R;
    constexpr bool PREFETCH = GS == 1;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int row = lane / LPR, col = lane % LPR;
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = blockIdx.x, hk = blockIdx.y, seq = blockIdx.z;
    const uint32_t num_qo_heads = p.num_kv_heads * GS;
    // the sequence's operands: rows of the batched tensors ([n_seqs][Hq][...]); the pools are shared
    const size_t head_row = (size_t)seq * num_qo_heads + (size_t)hk * GS;
    const half_t* q_rows = p.q + head_row * D;
    const uint16_t* srow = p.scores + head_row * p.score_stride;
    const int32_t* table = p.tables + (size_t)seq * p.table_stride;

    // ---- front-end loads: their addresses depend on the row CAPACITY only, not on the live lengths below
    const uint32_t n_cap = p.n_cap, cpt = p.cpt, c0 = tid * cpt, cc = c0 < n_cap ? c0 : 0u;
    const int4 live = *(p.state ? reinterpret_cast<const int4*>(p.state + seq)
                                : reinterpret_cast<const int4*>(p.q));  // seq_len, n_pages, kv_last_page_len, kv_last_page_idx
    uint32_t key[FC];
#pragma unroll
    for (int i = 0; i < FC; ++i) key[i] = 0u;  // below every key of a finite, infinite or NaN score
    if (p.vec_scores) {  // launch-uniform: 8-byte aligned rows, readable up to the next multiple of 4 columns
        const uint32_t cc2 = (cpt == 8u && cc + 4u < n_cap) ? cc + 4u : cc;  // (a repeat is masked: its columns are >= n)
#pragma unroll
        for (int g = 0; g < GS; ++g) {
            const uint2 lo = *reinterpret_cast<const uint2*>(srow + (size_t)g * p.score_stride + cc);
            const uint2 hi = *reinterpret_cast<const uint2*>(srow + (size_t)g * p.score_stride + cc2);
            const uint32_t w[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
            for (int i = 0; i < FC; ++i) {
                const uint32_t k = half_key((uint16_t)((i & 1) ? w[i >> 1] >> 16 : w[i >> 1] & 0xffffu));
                key[i] = key[i] > k ? key[i] : k;
            }
        }
    } else {
#pragma unroll
        for (int g = 0; g < GS; ++g) {
#pragma unroll
            for (int i = 0; i < FC; ++i) {
                const uint32_t c = cc + (uint32_t)i, ci = ((uint32_t)i < cpt && c < n_cap) ? c : cc;
                const uint32_t k = half_key(srow[(size_t)g * p.score_stride + ci]);
                key[i] = key[i] > k ? key[i] : k;
            }
        }
    }
    // the page ids of the thread's own columns (the table has n_cap + 1 entries)
    uint32_t ids[FC];
    {
        const uint32_t table_len = n_cap + 1u, last = n_cap;
#pragma unroll
        for (int v = 0; v < FC / 4; ++v) {
            const uint32_t c = cc + 4u * v;
            if (p.table_vec && (uint32_t)(4 * v) < cpt && c + 4u <= table_len) {
                const uint4 q4 = *reinterpret_cast<const uint4*>(table + c);
                ids[4 * v] = q4.x, ids[4 * v + 1] = q4.y, ids[4 * v + 2] = q4.z, ids[4 * v + 3] = q4.w;
            } else if ((uint32_t)(4 * v) < cpt) {  // unaligned tables, or the tail of a table whose length is not a multiple of 4
#pragma unroll
                for (int j = 0; j < 4; ++j) ids[4 * v + j] = (uint32_t)table[c + j < last ? c + j : last];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) ids[4 * v + j] = 0u;
            }
        }
    }
    __shared__ TopkSmem<NT> sm;
    __shared__ int32_t s_sel[kFusedMaxPpc];
    topk_clear<NT>(sm);  // under the loads above
    const int32_t budget_raw = ld_uniform_i32(p.budgets ? p.budgets + seq : reinterpret_cast<const int32_t*>(p.q));

    // ---- live lengths: from the step state (state-driven), else as launched
    uint32_t n = p.n_scores, n_sel = p.n_sel, last_page_len = p.last_page_len;
    int32_t last_page_idx = p.last_page_idx;
    if (p.state) {
        n = (uint32_t)(live.y - 1);
        last_page_len = (uint32_t)live.z;
        last_page_idx = live.w;
        if (p.budgets) n_sel = min(n_sel, (uint32_t)max(budget_raw - 1, 0));
        n_sel = min(n_sel, n);  // a sequence shorter than its budget attends all of its pages
    }
    const uint32_t n_slots = n_sel + 1;
    const uint32_t slot_begin = min(n_slots, chunk * p.pages_per_chunk);
    const uint32_t slot_end = min(n_slots, slot_begin + p.pages_per_chunk);

    // ---- selection (block-uniform: workgroups that hold no selected slot -- past the live list, or the current page
    // alone -- skip it)
    if (slot_begin < n_sel) {
        uint32_t mm = kMmNeutral;
#pragma unroll
        for (int i = 0; i < FC; ++i)
            if ((uint32_t)i < cpt && c0 + i < n) mm = pk_max_u16(mm, mm_pack(key[i]));
        topk_publish_range<NT>(sm, mm);
        __syncthreads();
        TopkCursor cur = topk_select<NT, FC>(sm, key, n, n_sel, cpt);
        uint32_t my_slot[FC];
        bool mine[FC];
#pragma unroll
        for (int i = 0; i < FC; ++i) {
            uint32_t slot;
            mine[i] = topk_take(cur, key[i], (uint32_t)i < cpt && c0 + i < n, slot) && slot >= slot_begin && slot < slot_end;
            my_slot[i] = slot;
            if (mine[i]) s_sel[slot - slot_begin] = (int32_t)ids[i];
        }
        __syncthreads();
        // optional copy of the selection ([n_seqs][kv heads][sel_stride]): after the barrier, so that nobody waits on
        // these stores before fetching K/V; every workgroup writes the slots of its own chunk
        if (p.sel_idx_out) {
            const size_t out_row = ((size_t)seq * p.num_kv_heads + hk) * p.sel_stride;
#pragma unroll
            for (int i = 0; i < FC; ++i)
                if (mine[i]) {
                    p.sel_idx_out[out_row + my_slot[i]] = (int32_t)ids[i];
                    if (p.sel_val_out) p.sel_val_out[out_row + my_slot[i]] = key_to_half_bits(key[i]);
                }
        }
    }

    // ---- gather: GS states, each K/V tile fetched once
    float8 qv[GS];
#pragma unroll
    for (int g = 0; g < GS; ++g) {
        qv[g] = to_f32<T>(ld8(q_rows + (size_t)g * D + col * kVec));
        qv[g] *= p.scale_log2;
    }
    const uint32_t lane_off = walk_lane_off(p.st, hk, R, row, col * kVec);
    const uint32_t v_off = pool_v_off(p.st, hk);
    uint32_t uni[T_];
#pragma unroll
    for (int t = 0; t < T_; ++t) uni[t] = walk_uniform(p.st, hk, R, t);
    RowState<D> st[GS];

    auto issue = [&](uint32_t s0, half8 (&k)[T_], half8 (&v)[T_]) {
        const int32_t pg = __builtin_amdgcn_readfirstlane(s0 < n_sel ? s_sel[s0 - slot_begin] : last_page_idx);
        const half_t* b0 = p.kv + (size_t)pg * p.st.page;
#pragma unroll
        for (int t = 0; t < T_; ++t) {
            k[t] = ld8_stream(b0 + uni[t] + lane_off);
            v[t] = ld8_stream(b0 + uni[t] + lane_off + v_off);
        }
    };
    auto fold = [&](uint32_t s0, half8 (&k)[T_], half8 (&v)[T_]) {
        const int len = s0 < n_sel ? S_T : (int)last_page_len;
        float8 kf[T_], vf[T_];
        bool valid[T_];
#pragma unroll
        for (int t = 0; t < T_; ++t) {
            valid[t] = row < len - t * R;
            kf[t] = to_f32<T>(k[t]);
            vf[t] = valid[t] ? to_f32<T>(v[t]) : (float8)(0.f);  // stale rows past the page length: select
        }
#pragma unroll
        for (int g = 0; g < GS; ++g) {
            float sc[T_];
            float m_new = st[g].m;
#pragma unroll
            for (int t = 0; t < T_; ++t) {
                float dot = 0.f;
#pragma unroll
                for (int i = 0; i < kVec; ++i) dot = __builtin_fmaf(qv[g][i], kf[t][i], dot);
                dot = row_allreduce_sum_fast<LPR>(dot);
                sc[t] = valid[t] ? dot : kNegFloor;
                m_new = __builtin_fmaxf(m_new, sc[t]);
            }
            const float scale = __builtin_amdgcn_exp2f(st[g].m - m_new);
            st[g].d *= scale;
            st[g].acc *= scale;
#pragma unroll
            for (int t = 0; t < T_; ++t) {
                const float pr = valid[t] ? __builtin_amdgcn_exp2f(sc[t] - m_new) : 0.f;
                st[g].d += pr;
#pragma unroll
                for (int i = 0; i < kVec; ++i) st[g].acc[i] = __builtin_fmaf(pr, vf[t][i], st[g].acc[i]);
            }
            st[g].m = m_new;
        }
    };
    if constexpr (PREFETCH) {  // one head per kv head (registers to spare): the next page is requested before this one is folded
        uint32_t s0 = slot_begin + wave;
        if (s0 < slot_end) {
            half8 k0[T_], v0[T_], k1[T_], v1[T_];
            issue(s0, k0, v0);
            while (true) {
                uint32_t s1 = s0 + NW;
                if (s1 >= slot_end) {
                    fold(s0, k0, v0);
                    break;
                }
                issue(s1, k1, v1);
                fold(s0, k0, v0);
                s0 = s1 + NW;
                if (s0 >= slot_end) {
                    fold(s1, k1, v1);
                    break;
                }
                issue(s0, k0, v0);
                fold(s1, k1, v1);
            }
        }
    } else {
        for (uint32_t s0 = slot_begin + wave; s0 < slot_end; s0 += NW) {
            half8 k[T_], v[T_];
            issue(s0, k, v);
            fold(s0, k, v);
        }
    }

    __shared__ float s_acc[NW][GS][D];
    __shared__ float s_md[NW][GS][2];
#pragma unroll
    for (int g = 0; g < GS; ++g) {
        for_each_row_distance<LPR>([&](auto off_c) {  // rows of the wave -> one state
            constexpr int OFF = decltype(off_c)::value;
            const float m_o = lane_xor<OFF>(st[g].m, lane), d_o = lane_xor<OFF>(st[g].d, lane);
            const float m_n = __builtin_fmaxf(st[g].m, m_o);
            const float a = __builtin_amdgcn_exp2f(st[g].m - m_n), b = __builtin_amdgcn_exp2f(m_o - m_n);
            st[g].d = st[g].d * a + d_o * b;
#pragma unroll
            for (int i = 0; i < kVec; ++i) st[g].acc[i] = st[g].acc[i] * a + lane_xor<OFF>(st[g].acc[i], lane) * b;
            st[g].m = m_n;
        });
        if (row == 0) {
#pragma unroll
            for (int i = 0; i < kVec; ++i) s_acc[wave][g][col * kVec + i] = st[g].acc[i];
            if (col == 0) {
                s_md[wave][g][0] = st[g].m;
                s_md[wave][g][1] = st[g].d;
            }
        }
    }
    __syncthreads();
    half_t* o_rows = p.o + head_row * D;
    float* ws_rows = p.ws + head_row * p.n_chunks * p.ws_stride;  // only dereferenced when n_chunks > 1
    for (uint32_t t = tid; t < (uint32_t)(GS * D); t += NT) {
        const uint32_t g = t / D, f = t % D;
        float M = s_md[0][g][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) M = __builtin_fmaxf(M, s_md[w][g][0]);
        float acc = 0.f, den = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float e = __builtin_amdgcn_exp2f(s_md[w][g][0] - M);
            acc += e * s_acc[w][g][f];
            den += e * s_md[w][g][1];
        }
        if (p.n_chunks == 1) {
            o_rows[(size_t)g * D + f] = from_f32<T>(acc / den);
            if (p.lse && f == 0) p.lse[head_row + g] = (M + __builtin_amdgcn_logf(den)) * 0.6931471805599453f;
        } else {
            float* w = ws_rows + ((size_t)g * p.n_chunks + chunk) * p.ws_stride;
            w[f] = acc;
            if (f == 0) {
                w[D] = M;
                w[D + 1] = den;
            }
        }
    }
}

}  // namespace quest
