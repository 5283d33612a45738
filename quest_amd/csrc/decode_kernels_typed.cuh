// shared_decode_kernel and merge_states_kernel, written ONCE and compiled once per element type: decode_kernels.cuh includes
// this file twice, with QUEST_ELEM = half_t / QUEST_KNAME(n) = n and with QUEST_ELEM = bf16_t / QUEST_KNAME(n) = n_bf16 (no
// include guard on purpose).  Why text and not a body template like sparse_decode_kernel's: these kernels ARE their bodies
// (lambdas over the by-value kernel parameters), and moving them into an inlined device function changed the fp16 kernels'
// code (fewer / more VGPRs, other unrolling) -- here the fp16 kernels compile from the text they always had.  T is the
// element type; everything they call (decode_device.cuh, append_device.cuh) is templated on it.
namespace quest {

// ------------------------------------------------------------------------------------------------
// Group-shared variant: all GS query heads of a kv head attend the SAME page list (full-KV decode: the
// model's dense first layers, contexts shorter than the budget).  One workgroup per (chunk, kv head)
// fetches each K/V tile once and folds it into GS online-softmax states, instead of once per query head
// as the per-head-list kernel above would (4x the traffic at Llama-3 GQA).  Same work split, same partial
// records, same merge kernel.
//
// APPEND (round 4): the decode append rides in the same launch.  The reference issues append_kv_cache_decode and the
// attention as two calls (QuestAttention.py:106 then :125-132, page.cu:6-99); here a dense layer of a captured step was
// three launches (append, attention, merge).  The new token's row of the current page is touched by exactly ONE
// workgroup per kv head -- the one whose chunk holds the last slot -- so that workgroup takes the row from the inputs
// instead of from the pool, writes it to the pool and folds the key into the page's (max, min) metadata entry
// (append_decode_body's arithmetic, same bits); nobody else reads or writes those bytes during the launch.
template <int D, int GS, int NW, bool APPEND = false>
__global__ __launch_bounds__(NW* kWave, NW / 2) void QUEST_KNAME(shared_decode_kernel)(QUEST_DECODE_HEAD_PARAMS, DecodeParams p) {
    using T = QUEST_ELEM;
    // MHA (one query head per kv head: registers to spare): the next page's rows are requested before the current page is
    // folded.  cfg 2: 14.35 -> 14.11 us per launch, 16.40 -> 16.20 per layer; the 32K dense launch 85.0 -> 84.4 us
    // (profiles/r05_ab_dense_kernel_prefetch.txt).
    constexpr bool PREFETCH = GS == 1;
    QUEST_DECODE_HEAD_TAKE(p);
    constexpr int LPR = D / kVec, R = kWave / LPR, S_T = 16, T_ = (S_T + R - 1) / R;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int row = lane / LPR, col = lane % LPR;
    // grid order (launch_shared): (chunks, kv heads) or, with the NHD pool, (kv heads, chunks) -- p.xcd_period != 0, the
    // preloaded field the per-head kernel uses for its own grid order -- so that workgroups adjacent in dispatch order read
    // the 256-byte pieces of the SAME token rows next to each other (a page's rows are 8 KiB of heads side by side)
    const bool heads_first = p.xcd_period != 0;
    const uint32_t chunk = heads_first ? blockIdx.y : blockIdx.x, hk = heads_first ? blockIdx.x : blockIdx.y;
    const SeqView sv = select_sequence(p, a_num_qo_heads, D, blockIdx.z);
    if (p.state) {  // state-driven launch: the plan (chunks) was made for the pool capacity; workgroups whose
                    // chunk lies past the live page list write an empty partial (weight 0 in the merge)
        const quest_step_state_t st = *sv.state;
        p.n_sel = (uint32_t)(st.n_pages - 1);
        p.last_page_len = (uint32_t)st.kv_last_page_len;
        p.last_page_idx = st.kv_last_page_idx;
        if constexpr (APPEND) {
            p.meta_last_page_len = (uint32_t)st.meta_last_page_len;
            p.meta_last_page_idx = st.meta_last_page_idx;
        }
    }
    const uint32_t n_slots = p.n_sel + 1;
    const uint32_t slot_begin = min(n_slots, chunk * p.pages_per_chunk);
    const uint32_t slot_end = min(n_slots, slot_begin + p.pages_per_chunk);

    float8 qv[GS];
#pragma unroll
    for (int g = 0; g < GS; ++g) {
        qv[g] = to_f32<T>(ld8(sv.q + ((size_t)hk * GS + g) * D + col * kVec));
        qv[g] *= p.scale_log2;
    }
    // page base + uni[t] + lane_off (+ v_off): the walk of quest_common.cuh (walk_*), the same for every pool layout
    const uint32_t lane_off = walk_lane_off(p.st, hk, R, row, col * kVec);
    const uint32_t v_off = pool_v_off(p.st, hk);
    uint32_t uni[T_];
#pragma unroll
    for (int t = 0; t < T_; ++t) uni[t] = walk_uniform(p.st, hk, R, t);
    RowState<D> st[GS];

    [[maybe_unused]] const size_t app_in_off = ((size_t)blockIdx.z * (a_num_qo_heads / GS) + hk) * D + col * kVec;
    // APPEND: the lanes (of the ONE wave per kv head that attends the current page) that hold the new token's row.  Their
    // metadata loads are issued here and consumed after the page loop; the stores come after the loop as well -- issued in
    // front of it they sat in the wave's vmcnt queue ahead of its K/V loads, whose first wait then also waited for the
    // write acknowledgements (measured: the fused launch lost its gain whenever the last chunk was long).
    [[maybe_unused]] bool app_mine = false;
    [[maybe_unused]] uint16_t* app_mmax = nullptr;
    [[maybe_unused]] ushort8 app_mx = (ushort8)(kElemNegMax<T>), app_mn = (ushort8)(kElemMax<T>);
    if constexpr (APPEND) {
        const uint32_t e = p.last_page_len - 1u;
        app_mine = slot_begin <= p.n_sel && p.n_sel < slot_end && (uint32_t)wave == (p.n_sel - slot_begin) % NW &&
                   (uint32_t)row == e % R;
        if (app_mine) {
            // metadata entry of the page: entry meta_last_page_len - 1 of the last metadata page (same pool geometry as
            // the KV pool); a token that opens a page starts from the sentinels, not from stale pool bytes
            const uint32_t me = p.meta_last_page_len - 1u;
            app_mmax = reinterpret_cast<uint16_t*>(p.app_meta) + (size_t)p.meta_last_page_idx * p.st.page +
                       (size_t)pool_slot(p.st, hk, me) * p.st.head + (size_t)me * p.st.entry + col * kVec;
            if (e > 0) {
                app_mx = *reinterpret_cast<const ushort8*>(app_mmax);
                app_mn = *reinterpret_cast<const ushort8*>(app_mmax + v_off);
            }
        }
    }

    // request the K/V rows of slot s0
    auto issue = [&](uint32_t s0, half8 (&k)[T_], half8 (&v)[T_]) {
        const int32_t pg = __builtin_amdgcn_readfirstlane(s0 < p.n_sel ? sv.indices[s0] : p.last_page_idx);
        const half_t* b0 = p.kv + (size_t)pg * p.st.page;
#pragma unroll
        for (int t = 0; t < T_; ++t) {
            k[t] = ld8_stream(b0 + uni[t] + lane_off);
            v[t] = ld8_stream(b0 + uni[t] + lane_off + v_off);
        }
    };
    // fold the rows of slot s0 into the GS states
    auto fold = [&](uint32_t s0, half8 (&k)[T_], half8 (&v)[T_]) {
        const int len = s0 < p.n_sel ? S_T : (int)p.last_page_len;
        if constexpr (APPEND) {
            if (s0 >= p.n_sel) {  // wave-uniform: the current page -- its newest row is the token being decoded, which is
                                  // not in the pool yet (written after this loop): it comes from the inputs
                const uint32_t e = (uint32_t)len - 1u;
                const half8 kn = ld8(p.app_k + app_in_off), vn = ld8(p.app_v + app_in_off);
#pragma unroll
                for (int t = 0; t < T_; ++t)
                    if ((uint32_t)(t * R + row) == e) {
                        k[t] = kn;
                        v[t] = vn;
                    }
            }
        }
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
    if constexpr (PREFETCH) {
        // the next page's rows are requested before the current page is folded (two register sets, 16 loads in flight per
        // lane); same pages in the same order per wave, hence the same bits.  Straight-line issue -> fold segments: a load
        // under a branch would be waited for at the join
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

    if constexpr (APPEND) {
        if (app_mine) {  // write the new token to the pool and fold its key into the page's (max, min) entry
            const uint32_t e = p.last_page_len - 1u;
            const half8 kn = ld8(p.app_k + app_in_off), vn = ld8(p.app_v + app_in_off);
            half_t* dst = const_cast<half_t*>(p.kv) + (size_t)p.last_page_idx * p.st.page + lane_off + walk_uniform(p.st, hk, R, e / R);
            st8(dst, kn);
            st8(dst + v_off, vn);
            const ushort8 k8 = __builtin_bit_cast(ushort8, kn);
            *reinterpret_cast<ushort8*>(app_mmax) = fold_max<T>(app_mx, k8);
            *reinterpret_cast<ushort8*>(app_mmax + v_off) = fold_min<T>(app_mn, k8);
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
    for (uint32_t t = threadIdx.x; t < (uint32_t)(GS * D); t += NW * kWave) {
        const uint32_t g = t / D, f = t % D, hq = hk * GS + g;
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
            sv.o[(size_t)hq * D + f] = from_f32<T>(acc / den);
            if (p.lse && f == 0) sv.lse[hq] = (M + __builtin_amdgcn_logf(den)) * 0.6931471805599453f;
        } else {
            float* w = sv.ws + ((size_t)hq * p.n_chunks + chunk) * p.ws_stride;
            w[f] = acc;
            if (f == 0) {
                w[D] = M;
                w[D + 1] = den;
            }
        }
    }
}
// Merge the per-chunk partial states of a head, normalise, cast to fp16 (the job of flashinfer's
// VariableLengthMergeStates).  kMergeGroups thread groups each take every kMergeGroups-th chunk with all of
// their loads independent (unrolled), then combine through LDS: two memory round trips total.
// Merging INSIDE the attention launch (the workgroup of a head that draws the last arrival ticket merges; partial
// records leave by write-through stores) was built twice -- round 1, and round 3 with the recipe of VERDICT r2 item 1a
// -- bit-identical and slower: every workgroup's tail gains a store acknowledgement and an atomic round trip that
// queue behind the launch's own streaming reads.  Same box, us per launch incl. merge: cfg 3 14.7 (this launch) vs
// 22.4 (in-kernel), cfg 2 17.7 vs 20.6, cfg 4 23.8 vs 26.9 (gpurun_out/r3a_*).
// (the partial records are fp32 whatever the element type: only the final cast differs)
template <int D>
__global__ __launch_bounds__(D* kMergeGroups) void QUEST_KNAME(merge_states_kernel)(const float* __restrict__ ws,
                                                                                     half_t* __restrict__ o,
                                                                                     float* __restrict__ lse, uint32_t n_chunks,
                                                                                     uint32_t ws_stride, StepAdvance adv) {
    using T = QUEST_ELEM;
    __shared__ float s_w[1024];  // per-chunk weight exp2(m_c - M); planner keeps n_chunks <= 1024
    __shared__ float s_red[kMergeGroups][D + 1];
    __shared__ float s_M;
    const uint32_t hq = blockIdx.x, tid = threadIdx.x;
    const uint32_t f = tid % D, g = tid / D;
    const float* w = ws + (size_t)hq * n_chunks * ws_stride;
    // the next step's reservation (StepAdvance, append_device.cuh): nothing in or after this launch reads the state
    if (adv.st && hq == 0 && tid < adv.batch.n_seqs)
        step_state_advance_one(adv.st + tid, adv.kv_table + (size_t)tid * adv.batch.kv_table_stride,
                               adv.meta_table + (size_t)tid * adv.batch.meta_table_stride, adv.page_size, adv.max_kv_pages,
                               adv.max_meta_pages);
    if (n_chunks <= kMergeFastChunks) {  // launch-uniform
        merge_head_fast<T, D, D * kMergeGroups>(w, o + (size_t)hq * D, lse ? lse + hq : nullptr, n_chunks, ws_stride, tid,
                                                    &s_red[0][0]);
        return;
    }
    // the first kPre partial rows of this thread's chunks are requested up front
    constexpr int kPre = kMergePre;
    float pre[kPre];
#pragma unroll
    for (int j = 0; j < kPre; ++j) {
        const uint32_t c = g + j * kMergeGroups, cc = c < n_chunks ? c : n_chunks - 1;  // clamped: no branch
        pre[j] = w[(size_t)cc * ws_stride + f];
    }
    // pass 1: chunk maxima -> M, weights, denominator
    float M = kNegFloor;
    for (uint32_t c = tid; c < n_chunks; c += blockDim.x) M = __builtin_fmaxf(M, w[(size_t)c * ws_stride + D]);
    M = wave_allreduce_max(M, (int)(tid & 63));
    if ((tid & 63) == 0) s_red[0][tid >> 6] = M;
    __syncthreads();
    if (tid == 0) {
        float mm = s_red[0][0];
        for (uint32_t i = 1; i < (blockDim.x >> 6); ++i) mm = __builtin_fmaxf(mm, s_red[0][i]);
        s_M = mm;
    }
    __syncthreads();
    M = s_M;
    float den = 0.f;
    for (uint32_t c = tid; c < n_chunks; c += blockDim.x) {
        const float e = __builtin_amdgcn_exp2f(w[(size_t)c * ws_stride + D] - M);
        s_w[c] = e;
        den += e * w[(size_t)c * ws_stride + D + 1];
    }
    __syncthreads();
    // pass 2: weighted sum of the partial outputs
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < kPre; ++j) {
        const uint32_t c = g + j * kMergeGroups;
        if (c < n_chunks) acc += s_w[c] * pre[j];
    }
#pragma unroll 8
    for (uint32_t c = g + kPre * kMergeGroups; c < n_chunks; c += kMergeGroups)
        acc += s_w[c] * w[(size_t)c * ws_stride + f];
    den = wave_allreduce_sum(den, (int)(tid & 63));
    s_red[g][f] = acc;
    __shared__ float s_den[16];
    if ((tid & 63) == 0) s_den[tid >> 6] = den;
    __syncthreads();
    if (g == 0) {
        float a = s_red[0][f];
#pragma unroll
        for (int j = 1; j < kMergeGroups; ++j) a += s_red[j][f];
        float dn = 0.f;
        for (uint32_t i = 0; i < (blockDim.x >> 6); ++i) dn += s_den[i];
        o[(size_t)hq * D + f] = from_f32<T>(a / dn);
        if (lse && f == 0) lse[hq] = (M + __builtin_amdgcn_logf(dn)) * 0.6931471805599453f;
    }
}

}  // namespace quest
