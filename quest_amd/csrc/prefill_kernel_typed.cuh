// prefill_kernel, written ONCE and compiled once per element type: prefill.hip includes this file twice, with QUEST_ELEM =
// half_t / QUEST_KNAME(n) = n and with QUEST_ELEM = bf16_t / QUEST_KNAME(n) = n_bf16 (no include guard on purpose).  The
// kernel is its body (lambdas over the kernel parameter): as an inlined body template its fp16 code came out differently
// (other unrolling of the tile loop); from this text the fp16 kernels compile as they always did.
namespace quest {

// Two 32-row blocks per wave (256-row workgroups, one wave per SIMD, each K / V fragment feeding two MFMAs) was built and
// measured: 0.65-0.69 against 0.84-0.91 PFLOP/s -- hipcc keeps the second set of accumulators in AGPRs and copies them to
// and from VGPRs around every vector instruction (1250 v_accvgpr moves per two tiles).
//
// D = 64 / 128: two LDS buffers (32 / 64 KiB), two workgroups per CU.  D = 256: the output accumulators alone are 128
// registers, so one wave per SIMD and ONE 64 KiB buffer (a second barrier per tile instead of the second buffer).
template <int D, bool S16>
__global__ __launch_bounds__(256, D <= 128 ? 2 : 1) void QUEST_KNAME(prefill_kernel)(const PrefillParams p) {
    using T = QUEST_ELEM;
    constexpr uint32_t IMG = kPfKeys * 2 * D;        // bytes of one K (or V) tile image
    constexpr uint32_t BUFB = 2 * IMG;               // one buffer: K image then V image
    constexpr int NBUF = D <= 128 ? 2 : 1;
    constexpr uint32_t CPR = D / 8;                  // 16-byte chunks per row
    constexpr uint32_t RP = 256 / CPR;               // rows staged per pass of the 256 threads
    constexpr int NP = kPfKeys / RP;                 // passes per tile
    __shared__ __attribute__((aligned(16))) unsigned char s_img[NBUF * BUFB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;

    // workgroup -> (head, query block): the heads of an XCD are neighbours (a GQA group shares its K/V through one L2),
    // and the query blocks with the most keys under the causal mask are dispatched first
    uint32_t head, qblk;
    {
        const uint32_t id = blockIdx.x;
        if ((p.num_qo_heads & 7u) == 0) {
            const uint32_t hpx = p.num_qo_heads >> 3, slot = id >> 3;
            head = (id & 7u) * hpx + slot % hpx;
            qblk = slot / hpx;
        } else {
            head = id % p.num_qo_heads;
            qblk = id / p.num_qo_heads;
        }
        qblk = p.q_blocks - 1 - qblk;
    }
    const uint32_t kv_head = head / p.group;
    const uint32_t q0 = qblk * kPfRows, q0w = q0 + wave * 32;
    const uint32_t last_q = p.n_q - 1, last_key = p.kv_len - 1;
    const uint32_t shift = p.kv_len - p.n_q;  // query i sees keys <= shift + i (causal)
    const uint32_t limit = p.causal ? shift + min(q0w + r, last_q) : last_key;        // this lane's query
    const uint32_t limit_lo = p.causal ? shift + min(q0w, last_q) : last_key;         // first query of the wave (uniform)
    const uint32_t limit_hi = p.causal ? shift + min(q0w + 31, last_q) : last_key;    // last query of the wave
    const uint32_t limit_wg = p.causal ? shift + min(q0 + kPfRows - 1, last_q) : last_key;
    const uint32_t n_tiles = limit_wg / kPfKeys + 1;
    const bool wave_live = q0w < p.n_q;

    // Q^T fragments (B operand): lane (r, h) holds q[row r][16 s + 8 h ..] of k-step s.  Unscaled: the reference folds
    // log2(e) / sqrt(D) into q in fp16 (prefill.cuh:758), which rounds every score by up to 2^-11 of its terms -- 4e-3 of
    // an output once |score| reaches ~100; here the factor multiplies the fp32 score on its way into the exponent.
    // Rows past the end of q repeat the last row (computed, never stored).
    half8 qf[D / 16];
    {
        const half_t* qrow = p.q + ((size_t)min(q0w + r, last_q) * p.num_qo_heads + head) * D + 8 * h;
#pragma unroll
        for (int s = 0; s < D / 16; ++s) qf[s] = ld8(qrow + 16 * s);
    }

    // LDS addresses, loop-invariant up to immediates (buffer, key block, k-step pair, 16-key step, d-block): every read
    // below is `register + constant`, no address arithmetic in the loop
    const uint32_t lds0 = (uint32_t)(uintptr_t)(QUEST_LDS unsigned char*)s_img;
    // K row read of k-step s: row 32 kb + r, chunk 2 s + h = subtile s >> 1, chunk 2 (s & 1) + h of it
    const uint32_t ka[2] = {lds0 + img_off<D>(r, h), lds0 + img_off<D>(r, 2 + h)};
    // V transposed read of d-block db, half u of 16-key step s: rows 16 s + 8 u + 4 h + tq, 16-lane group tg = the d half,
    // lane 4 tq + tp of the group supplies row tq, columns 4 tp .. 4 tp + 3 of the block
    const uint32_t tg = (lane >> 4) & 1u, tq = (lane & 15u) >> 2, tp = lane & 3u;
    const uint32_t va[2] = {lds0 + IMG + img_off<D>(4 * h + tq, 2 * tg + (tp >> 1)) + 8 * (tp & 1u),
                            lds0 + IMG + img_off<D>(8 + 4 * h + tq, 2 * tg + (tp >> 1)) + 8 * (tp & 1u)};

    // staging: thread -> chunk sch of rows srow + RP i of a tile.  Four lanes take the four chunks of a subtile row, the
    // next lanes the next ROW of the same subtile: a wave writes whole 512-byte subtiles (no bank conflict on the
    // ds_write_b128) and still reads 128 contiguous bytes of each of its 8 rows from memory.
    constexpr uint32_t SUB = CPR / 4;  // subtiles per 8-row group
    const uint32_t srow = 8u * (tid / (32u * SUB)) + ((tid >> 2) & 7u), sch = 4u * ((tid >> 5) % SUB) + (tid & 3u);
    uint32_t wa[NP];  // (for RP = 16 / 32 the passes differ by a constant)
#pragma unroll
    for (int i = 0; i < NP; ++i) wa[i] = lds0 + img_off<D>(srow + RP * i, sch);
    // address of (page, entry, kv head) = pool + page * st.page + entry * st.entry + pool_slot(head, entry) * st.head: on the
    // row-rotated pool (QUEST_LAYOUT_NHD_ROT) the head's slot depends on the entry, so the head term is per lane
    const unsigned char* kv_base = reinterpret_cast<const unsigned char*>(p.kv);
    const uint32_t v_bytes = pool_v_off(p.st, kv_head) * 2u;
    auto issue = [&](uint32_t t, half8(&kr)[NP], half8(&vr)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t row = srow + RP * i;
            if constexpr (S16) {
                // one page per 16-row group -- the same one for every lane of a wave --, its id a scalar load; rows past the
                // end of the sequence read stale slots of the last page (inside the pool): their scores are masked, their
                // V rows zeroed below
                const uint32_t pi = t * 4 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(row >> 4));
                const uint32_t pg = (uint32_t)ld_uniform_i32(p.table + min(pi, last_key >> 4));
                const unsigned char* src = kv_base + (size_t)pg * p.st.page * 2u;
                const uint32_t lane_bytes = ((row & 15u) * p.st.entry + pool_slot(p.st, kv_head, row & 15u) * p.st.head + sch * 8u) * 2u;
                kr[i] = *reinterpret_cast<const half8*>(src + lane_bytes);
                vr[i] = *reinterpret_cast<const half8*>(src + v_bytes + lane_bytes);
            } else {
                const uint32_t key = min(t * kPfKeys + row, last_key);
                const uint32_t pi = key / p.page_size;
                const uint32_t pg = (uint32_t)p.table[pi], slot = key - pi * p.page_size;
                const unsigned char* src = kv_base + ((size_t)pg * p.st.page + (size_t)slot * p.st.entry +
                                                      (size_t)pool_slot(p.st, kv_head, slot) * p.st.head + sch * 8u) * 2u;
                kr[i] = *reinterpret_cast<const half8*>(src);
                vr[i] = *reinterpret_cast<const half8*>(src + v_bytes);
            }
        }
        if constexpr (S16) {
            if (t * kPfKeys + kPfKeys - 1 > last_key) {  // 0 x stale bits must stay 0
#pragma unroll
                for (int i = 0; i < NP; ++i)
                    if (t * kPfKeys + srow + RP * i > last_key) vr[i] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
    };
    auto stash = [&](uint32_t base, const half8(&kr)[NP], const half8(&vr)[NP]) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            lds_write16(wa[i] + base, kr[i]);
            lds_write16(wa[i] + base + IMG, vr[i]);
        }
    };

    f32x16 oacc[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[db][e] = 0.f;
    // online softmax with a deferred maximum (guide T13): m_ref, the reference the exponents are taken against, follows a
    // row's maximum only when that runs ahead by more than kPfDefer (so p <= 2^8: exact range for fp16 and fp32 sums), and
    // then everything still at the old reference (O and l) is moved exactly once, before the tile's exponents are taken
    float m_ref = 0.f, l = 0.f;
    const float c = p.scale_log2, defer = kPfDefer / c;  // scores are in raw units, the exponent in log2 units

    half8 kr[NP], vr[NP];

    auto tile = [&](auto buf_c, uint32_t t) {
        constexpr uint32_t base = decltype(buf_c)::value * BUFB;
        const uint32_t key0 = t * kPfKeys;
        if (wave_live && key0 <= limit_hi) {
            f32x16 sacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int e = 0; e < 16; ++e) sacc[kb][e] = 0.f;
#pragma unroll
                for (int s = 0; s < D / 16; ++s) {
                    const half8 kf = lds_read16(ka[s & 1] + base + kb * (64 * D) + 512 * (s >> 1));
                    sacc[kb] = mfma_32x32x16<T>(kf, qf[s], sacc[kb]);
                }
            }
            // keys beyond this lane's limit (causal mask, tail of the last tile) never enter the softmax
            if (key0 + kPfKeys - 1 > limit_lo) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const uint32_t key = key0 + 32 * kb + (e & 3) + 8 * (e >> 2) + 4 * h;
                        sacc[kb][e] = key <= limit ? sacc[kb][e] : -INFINITY;
                    }
            }
            float g = sacc[0][0];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) g = __builtin_fmaxf(g, sacc[kb][e]);
            g = __builtin_fmaxf(g, lane_xor<32>(g, lane));  // the row's maximum in this tile
            // key 0 is visible to every query, so tile 0 gives every row a finite reference (NaN in, NaN out)
            if (t == 0 || __builtin_amdgcn_ballot_w64(g - m_ref > defer)) {
                const float m_new = t == 0 ? g : __builtin_fmaxf(m_ref, g);
                // tile 0 has nothing to move (l and O are still zero): alpha = 1 -- exp2((0 - g) c) overflows to +inf for a row
                // whose first-tile maximum is below about -128 log2 units, and 0 x inf would turn the whole row into NaN
                const float alpha = t == 0 ? 1.f : __builtin_amdgcn_exp2f((m_ref - m_new) * c);
                m_ref = m_new;
                l *= alpha;
#pragma unroll
                for (int db = 0; db < D / 32; ++db)
#pragma unroll
                    for (int e = 0; e < 16; ++e) oacc[db][e] *= alpha;
            }
            const float mc = m_ref * c;
            float psum = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb][e], c, -mc));
                    sacc[kb][e] = pe;
                    psum += pe;
                }
            l += psum;
            // O^T += V^T P^T over the tile's four 16-key steps
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                half8 pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = from_f32<T>(sacc[s >> 1][8 * (s & 1) + j]);
#pragma unroll
                for (int db = 0; db < D / 32; ++db) {
                    const half4 lo = lds_read_tr(va[0] + base + s * (32 * D) + 512 * db);
                    const half4 hi = lds_read_tr(va[1] + base + s * (32 * D) + 512 * db);
                    const half8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    oacc[db] = mfma_32x32x16<T>(vf, pf, oacc[db]);
                }
            }
        }
        if constexpr (NBUF == 2) {
            // tile t + 1 into the other buffer: its last readers passed the previous barrier
            if (t + 1 < n_tiles) stash(base ^ BUFB, kr, vr);
            __syncthreads();
        } else {
            __syncthreads();  // every wave is done reading tile t
            if (t + 1 < n_tiles) stash(0, kr, vr);
            __syncthreads();
        }
        if (t + 2 < n_tiles) issue(t + 2, kr, vr);
    };

    issue(0, kr, vr);
    stash(0, kr, vr);
    __syncthreads();
    if (n_tiles > 1) issue(1, kr, vr);
    if constexpr (NBUF == 2) {
        for (uint32_t t = 0; t < n_tiles; t += 2) {
            tile(std::integral_constant<uint32_t, 0>{}, t);
            if (t + 1 < n_tiles) tile(std::integral_constant<uint32_t, 1>{}, t + 1);
        }
    } else {
        for (uint32_t t = 0; t < n_tiles; ++t) tile(std::integral_constant<uint32_t, 0>{}, t);
    }

    if (wave_live && q0w + r < p.n_q) {
        const float inv = 1.0f / (l + lane_xor<32>(l, lane));
        half_t* orow = p.o + ((size_t)(q0w + r) * p.num_qo_heads + head) * D + 4 * h;
#pragma unroll
        for (int db = 0; db < D / 32; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                half4 out;
#pragma unroll
                for (int e = 0; e < 4; ++e) out[e] = from_f32<T>(oacc[db][4 * g4 + e] * inv);
                *reinterpret_cast<half4*>(orow + 32 * db + 8 * g4) = out;
            }
    }
}

}  // namespace quest
