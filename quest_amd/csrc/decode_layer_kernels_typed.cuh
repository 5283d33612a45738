// gemv_kernel, skinny_kernel and persist_kernel of decode_layer.hip, written ONCE and compiled once per element type:
// decode_layer.hip includes this file twice, with QUEST_ELEM = half_t / QUEST_KNAME(n) = n and with QUEST_ELEM = bf16_t /
// QUEST_KNAME(n) = n_b16 (no include guard on purpose), like prefill_kernel_typed.cuh and decode_kernels_typed.cuh.  The
// argument structs, the row orders and everything the host plans with are in decode_layer.hip and have no element type:
// storage is 16-bit either way.  What depends on T: to_f32<T> / a bit cast to T where a stored value is read, from_f32<T> (round to
// nearest even, once per output) where one is made, dot8<T> (v_dot2_f32_f16 / v_dot2c_f32_bf16) and mfma_4x4x4<T>
// (v_mfma_f32_4x4x4_16b_f16 / _bf16: the same operand layout).  From this text the fp16 kernels compile to the code they had
// when they lived in decode_layer.hip (profiles/bf16_gemv_fp16_unchanged.txt).
namespace quest {

// ---- the batch-1 launch (decode_layer.hip, first section)
template <int MODE, int kGvWaves, int kGvRows, int kGvUnroll>
__global__ __launch_bounds__(kGvWaves* kWave, kGvWaves / 2) void QUEST_KNAME(gemv_kernel)(GemvArgs p) {  // 2 workgroups per CU
    using T = QUEST_ELEM;
    static_assert(MODE == kGvPlain || MODE == kGvResidual || kGvRows % 2 == 0, "pairs of row-dots stay in one wave");
    extern __shared__ __attribute__((aligned(16))) unsigned char gv_smem[];
    half_t* x_s = reinterpret_cast<half_t*>(gv_smem);  // in_dim halves, zero-padded to a multiple of 64 * 8 * kGvUnroll
    __shared__ float s_part[kGvWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_vec = p.in_dim / kVec;
    const uint32_t iters = (n_vec + kWave - 1) / kWave;
    const uint32_t outer = (iters + kGvUnroll - 1) / kGvUnroll;

    // ---- rows of this wave
    const uint32_t vr0 = (blockIdx.x * kGvWaves + wave) * kGvRows;  // first virtual row-dot of the wave
    const half_t* wrow[kGvRows];
    uint32_t mat[kGvRows], row[kGvRows];
    bool live[kGvRows];
#pragma unroll
    for (int r = 0; r < kGvRows; ++r) {
        uint32_t vr = vr0 + r, m = 0, rr;
        if constexpr (MODE == kGvSiluMul) {  // (gate, up) of the same output row side by side
            m = vr & 1u;
            rr = vr >> 1;
            live[r] = rr < p.rows[0];
        } else {
            while (m < 2 && vr >= p.rows[m]) vr -= p.rows[m], ++m;
            live[r] = vr < p.rows[m];
            rr = vr;
            if constexpr (MODE == kGvQkvRope) {
                // pair-major order inside a head: virtual rows 2j, 2j+1 are features j and j + head_dim/2, so that a
                // wave's 4 row-dots are two complete rotation pairs
                const uint32_t hd = p.head_dim, head = rr / hd, j = rr % hd;
                rr = head * hd + (j >> 1) + (j & 1u) * (hd / 2);
            }
        }
        mat[r] = m;
        row[r] = live[r] ? rr : 0u;
        wrow[r] = p.w[live[r] ? m : 0] + (size_t)row[r] * p.in_dim;
    }

    // ---- the first weight loads leave before the input vector is staged (they do not depend on it).  Addressing: the
    // row base is wave-uniform (an SGPR pair, advanced per round), the lane's part one 32-bit offset, the slot
    // an immediate -- except in the last round of a row whose length is not a multiple of a round, where the vector index
    // is clamped (kClamp).  A round = kGvUnroll slots x 64 lanes x 16 bytes per row.
    constexpr uint32_t kRoundHalves = kGvUnroll * kWave * kVec;
    const uint32_t full = n_vec / (kGvUnroll * kWave);  // rounds whose every slot lies inside the row for every lane
    half8 wv[kGvUnroll][kGvRows];
    const uint32_t lane_off = lane * kVec;
    const half_t* const* rbase = wrow;  // (already wave-uniform for the compiler: built from blockIdx and the SGPR wave index)
    // request round `o` of every row into slot u (kClamp: the round may reach past the row's end)
    auto issue = [&](uint32_t o, int u, auto clamp_c) {
        constexpr bool kClamp = decltype(clamp_c)::value;
        if constexpr (!kClamp) {
            const uint32_t off = lane_off + (uint32_t)u * (kWave * kVec);
#pragma unroll
            for (int r = 0; r < kGvRows; ++r) wv[u][r] = ld8_stream(rbase[r] + (size_t)o * kRoundHalves + off);
        } else {
            const uint32_t v = lane + (o * kGvUnroll + (uint32_t)u) * kWave, vc = v < n_vec ? v : n_vec - 1;
#pragma unroll
            for (int r = 0; r < kGvRows; ++r) wv[u][r] = ld8_stream(rbase[r] + (size_t)vc * kVec);
        }
    };
    if (full > 0) {  // block-uniform
#pragma unroll
        for (int u = 0; u < kGvUnroll; ++u) issue(0, u, std::false_type{});
    } else {
#pragma unroll
        for (int u = 0; u < kGvUnroll; ++u) issue(0, u, std::true_type{});
    }

    // ---- input vector -> LDS (RMSNorm prologue: x * rsqrt(mean(x^2) + eps) * gamma, rounded to fp16 like the
    // stand-alone rms_norm_forward's output)
    const uint32_t pad_vec = outer * kGvUnroll * kWave;  // vectors the loop touches
    if (p.gamma) {
        float ss = 0.f;
        for (uint32_t v = tid; v < n_vec; v += kGvWaves * kWave) {
            const float8 xf = to_f32<T>(ld8(p.x + (size_t)v * kVec));
#pragma unroll
            for (int i = 0; i < kVec; ++i) ss = __builtin_fmaf(xf[i], xf[i], ss);
        }
        ss = wave_allreduce_sum(ss, (int)lane);
        if (lane == 0) s_part[wave] = ss;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < kGvWaves; ++w) tot += s_part[w];
        const float inv = 1.0f / sqrtf(tot / (float)p.in_dim + p.eps);
        for (uint32_t v = tid; v < pad_vec; v += kGvWaves * kWave) {
            half8 o = (half8)(half_t)0;
            if (v < n_vec) {
                const float8 xf = to_f32<T>(ld8(p.x + (size_t)v * kVec)), g = to_f32<T>(ld8(p.gamma + (size_t)v * kVec));
                float8 rr;
#pragma unroll
                for (int i = 0; i < kVec; ++i) rr[i] = xf[i] * inv * g[i];
                o = from_f32<T>(rr);
            }
            st8(x_s + (size_t)v * kVec, o);
        }
    } else {
        for (uint32_t v = tid; v < pad_vec; v += kGvWaves * kWave)
            st8(x_s + (size_t)v * kVec, v < n_vec ? ld8(p.x + (size_t)v * kVec) : (half8)(half_t)0);
    }
    __syncthreads();

    // ---- stream the rows: a slot is re-issued for the next round as soon as it has been consumed (loads complete in
    // order, so the wait for slot u leaves the younger ones in flight).  Three copies of the round body keep the
    // steady state free of per-slot branches: next round full / next round clamped / last round.
    float acc[kGvRows] = {};
    auto consume = [&](uint32_t o, int u) {
        const uint32_t v = lane + (o * kGvUnroll + (uint32_t)u) * kWave;
        const half8 xv = ld8(x_s + (size_t)v * kVec);  // zero beyond in_dim: clamped weight vectors contribute nothing
#pragma unroll
        for (int r = 0; r < kGvRows; ++r) acc[r] = dot8<T>(wv[u][r], xv, acc[r]);
    };
    for (uint32_t o = 0; o < outer; ++o) {
        if (o + 1 < full) {
#pragma unroll
            for (int u = 0; u < kGvUnroll; ++u) {
                consume(o, u);
                issue(o + 1, u, std::false_type{});
            }
        } else if (o + 1 < outer) {
#pragma unroll
            for (int u = 0; u < kGvUnroll; ++u) {
                consume(o, u);
                issue(o + 1, u, std::true_type{});
            }
        } else {
#pragma unroll
            for (int u = 0; u < kGvUnroll; ++u) consume(o, u);
        }
    }
#pragma unroll
    for (int r = 0; r < kGvRows; ++r) acc[r] = wave_allreduce_sum(acc[r], (int)lane);

    // ---- epilogue (every lane holds the four totals; lane 0 writes)
    if (lane != 0) return;
    if constexpr (MODE == kGvPlain) {
#pragma unroll
        for (int r = 0; r < kGvRows; ++r)
            if (live[r]) p.out[mat[r]][row[r]] = from_f32<T>(acc[r]);
    } else if constexpr (MODE == kGvResidual) {
#pragma unroll
        for (int r = 0; r < kGvRows; ++r)
            if (live[r]) p.out[0][row[r]] = from_f32<T>((float)__builtin_bit_cast(T, p.residual[row[r]]) + acc[r]);
    } else if constexpr (MODE == kGvSiluMul) {
#pragma unroll
        for (int r = 0; r < kGvRows; r += 2)
            if (live[r]) {
                const float g = acc[r], u = acc[r + 1];
                p.out[0][row[r]] = from_f32<T>(g / (1.0f + __expf(-g)) * u);
            }
    } else {  // kGvQkvRope
        const float pos = (float)(p.state->seq_len - 1);
#pragma unroll
        for (int r = 0; r < kGvRows; r += 2) {
            if (!live[r]) continue;
            if (mat[r] < 2) {  // q / k: (acc[r], acc[r+1]) = features (d, d + D/2) of one head
                float s, c;
                rope_cos_sin(p, row[r] % p.head_dim, pos, c, s);  // row[r] % head_dim < D/2
                p.out[mat[r]][row[r]] = from_f32<T>(acc[r] * c - acc[r + 1] * s);
                p.out[mat[r]][row[r + 1]] = from_f32<T>(acc[r + 1] * c + acc[r] * s);
            } else {
                p.out[2][row[r]] = from_f32<T>(acc[r]);
                p.out[2][row[r + 1]] = from_f32<T>(acc[r + 1]);
            }
        }
    }
}

// ---- n tokens, inputs from L2 (decode_layer.hip, second section)
template <int MODE, int NW, int U, int TG>
__global__ __launch_bounds__(NW* kWave, 2) void QUEST_KNAME(skinny_kernel)(SkinnyArgs a) {  // 8 waves per CU: <= 256 VGPRs
    using T = QUEST_ELEM;
    const GemvArgs& p = a.g;
    extern __shared__ __attribute__((aligned(16))) unsigned char sk_smem[];
    half_t* gamma_s = reinterpret_cast<half_t*>(sk_smem);  // RMSNorm weight (in_dim halves; launches with a prologue only)
    __shared__ float s_ss[4 * TG][NW];                     // per token, per wave: sum of squares
    __shared__ float s_part[NW][16][4 * TG];               // the waves' partial tiles [row][token]
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t j = lane & 3u, blk = lane >> 2;  // B column (weight row of a quad) = A row (token of a group); k chunk

    // ---- the lane's four weight rows (quad q: virtual row 16 block + 4 q + j) and TG input rows (token 4 t + j)
    const half_t* wrow[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t m, rr;
        const bool live = skinny_row<MODE>(p, blockIdx.x * 16u + 4u * (uint32_t)q + j, m, rr);
        wrow[q] = p.w[live ? m : 0] + (size_t)(live ? rr : 0u) * p.in_dim;  // dead rows read row 0 (never written out)
    }
    const half_t* xrow[TG];
    bool tok[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        tok[t] = 4u * (uint32_t)t + j < a.n_tokens;
        xrow[t] = p.x + (size_t)(tok[t] ? 4u * (uint32_t)t + j : 0u) * a.x_stride;
    }
    const bool norm = p.gamma != nullptr;  // block-uniform

    const uint32_t n_steps = (p.in_dim + 127u) / 128u;
    const uint32_t mine = wave < n_steps ? (n_steps - wave + NW - 1) / NW : 0u;  // this wave's steps
    half8 wv[U][4], xv[U][TG];
    auto issue = [&](uint32_t s, int u) {
        const uint32_t k0 = (wave + NW * s) * 128u + blk * 8u;
        const uint32_t kc = k0 < p.in_dim ? k0 : 0u;  // clamped; masked at use
#pragma unroll
        for (int q = 0; q < 4; ++q) wv[u][q] = ld8_stream(wrow[q] + kc);
#pragma unroll
        for (int t = 0; t < TG; ++t) xv[u][t] = ld8(xrow[t] + kc);
    };
#pragma unroll
    for (int u = 0; u < U; ++u) issue((uint32_t)u, u);

    // ---- RMSNorm prologue: 1 / rms of every token (every workgroup recomputes them; their loads queue behind the first
    // weight fragments)
    float inv[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) inv[t] = 1.0f;
    if (norm) {
        const uint32_t n_vec = p.in_dim / kVec;
        for (uint32_t t = 0; t < a.n_tokens; ++t) {
            float ss = 0.f;
            for (uint32_t v = tid; v < n_vec; v += NW * kWave) {
                const float8 xf = to_f32<T>(ld8(p.x + (size_t)t * a.x_stride + (size_t)v * kVec));
#pragma unroll
                for (int i = 0; i < kVec; ++i) ss = __builtin_fmaf(xf[i], xf[i], ss);
            }
            ss = wave_allreduce_sum(ss, (int)lane);
            if (lane == 0) s_ss[t][wave] = ss;
        }
        for (uint32_t v = tid; v < n_vec; v += NW * kWave) st8(gamma_s + (size_t)v * kVec, ld8(p.gamma + (size_t)v * kVec));
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TG; ++t)
            if (tok[t]) {
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) tot += s_ss[4 * t + j][w];
                inv[t] = 1.0f / sqrtf(tot / (float)p.in_dim + p.eps);
            }
    }

    // ---- stream
    float4_t acc[4][TG];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < TG; ++t) acc[q][t] = float4_t{0.f, 0.f, 0.f, 0.f};
    auto consume = [&](uint32_t s, int u) {
        const uint32_t k0 = (wave + NW * s) * 128u + blk * 8u;
        const bool in = k0 < p.in_dim;
        float8 gf;
        if (norm) gf = to_f32<T>(ld8(gamma_s + (in ? k0 : 0u)));
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            half8 b = xv[u][t];
            if (norm) {
                const float8 xf = to_f32<T>(b);
                float8 rr;
#pragma unroll
                for (int i = 0; i < kVec; ++i) rr[i] = xf[i] * inv[t] * gf[i];
                b = from_f32<T>(rr);
            }
            if (!tok[t] || !in) b = (half8)(half_t)0;  // dead token / past the row's end: contributes nothing
            const half4_t b0 = {b[0], b[1], b[2], b[3]}, b1 = {b[4], b[5], b[6], b[7]};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const half8 w8 = wv[u][q];
                const half4_t w0 = {w8[0], w8[1], w8[2], w8[3]}, w1 = {w8[4], w8[5], w8[6], w8[7]};
                acc[q][t] = mfma_4x4x4<T>(b0, w0, acc[q][t]);  // A = tokens, B = weight rows
                acc[q][t] = mfma_4x4x4<T>(b1, w1, acc[q][t]);
            }
        }
    };
    const uint32_t rounds = (mine + U - 1) / U;
    for (uint32_t o = 0; o < rounds; ++o) {
        if (o + 1 < rounds) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                consume(o * U + (uint32_t)u, u);
                issue((o + 1) * U + (uint32_t)u, u);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) consume(o * U + (uint32_t)u, u);
        }
    }
    // ---- the 16 k chunks of the wave meet: lanes 4 b + j over b (distances 4, 8 inside a row of 16 lanes, then 16, 32);
    // D element e of acc[q][t] at lane (b, j) = token 4 t + e, row 4 q + j
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[q][t][e];
                v += dpp_f<kDppRowRor + 8>(v);
                v += dpp_f<kDppRowRor + 4>(v);
                v += lane_xor<16>(v, (int)lane);
                v += lane_xor<32>(v, (int)lane);
                if (lane < 4u) s_part[wave][4 * q + lane][4 * t + e] = v;
            }
    __syncthreads();

    // ---- 128 threads: (token, row pair)
    if (tid >= 128u) return;
    const uint32_t token = tid & 15u, pair = tid >> 4;
    if (token >= a.n_tokens) return;
    float v0 = 0.f, v1 = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v0 += s_part[w][2u * pair][token], v1 += s_part[w][2u * pair + 1u][token];
    // the pair's two virtual rows -> (matrix, row)
    uint32_t mat[2], row[2];
    bool live[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) live[i] = skinny_row<MODE>(p, blockIdx.x * 16u + 2u * pair + (uint32_t)i, mat[i], row[i]);
    if constexpr (MODE == kGvPlain) {
        if (live[0]) p.out[mat[0]][(size_t)token * a.out_stride[mat[0]] + row[0]] = from_f32<T>(v0);
        if (live[1]) p.out[mat[1]][(size_t)token * a.out_stride[mat[1]] + row[1]] = from_f32<T>(v1);
    } else if constexpr (MODE == kGvResidual) {
        // (the cast to T spelt out, not from_f32<T>: behind the call the fp16 kernels' address arithmetic of these two stores
        // came out in another order -- the same values, but not the code they had; (T) of a float rounds to nearest even)
        const size_t base = (size_t)token * a.out_stride[0];
        if (live[0]) p.out[0][base + row[0]] = __builtin_bit_cast(half_t, (T)((float)__builtin_bit_cast(T, p.residual[base + row[0]]) + v0));
        if (live[1]) p.out[0][base + row[1]] = __builtin_bit_cast(half_t, (T)((float)__builtin_bit_cast(T, p.residual[base + row[1]]) + v1));
    } else if constexpr (MODE == kGvSiluMul) {
        if (live[0]) p.out[0][(size_t)token * a.out_stride[0] + row[0]] = from_f32<T>(v0 / (1.0f + __expf(-v0)) * v1);
    } else {  // kGvQkvRope: rows come in (d, d + D/2) pairs of one head of one matrix
        if (!live[0]) return;
        half_t* o = p.out[mat[0]] + (size_t)token * a.out_stride[mat[0]];
        if (mat[0] < 2) {
            const float pos = (float)(p.state[(size_t)token * a.state_stride].seq_len - 1);
            float sn, cs;
            rope_cos_sin(p, row[0] % p.head_dim, pos, cs, sn);
            o[row[0]] = from_f32<T>(v0 * cs - v1 * sn);
            o[row[1]] = from_f32<T>(v1 * cs + v0 * sn);
        } else {
            o[row[0]] = from_f32<T>(v0);
            o[row[1]] = from_f32<T>(v1);
        }
    }
}

// ---- n tokens, inputs in LDS (decode_layer.hip, third section)
template <int MODE, int TG, int CM>
__global__ __launch_bounds__(kPsWaves* kWave, 4) void QUEST_KNAME(persist_kernel)(SkinnyArgs a, PersistPlan pl) {
    using T = QUEST_ELEM;
    const GemvArgs& p = a.g;
    constexpr int kXV = ps_input_vectors(TG);
    extern __shared__ __attribute__((aligned(16))) unsigned char ps_smem[];
    half_t* x_s = reinterpret_cast<half_t*>(ps_smem);  // [4 TG][x_row] (normalised) inputs
    __shared__ float s_inv[4 * TG];
    __shared__ float s_ssq[kXV][kPsWaves][2];  // RMSNorm prologue: per (input slot, wave) the sums of squares of its two tokens
    __shared__ float s_part[2][kPsWaves][4][4 * TG];  // [buffer][wave = quad slot x slice][row of the quad][token]
    // kGvQkvRope: (cos, sin) of every (token, frequency), computed once per workgroup while the first weights are on their
    // way; a round's epilogue reads it (no sincosf, with its large-argument path, per round)
    constexpr int kRopeMaxHalfD = 128;
    __shared__ float2 s_rope[MODE == kGvQkvRope ? 4 * TG * kRopeMaxHalfD : 1];
    static_assert(sizeof(s_inv) + sizeof(s_ssq) + sizeof(s_part) + sizeof(s_rope) + persist_lds_budget(TG, MODE == kGvQkvRope)
                      <= kCuLdsBytes, "static arrays + the largest dynamic request must fit the CU's LDS");
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef QUEST_PS_TIMELINE  // tuning build: s_memtime stamps of (workgroup 0 | last, wave 0 | 15) -> p.out[2] (16 x 4 x int64)
    long long ps_t[16];
    int ps_n = 0;
#define PS_STAMP() do { if (ps_n < 16) ps_t[ps_n++] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define PS_STAMP() do {} while (0)
#endif
    PS_STAMP();
    const uint32_t j = lane & 3u, blk = lane >> 2;
    const uint32_t ks = pl.ks, slice = wave & (ks - 1u), qslot = wave >> pl.ks_log2, qw = kPsWaves >> pl.ks_log2;
    const bool norm = p.gamma != nullptr;
    const uint32_t n_steps = (p.in_dim + 127u) / 128u;
    // workgroup barrier that publishes LDS only: __syncthreads() also waits for the global loads in flight (vmcnt(0))
    // whenever global stores are pending -- the epilogue's -- which would drain the prefetched set every round
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    const uint32_t n_seg = pl.rounds;  // a segment = one round of tasks
    auto seg_quad = [&](uint32_t seg) { return (seg * gridDim.x + blockIdx.x) * qw + qslot; };
    auto row_ptr = [&](uint32_t quad) -> const half_t* {
        uint32_t m, rr;
        const bool live = quad < pl.n_quads && skinny_row<MODE>(p, 4u * quad + j, m, rr);
        return p.w[live ? m : 0] + (size_t)(live ? rr : 0u) * p.in_dim;  // dead rows read row 0 (never written out)
    };
    // Every call requests exactly CM fragments, whatever the task: steps past the slice's end and quads past the matrix
    // re-read cached bytes.  (A load under a branch makes the compiler's s_waitcnt bookkeeping assume it may not have been
    // issued: every later wait for an OLDER load became vmcnt(0) -- the consumption of a set waited for the set requested
    // just before it, i.e. nothing was in flight under the MFMAs.  For the same reason the requests past the last segment
    // are issued all the same -- one cached line -- instead of being guarded.)
    half8 wa[CM], wb[CM];
    auto issue = [&](half8 (&w)[CM], uint32_t seg) {
        const bool real = seg < n_seg;  // block-uniform; past the end: CM requests of ONE cached line, nobody waits for them
        const half_t* wrow = real ? row_ptr(seg_quad(seg)) : p.w[0];
        const uint32_t s1 = real ? n_steps : 0u;
#pragma unroll
        for (int i = 0; i < CM; ++i) {
            const uint32_t st = slice + ks * (uint32_t)i, k0 = st * 128u + blk * 8u;
            w[i] = ld8_stream(wrow + (st < s1 && k0 < p.in_dim ? k0 : 0u));
        }
    };

    // ---- the inputs: element e = tid + 1024 i -> (token e / vpp, vector e % vpp), vpp = 16 spp vectors per token (the
    // host guarantees tokens x vpp <= kXV x 1024); always kXV loads (clamped)
    const uint32_t vpp = pl.spp * 16u, x_tot = a.n_tokens * vpp;
    half8 xr[kXV];
    auto x_load = [&] {
#pragma unroll
        for (int i = 0; i < kXV; ++i) {
            const uint32_t e = tid + (uint32_t)i * kPsWaves * kWave, t = __umulhi(e, pl.vpp_magic), k0 = (e - t * vpp) * kVec;
            const bool in = e < x_tot && k0 < p.in_dim;
            xr[i] = ld8(p.x + (in ? (size_t)t * a.x_stride + k0 : (size_t)0));
        }
    };
    auto x_store = [&](half_t* dst) {  // zero for dead tokens and past the row's end
#pragma unroll
        for (int i = 0; i < kXV; ++i) {
            const uint32_t e = tid + (uint32_t)i * kPsWaves * kWave, t = __umulhi(e, pl.vpp_magic), v = e - t * vpp;
            if (e >= 4u * TG * vpp) continue;
            half8 o = xr[i];
            const bool in = e < x_tot && v * kVec < p.in_dim;
            if (norm && in) {
                const float8 xf = to_f32<T>(o), g = to_f32<T>(ld8(p.gamma + v * kVec));
                const float inv = s_inv[t];
                float8 rr;
#pragma unroll
                for (int c = 0; c < kVec; ++c) rr[c] = xf[c] * inv * g[c];
                o = from_f32<T>(rr);
            }
            st8(dst + (size_t)t * pl.x_row + (size_t)v * kVec, in ? o : (half8)(half_t)0);
        }
    };

    // ---- prologue: inputs first (see above)
    x_load();
    if constexpr (MODE == kGvQkvRope) {  // under the inputs' latency; published by the staging barrier
        const uint32_t half_d = p.head_dim / 2u;
        for (uint32_t e = tid; e < a.n_tokens * half_d; e += kPsWaves * kWave) {
            const uint32_t t = e / half_d, d = e % half_d;
            const float pos = (float)(p.state[(size_t)t * a.state_stride].seq_len - 1);
            float sn, cs;
            rope_cos_sin(p, d, pos, cs, sn);
            s_rope[t * kRopeMaxHalfD + d] = make_float2(cs, sn);
        }
    }

    __builtin_amdgcn_s_barrier();
    PS_STAMP();
    if (norm) {
        // 1 / rms per token.  A thread's vector i lies in ONE token and the lanes of a wave hold at most two tokens
        // (vpp >= 64): every (slot i, wave) leaves the sums of its two sides t0, t0 + 1 in LDS, and wave t adds token t's
        // entries in a FIXED order -- the result does not depend on the order in which the waves arrive (per-token LDS
        // atomics did: two launches over the same inputs, or two workgroups of one launch, could normalise a token with
        // 1 / rms values one fp32 ulp apart, and then differ in the fp16 rounding of an input).
#pragma unroll
        for (int i = 0; i < kXV; ++i) {
            const uint32_t e = tid + (uint32_t)i * kPsWaves * kWave, t = __umulhi(e, pl.vpp_magic);
            float ss = 0.f;
            if (e < x_tot && (e - t * vpp) * kVec < p.in_dim) {
                const float8 xf = to_f32<T>(xr[i]);
#pragma unroll
                for (int c = 0; c < kVec; ++c) ss = __builtin_fmaf(xf[c], xf[c], ss);
            }
            const uint32_t t0 = __builtin_amdgcn_readfirstlane(t);
            const float s_lo = wave_allreduce_sum(t == t0 ? ss : 0.f, (int)lane), s_hi = wave_allreduce_sum(t == t0 ? 0.f : ss, (int)lane);
            if (lane == 0) s_ssq[i][wave][0] = s_lo, s_ssq[i][wave][1] = s_hi;
        }
        __syncthreads();
        if (wave < 4u * TG) {  // wave-uniform: wave t owns token t
            float tot = 0.f;
            for (uint32_t idx = lane; idx < (uint32_t)kXV * kPsWaves * 2u; idx += kWave) {
                const uint32_t i = idx / (kPsWaves * 2u), w = (idx >> 1) % kPsWaves, side = idx & 1u;
                const uint32_t tt = __umulhi(w * kWave + i * kPsWaves * kWave, pl.vpp_magic) + side;  // = that wave's t0 (+ 1)
                tot += tt == wave ? s_ssq[i][w][side] : 0.f;
            }
            tot = wave_allreduce_sum(tot, (int)lane);
            if (lane == 0) s_inv[wave] = 1.0f / sqrtf(tot / (float)p.in_dim + p.eps);
        }
        __syncthreads();
    }
    x_store(x_s);
    PS_STAMP();
    lds_barrier();
    issue(wa, 0);
    PS_STAMP();
    float4_t acc[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};
    auto consume = [&](const half8 (&w)[CM], uint32_t seg) {
        if (seg_quad(seg) >= pl.n_quads) return;  // wave-uniform
        const half_t* xb = x_s;
#pragma unroll
        for (int i = 0; i < CM; ++i) {
            const uint32_t st = slice + ks * (uint32_t)i;
            if (st < n_steps) {  // wave-uniform
                const uint32_t kl = st * 128u + blk * 8u;
                const half8 w8 = w[i];
                const half4_t w0 = {w8[0], w8[1], w8[2], w8[3]}, w1 = {w8[4], w8[5], w8[6], w8[7]};
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    const half8 x8 = ld8(xb + (size_t)(4u * (uint32_t)t + j) * pl.x_row + kl);
                    const half4_t x0 = {x8[0], x8[1], x8[2], x8[3]}, x1 = {x8[4], x8[5], x8[6], x8[7]};
                    acc[t] = mfma_4x4x4<T>(x0, w0, acc[t]);  // A = tokens, B = weight rows
                    acc[t] = mfma_4x4x4<T>(x1, w1, acc[t]);
                }
            }
        }
    };
    // the k slices of the quads meet; epilogue
    auto finish = [&](uint32_t seg) {
        const uint32_t buf = seg & 1u;
#pragma unroll
        for (int t = 0; t < TG; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {  // D element e at lane (b, j) = token 4 t + e, row j of the quad; sum over b
                float v = acc[t][e];
                v += dpp_f<kDppRowRor + 8>(v);
                v += dpp_f<kDppRowRor + 4>(v);
                v += lane_xor<16>(v, (int)lane);
                v += lane_xor<32>(v, (int)lane);
                if (lane < 4u) s_part[buf][wave][lane][4 * t + e] = v;
                acc[t][e] = 0.f;
            }
        lds_barrier();
        // (quad slot, row pair, token) threads
        const uint32_t token = tid & 15u, pair = (tid >> 4) & 1u, qs = tid >> 5;
        if (qs >= qw || token >= a.n_tokens) return;
        const uint32_t quad = (seg * gridDim.x + blockIdx.x) * qw + qs;
        if (quad >= pl.n_quads) return;
        float v0 = 0.f, v1 = 0.f;
        for (uint32_t sl = 0; sl < ks; ++sl) {
            v0 += s_part[buf][qs * ks + sl][2u * pair][token];
            v1 += s_part[buf][qs * ks + sl][2u * pair + 1u][token];
        }
        uint32_t mat[2], row[2];
        bool live[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) live[i] = skinny_row<MODE>(p, 4u * quad + 2u * pair + (uint32_t)i, mat[i], row[i]);
        if constexpr (MODE == kGvPlain) {
            if (live[0]) p.out[mat[0]][(size_t)token * a.out_stride[mat[0]] + row[0]] = from_f32<T>(v0);
            if (live[1]) p.out[mat[1]][(size_t)token * a.out_stride[mat[1]] + row[1]] = from_f32<T>(v1);
        } else if constexpr (MODE == kGvResidual) {
            // (the cast to T spelt out, as in skinny_kernel: the fp16 code stays what it was)
            const size_t base = (size_t)token * a.out_stride[0];
            if (live[0]) p.out[0][base + row[0]] = __builtin_bit_cast(half_t, (T)((float)__builtin_bit_cast(T, p.residual[base + row[0]]) + v0));
            if (live[1]) p.out[0][base + row[1]] = __builtin_bit_cast(half_t, (T)((float)__builtin_bit_cast(T, p.residual[base + row[1]]) + v1));
        } else if constexpr (MODE == kGvSiluMul) {
            if (live[0]) p.out[0][(size_t)token * a.out_stride[0] + row[0]] = from_f32<T>(v0 / (1.0f + __expf(-v0)) * v1);
        } else {  // kGvQkvRope: rows come in (d, d + D/2) pairs of one head of one matrix
            if (!live[0]) return;
            half_t* o = p.out[mat[0]] + (size_t)token * a.out_stride[mat[0]];
            if (mat[0] < 2) {
                const float2 r = s_rope[token * kRopeMaxHalfD + row[0] % p.head_dim];  // row[0] % head_dim < D / 2
                const float cs = r.x, sn = r.y;
                o[row[0]] = from_f32<T>(v0 * cs - v1 * sn);
                o[row[1]] = from_f32<T>(v1 * cs + v0 * sn);
            } else {
                o[row[0]] = from_f32<T>(v0);
                o[row[1]] = from_f32<T>(v1);
            }
        }
    };
    // Segment s: request segment s + 1, consume the set of s, let the slices meet.  A CU's memory
    // pipeline holds ~64 KiB of requests; a wave whose requests do not fit stalls at issue.  Requested HERE, after the
    // previous segment's barrier, a stalled wave holds nobody up; requested two segments ahead, right after the
    // consumption and before the barrier, the stall sat in front of the barrier: 40.3 us instead of 36.8 for the gate/up
    // launch (more in flight than the pipeline holds buys nothing).
    auto body = [&](const half8 (&cur)[CM], half8 (&nxt)[CM], uint32_t sg) {
        issue(nxt, sg + 1);
        PS_STAMP();
        consume(cur, sg);
        PS_STAMP();
        finish(sg);
        PS_STAMP();
    };
    for (uint32_t seg = 0;; seg += 2) {  // wa holds segment seg; leaves by break (no merge with loads behind it)
        body(wa, wb, seg);
        if (seg + 1 >= n_seg) break;
        body(wb, wa, seg + 1);
        if (seg + 2 >= n_seg) break;
    }
    PS_STAMP();
#ifdef QUEST_PS_TIMELINE
    if (lane == 0 && (wave == 0 || wave == kPsWaves - 1) && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1) && p.out[2]) {
        long long* o = reinterpret_cast<long long*>(p.out[2]) + ((blockIdx.x ? 2 : 0) + (wave ? 1 : 0)) * 16;
        for (int i = 0; i < 16; ++i) o[i] = i < ps_n ? ps_t[i] : 0;
    }
#endif
}

}  // namespace quest
