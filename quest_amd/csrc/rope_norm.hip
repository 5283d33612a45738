// RoPE in place on q/k and RMSNorm -- the two remaining `_kernels` ops the decode layer calls
// around the sparse path (SURVEY.md 8f "next" rows, built so the whole operator surface is native).
//
// Reference behaviour restated (not translated):
//   rope     QKApplyRotaryInPlaceKernel   kernels/include/decode/decode_page.cuh:644-692
//            (rotate-half, freq_i = (1/scale) * theta^(-2*(i mod D/2)/D), position = past_len + row)
//            table form (llama3 / yarn scaling): freq_i = inv_freq[i mod D/2], cos and sin times attention_factor
//   rmsnorm  rmsnorm_twoPassAlgo_e8       quest/ops/csrc/rms_norm.cu:82-158
//   q/k norm + rope (EXTENSION: Qwen3's per-head RMSNorm of q and k, no counterpart in the reference): one pass over the
//            head row, see qk_norm_rope_body
// Both are elementwise / one-row reductions: HBM-bound, 16 B per lane accesses.
#include <cmath>

#include "quest_common.cuh"

namespace quest {

#define QUEST_ROPE_PARAMS                                                                                         \
    half_t *__restrict__ q, half_t *__restrict__ k, uint32_t n, uint32_t past_len, uint32_t hq, uint32_t hk,      \
        float rcp_scale, float log2_rcp_theta, const float *__restrict__ inv_freq, float attn, const quest_step_state_t *state
// T: the element type of q and k (the arithmetic is fp32 either way; the result is rounded to T once, to nearest even)
template <typename T, int D>
__device__ __forceinline__ void rope_body(QUEST_ROPE_PARAMS) {
    // state-driven: row i is the decode token of sequence i (one row for a single sequence)
    // inv_freq (uniform): NULL = the formula, else the [D/2] frequency table with cos / sin scaled by attn
    constexpr int LPR = D / kVec;
    constexpr int RPB = 256 / LPR;  // vectors per block
    const uint32_t vec = blockIdx.x * RPB + threadIdx.x / LPR;
    const int col = threadIdx.x % LPR;
    const uint32_t per_tok = hq + hk;
    if (vec >= n * per_tok) return;
    const uint32_t tok = vec / per_tok, h = vec % per_tok;
    half_t* x = (h < hq) ? q + ((size_t)tok * hq + h) * D : k + ((size_t)tok * hk + (h - hq)) * D;
    x += col * kVec;
    const float8 self = to_f32<T>(ld8(x));
    const float pos = state ? (float)(state[tok].seq_len - 1) : (float)(past_len + tok);
    float8 out;
#pragma unroll
    for (int i = 0; i < kVec; ++i) {
        const int d = col * kVec + i;
        // partner element d +- D/2 lives in lane col +- LPR/2, same i
        const float other = __shfl_xor(self[i], LPR / 2, kWave);
        const float freq = inv_freq ? inv_freq[d % (D / 2)]
                                    : rcp_scale * exp2f(log2_rcp_theta * (float)(2 * (d % (D / 2))) / (float)D);
        float s, c;
        sincosf(pos * freq, &s, &c);
        if (inv_freq) s *= attn, c *= attn;
        out[i] = self[i] * c + (d < D / 2 ? -other : other) * s;
    }
    st8(x, from_f32<T>(out));
}
template <int D>
__global__ __launch_bounds__(256) void rope_kernel(QUEST_ROPE_PARAMS) {
    rope_body<half_t, D>(q, k, n, past_len, hq, hk, rcp_scale, log2_rcp_theta, inv_freq, attn, state);
}
template <int D>
__global__ __launch_bounds__(256) void rope_kernel_bf16(QUEST_ROPE_PARAMS) {
    rope_body<bf16_t, D>(q, k, n, past_len, hq, hk, rcp_scale, log2_rcp_theta, inv_freq, attn, state);
}

// Per-head RMSNorm of q and k (weights wq / wk: [D], shared by the heads) fused with the rotation above, in place, one
// pass: the row of a head is the LPR = D / 8 lanes of rope_body, so the sum of squares is a DPP reduction over exactly
// those 8 / 16 / 32 lanes (row_allreduce_sum_fast: every lane of the row ends with the same bits) -- no LDS, no second
// read.  fp32 throughout: inv = 1 / sqrtf(sum x^2 / D + eps) (rms_norm_body's form), n_d = x_d * inv * w_d, rotate-half
// on n, ONE rounding to T.  Deviation from transformers' Qwen3 (Qwen3RMSNorm then apply_rotary_pos_emb in the model's
// type): that rounds x * inv to T, rounds the product with the weight to T, and rounds cos / sin to T before the
// rotation; this kernel keeps all of them in fp32, so it is the closer of the two to the fp32 model (the logits tests of
// tests/test_gpu_model_families.py are the arbiter).
#define QUEST_QK_NORM_ROPE_PARAMS QUEST_ROPE_PARAMS, const half_t *__restrict__ wq, const half_t *__restrict__ wk, float eps
template <typename T, int D>
__device__ __forceinline__ void qk_norm_rope_body(QUEST_QK_NORM_ROPE_PARAMS) {
    constexpr int LPR = D / kVec;
    constexpr int RPB = 256 / LPR;
    const uint32_t vec = blockIdx.x * RPB + threadIdx.x / LPR;
    const int col = threadIdx.x % LPR;
    const uint32_t per_tok = hq + hk;
    if (vec >= n * per_tok) return;  // whole rows leave together: the cross-lane steps below stay inside a row
    const uint32_t tok = vec / per_tok, h = vec % per_tok;
    half_t* x = (h < hq) ? q + ((size_t)tok * hq + h) * D : k + ((size_t)tok * hk + (h - hq)) * D;
    x += col * kVec;
    const float8 self = to_f32<T>(ld8(x)), g = to_f32<T>(ld8((h < hq ? wq : wk) + col * kVec));
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < kVec; ++i) ss = __builtin_fmaf(self[i], self[i], ss);
    ss = row_allreduce_sum_fast<LPR>(ss);
    const float inv = 1.0f / sqrtf(ss / (float)D + eps);
    const float pos = state ? (float)(state[tok].seq_len - 1) : (float)(past_len + tok);
    float8 out;
#pragma unroll
    for (int i = 0; i < kVec; ++i) {
        const int d = col * kVec + i;
        const float nrm = self[i] * inv * g[i];
        // partner element d +- D/2 (normalised with ITS weight) lives in lane col +- LPR/2, same i
        float other;
        if constexpr (LPR / 2 == 4) other = __shfl_xor(nrm, 4, kWave);
        else other = lane_xor<LPR / 2>(nrm, (int)(threadIdx.x & 63));
        const float freq = inv_freq ? inv_freq[d % (D / 2)]
                                    : rcp_scale * exp2f(log2_rcp_theta * (float)(2 * (d % (D / 2))) / (float)D);
        float s, c;
        sincosf(pos * freq, &s, &c);
        if (inv_freq) s *= attn, c *= attn;
        out[i] = nrm * c + (d < D / 2 ? -other : other) * s;
    }
    st8(x, from_f32<T>(out));
}
template <int D>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(QUEST_QK_NORM_ROPE_PARAMS) {
    qk_norm_rope_body<half_t, D>(q, k, n, past_len, hq, hk, rcp_scale, log2_rcp_theta, inv_freq, attn, state, wq, wk, eps);
}
template <int D>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel_bf16(QUEST_QK_NORM_ROPE_PARAMS) {
    qk_norm_rope_body<bf16_t, D>(q, k, n, past_len, hq, hk, rcp_scale, log2_rcp_theta, inv_freq, attn, state, wq, wk, eps);
}

template <typename T>
__device__ __forceinline__ void rms_norm_body(const half_t* __restrict__ in, const half_t* __restrict__ w,
                                              half_t* __restrict__ out, uint32_t cols, float eps) {
    __shared__ float s_part[16];
    __shared__ float s_inv;
    const size_t row = blockIdx.x;
    const half_t* x = in + row * cols;
    float ss = 0.f;
    for (uint32_t c = threadIdx.x * kVec; c < cols; c += blockDim.x * kVec) {
        const float8 v = to_f32<T>(ld8(x + c));
#pragma unroll
        for (int i = 0; i < kVec; ++i) ss = __builtin_fmaf(v[i], v[i], ss);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) ss += __shfl_xor(ss, off, kWave);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (uint32_t i = 0; i < (blockDim.x + 63) / 64; ++i) t += s_part[i];
        s_inv = 1.0f / sqrtf(t / (float)cols + eps);
    }
    __syncthreads();
    const float inv = s_inv;
    for (uint32_t c = threadIdx.x * kVec; c < cols; c += blockDim.x * kVec) {
        const float8 v = to_f32<T>(ld8(x + c)), g = to_f32<T>(ld8(w + c));
        float8 r;
#pragma unroll
        for (int i = 0; i < kVec; ++i) r[i] = v[i] * inv * g[i];
        st8(out + row * cols + c, from_f32<T>(r));
    }
}
__global__ __launch_bounds__(1024) void rms_norm_kernel(const half_t* __restrict__ in, const half_t* __restrict__ w,
                                                        half_t* __restrict__ out, uint32_t cols, float eps) {
    rms_norm_body<half_t>(in, w, out, cols, eps);
}
__global__ __launch_bounds__(1024) void rms_norm_kernel_bf16(const half_t* __restrict__ in, const half_t* __restrict__ w,
                                                             half_t* __restrict__ out, uint32_t cols, float eps) {
    rms_norm_body<bf16_t>(in, w, out, cols, eps);
}

}  // namespace quest

using namespace quest;

static int rope_launch(void* q, void* k, uint32_t n, uint32_t past_kv_len, uint32_t num_qo_heads, uint32_t num_kv_heads,
                       uint32_t head_dim, float rcp_scale, float log2_rcp_theta, const float* inv_freq, float attn,
                       const quest_step_state_t* state, quest_stream_t stream, uint32_t dtype) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!q || !k || num_qo_heads == 0 || num_kv_heads == 0) return QUEST_EINVAL;
    if (n == 0) return 0;
    const bool bf = dtype == QUEST_DTYPE_BF16;
    const uint32_t vecs = n * (num_qo_heads + num_kv_heads);
    hipStream_t s = (hipStream_t)stream;
#define QUEST_ROPE_CASE(DD)                                                                                       \
    case DD: {                                                                                                    \
        const uint32_t rpb = 256 / (DD / kVec);                                                                   \
        hipLaunchKernelGGL((bf ? rope_kernel_bf16<DD> : rope_kernel<DD>), dim3((vecs + rpb - 1) / rpb), dim3(256), 0, s, (half_t*)q,          \
                           (half_t*)k, n, past_kv_len, num_qo_heads, num_kv_heads, rcp_scale, log2_rcp_theta,    \
                           inv_freq, attn, state);                                                               \
        break;                                                                                                    \
    }
    switch (head_dim) {
        QUEST_ROPE_CASE(64)
        QUEST_ROPE_CASE(128)
        QUEST_ROPE_CASE(256)
        default: return QUEST_EUNSUPPORTED;
    }
#undef QUEST_ROPE_CASE
    QUEST_LAUNCH_CHECK();
    return 0;
}

// The two operators that come with neither a pool view nor a handler get ONE typed entry each (the element type as an
// argument); the entries with the reference's argument lists mean fp16.
extern "C" int quest_apply_rope_in_place_dtype(void* q, void* k, uint32_t n, uint32_t past_kv_len, uint32_t num_qo_heads,
                                               uint32_t num_kv_heads, uint32_t head_dim, float rope_scale, float rope_theta,
                                               const float* inv_freq, float attention_factor,
                                               const quest_step_state_t* states, uint32_t dtype, quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (inv_freq) {
        if (bad_rope_table(inv_freq, attention_factor)) return QUEST_EINVAL;
        return rope_launch(q, k, n, past_kv_len, num_qo_heads, num_kv_heads, head_dim, 1.0f, 0.f, inv_freq, attention_factor,
                           states, stream, dtype);
    }
    if (rope_scale == 0.f || rope_theta <= 0.f) return QUEST_EINVAL;
    return rope_launch(q, k, n, past_kv_len, num_qo_heads, num_kv_heads, head_dim, 1.0f / rope_scale, -log2f(rope_theta),
                       nullptr, 1.0f, states, stream, dtype);
}

extern "C" int quest_apply_rope_in_place(void* q, void* k, uint32_t n, uint32_t past_kv_len, uint32_t num_qo_heads,
                                         uint32_t num_kv_heads, uint32_t head_dim, float rope_scale, float rope_theta,
                                         quest_stream_t stream) {
    return quest_apply_rope_in_place_dtype(q, k, n, past_kv_len, num_qo_heads, num_kv_heads, head_dim, rope_scale, rope_theta,
                                           nullptr, 1.0f, nullptr, QUEST_DTYPE_F16, stream);
}

// Per-head q/k RMSNorm + RoPE in place (qk_norm_rope_kernel): the rows and the position sources of
// quest_apply_rope_in_place_dtype (states NULL: row i at past_kv_len + i; else row i = the decode token of states[i]).
extern "C" int quest_apply_qk_norm_rope_in_place_dtype(void* q, void* k, uint32_t n, uint32_t past_kv_len,
                                                       uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t head_dim,
                                                       const void* q_norm_weight, const void* k_norm_weight, float eps,
                                                       float rope_scale, float rope_theta, const float* inv_freq,
                                                       float attention_factor, const quest_step_state_t* states,
                                                       uint32_t dtype, quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!q || !k || !q_norm_weight || !k_norm_weight || num_qo_heads == 0 || num_kv_heads == 0) return QUEST_EINVAL;
    if (!(eps >= 0.f) || !std::isfinite(eps)) return QUEST_EINVAL;
    float rcp_scale = 1.0f, log2_rcp_theta = 0.f, attn = 1.0f;
    if (inv_freq) {
        if (bad_rope_table(inv_freq, attention_factor)) return QUEST_EINVAL;
        attn = attention_factor;
    } else {
        if (rope_scale == 0.f || rope_theta <= 0.f) return QUEST_EINVAL;
        rcp_scale = 1.0f / rope_scale, log2_rcp_theta = -log2f(rope_theta);
    }
    if (head_dim != 64 && head_dim != 128 && head_dim != 256) return QUEST_EUNSUPPORTED;
    if (n == 0) return 0;
    const bool bf = dtype == QUEST_DTYPE_BF16;
    const uint32_t vecs = n * (num_qo_heads + num_kv_heads);
    hipStream_t s = (hipStream_t)stream;
#define QUEST_QK_NORM_ROPE_CASE(DD)                                                                                          \
    case DD: {                                                                                                               \
        const uint32_t rpb = 256 / (DD / kVec);                                                                              \
        hipLaunchKernelGGL((bf ? qk_norm_rope_kernel_bf16<DD> : qk_norm_rope_kernel<DD>), dim3((vecs + rpb - 1) / rpb),      \
                           dim3(256), 0, s, (half_t*)q, (half_t*)k, n, past_kv_len, num_qo_heads, num_kv_heads, rcp_scale,   \
                           log2_rcp_theta, inv_freq, attn, states, (const half_t*)q_norm_weight,                             \
                           (const half_t*)k_norm_weight, eps);                                                               \
        break;                                                                                                               \
    }
    switch (head_dim) {
        QUEST_QK_NORM_ROPE_CASE(64)
        QUEST_QK_NORM_ROPE_CASE(128)
        QUEST_QK_NORM_ROPE_CASE(256)
        default: return QUEST_EUNSUPPORTED;
    }
#undef QUEST_QK_NORM_ROPE_CASE
    QUEST_LAUNCH_CHECK();
    return 0;
}

static int rms_norm(const void* input, const void* weight, void* output, uint32_t rows, uint32_t cols, float epsilon,
                    uint32_t dtype, quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!input || !weight || !output) return QUEST_EINVAL;
    if (cols == 0 || cols % 8 != 0) return QUEST_EUNSUPPORTED;  // rms_norm.cu:164-166
    if (rows == 0) return 0;
    uint32_t threads = (cols / 8 + 63) / 64 * 64;
    if (threads > 1024) threads = 1024;
    hipLaunchKernelGGL((dtype == QUEST_DTYPE_BF16 ? rms_norm_kernel_bf16 : rms_norm_kernel), dim3(rows), dim3(threads), 0, (hipStream_t)stream, (const half_t*)input,
                       (const half_t*)weight, (half_t*)output, cols, epsilon);
    QUEST_LAUNCH_CHECK();
    return 0;
}

extern "C" int quest_rms_norm_forward(const void* input, const void* weight, void* output, uint32_t rows, uint32_t cols,
                                      float epsilon, quest_stream_t stream) {
    return rms_norm(input, weight, output, rows, cols, epsilon, QUEST_DTYPE_F16, stream);
}

extern "C" int quest_rms_norm_forward_dtype(const void* input, const void* weight, void* output, uint32_t rows, uint32_t cols,
                                            float epsilon, uint32_t dtype, quest_stream_t stream) {
    return rms_norm(input, weight, output, rows, cols, epsilon, dtype, stream);
}
