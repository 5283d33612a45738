// Device side of quest_sample_tokens (include/quest_hip.h, "Token sampling"): one workgroup per logits row.
//
// Everything that decides a token is an integer or a function of one element alone, so the result does not depend on how
// waves are scheduled or how partial results are combined:
//   * order: 16-bit key (half_key) descending, token index ascending -- packed as (key << 32 | ~index), larger = earlier;
//   * top-k: a two-level radix over the key (high byte, low byte) with integer LDS counters -> threshold key + tie count;
//   * top-p: the mass of an element is a function of its KEY alone, W(key) = floor(expf((s - m) / T) * 2^40), summed as
//     64-bit integers (LDS integer adds commute exactly) per high byte; the cut is found in the same two levels as
//     count x W(key) per key, in descending key order;
//   * partial ties (only some of the tokens of the boundary key are kept): a two-level radix over the token INDEX of the
//     tokens with that key (2 x 9 bits) -> the largest index kept;
//   * draw: z = (s - m) / T - logf(-logf(u)) with u from Philox4x32-10 of (seed, position, index); argmax of (z, order).
// The row is re-read from L2 for each pass (the lm_head launch has just written it): 1 pass for a greedy row, 3 for a
// sampled one, +1 when the top-p cut falls into another high byte than the top-k threshold, +2 on a partial tie.
#pragma once
#include "quest_common.cuh"

namespace quest {

constexpr uint32_t kSampleMaxVocab = 1u << 18;
constexpr uint32_t kSampleMaxEos = 8;

struct SampleArgs {
    const uint16_t* logits;
    const float* temperature;
    const int32_t* top_k;
    const float* top_p;
    const uint64_t* seed;
    const quest_step_state_t* states;
    const int32_t* positions;
    int32_t* tokens;
    int32_t* kept;
    const int32_t* eos_ids;
    int32_t* finished;
    int32_t* history;
    int32_t* history_len;
    const uint16_t* embed;
    uint16_t* next_input;
    uint32_t logits_stride, vocab, n_eos, history_stride, hidden;
    int32_t pad_id;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's philox4x32).
struct Philox4 {
    uint32_t w[4];
};
__host__ __device__ inline uint32_t philox_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}
// the uniform of a 32-bit word: ((word >> 9) + 0.5) 2^-23, exact in fp32, inside (0, 1)
__host__ __device__ inline float philox_uniform(uint32_t word) { return ((float)(word >> 9) + 0.5f) * 0x1p-23f; }

// 16-bit key <-> stored bits <-> value
__device__ __forceinline__ uint32_t key_bits(uint32_t key) { return (key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xFFFFu); }
template <typename T>
__device__ __forceinline__ float key_value(uint32_t key) {
    const uint32_t b = key_bits(key);
    if constexpr (kIsBf16<T>) return __builtin_bit_cast(float, b << 16);
    else return (float)bits_half((uint16_t)b);
}
template <typename T>
constexpr uint32_t kKeyPosInf = kIsBf16<T> ? 0xFF80u : 0xFC00u;  // keys >= this: +inf and the NaNs with the sign clear
template <typename T>
constexpr uint32_t kKeyNegInf = kIsBf16<T> ? 0x007Fu : 0x03FFu;  // keys < this: the NaNs with the sign set

// f(index, 16 stored bits) for every element of a row that is only 2-byte aligned: scalar head up to the first 16-byte
// boundary, 16-byte loads over the middle, scalar tail.  A thread sees its elements in ascending index order.
template <typename F>
__device__ __forceinline__ void for_each_element(const uint16_t* row, uint32_t V, F&& f) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)row & 15u)) & 15u) >> 1;
    if (head > V) head = V;
    if (tid < head) f(tid, (uint32_t)row[tid]);
    const uint32_t nvec = (V - head) >> 3;
    const uint4* vp = reinterpret_cast<const uint4*>(row + head);
    for (uint32_t v = tid; v < nvec; v += nt) {
        const uint4 q = vp[v];
        const uint32_t j = head + 8u * v;
        f(j + 0, q.x & 0xFFFFu);
        f(j + 1, q.x >> 16);
        f(j + 2, q.y & 0xFFFFu);
        f(j + 3, q.y >> 16);
        f(j + 4, q.z & 0xFFFFu);
        f(j + 5, q.z >> 16);
        f(j + 6, q.w & 0xFFFFu);
        f(j + 7, q.w >> 16);
    }
    const uint32_t t = head + 8u * nvec + tid;
    if (t < V) f(t, (uint32_t)row[t]);
}

struct SampleShared {
    uint32_t cnt[512];              // key high-byte counts; later the token-index counts of a partial tie
    uint32_t lo[256];               // counts per low byte inside one high byte
    unsigned long long mass[256];   // fixed-point mass per high byte; later per low byte
    unsigned long long red[16];
    float redf[16];
    unsigned long long found_excl;
    uint32_t found_bin;
    int32_t token;
};

__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, SampleShared& sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, kWave);
        v = o > v ? o : v;
    }
    const uint32_t wave = threadIdx.x >> 6, nw = (blockDim.x + 63u) >> 6;
    if ((threadIdx.x & 63u) == 0) sh.red[wave] = v;
    __syncthreads();
    v = sh.red[0];
    for (uint32_t w = 1; w < nw; ++w) v = sh.red[w] > v ? sh.red[w] : v;
    __syncthreads();
    return v;
}
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, SampleShared& sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    const uint32_t wave = threadIdx.x >> 6, nw = (blockDim.x + 63u) >> 6;
    if ((threadIdx.x & 63u) == 0) sh.red[wave] = v;
    __syncthreads();
    v = sh.red[0];
    for (uint32_t w = 1; w < nw; ++w) v += sh.red[w];
    __syncthreads();
    return v;
}
// argmax of (z, order): the larger z, on equal z the larger `order` (= the earlier token)
__device__ __forceinline__ unsigned long long block_argmax(float z, unsigned long long order, SampleShared& sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float oz = __shfl_xor(z, off, kWave);
        const unsigned long long oo = __shfl_xor(order, off, kWave);
        if (oz > z || (oz == z && oo > order)) z = oz, order = oo;
    }
    const uint32_t wave = threadIdx.x >> 6, nw = (blockDim.x + 63u) >> 6;
    if ((threadIdx.x & 63u) == 0) sh.redf[wave] = z, sh.red[wave] = order;
    __syncthreads();
    z = sh.redf[0], order = sh.red[0];
    for (uint32_t w = 1; w < nw; ++w) {
        const float oz = sh.redf[w];
        const unsigned long long oo = sh.red[w];
        if (oz > z || (oz == z && oo > order)) z = oz, order = oo;
    }
    __syncthreads();
    return order;
}

// The first position i of 64 * PER values get(0), get(1), ... whose inclusive prefix sum reaches `target` (>= 1, at most
// the total), and the sum in front of it.  Wave 0 scans (PER consecutive values per lane); every thread gets the answer.
// The caller has a barrier between the last write of what `get` reads and this call.
template <int PER, typename G>
__device__ __forceinline__ void block_find_prefix(G&& get, unsigned long long target, SampleShared& sh, uint32_t& bin,
                                                  unsigned long long& excl) {
    if (threadIdx.x < 64u) {
        const uint32_t lane = threadIdx.x;
        if (lane == 0) sh.found_bin = 64u * PER - 1u, sh.found_excl = 0;  // (unreachable for a valid target)
        unsigned long long loc[PER], sum = 0;
#pragma unroll
        for (int p = 0; p < PER; ++p) loc[p] = get(lane * PER + p), sum += loc[p];
        unsigned long long incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_up(incl, (unsigned)off, kWave);
            if (lane >= (uint32_t)off) incl += o;
        }
        unsigned long long run = incl - sum;
        if (run < target && incl >= target) {
            bool done = false;
#pragma unroll
            for (int p = 0; p < PER; ++p) {
                if (!done && run + loc[p] >= target) sh.found_bin = lane * PER + p, sh.found_excl = run, done = true;
                if (!done) run += loc[p];
            }
        }
    }
    __syncthreads();
    bin = sh.found_bin, excl = sh.found_excl;
    __syncthreads();
}

template <typename T>
__device__ __forceinline__ unsigned long long key_mass(uint32_t key, float m, float temperature) {
    return (unsigned long long)(expf((key_value<T>(key) - m) / temperature) * 0x1p40f);
}

template <typename T>
__global__ __launch_bounds__(1024) void sample_tokens_kernel(const SampleArgs a) {
    __shared__ SampleShared sh;
    const uint32_t row_i = blockIdx.x, tid = threadIdx.x, V = a.vocab;
    const uint16_t* row = a.logits + (size_t)row_i * a.logits_stride;
    int32_t token = a.pad_id, kept = 0;
    const bool was_finished = a.finished != nullptr && a.finished[row_i] != 0;
    if (!was_finished) {
        const float temperature = a.temperature[row_i], top_p = a.top_p[row_i];
        const int32_t top_k = a.top_k[row_i];
        const bool sampled = temperature > 0.f && temperature < __builtin_inff();
        for (uint32_t t = tid; t < 256u; t += blockDim.x) sh.cnt[t] = 0, sh.lo[t] = 0, sh.mass[t] = 0;
        __syncthreads();
        // ---- pass 1: the first token of the order, the smallest key, counts per high byte
        unsigned long long best = 0;
        uint32_t inv_min = 0;
        for_each_element(row, V, [&](uint32_t j, uint32_t bits) {
            const uint32_t key = half_key((uint16_t)bits);
            const unsigned long long o = ((unsigned long long)key << 32) | (0xFFFFFFFFu - j);
            best = o > best ? o : best;
            inv_min = max(inv_min, 0xFFFFu - key);
            if (sampled) atomicAdd(&sh.cnt[key >> 8], 1u);
        });
        best = block_max_u64(best, sh);
        const uint32_t max_key = (uint32_t)(best >> 32), min_key = 0xFFFFu - (uint32_t)block_max_u64(inv_min, sh);
        token = (int32_t)(0xFFFFFFFFu - (uint32_t)best);
        kept = 1;
        const uint32_t k_eff = (top_k <= 0 || (uint32_t)top_k > V) ? V : (uint32_t)top_k;
        const bool greedy = !sampled || max_key >= kKeyPosInf<T> || max_key <= kKeyNegInf<T> || min_key < kKeyNegInf<T>;
        if (!greedy && k_eff > 1u && top_p > 0.f) {
            const float m = key_value<T>(max_key);
            // ---- top-k threshold: high byte, then (pass 2) low byte; pass 2 also sums the mass per high byte
            uint32_t pos;
            unsigned long long excl;
            block_find_prefix<4>([&](uint32_t i) { return (unsigned long long)sh.cnt[255u - i]; }, k_eff, sh, pos, excl);
            const uint32_t hi_k = 255u - pos;
            const uint32_t above_hi_k = (uint32_t)excl;
            for_each_element(row, V, [&](uint32_t j, uint32_t bits) {
                const uint32_t key = half_key((uint16_t)bits);
                atomicAdd(&sh.mass[key >> 8], key_mass<T>(key, m, temperature));
                if ((key >> 8) == hi_k) atomicAdd(&sh.lo[key & 255u], 1u);
            });
            __syncthreads();
            block_find_prefix<4>([&](uint32_t i) { return (unsigned long long)sh.lo[255u - i]; }, k_eff - above_hi_k, sh, pos, excl);
            const uint32_t key_k = (hi_k << 8) | (255u - pos);           // the last key of K1
            const uint32_t above_key_k = above_hi_k + (uint32_t)excl;    // tokens with a larger key
            const uint32_t ties_k = k_eff - above_key_k;                 // tokens of key_k inside K1
            const uint32_t full_k = sh.lo[key_k & 255u];                 // tokens of key_k in the row
            uint32_t key_p = key_k, ties_p = ties_k, full_p = full_k;    // the same three for K2
            kept = (int32_t)k_eff;
            if (top_p < 1.f) {
                // K1 in the counters: nothing below key_k, ties_k tokens of key_k; the mass of hi_k follows them
                __syncthreads();
                if (tid < 256u) {
                    if (tid < (key_k & 255u)) sh.lo[tid] = 0;
                    if (tid == (key_k & 255u)) sh.lo[tid] = ties_k;
                    if (tid < hi_k) sh.mass[tid] = 0;
                }
                __syncthreads();
                unsigned long long part = tid < 256u ? sh.lo[tid] * key_mass<T>((hi_k << 8) | tid, m, temperature) : 0ull;
                part = block_sum_u64(part, sh);
                if (tid == 0) sh.mass[hi_k] = part;
                __syncthreads();
                const unsigned long long total = block_sum_u64(tid < 256u ? sh.mass[tid] : 0ull, sh);
                unsigned long long target = (unsigned long long)ceil((double)top_p * (double)total);
                target = target < 1ull ? 1ull : (target > total ? total : target);
                block_find_prefix<4>([&](uint32_t i) { return sh.mass[255u - i]; }, target, sh, pos, excl);
                const uint32_t hi_p = 255u - pos;
                const unsigned long long mass_above_hi_p = excl;
                const uint32_t above_hi_p = (uint32_t)block_sum_u64(tid < 256u && tid > hi_p ? sh.cnt[tid] : 0u, sh);
                if (hi_p != hi_k) {  // ---- pass 3: counts per low byte inside the cut's high byte
                    if (tid < 256u) sh.lo[tid] = 0;
                    __syncthreads();
                    for_each_element(row, V, [&](uint32_t j, uint32_t bits) {
                        const uint32_t key = half_key((uint16_t)bits);
                        if ((key >> 8) == hi_p) atomicAdd(&sh.lo[key & 255u], 1u);
                    });
                    __syncthreads();
                }
                if (tid < 256u) sh.mass[tid] = sh.lo[tid] * key_mass<T>((hi_p << 8) | tid, m, temperature);
                __syncthreads();
                block_find_prefix<4>([&](uint32_t i) { return sh.mass[255u - i]; }, target - mass_above_hi_p, sh, pos, excl);
                key_p = (hi_p << 8) | (255u - pos);
                const unsigned long long w_p = key_mass<T>(key_p, m, temperature);  // > 0: its tokens carried the sum over
                const unsigned long long need = target - mass_above_hi_p - excl;
                const uint32_t in_k1 = sh.lo[key_p & 255u];
                ties_p = w_p ? (uint32_t)((need + w_p - 1ull) / w_p) : in_k1;
                full_p = key_p == key_k ? full_k : in_k1;
                if (ties_p > in_k1) ties_p = in_k1;
                const uint32_t above_lo = (uint32_t)block_sum_u64(tid < 256u && tid > (key_p & 255u) ? sh.lo[tid] : 0u, sh);
                kept = (int32_t)(above_hi_p + above_lo + ties_p);
            }
            // ---- a partial tie: the ties_p lowest token indices of key_p, as the largest index kept
            uint32_t last_tie = 0xFFFFFFFFu;
            if (ties_p < full_p) {
                __syncthreads();
                for (uint32_t t = tid; t < 512u; t += blockDim.x) sh.cnt[t] = 0;
                __syncthreads();
                for_each_element(row, V, [&](uint32_t j, uint32_t bits) {
                    if (half_key((uint16_t)bits) == key_p) atomicAdd(&sh.cnt[j >> 9], 1u);
                });
                __syncthreads();
                block_find_prefix<8>([&](uint32_t i) { return (unsigned long long)sh.cnt[i]; }, ties_p, sh, pos, excl);
                const uint32_t idx_hi = pos, before = (uint32_t)excl;
                for (uint32_t t = tid; t < 512u; t += blockDim.x) sh.cnt[t] = 0;
                __syncthreads();
                for_each_element(row, V, [&](uint32_t j, uint32_t bits) {
                    if (half_key((uint16_t)bits) == key_p && (j >> 9) == idx_hi) atomicAdd(&sh.cnt[j & 511u], 1u);
                });
                __syncthreads();
                block_find_prefix<8>([&](uint32_t i) { return (unsigned long long)sh.cnt[i]; }, ties_p - before, sh, pos, excl);
                last_tie = (idx_hi << 9) | pos;
            }
            if (kept > 1) {
                // ---- the draw over K2
                const uint64_t seed = a.seed[row_i];
                const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
                const uint32_t position = (uint32_t)(a.states ? a.states[row_i].seq_len : a.positions[row_i]);
                float best_z = -__builtin_inff();
                unsigned long long best_o = 0;
                uint32_t group = 0xFFFFFFFFu;
                Philox4 ph = {{0, 0, 0, 0}};
                for_each_element(row, V, [&](uint32_t j, uint32_t bits) {
                    const uint32_t key = half_key((uint16_t)bits);
                    if (key > key_p || (key == key_p && j <= last_tie)) {
                        if ((j >> 2) != group) group = j >> 2, ph = philox4x32_10(group, position, 0x51554553u, 0u, k0, k1);
                        const uint32_t s = j & 3u;
                        const uint32_t word = s == 0 ? ph.w[0] : s == 1 ? ph.w[1] : s == 2 ? ph.w[2] : ph.w[3];
                        const float z = (key_value<T>(key) - m) / temperature - logf(-logf(philox_uniform(word)));
                        const unsigned long long o = ((unsigned long long)key << 32) | (0xFFFFFFFFu - j);
                        if (z > best_z || (z == best_z && o > best_o)) best_z = z, best_o = o;
                    }
                });
                best_o = block_argmax(best_z, best_o, sh);
                token = (int32_t)(0xFFFFFFFFu - (uint32_t)best_o);
            }
        }
    }
    // ---- outputs: one thread writes the row's records, then the whole workgroup copies the embedding row
    if (tid == 0) {
        if ((uint32_t)token >= V) token = 0;  // (cannot happen: every path above ends on an index of the row)
        a.tokens[row_i] = token;
        if (a.kept) a.kept[row_i] = kept;
        if (!was_finished) {
            if (a.finished) {
                bool eos = false;
                for (uint32_t e = 0; e < a.n_eos; ++e) eos |= a.eos_ids[e] == token;
                if (eos) a.finished[row_i] = 1;
            }
            if (a.history) {
                const int32_t len = a.history_len[row_i];
                if (len >= 0 && (uint32_t)len < a.history_stride) {
                    a.history[(size_t)row_i * a.history_stride + (uint32_t)len] = token;
                    a.history_len[row_i] = len + 1;
                }
            }
        }
        sh.token = token;
    }
    if (a.embed) {
        __syncthreads();
        const uint16_t* src = a.embed + (size_t)sh.token * a.hidden;
        uint16_t* dst = a.next_input + (size_t)row_i * a.hidden;
        if ((a.hidden & 7u) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
            for (uint32_t c = tid; c < (a.hidden >> 3); c += blockDim.x)
                reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
        } else {
            for (uint32_t c = tid; c < a.hidden; c += blockDim.x) dst[c] = src[c];
        }
    }
}

}  // namespace quest
