// Batch-1 decode-token projections around the sparse attention path, fused so that a decoder layer is 4 launches besides
// its attention (EXTENSION, SURVEY.md 8f-4 "drop into the HF pipeline" / VERDICT r2 item 8).
//
// The reference leaves these to cuBLAS + small PyTorch kernels: per layer RMSNorm (quest/ops/csrc/rms_norm.cu:82-213,
// called at quest/models/llama.py:72), q/k/v projections (QuestAttention.py:64-66), RoPE (decode_page.cuh:644-728 via
// QuestAttention.py:70), o_proj (:118), residual adds, gate/up projections, SiLU * up, down projection
// (llama.py LlamaMLP) -- 14 launches of which 7 are fp16 GEMVs (M = 1) that stream the layer's 386 MiB of weights.
// On MI355X a decode token of Llama-2-7B spent 4.5 of its 5.4 ms there (~450 launches, profiles/r02_e2e_*).  Here:
//
//   quest_decode_qkv_rope      h -> RMSNorm -> [Wq; Wk; Wv] x -> RoPE(q, k) -> q, k, v          (1 launch)
//   quest_decode_gemv_residual h += W x            (o_proj on the attention output, down_proj on the MLP activation)
//   quest_decode_mlp_gate_up   h -> RMSNorm -> SiLU(Wg x) * (Wu x)                               (1 launch)
//   quest_decode_norm_gemv     h -> RMSNorm -> W x                                               (final norm + lm_head)
//
// One kernel: 8-wave workgroups, a wave owns 1 / 2 / 4 output row-dots (the host picks the largest count that still gives
// two workgroups per CU), a lane every 64th 16-byte vector of a row, 8 loads of 16 bytes in flight per lane (80-90 VGPRs,
// 128 KiB in flight per CU), fp16 x fp16 -> fp32 by v_dot2_f32_f16; the input vector sits in LDS (normalised there when the
// launch carries a RMSNorm prologue -- every workgroup recomputes the 8 KiB reduction rather than pay a launch for it),
// the weight loads of the first round are issued BEFORE the prologue so its latency hides under them.  HBM-bound
// (weights read exactly once): 4.9-5.7 TB/s at Llama-2-7B shapes; no MFMA: M = 1.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "quest_common.cuh"

namespace quest {

// Workgroup shape: NWV waves, RW row-dots per wave, U iterations (x 64 lanes x 16 B x RW rows) in flight -- template
// parameters picked by the host (launch_gemv): 8-wave workgroups so that the input vector is staged in LDS once per
// 8-32 rows (with 4-wave, 4-row workgroups the 22 KiB vector of down_proj was re-staged 1024 times: +26 % of L2 traffic),
// and the largest RW that still gives >= 2 workgroups per CU.  Round-3 history (profiles/r03_e2e_kernel_stats*.csv):
// 4 x 4 rows everywhere -> o_proj / down_proj at 3.9 TB/s (256 workgroups: one per CU); 1 row per wave there -> 4.5-4.9.
enum GemvMode { kGvPlain = 0, kGvResidual = 1, kGvSiluMul = 2, kGvQkvRope = 3 };

struct GemvArgs {
    const half_t* x;       // [in_dim] input vector
    const half_t* gamma;   // RMSNorm weight [in_dim] or nullptr (no prologue)
    float eps;
    uint32_t in_dim;       // multiple of 8
    const half_t* w[3];    // row-major [rows[i]][in_dim]
    uint32_t rows[3];
    half_t* out[3];
    const half_t* residual;  // kGvResidual: out[0][r] = residual[r] + W[r] . x  (may alias out[0])
    // kGvQkvRope: w = {Wq, Wk, Wv}; rotate-half RoPE on the first two (decode_page.cuh:644-692)
    uint32_t head_dim;
    float rcp_scale, log2_rcp_theta;
    const quest_step_state_t* state;  // position = state->seq_len - 1
    // frequency table form (llama3 / yarn): NULL = the formula above; else freq_d = inv_freq[d] ([head_dim / 2] fp32) and
    // cos / sin scaled by attn_factor
    const float* inv_freq;
    float attn_factor;
};

// (cos, sin) of RoPE pair d at position pos: the formula, or the frequency table (p.inv_freq: uniform)
__device__ __forceinline__ void rope_cos_sin(const GemvArgs& p, uint32_t d, float pos, float& cs, float& sn) {
    const float freq = p.inv_freq ? p.inv_freq[d] : p.rcp_scale * exp2f(p.log2_rcp_theta * (float)(2 * d) / (float)p.head_dim);
    sincosf(pos * freq, &sn, &cs);
    if (p.inv_freq) sn *= p.attn_factor, cs *= p.attn_factor;
}

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// 8 products of stored elements of type T onto an fp32 accumulator: four packed dots (v_dot2_f32_f16 / v_dot2c_f32_bf16)
template <typename T>
__device__ __forceinline__ float dot8(const half8& a, const half8& b, float acc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const half2_t x = {a[2 * i], a[2 * i + 1]}, y = {b[2 * i], b[2 * i + 1]};
        if constexpr (kIsBf16<T>) acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, x), __builtin_bit_cast(bf16x2, y), acc, false);
        else acc = __builtin_amdgcn_fdot2(x, y, acc, false);
    }
    return acc;
}
// ---------------------------------------------------------------------------------------------------------------------
// The same four launches for n <= 16 decode tokens at once (one per sequence of a batch: BatchedInferenceController).
// The weights are still read exactly once, so the launch is as HBM-bound as the batch-1 one, but 8 tokens x 2 flops per
// weight no longer fit the vector ALUs next to the loads (44 TFLOP/s of v_dot2 at 5.5 TB/s): the products go through the
// matrix cores -- in the one MFMA shape whose operand layout IS a coalesced row sweep.
//
//   v_mfma_f32_4x4x4_16B_f16 = 16 independent 4 x 4 x 4 products, lane 4b + i holding row i of block b's A, lane 4b + j
//   column j of its B (4 halves each), lane 4b + j column j of its D (4 floats).  With block = a k chunk, A = 4 tokens and
//   B = 4 weight rows, a lane (b, j) loads 16 contiguous bytes of weight row j at k = 128 s + 8 b: one wave instruction
//   reads 4 rows x 256 contiguous bytes -- full 128-byte lines, like the batch-1 kernel -- and feeds two MFMAs (k halves)
//   per token group with no staging and no shuffle.  (The 16 x 16 x 32 shape, first version of this kernel, wants 16 rows
//   x 64 bytes per instruction: twice the lines per byte through the texture addresser -- 3.1 TB/s against 5.1-5.6.)
//   The tokens' inputs are loaded the same way (lane (b, i): token i, same k chunk; L2 hits, 4 tokens x 256 bytes per
//   instruction), 0.5 input bytes per weight byte at 8 tokens x 16 rows; the RMSNorm prologue is applied to that
//   fragment in registers (x * inv_rms[token] * gamma, rounded to fp16 like rms_norm_forward), gamma from LDS.
//
//   workgroup = 16 consecutive (virtual) weight rows (4 quads) x the whole reduction, split over its NW waves by k: wave w
//   takes the 128-wide k steps w, w + NW, ...; U steps in flight per lane.  The 16 k chunks of a lane's accumulators meet
//   by DPP at the end of the wave, the waves' 16 x n tiles in LDS; 128 threads then own one (token, row pair) each and
//   run the same epilogues as the batch-1 kernel.  TG = token groups of 4 (n <= 4 TG).
struct SkinnyArgs {
    GemvArgs g;              // x: [n_tokens][x_stride], out[i]: [n_tokens][out_stride[i]], residual like out[0]
    uint32_t n_tokens;       // 1..16
    uint32_t x_stride;       // halves between the inputs of consecutive tokens
    uint32_t out_stride[3];  // halves between the outputs of consecutive tokens
    uint32_t state_stride;   // kGvQkvRope: quest_step_state_t records between consecutive tokens' states (batched state: 1)
};

typedef float float4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

// (matrix, row) of virtual row vr of a launch (the batch-1 kernel's order: gate / up interleaved; rotation pairs adjacent)
template <int MODE>
__device__ __forceinline__ bool skinny_row(const GemvArgs& p, uint32_t vr, uint32_t& m, uint32_t& rr) {
    bool live;
    m = 0;
    if constexpr (MODE == kGvSiluMul) {
        m = vr & 1u, rr = vr >> 1, live = rr < p.rows[0];
    } else {
        while (m < 2 && vr >= p.rows[m]) vr -= p.rows[m], ++m;
        live = vr < p.rows[m], rr = vr;
        if constexpr (MODE == kGvQkvRope) {
            const uint32_t hd = p.head_dim, head = rr / hd, j = rr % hd;
            rr = head * hd + (j >> 1) + (j & 1u) * (hd / 2);
        }
    }
    return live;
}

// D += A B of sixteen 4 x 4 x 4 blocks of stored elements of type T (v_mfma_f32_4x4x4_16b_f16 / _bf16: one operand layout)
template <typename T>
__device__ __forceinline__ float4_t mfma_4x4x4(half4_t a, half4_t b, float4_t c) {
    if constexpr (kIsBf16<T>) return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(bf16x4, a), __builtin_bit_cast(bf16x4, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_4x4x4f16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// The n-token launches proper: ONE 16-wave workgroup per CU, resident for the whole launch, with the tokens' inputs --
// normalised once -- in ITS LDS (8 tokens x 4096 x 2 bytes = 64 KiB of the CU's 160), so that the weight stream is the
// only thing that crosses the memory system: the first n-token kernel above re-reads the inputs from L2 for every 16 rows
// (0.5 bytes per weight byte, and a RMSNorm per fragment); the batch-1 kernel with 8 accumulators per row-dot spends the
// vector ALUs (61 us against 32 for the gate/up launch).
//
//   task = one quad of weight rows (the B operand of the 4x4x4 MFMA: lane (b, j) = 16 bytes of row j at k chunk b, a
//   fully coalesced 4 x 256-byte sweep) x one of `ks` interleaved k slices (k steps slice, slice + ks, ...: at most CM
//   per task).  A wave holds TWO sets of CM fragments: it requests the next task's set, then consumes the current one
//   against the A fragments (lane (b, i) = token i, chunk b) read from LDS -- row stride = 64 bytes mod 256, conflict-free
//   for ds_read_b128's four 16-lane groups -- so a task's loads fly during the previous task's MFMAs, its k-chunk
//   reduction (8 TG values by DPP), and the round's barrier.  The 16 waves of the workgroup = 16 / ks quads x ks slices;
//   the slices of a quad meet in LDS (double-buffered, one barrier per round), (quad, row pair, token) threads run the
//   batch-1 kernel's epilogues.  Rounds: quad = (round x workgroups + workgroup) x (16 / ks) + wave / ks.
//
//   Inputs too large for LDS (down_proj: 8 x 11008 x 2 = 172 KiB) take the first kernel.  (Staging them in k ranges through
//   two LDS buffers, the accumulators living across the ranges, was built and measured: 32.8 us against that kernel's
//   23.7 at 8 tokens -- removed.)
//
//   Order of requests (in-kernel stamps, scripts/ps_timeline.py): a CU's memory pipeline holds about 64 KiB of requests;
//   a wave whose loads do not fit stalls at issue (up to 4 us at the start of a launch), and a wave's loads return in
//   order.  The prologue requests the inputs first (every wave its share, a bare barrier so that all 16 have, before
//   anybody's weights), normalises and stores them, and then starts the weights; with the first weight set requested
//   ahead of the inputs the launch takes the same time (37.3 vs 37.1 us).
constexpr int kPsWaves = 16, kCM = 4;  // kCM: k steps per task = fragments per set (two sets of 8 spill next to the inputs' registers)
// input vectors (16 bytes) per thread and staged range: 4096 per workgroup, 8192 for 9-16 tokens
constexpr int ps_input_vectors(int tg) { return (tg <= 2 ? 64 : 128) / kPsWaves; }
struct PersistPlan {
    uint32_t ks, ks_log2;     // k slices per quad (power of two <= 16)
    uint32_t rounds;
    uint32_t spp;             // 128-wide k steps of a row
    uint32_t x_row;           // halves between tokens in LDS (>= 128 spp, = 32 mod 128)
    uint32_t n_quads;
    uint32_t vpp_magic;       // ceil(2^32 / (16 spp)): e / (16 spp) = umulhi(e, magic) for e < 2^16
};

// dynamic LDS a workgroup may ask for: the CU's 160 KiB less the kernel's static arrays (s_part 2 TG KiB, the rotation table
// 4 TG KiB, s_ssq <= 1 KiB, s_inv) and some slack -- persist_kernel checks the sum at compile time
constexpr size_t kCuLdsBytes = 160 * 1024;
constexpr size_t persist_lds_budget(uint32_t tg, bool rope) { return (size_t)(158 - tg * (2 + (rope ? 4 : 0))) * 1024; }

}  // namespace quest

// gemv_kernel, skinny_kernel, persist_kernel and their bf16 forms <name>_b16: decode_layer_kernels_typed.cuh, once per
// element type.  (_b16, not the attention path's _bf16: tests/test_bf16_host.py counts the kernels named _bf16 against
// the attention path's fp16 kernels, one twin each with the same template arguments, and these are not among them.)
#define QUEST_ELEM half_t
#define QUEST_KNAME(n) n
#include "decode_layer_kernels_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME
#define QUEST_ELEM bf16_t
#define QUEST_KNAME(n) n##_b16
#include "decode_layer_kernels_typed.cuh"
#undef QUEST_ELEM
#undef QUEST_KNAME

namespace quest {

template <int MODE, int NWV, int RW, int U>
static int launch_gemv_rw(const GemvArgs& p, uint32_t virtual_rows, hipStream_t s, bool bf) {
    const uint32_t n_vec = p.in_dim / kVec, iters = (n_vec + kWave - 1) / kWave;
    const uint32_t outer = (iters + U - 1) / U;
    const size_t lds = (size_t)outer * U * kWave * kVec * sizeof(half_t);
    if (lds > 60 * 1024) return QUEST_EUNSUPPORTED;  // in_dim <= 30720
    const uint32_t per_wg = NWV * RW;
    hipLaunchKernelGGL((bf ? gemv_kernel_b16<MODE, NWV, RW, U> : gemv_kernel<MODE, NWV, RW, U>), dim3((virtual_rows + per_wg - 1) / per_wg),
                       dim3(NWV * kWave), lds, s, p);
    QUEST_LAUNCH_CHECK();
    return 0;
}

// 8-wave workgroups, 8 loads of 16 bytes in flight per lane (RW x U = 8: <= 100 VGPRs, two workgroups = 16 waves = 128 KiB
// in flight per CU, the attention kernel's shape; 16 per lane needed 146-176 VGPRs and spilled under the 128 cap);
// the largest rows-per-wave that still gives two workgroups per CU (512).  QUEST_GEMV_CFG="RW,U" forces one of the
// built shapes (tuning).
template <int MODE>
static int launch_gemv(const GemvArgs& p, uint32_t virtual_rows, hipStream_t s, bool bf) {
    constexpr uint32_t kWant = 512;
    static const int forced = [] {
        const char* e = quest_tuning_env("QUEST_GEMV_CFG");
        int rw = 0, u = 0;
        return e && sscanf(e, "%d,%d", &rw, &u) == 2 ? rw * 100 + u : 0;
    }();
    constexpr bool kPairs = !(MODE == kGvPlain || MODE == kGvResidual);  // row-dots come in pairs: RW even
    switch (forced) {
        case 402: return launch_gemv_rw<MODE, 8, 4, 2>(p, virtual_rows, s, bf);
        case 204: return launch_gemv_rw<MODE, 8, 2, 4>(p, virtual_rows, s, bf);
        case 401: return launch_gemv_rw<MODE, 8, 4, 1>(p, virtual_rows, s, bf);
        case 202: return launch_gemv_rw<MODE, 8, 2, 2>(p, virtual_rows, s, bf);
        case 201: return launch_gemv_rw<MODE, 8, 2, 1>(p, virtual_rows, s, bf);
        case 104: if constexpr (!kPairs) return launch_gemv_rw<MODE, 8, 1, 4>(p, virtual_rows, s, bf); break;
        case 102: if constexpr (!kPairs) return launch_gemv_rw<MODE, 8, 1, 2>(p, virtual_rows, s, bf); break;
        case 108: if constexpr (!kPairs) return launch_gemv_rw<MODE, 8, 1, 8>(p, virtual_rows, s, bf); break;
        default: break;
    }
    if (virtual_rows / (8 * 4) >= kWant) return launch_gemv_rw<MODE, 8, 4, 2>(p, virtual_rows, s, bf);
    if constexpr (!kPairs) {
        if (virtual_rows / (8 * 2) >= kWant) return launch_gemv_rw<MODE, 8, 2, 4>(p, virtual_rows, s, bf);
        // the staged vector is padded to whole rounds: U = 8 rounds (4096 halves) end at 28672 under the 60 KiB stage, U = 4
        // rounds (2048) reach the 30720 the other two shapes serve
        if (p.in_dim > 7 * 8 * kWave * kVec) return launch_gemv_rw<MODE, 8, 1, 4>(p, virtual_rows, s, bf);
        return launch_gemv_rw<MODE, 8, 1, 8>(p, virtual_rows, s, bf);
    } else {
        return launch_gemv_rw<MODE, 8, 2, 4>(p, virtual_rows, s, bf);
    }
}


// One 8-wave workgroup per CU (two waves per SIMD: 256 VGPRs each -- U x (4 + TG) fragments of 16 bytes in flight per lane
// next to 16 TG accumulators; 128 KiB of weights in flight per CU at U = 4.  16 waves at 128 VGPRs spilled from TG = 2 on).
// The fallback of the persistent kernel below: any n x in_dim, inputs from L2 (3.0-3.8 TB/s at 8 tokens).
template <int MODE, int TG>
static int launch_skinny_tg(const SkinnyArgs& a, uint32_t blocks, size_t lds, hipStream_t s, bool bf) {
    constexpr int U = TG <= 2 ? 4 : 2;
    // bf16 at 9-16 tokens: one step in flight -- with two, the 16 accumulator tiles, the fragments and the bf16 conversions'
    // temporaries do not fit the 256 registers (10-12 spilled; the fp16 kernel spills 8-10 there and is left as it is)
    constexpr int UB = TG <= 2 ? 4 : 1;
    hipLaunchKernelGGL((bf ? skinny_kernel_b16<MODE, 8, UB, TG> : skinny_kernel<MODE, 8, U, TG>), dim3(blocks), dim3(8 * kWave), lds, s, a);
    QUEST_LAUNCH_CHECK();
    return 0;
}
template <int MODE>
static int launch_skinny(const SkinnyArgs& a, uint32_t virtual_rows, hipStream_t s, bool bf) {
    const uint32_t blocks = (virtual_rows + 15u) / 16u;
    const size_t lds = a.g.gamma ? (size_t)a.g.in_dim * sizeof(half_t) : 0;
    if (lds > 48 * 1024) return QUEST_EUNSUPPORTED;  // in_dim <= 24576 with a RMSNorm prologue
    if (a.n_tokens <= 4) return launch_skinny_tg<MODE, 1>(a, blocks, lds, s, bf);
    if (a.n_tokens <= 8) return launch_skinny_tg<MODE, 2>(a, blocks, lds, s, bf);
    return launch_skinny_tg<MODE, 4>(a, blocks, lds, s, bf);
}


constexpr int kMaxDevices = 64;
static int current_device() {  // index into the per-device caches below; -1: unknown (no caching)
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return -1;
    return dev;
}

template <int MODE, int TG>
static int launch_persist_tg(const SkinnyArgs& a, const PersistPlan& pl, uint32_t grid, size_t lds, hipStream_t s, bool bf) {
    // more than 64 KiB of dynamic LDS needs the opt-in, once per KERNEL and DEVICE (a process may drive several GPUs) -- kept in a
    // per-device table of atomics so that two threads launching on different devices do not race on one flag
    static std::atomic<bool> attr[2][kMaxDevices];  // [element type][device]
    const int dev = current_device();
    if (dev < 0 || !attr[bf][dev].load(std::memory_order_acquire)) {
        const hipError_t e = hipFuncSetAttribute(bf ? reinterpret_cast<const void*>(&persist_kernel_b16<MODE, TG, kCM>)
                                                    : reinterpret_cast<const void*>(&persist_kernel<MODE, TG, kCM>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)persist_lds_budget(TG, MODE == kGvQkvRope));
        if (e != hipSuccess) return (int)e;
        if (dev >= 0) attr[bf][dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL((bf ? persist_kernel_b16<MODE, TG, kCM> : persist_kernel<MODE, TG, kCM>), dim3(grid), dim3(kPsWaves * kWave), lds, s,
                       a, pl);
    QUEST_LAUNCH_CHECK();
    return 0;
}

static int persist_cus() {  // compute units of the CURRENT device (cached per device)
    static std::atomic<int> cus[kMaxDevices];
    const int dev = current_device();
    int n = dev >= 0 ? cus[dev].load(std::memory_order_relaxed) : 0;
    if (n <= 0) {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess) n = 0;
        n = n > 0 ? n : 256;
        if (dev >= 0) cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// Plan of the persistent kernel, or false when the shape does not fit it (then: launch_skinny).
static bool plan_persist(const SkinnyArgs& a, uint32_t virtual_rows, uint32_t tg, bool rope, PersistPlan& pl, uint32_t& grid,
                         size_t& lds) {
    const uint32_t spp = (a.g.in_dim + 127u) / 128u, tokens = 4u * tg;  // 128-wide k steps of a row
    const size_t budget = persist_lds_budget(tg, rope);
    pl.n_quads = (virtual_rows + 3u) / 4u;
    grid = (uint32_t)persist_cus();
    const uint32_t x_row = spp * 128u + 32u;  // + 64 bytes: = 64 mod 256 bytes
    const size_t need = (size_t)tokens * x_row * sizeof(half_t);
    if (need > budget) return false;  // the inputs do not fit LDS (down_proj at 8 tokens)
    if ((size_t)tokens * spp * 16u > (size_t)ps_input_vectors((int)tg) * kPsWaves * kWave) return false;  // <= kXV vectors per thread
    if (spp * 16u < (uint32_t)kWave) return false;  // (the 1 / rms reduction assumes <= 2 tokens per wave sweep)
    uint32_t ks = 1, lg = 0;
    while (ks < (uint32_t)kPsWaves && (spp + ks - 1) / ks > (uint32_t)kCM) ks *= 2, ++lg;
    if ((spp + ks - 1) / ks > (uint32_t)kCM) return false;  // rows longer than 16 slices x 4 steps x 128
    // more slices per quad = fewer quads per workgroup and round = more, smaller rounds: take the split whose last round
    // is fullest, as long as a task keeps >= 2 loads per lane
    auto rounds_of = [&](uint32_t k) { return (pl.n_quads + grid * ((uint32_t)kPsWaves / k) - 1) / (grid * ((uint32_t)kPsWaves / k)); };
    auto eff_of = [&](uint32_t k) { return (double)pl.n_quads / ((double)rounds_of(k) * grid * ((uint32_t)kPsWaves / k)); };
    for (uint32_t k = ks * 2, l = lg + 1; k <= (uint32_t)kPsWaves && (spp + k - 1) / k >= 2; k *= 2, ++l)
        if (eff_of(k) > eff_of(ks) + 0.04) ks = k, lg = l;
    pl.ks = ks, pl.ks_log2 = lg, pl.rounds = rounds_of(ks), pl.spp = spp, pl.x_row = x_row;
    pl.vpp_magic = (uint32_t)(0xffffffffu / (spp * 16u)) + 1u;
    constexpr size_t kFloor = 81 * 1024;  // more than half of the CU's LDS: exactly one workgroup per CU
    lds = need > kFloor ? need : kFloor;
    return true;
}

// groups of 4 tokens a workgroup of the n-token kernels carries: the TG instantiation
static uint32_t token_groups(uint32_t n_tokens) { return n_tokens <= 4 ? 1 : (n_tokens <= 8 ? 2 : 4); }

// QUEST_BATCHED_GEMV=skinny forces the first kernel (tuning / tests).
// plan_as_rope: plan with the rotating q/k/v launch's (smaller) LDS budget, so that the unrotated q/k/v launch takes the
// same n-token kernel as the rotating one at every shape (its v is then the same bits)
template <int MODE>
static int launch_batched(const SkinnyArgs& a, uint32_t virtual_rows, hipStream_t s, bool bf, bool plan_as_rope = false) {
    if (a.n_tokens == 0 || a.n_tokens > 16) return QUEST_EINVAL;
    if (a.g.in_dim % 8 != 0) return QUEST_EUNSUPPORTED;
    static const bool force_skinny = [] {
        const char* e = quest_tuning_env("QUEST_BATCHED_GEMV");
        return e && e[0] == 's';
    }();
    const uint32_t tg = token_groups(a.n_tokens);
    PersistPlan pl{};
    uint32_t grid = 0;
    size_t lds = 0;
    if (MODE == kGvQkvRope && a.g.head_dim > 256) return launch_skinny<MODE>(a, virtual_rows, s, bf);  // (the LDS rotation table)
    if (!force_skinny && plan_persist(a, virtual_rows, tg, MODE == kGvQkvRope || plan_as_rope, pl, grid, lds)) {
        if (tg == 1) return launch_persist_tg<MODE, 1>(a, pl, grid, lds, s, bf);
        if (tg == 2) return launch_persist_tg<MODE, 2>(a, pl, grid, lds, s, bf);
        return launch_persist_tg<MODE, 4>(a, pl, grid, lds, s, bf);
    }
    return launch_skinny<MODE>(a, virtual_rows, s, bf);
}

}  // namespace quest

using namespace quest;

// ---- The five projection operators.  Each is one host function that fills the GemvArgs, validates, and launches the
// single-token kernel or -- batched -- the n-token one (x: [n_tokens][in_dim], outputs [n_tokens][out_dim], contiguous);
// its two C entries are the two values of `batched`.  Order of refusals: unknown dtype, null operand / zero dimension
// (QUEST_EINVAL); then n_tokens outside 1..16 (QUEST_EINVAL, launch_batched) and in_dim % 8 (QUEST_EUNSUPPORTED).
static GemvArgs plain_args(const void* x, const void* gamma, float eps, const void* w, void* out, uint32_t in_dim, uint32_t out_dim) {
    GemvArgs p{};
    p.x = (const half_t*)x, p.gamma = (const half_t*)gamma, p.eps = eps, p.in_dim = in_dim;
    p.w[0] = (const half_t*)w, p.rows[0] = out_dim, p.out[0] = (half_t*)out;
    return p;
}
// n-token form of a launch: contiguous rows of inputs and of the (first) output
static SkinnyArgs skinny_args(const GemvArgs& g, uint32_t n_tokens) {
    SkinnyArgs a{};
    a.g = g;
    a.n_tokens = n_tokens, a.x_stride = g.in_dim, a.out_stride[0] = g.rows[0];
    return a;
}

static int norm_gemv(const void* x, const void* gamma, float eps, const void* w, void* out, uint32_t in_dim, uint32_t out_dim,
                     bool batched, uint32_t n_tokens, uint32_t dtype, quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!x || !w || !out || in_dim == 0 || out_dim == 0) return QUEST_EINVAL;
    const GemvArgs p = plain_args(x, gamma, eps, w, out, in_dim, out_dim);
    const bool bf = dtype == QUEST_DTYPE_BF16;
    if (batched) return launch_batched<kGvPlain>(skinny_args(p, n_tokens), out_dim, (hipStream_t)stream, bf);
    if (in_dim % 8 != 0) return QUEST_EUNSUPPORTED;
    return launch_gemv<kGvPlain>(p, out_dim, (hipStream_t)stream, bf);
}

static int gemv_residual(const void* x, const void* w, void* h, uint32_t in_dim, uint32_t out_dim, bool batched,
                         uint32_t n_tokens, uint32_t dtype, quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!x || !w || !h || in_dim == 0 || out_dim == 0) return QUEST_EINVAL;
    GemvArgs p = plain_args(x, nullptr, 0.f, w, h, in_dim, out_dim);
    p.residual = (const half_t*)h;
    const bool bf = dtype == QUEST_DTYPE_BF16;
    if (batched) {
        SkinnyArgs a = skinny_args(p, n_tokens);
#ifdef QUEST_PS_TIMELINE
        if (const char* e = quest_tuning_env("QUEST_PS_DEBUG_PTR")) a.g.out[2] = reinterpret_cast<half_t*>(strtoull(e, nullptr, 0));
#endif
        return launch_batched<kGvResidual>(a, out_dim, (hipStream_t)stream, bf);
    }
    if (in_dim % 8 != 0) return QUEST_EUNSUPPORTED;
    return launch_gemv<kGvResidual>(p, out_dim, (hipStream_t)stream, bf);
}

static int mlp_gate_up(const void* h, const void* gamma, float eps, const void* w_gate, const void* w_up, void* act,
                       uint32_t hidden, uint32_t intermediate, bool batched, uint32_t n_tokens, uint32_t dtype,
                       quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!h || !gamma || !w_gate || !w_up || !act || hidden == 0 || intermediate == 0) return QUEST_EINVAL;
    GemvArgs p = plain_args(h, gamma, eps, w_gate, act, hidden, intermediate);
    p.w[1] = (const half_t*)w_up, p.rows[1] = intermediate;
    const bool bf = dtype == QUEST_DTYPE_BF16;
    if (batched) return launch_batched<kGvSiluMul>(skinny_args(p, n_tokens), 2 * intermediate, (hipStream_t)stream, bf);
    if (hidden % 8 != 0) return QUEST_EUNSUPPORTED;
    return launch_gemv<kGvSiluMul>(p, 2 * intermediate, (hipStream_t)stream, bf);
}

// GemvArgs of a launch with the three matrices Wq, Wk, Wv
static GemvArgs qkv_args(const void* h, const void* gamma, float eps, const void* wq, const void* wk, const void* wv, void* q,
                         void* k, void* v, uint32_t hidden, uint32_t q_rows, uint32_t kv_rows) {
    GemvArgs p = plain_args(h, gamma, eps, wq, q, hidden, q_rows);
    p.w[1] = (const half_t*)wk, p.w[2] = (const half_t*)wv;
    p.rows[1] = p.rows[2] = kv_rows;
    p.out[1] = (half_t*)k, p.out[2] = (half_t*)v;
    return p;
}
static SkinnyArgs qkv_skinny_args(const GemvArgs& g, uint32_t n_tokens) {
    SkinnyArgs a = skinny_args(g, n_tokens);
    a.out_stride[1] = g.rows[1], a.out_stride[2] = g.rows[2];
    return a;
}

// The rotating q-k-v launch: closed form (inv_freq NULL) or a frequency table, as quest_apply_rope_in_place_dtype.
// batched: one state per token, else `states` = the one state
static int qkv_rope(const void* h, const void* gamma, float eps, const void* wq, const void* wk, const void* wv, void* q,
                    void* k, void* v, uint32_t hidden, uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t head_dim,
                    float rope_scale, float rope_theta, const float* inv_freq, float attention_factor,
                    const quest_step_state_t* states, bool batched, uint32_t n_tokens, uint32_t dtype, quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (inv_freq ? bad_rope_table(inv_freq, attention_factor) : (rope_scale == 0.f || rope_theta <= 0.f)) return QUEST_EINVAL;
    if (!h || !gamma || !wq || !wk || !wv || !q || !k || !v || !states) return QUEST_EINVAL;
    if (hidden == 0 || num_qo_heads == 0 || num_kv_heads == 0) return QUEST_EINVAL;
    // one token: a wave's 4 row-dots = two rotation pairs of one head; n tokens: a 16-row block = 8 rotation pairs of ONE
    // head of ONE matrix
    if (batched ? head_dim % 16 != 0 : (hidden % 8 != 0 || head_dim % 4 != 0)) return QUEST_EUNSUPPORTED;
    GemvArgs p = qkv_args(h, gamma, eps, wq, wk, wv, q, k, v, hidden, num_qo_heads * head_dim, num_kv_heads * head_dim);
    p.head_dim = head_dim, p.state = states;
    p.rcp_scale = inv_freq ? 1.0f : 1.0f / rope_scale, p.log2_rcp_theta = inv_freq ? 0.f : -log2f(rope_theta);
    p.inv_freq = inv_freq, p.attn_factor = inv_freq ? attention_factor : 1.0f;
    const uint32_t rows = p.rows[0] + p.rows[1] + p.rows[2];
    if (!batched) return launch_gemv<kGvQkvRope>(p, rows, (hipStream_t)stream, dtype == QUEST_DTYPE_BF16);
    SkinnyArgs a = qkv_skinny_args(p, n_tokens);
    a.state_stride = 1;
    return launch_batched<kGvQkvRope>(a, rows, (hipStream_t)stream, dtype == QUEST_DTYPE_BF16);
}

// q, k, v projections WITHOUT the rotation (models with a per-head q/k norm between the projection and RoPE: the norm
// needs a whole head row, which this launch spreads over several workgroups -- quest_apply_qk_norm_rope_in_place_dtype
// follows as a launch of its own).  The plain launch with three matrices: the same row-dots in the same k order as
// the rotating launch, the epilogue stores them as they are; batched, it is planned as the rotating launch (plan_as_rope).
static int qkv(const void* h, const void* gamma, float eps, const void* wq, const void* wk, const void* wv, void* q, void* k,
               void* v, uint32_t hidden, uint32_t q_rows, uint32_t kv_rows, bool batched, uint32_t n_tokens, uint32_t dtype,
               quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!h || !gamma || !wq || !wk || !wv || !q || !k || !v) return QUEST_EINVAL;
    if (hidden == 0 || q_rows == 0 || kv_rows == 0) return QUEST_EINVAL;
    const GemvArgs p = qkv_args(h, gamma, eps, wq, wk, wv, q, k, v, hidden, q_rows, kv_rows);
    const bool bf = dtype == QUEST_DTYPE_BF16;
    if (batched) return launch_batched<kGvPlain>(qkv_skinny_args(p, n_tokens), q_rows + 2 * kv_rows, (hipStream_t)stream, bf, true);
    if (hidden % 8 != 0) return QUEST_EUNSUPPORTED;
    return launch_gemv<kGvPlain>(p, q_rows + 2 * kv_rows, (hipStream_t)stream, bf);
}

// ---- the C entries: one per operator and form
extern "C" int quest_decode_norm_gemv(const void* x, const void* gamma, float eps, const void* w, void* out, uint32_t in_dim,
                                      uint32_t out_dim, uint32_t dtype, quest_stream_t stream) {
    return norm_gemv(x, gamma, eps, w, out, in_dim, out_dim, false, 0, dtype, stream);
}
extern "C" int quest_decode_norm_gemv_batched(const void* x, const void* gamma, float eps, const void* w, void* out,
                                              uint32_t in_dim, uint32_t out_dim, uint32_t n_tokens, uint32_t dtype,
                                              quest_stream_t stream) {
    return norm_gemv(x, gamma, eps, w, out, in_dim, out_dim, true, n_tokens, dtype, stream);
}
extern "C" int quest_decode_gemv_residual(const void* x, const void* w, void* h, uint32_t in_dim, uint32_t out_dim,
                                          uint32_t dtype, quest_stream_t stream) {
    return gemv_residual(x, w, h, in_dim, out_dim, false, 0, dtype, stream);
}
extern "C" int quest_decode_gemv_residual_batched(const void* x, const void* w, void* h, uint32_t in_dim, uint32_t out_dim,
                                                  uint32_t n_tokens, uint32_t dtype, quest_stream_t stream) {
    return gemv_residual(x, w, h, in_dim, out_dim, true, n_tokens, dtype, stream);
}
extern "C" int quest_decode_mlp_gate_up(const void* h, const void* gamma, float eps, const void* w_gate, const void* w_up,
                                        void* act, uint32_t hidden, uint32_t intermediate, uint32_t dtype,
                                        quest_stream_t stream) {
    return mlp_gate_up(h, gamma, eps, w_gate, w_up, act, hidden, intermediate, false, 0, dtype, stream);
}
extern "C" int quest_decode_mlp_gate_up_batched(const void* h, const void* gamma, float eps, const void* w_gate,
                                                const void* w_up, void* act, uint32_t hidden, uint32_t intermediate,
                                                uint32_t n_tokens, uint32_t dtype, quest_stream_t stream) {
    return mlp_gate_up(h, gamma, eps, w_gate, w_up, act, hidden, intermediate, true, n_tokens, dtype, stream);
}
extern "C" int quest_decode_qkv_rope(const void* h, const void* gamma, float eps, const void* wq, const void* wk,
                                     const void* wv, void* q, void* k, void* v, uint32_t hidden, uint32_t num_qo_heads,
                                     uint32_t num_kv_heads, uint32_t head_dim, float rope_scale, float rope_theta,
                                     const float* inv_freq, float attention_factor, const quest_step_state_t* state,
                                     uint32_t dtype, quest_stream_t stream) {
    return qkv_rope(h, gamma, eps, wq, wk, wv, q, k, v, hidden, num_qo_heads, num_kv_heads, head_dim, rope_scale, rope_theta,
                    inv_freq, attention_factor, state, false, 0, dtype, stream);
}
extern "C" int quest_decode_qkv_rope_batched(const void* h, const void* gamma, float eps, const void* wq, const void* wk,
                                             const void* wv, void* q, void* k, void* v, uint32_t hidden,
                                             uint32_t num_qo_heads, uint32_t num_kv_heads, uint32_t head_dim,
                                             float rope_scale, float rope_theta, const float* inv_freq,
                                             float attention_factor, const quest_step_state_t* states, uint32_t n_tokens,
                                             uint32_t dtype, quest_stream_t stream) {
    return qkv_rope(h, gamma, eps, wq, wk, wv, q, k, v, hidden, num_qo_heads, num_kv_heads, head_dim, rope_scale, rope_theta,
                    inv_freq, attention_factor, states, true, n_tokens, dtype, stream);
}
extern "C" int quest_decode_qkv(const void* h, const void* gamma, float eps, const void* wq, const void* wk, const void* wv,
                                void* q, void* k, void* v, uint32_t hidden, uint32_t q_rows, uint32_t kv_rows, uint32_t dtype,
                                quest_stream_t stream) {
    return qkv(h, gamma, eps, wq, wk, wv, q, k, v, hidden, q_rows, kv_rows, false, 0, dtype, stream);
}
extern "C" int quest_decode_qkv_batched(const void* h, const void* gamma, float eps, const void* wq, const void* wk,
                                        const void* wv, void* q, void* k, void* v, uint32_t hidden, uint32_t q_rows,
                                        uint32_t kv_rows, uint32_t n_tokens, uint32_t dtype, quest_stream_t stream) {
    return qkv(h, gamma, eps, wq, wk, wv, q, k, v, hidden, q_rows, kv_rows, true, n_tokens, dtype, stream);
}

// Which kernel an n-token launch of this shape takes, whatever its element type (both are 16 bits wide: the plan has no
// dtype) (tests / tuning; no launch): returns 1 and fills
// info = {k slices per quad, rounds, dynamic LDS bytes, workgroups, 128-wide k steps per row, fragments per set} for the
// persistent kernel, 0 for the first (inputs-from-L2) kernel, < 0 for argument errors as the launches return them.
extern "C" int quest_decode_batched_plan(uint32_t in_dim, uint32_t virtual_rows, uint32_t n_tokens, int rope, uint32_t
                                         info[6]) {
    if (in_dim == 0 || virtual_rows == 0 || n_tokens == 0 || n_tokens > 16 || !info) return QUEST_EINVAL;
    if (in_dim % 8 != 0) return QUEST_EUNSUPPORTED;
    SkinnyArgs a{};
    a.g.in_dim = in_dim, a.n_tokens = n_tokens;
    const uint32_t tg = token_groups(n_tokens);
    PersistPlan pl{};
    uint32_t grid = 0;
    size_t lds = 0;
    if (!plan_persist(a, virtual_rows, tg, rope != 0, pl, grid, lds)) return 0;
    info[0] = pl.ks, info[1] = pl.rounds, info[2] = (uint32_t)lds, info[3] = grid, info[4] = pl.spp, info[5] = (uint32_t)kCM;
    return 1;
}
