// quest_sample_tokens: the token choice of a decode step on the device (include/quest_hip.h, "Token sampling").
#include "sampling_device.cuh"

using namespace quest;

extern "C" int quest_sample_tokens(const void* logits, uint32_t logits_stride, uint32_t vocab, uint32_t n_rows, uint32_t dtype,
                                   const float* temperature, const int32_t* top_k, const float* top_p, const uint64_t* seed,
                                   const quest_step_state_t* states, const int32_t* positions, int32_t* tokens, int32_t* kept,
                                   const int32_t* eos_ids, uint32_t n_eos, int32_t pad_id, int32_t* finished,
                                   int32_t* history, uint32_t history_stride, int32_t* history_len, const void* embed,
                                   uint32_t hidden, void* next_input, quest_stream_t stream) {
    if (dtype > QUEST_DTYPE_BF16) return QUEST_EINVAL;
    if (!logits || !temperature || !top_k || !top_p || !seed || !tokens) return QUEST_EINVAL;
    if ((states != nullptr) == (positions != nullptr)) return QUEST_EINVAL;
    if (vocab == 0 || n_rows == 0 || logits_stride < vocab || ((uintptr_t)logits & 1u)) return QUEST_EINVAL;
    if (n_eos > kSampleMaxEos || (n_eos > 0 && !eos_ids)) return QUEST_EINVAL;
    if (pad_id < 0 || (uint32_t)pad_id >= vocab) return QUEST_EINVAL;
    if ((history != nullptr) != (history_len != nullptr) || (history && history_stride == 0)) return QUEST_EINVAL;
    if ((embed != nullptr) != (next_input != nullptr) || (embed && hidden == 0)) return QUEST_EINVAL;
    if (vocab > kSampleMaxVocab) return QUEST_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (n_eos > 0) {
        // The ids live in device memory.  Outside a stream capture they are read back (32 bytes, one wait on `stream`) and
        // an id outside the vocabulary is refused; while `stream` is capturing nothing can be read, and such an id is
        // harmless: the kernel compares it with tokens of [0, vocab), which it never equals.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) return (int)hipGetLastError();
        if (cap == hipStreamCaptureStatusNone) {
            int32_t ids[kSampleMaxEos];
            hipError_t e = hipMemcpyAsync(ids, eos_ids, n_eos * sizeof(int32_t), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return (int)e;
            for (uint32_t i = 0; i < n_eos; ++i)
                if (ids[i] < 0 || (uint32_t)ids[i] >= vocab) return QUEST_EINVAL;
        }
    }
    SampleArgs a;
    a.logits = (const uint16_t*)logits;
    a.temperature = temperature, a.top_k = top_k, a.top_p = top_p, a.seed = seed;
    a.states = states, a.positions = positions;
    a.tokens = tokens, a.kept = kept;
    a.eos_ids = eos_ids, a.finished = finished;
    a.history = history, a.history_len = history_len;
    a.embed = (const uint16_t*)embed, a.next_input = (uint16_t*)next_input;
    a.logits_stride = logits_stride, a.vocab = vocab, a.n_eos = n_eos, a.history_stride = history_stride, a.hidden = hidden;
    a.pad_id = pad_id;
    // 16 waves per row from 8192 columns up (one 16-byte load per thread there); 4 waves for short rows
    const uint32_t threads = vocab >= 8192u ? 1024u : 256u;
    if (dtype == QUEST_DTYPE_BF16) hipLaunchKernelGGL(sample_tokens_kernel<bf16_t>, dim3(n_rows), dim3(threads), 0, s, a);
    else hipLaunchKernelGGL(sample_tokens_kernel<half_t>, dim3(n_rows), dim3(threads), 0, s, a);
    QUEST_LAUNCH_CHECK();
    return 0;
}
