// C ABI of libkws_amd.so (include/kws_amd.h): CTC forced alignment as a whole-batch op.  Stateless and stream-ordered: it owns nothing,
// never waits for the device, and allocates only the stream-ordered block its host arrays travel in (as kws_ctc_loss).
#include "api_internal.h"

using namespace kws_host;

extern "C" {

int kws_ctc_align(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C, int S_max,
                  int32_t* states_or_null, int32_t* spans_or_null, float* score, float* loss_or_null, float* post_or_null, void* stream) {
    if (B < 0 || T < 1 || S_max < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d S_max=%d", B, T, S_max);
    if (C < 3 || C > 8) return fail(KWS_ERR_INVALID_ARGUMENT, "C=%d out of range [3,8]", C);
    if (S_max > 31) return fail(KWS_ERR_INVALID_ARGUMENT, "S_max=%d out of range [0,31]: one lane of a wave per state of the extended label", S_max);
    if (B == 0) return KWS_OK;
    if (!logits || !seq_len || !label_len || !score || (!labels && S_max > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(logits) || misaligned(states_or_null) || misaligned(spans_or_null) || misaligned(score) || misaligned(loss_or_null) ||
        misaligned(post_or_null))
        return fail(KWS_ERR_INVALID_ARGUMENT, "logits, states, spans, score, loss and post must be 4-byte aligned");
    KWS_TRY(check_labels(seq_len, labels, label_len, B, T, S_max, C));
    const bool with_alpha = loss_or_null || post_or_null;
    const size_t lds = kws::ctc_align_lds_bytes(T, S_max, with_alpha);
    if (lds > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "the alignment keeps %d frames x (8 log-probabilities + 4 words of back-pointers + 1 state + %d states "
                    "of alpha) in LDS: %zu bytes exceed the %zu a workgroup may hold", T, with_alpha ? 2 * S_max + 1 : 0, lds, kWindowIncLdsMax);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the lengths and labels travel as one stream-ordered block, released behind the launch that reads it
    std::vector<int32_t> ints;
    pack_ints(seq_len, labels, label_len, B, S_max, &ints);
    int32_t* d = nullptr;
    KWS_HIP(hipMallocAsync(reinterpret_cast<void**>(&d), ints.size() * sizeof(int32_t), st));
    hipError_t e = hipMemcpyAsync(d, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = kws::launch_ctc_align(logits, d, d + 2 * (size_t)B, d + B, B, T, C, S_max, states_or_null, spans_or_null, score, loss_or_null,
                                  post_or_null, st);
    (void)hipFreeAsync(d, st);
    return hip_done(e, "launch ctc_align");
}

}  // extern "C"
