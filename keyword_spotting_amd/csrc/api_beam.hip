// C ABI of libkws_amd.so (include/kws_amd.h): CTC prefix beam search as a whole-batch op.  Stateless and stream-ordered: it owns
// nothing, allocates nothing and never waits for the device.
#include "api_internal.h"

using namespace kws_host;

extern "C" {

int kws_ctc_beam_search(const float* logits, const int32_t* seq_len_or_null, int B, int T, int C, int beam_width, int top_paths, int L_max,
                        int merge_repeated, int32_t* paths, int32_t* lengths, float* log_prob, void* stream) {
    if (!logits || !paths || !lengths || !log_prob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (C < 3 || C > 8) return fail(KWS_ERR_INVALID_ARGUMENT, "C=%d out of range [3,8]", C);
    if (beam_width < 1 || beam_width > kws::kBeamMax)
        return fail(KWS_ERR_INVALID_ARGUMENT, "beam_width=%d out of range [1,%d]: one lane of a wave per beam entry, four candidates per lane",
                    beam_width, kws::kBeamMax);
    if (top_paths < 1 || top_paths > beam_width)
        return fail(KWS_ERR_INVALID_ARGUMENT, "top_paths=%d out of range [1,beam_width=%d]", top_paths, beam_width);
    if (L_max < 1 || L_max > kws::kBeamRow) return fail(KWS_ERR_INVALID_ARGUMENT, "L_max=%d out of range [1,%d]", L_max, kws::kBeamRow);
    if (B < 1 || T < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d", B, T);
    if ((reinterpret_cast<uintptr_t>(logits) & 15u) != 0) return fail(KWS_ERR_INVALID_ARGUMENT, "logits must be 16-byte aligned");
    if (((reinterpret_cast<uintptr_t>(seq_len_or_null) | reinterpret_cast<uintptr_t>(paths) | reinterpret_cast<uintptr_t>(lengths) |
          reinterpret_cast<uintptr_t>(log_prob)) & 3u) != 0)
        return fail(KWS_ERR_INVALID_ARGUMENT, "seq_len, paths, lengths and log_prob must be 4-byte aligned");
    const size_t lds = kws::ctc_beam_lds_bytes(T);
    if (lds > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "the beam search keeps %d frames x 8 log-probabilities and %zu bytes of beam in LDS: %zu bytes exceed the "
                    "%zu a workgroup may hold", T, kws::ctc_beam_lds_bytes(0), lds, kWindowIncLdsMax);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    return hip_done(kws::launch_ctc_beam(logits, seq_len_or_null, B, T, C, beam_width, top_paths, L_max, merge_repeated != 0 ? 1 : 0, paths,
                                         lengths, log_prob, static_cast<hipStream_t>(stream)),
                    "launch ctc_beam");
}

}  // extern "C"
