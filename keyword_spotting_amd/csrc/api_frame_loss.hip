// C ABI of libkws_amd.so (include/kws_amd.h, "Frame-wise targets"): the frame-wise cross-entropy as a whole-batch op, and what the two
// train handles share of their _frames entry points -- the refusals of a kws_frame_targets and the class weights' place in the
// handle's upload block.
#include "api_internal.h"

using namespace kws_host;

namespace kws_host {

int check_class_weight(const float* w, int C) {
    for (int c = 0; w && c < C; ++c)
        if (!(w[c] >= 0.f) || !std::isfinite(w[c]))
            return fail(KWS_ERR_INVALID_ARGUMENT, "class_weight[%d]=%g has to be finite and not negative", c, (double)w[c]);
    return KWS_OK;
}

int check_frame_targets(const kws_frame_targets* ft, int C) {
    if (!ft) return fail(KWS_ERR_INVALID_ARGUMENT, "frame targets are null");
    if (!ft->targets) return fail(KWS_ERR_INVALID_ARGUMENT, "ft->targets is null");
    const struct { const char* name; float v; } w[2] = {{"ctc_weight", ft->ctc_weight}, {"frame_weight", ft->frame_weight}};
    for (const auto& e : w)
        if (!(e.v >= 0.f) || !std::isfinite(e.v)) return fail(KWS_ERR_INVALID_ARGUMENT, "ft->%s=%g has to be finite and not negative", e.name, (double)e.v);
    if (ft->ctc_weight == 0.f && ft->frame_weight == 0.f)
        return fail(KWS_ERR_INVALID_ARGUMENT, "ft->ctc_weight and ft->frame_weight are both 0: no objective");
    if (ft->frame_weight == 0.f && ft->ctc_weight != 1.f)
        return fail(KWS_ERR_INVALID_ARGUMENT, "ft->frame_weight=0 is the plain call and takes ft->ctc_weight=1, not %g (scale the learning rate)",
                    (double)ft->ctc_weight);
    if (misaligned(ft->targets) || misaligned(ft->frame_loss)) return fail(KWS_ERR_INVALID_ARGUMENT, "ft->targets and ft->frame_loss must be 4-byte aligned");
    return check_class_weight(ft->class_weight, C);
}

int check_seq_len(const int32_t* seq_len, int B, int T) {
    for (int b = 0; b < B; ++b)
        if (seq_len[b] < 0 || seq_len[b] > T) return fail(KWS_ERR_INVALID_ARGUMENT, "seq_len[%d]=%d outside [0,%d]", b, seq_len[b], T);
    return KWS_OK;
}

void append_class_weights(const float* w, int C, std::vector<int32_t>* ints) {
    float row[kws::kMaxClasses] = {};
    for (int c = 0; c < C; ++c) row[c] = w ? w[c] : 1.0f;
    const size_t at = ints->size();
    ints->resize(at + kws::kMaxClasses);
    memcpy(ints->data() + at, row, sizeof(row));
}

kws::FrameLossParams train_frame_term(const kws_frame_targets& ft, int B) {
    kws::FrameLossParams p = {};
    const bool ctc = ft.ctc_weight > 0.f;
    p.targets = ft.targets; p.ce = ft.frame_loss;
    p.scale = ft.frame_weight / (float)B; p.mix_prev = ctc ? ft.ctc_weight : 0.f; p.mix_ce = ft.frame_weight; p.accumulate = ctc ? 1 : 0;
    return p;
}

}  // namespace kws_host

extern "C" {

size_t kws_sizeof_frame_targets(void) { return sizeof(kws_frame_targets); }

int kws_frame_loss(const float* logits, const int32_t* seq_len, const int32_t* targets, const float* class_weight_or_null, int B, int T, int C,
                   float* loss, float* grad_logits_or_null, void* stream) {
    if (B < 0 || T < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d", B, T);
    if (C < 3 || C > 8) return fail(KWS_ERR_INVALID_ARGUMENT, "C=%d out of range [3,8]", C);
    if ((size_t)B * T > (size_t)0x7fffffff) return fail(KWS_ERR_UNSUPPORTED, "B=%d x T=%d: more than 2^31 - 1 frames in one call", B, T);
    if (B == 0) return KWS_OK;
    if (!logits || !seq_len || !targets || !loss) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(logits) || misaligned(targets) || misaligned(loss) || misaligned(grad_logits_or_null))
        return fail(KWS_ERR_INVALID_ARGUMENT, "logits, targets, loss and grad_logits must be 4-byte aligned");
    KWS_TRY(check_seq_len(seq_len, B, T));
    KWS_TRY(check_class_weight(class_weight_or_null, C));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the lengths and the class weights travel as one stream-ordered block, released behind the launch that reads it
    std::vector<int32_t> ints(seq_len, seq_len + B);
    append_class_weights(class_weight_or_null, C, &ints);
    int32_t* d = nullptr;
    KWS_HIP(hipMallocAsync(reinterpret_cast<void**>(&d), ints.size() * sizeof(int32_t), st));
    hipError_t e = hipMemcpyAsync(d, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        kws::FrameLossParams p = {};
        p.logits = logits; p.seq_len = d; p.targets = targets; p.weight = reinterpret_cast<const float*>(d + B);
        p.ce = loss; p.grad = grad_logits_or_null; p.scale = 1.0f; p.T = T; p.C = C;
        e = kws::launch_frame_loss(p, B, st);
    }
    (void)hipFreeAsync(d, st);
    return hip_done(e, "launch frame_loss");
}

}  // extern "C"
