// C ABI of libkws_amd.so (include/kws_amd.h): the CTC loss as a whole-batch op and the customised-keyword enrolment handle.
#include <new>

#include "train_core.h"

using namespace kws_host;

struct kws_enroll {
    int H = 0, C = 0, n = 0, E = 0, K = 0;
    float* state = nullptr;          // one allocation: W [E,H,n], b [E,n], then Adam's m and v in the same two shapes
    float *W = nullptr, *b = nullptr, *mW = nullptr, *mb = nullptr, *vW = nullptr, *vb = nullptr;
    int steps = 0;                   // optimiser steps since kws_enroll_set: Adam's t (the bias corrections depend on it)
    // seq_len [B] | label_len [B] | labels [B,S_max] on the device, and the host copy it was filled from: a fit with the lengths
    // and labels of the call before (the steps of one enrolment) copies nothing
    int32_t* ints = nullptr;
    size_t ints_cap = 0;
    std::vector<int32_t> ints_host;
    int allocs = 0;                  // device (re)allocations after create; each one waited for the device
    std::atomic<int> in_call{0};
    CallOrder order;                 // against the handle's previous call, as a train handle's (train_core.h)
};

namespace kws_host {

// seq_len / label_len / labels (host memory) against the shape; what = the class count the labels index (blank = classes - 1)
int check_labels(const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int S_max, int classes) {
    for (int b = 0; b < B; ++b) {
        if (seq_len[b] < 0 || seq_len[b] > T) return fail(KWS_ERR_INVALID_ARGUMENT, "seq_len[%d]=%d outside [0,%d]", b, seq_len[b], T);
        if (label_len[b] < 0 || label_len[b] > S_max)
            return fail(KWS_ERR_INVALID_ARGUMENT, "label_len[%d]=%d outside [0,%d]", b, label_len[b], S_max);
        if (seq_len[b] == 0) continue;          // an empty slot: its label is ignored
        for (int i = 0; i < label_len[b]; ++i) {
            const int32_t l = labels[(size_t)b * S_max + i];
            if (l < 0 || l > classes - 2)
                return fail(KWS_ERR_INVALID_ARGUMENT, "labels[%d][%d]=%d outside [0,%d] (the blank is class %d)", b, i, l, classes - 2, classes - 1);
        }
    }
    return KWS_OK;
}

bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// [seq_len | label_len | labels] as one block
void pack_ints(const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int S_max, std::vector<int32_t>* out) {
    out->resize((size_t)B * (2 + S_max));
    std::copy(seq_len, seq_len + B, out->begin());
    std::copy(label_len, label_len + B, out->begin() + B);
    if (S_max > 0) std::copy(labels, labels + (size_t)B * S_max, out->begin() + 2 * (size_t)B);
}

}  // namespace kws_host

namespace {

// what kws_enroll_create refuses about the shape, before the device is probed
int check_enroll_shape(int H, int C, int n_new, int E, int K) {
    if (H != 64 && H != 128 && H != 256) return fail(KWS_ERR_UNSUPPORTED, "hidden=%d unsupported (64, 128, 256)", H);
    if (C < 3 || n_new < 1 || C + n_new > 8)
        return fail(KWS_ERR_INVALID_ARGUMENT, "C=%d n_new=%d: the trained head has 3..7 classes and the extended one C + n_new <= 8", C, n_new);
    if (E < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "E=%d enrolments: at least one", E);
    if (K < 1 || K > 4) return fail(KWS_ERR_INVALID_ARGUMENT, "K=%d utterance slots per enrolment out of range [1,4]", K);
    return KWS_OK;
}

// what kws_enroll_fit refuses about a call on B = E x K slots, in its order; with_labels false (the frame loss alone): nothing about the
// labels, and no LDS that grows with T.  null_ptr / odd_ptr: what the caller found about nn_outputs, logits1 and loss_trace (the host-only
// checks have none of them: false)
int check_enroll_call(int H, int n, int K, int B, int classes, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int T,
                      int S_max, float lr, int iterations, bool with_labels, bool null_ptr, bool odd_ptr) {
    if (T < 1 || S_max < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape T=%d S_max=%d", T, S_max);
    if (S_max > 31) return fail(KWS_ERR_INVALID_ARGUMENT, "S_max=%d out of range [0,31]: one lane of a wave per state of the extended label", S_max);
    if (iterations < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "iterations=%d: at least one", iterations);
    if (!(lr > 0.f) || !std::isfinite(lr)) return fail(KWS_ERR_INVALID_ARGUMENT, "lr=%g has to be positive and finite", (double)lr);
    if (null_ptr || !seq_len || (with_labels && (!label_len || (!labels && S_max > 0)))) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (odd_ptr) return fail(KWS_ERR_INVALID_ARGUMENT, "nn_outputs, logits1 and loss_trace must be 4-byte aligned");
    if (with_labels) KWS_TRY(check_labels(seq_len, labels, label_len, B, T, S_max, classes));
    else KWS_TRY(check_seq_len(seq_len, B, T));
    const size_t lds = kws::enroll_fit_frames_lds_bytes(H, n, K, T, S_max, with_labels);
    if (lds > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "an enrolment keeps %d utterances x %d frames x (8 log-probabilities + %d states) and %d x %d parameter "
                    "images in LDS: %zu bytes exceed the %zu a workgroup may hold (fewer frames, shorter labels or fewer slots)", K, T,
                    2 * S_max + 1, 3 + K, (H + 1) * n, lds, kWindowIncLdsMax);
    return KWS_OK;
}

// ... and kws_enroll_fit_frames, whose labels count only next to a CTC term
int check_enroll_frames(int H, int C, int n, int E, int K, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int T,
                        int S_max, const kws_frame_targets* ft, float lr, int iterations, bool null_ptr = false, bool odd_ptr = false) {
    KWS_TRY(check_frame_targets(ft, C + n));
    const bool ctc = ft->ctc_weight > 0.f;
    if ((size_t)E * K * (size_t)(T < 0 ? 0 : T) > (size_t)0x7fffffff)
        return fail(KWS_ERR_UNSUPPORTED, "E=%d x K=%d x T=%d: more than 2^31 - 1 frames in one call", E, K, T);
    return check_enroll_call(H, n, K, E * K, C + n, seq_len, labels, label_len, T, ctc ? S_max : 0, lr, iterations, ctc, null_ptr, odd_ptr);
}

int enroll_device_probe() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    return KWS_OK;
}

}  // namespace

extern "C" {

int kws_ctc_loss(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C, int S_max,
                 float* loss, float* grad_logits_or_null, void* stream) {
    if (B < 0 || T < 1 || S_max < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d S_max=%d", B, T, S_max);
    if (C < 3 || C > 8) return fail(KWS_ERR_INVALID_ARGUMENT, "C=%d out of range [3,8]", C);
    if (S_max > 31) return fail(KWS_ERR_INVALID_ARGUMENT, "S_max=%d out of range [0,31]: one lane of a wave per state of the extended label", S_max);
    if (B == 0) return KWS_OK;
    if (!logits || !seq_len || !label_len || !loss || (!labels && S_max > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(logits) || misaligned(loss) || misaligned(grad_logits_or_null))
        return fail(KWS_ERR_INVALID_ARGUMENT, "logits, loss and grad_logits must be 4-byte aligned");
    KWS_TRY(check_labels(seq_len, labels, label_len, B, T, S_max, C));
    KWS_TRY(enroll_device_probe());
    const size_t lds = kws::ctc_loss_lds_bytes(T, S_max);
    if (lds > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "the CTC loss keeps %d frames x (8 log-probabilities + %d states) in LDS: %zu bytes exceed the %zu a "
                    "workgroup may hold", T, 2 * S_max + 1, lds, kWindowIncLdsMax);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the lengths and labels travel as one stream-ordered block, released behind the launch that reads it
    std::vector<int32_t> ints;
    pack_ints(seq_len, labels, label_len, B, S_max, &ints);
    int32_t* d = nullptr;
    KWS_HIP(hipMallocAsync(reinterpret_cast<void**>(&d), ints.size() * sizeof(int32_t), st));
    hipError_t e = hipMemcpyAsync(d, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = kws::launch_ctc_loss(logits, d, d + 2 * (size_t)B, d + B, B, T, C, S_max, loss, grad_logits_or_null, st);
    (void)hipFreeAsync(d, st);
    return hip_done(e, "launch ctc_loss");
}

int kws_enroll_create(int H, int C, int n_new, int E, int K, kws_enroll_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    KWS_TRY(check_enroll_shape(H, C, n_new, E, K));
    KWS_TRY(enroll_device_probe());
    kws_enroll* h = new (std::nothrow) kws_enroll();
    if (!h) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->H = H; h->C = C; h->n = n_new; h->E = E; h->K = K;
    const size_t nw = (size_t)E * H * n_new, nb = (size_t)E * n_new;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->state), 3 * (nw + nb) * sizeof(float));
    if (e == hipSuccess) e = hipMemset(h->state, 0, 3 * (nw + nb) * sizeof(float));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->order.last_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { kws_enroll_destroy(h); return hip_fail(e, "kws_enroll_create"); }
    h->W = h->state; h->b = h->W + nw; h->mW = h->b + nb; h->mb = h->mW + nw; h->vW = h->mb + nb; h->vb = h->vW + nw;
    *out = h;
    return KWS_OK;
}

int kws_enroll_destroy(kws_enroll_handle h) {
    if (!h) return KWS_OK;
    hipDeviceSynchronize();
    if (h->state) hipFree(h->state);
    if (h->ints) hipFree(h->ints);
    if (h->order.last_done) hipEventDestroy(h->order.last_done);
    delete h;
    return KWS_OK;
}

int kws_enroll_set(kws_enroll_handle h, const float* Wn, const float* bn, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!Wn || !bn) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this enrolment handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nw = (size_t)h->E * h->H * h->n, nb = (size_t)h->E * h->n;
    KWS_TRY(h->order.enter(st));
    return h->order.finish(st, [&]() -> int {
        KWS_HIP(hipMemcpyAsync(h->W, Wn, nw * sizeof(float), hipMemcpyDeviceToDevice, st));
        KWS_HIP(hipMemcpyAsync(h->b, bn, nb * sizeof(float), hipMemcpyDeviceToDevice, st));
        KWS_HIP(hipMemsetAsync(h->mW, 0, 2 * (nw + nb) * sizeof(float), st));
        h->steps = 0;
        return KWS_OK;
    }());
}

// The launch both fit entry points end in, behind their refusals: the host ints (and, with frame targets, the class weights) into the
// handle's upload block -- [seq_len | label_len | labels | weights], re-sent only when it differs from the call before --, then the
// plain kernel (ft null) or the frames one.  ft->ctc_weight == 0: labels and label_len may be null and S_max is 0.
static int enroll_fit_launch(kws_enroll_handle h, const float* nn_outputs, const float* logits1, const int32_t* seq_len, const int32_t* labels,
                             const int32_t* label_len, int T, int S_max, const kws_frame_targets* ft, float lr, int iterations,
                             float* loss_trace_or_null, void* stream) {
    const int B = h->E * h->K;
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this enrolment handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(h->order.enter(st));
    return h->order.finish(st, [&]() -> int {
        std::vector<int32_t> ints;
        const std::vector<int32_t> no_labels((size_t)B, 0);
        pack_ints(seq_len, labels, label_len ? label_len : no_labels.data(), B, S_max, &ints);
        const size_t weights_at = ints.size();
        if (ft) append_class_weights(ft->class_weight, h->C + h->n, &ints);
        if (ints.size() > h->ints_cap) {          // the first call at this shape: the block only grows (waits for the device once)
            KWS_HIP(hipDeviceSynchronize());
            if (h->ints) (void)hipFree(h->ints);
            h->ints = nullptr; h->ints_cap = 0; h->ints_host.clear();
            KWS_HIP(hipMalloc(reinterpret_cast<void**>(&h->ints), ints.size() * sizeof(int32_t)));
            h->ints_cap = ints.size();
            ++h->allocs;
        }
        if (ints != h->ints_host) {
            KWS_HIP(hipMemcpyAsync(h->ints, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
            h->ints_host.swap(ints);
        }
        kws::EnrollFitParams p = {};
        p.nn = nn_outputs; p.logits1 = logits1;
        p.seq_len = h->ints; p.label_len = h->ints + B; p.labels = h->ints + 2 * (size_t)B;
        p.W = h->W; p.b = h->b; p.mW = h->mW; p.mb = h->mb; p.vW = h->vW; p.vb = h->vb;
        p.loss_trace = loss_trace_or_null; p.lr = lr;
        p.K = h->K; p.n = h->n; p.C = h->C; p.T = T; p.S_max = S_max; p.iterations = iterations; p.step0 = h->steps;
        if (!ft) {
            KWS_TRY(hip_done(kws::launch_enroll_fit(p, h->H, h->E, st), "launch enroll_fit"));
        } else {
            kws::EnrollFitFramesParams q = {};
            q.fit = p;
            q.targets = ft->targets; q.weight = reinterpret_cast<const float*>(h->ints + weights_at); q.frame_loss = ft->frame_loss;
            q.ctc_weight = ft->ctc_weight; q.frame_weight = ft->frame_weight;
            KWS_TRY(hip_done(kws::launch_enroll_fit_frames(q, h->H, h->E, st), "launch enroll_fit_frames"));
        }
        h->steps += iterations;
        return KWS_OK;
    }());
}

int kws_enroll_fit(kws_enroll_handle h, const float* nn_outputs, const float* logits1, const int32_t* seq_len, const int32_t* labels,
                   const int32_t* label_len, int T, int S_max, float lr, int iterations, float* loss_trace_or_null, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_enroll_call(h->H, h->n, h->K, h->E * h->K, h->C + h->n, seq_len, labels, label_len, T, S_max, lr, iterations, true,
                              !nn_outputs || !logits1, misaligned(nn_outputs) || misaligned(logits1) || misaligned(loss_trace_or_null)));
    return enroll_fit_launch(h, nn_outputs, logits1, seq_len, labels, label_len, T, S_max, nullptr, lr, iterations, loss_trace_or_null, stream);
}

int kws_enroll_check_frames(int H, int C, int n_new, int E, int K, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                            int T, int S_max, const kws_frame_targets* ft, float lr, int iterations) {
    KWS_TRY(check_enroll_shape(H, C, n_new, E, K));
    return check_enroll_frames(H, C, n_new, E, K, seq_len, labels, label_len, T, S_max, ft, lr, iterations);
}

int kws_enroll_fit_frames(kws_enroll_handle h, const float* nn_outputs, const float* logits1, const int32_t* seq_len,
                          const int32_t* labels_or_null, const int32_t* label_len_or_null, int T, int S_max, const kws_frame_targets* ft, float lr,
                          int iterations, float* loss_trace_or_null, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_enroll_frames(h->H, h->C, h->n, h->E, h->K, seq_len, labels_or_null, label_len_or_null, T, S_max, ft, lr, iterations,
                                !nn_outputs || !logits1, misaligned(nn_outputs) || misaligned(logits1) || misaligned(loss_trace_or_null)));
    if (ft->frame_weight == 0.f)          // the plain call: its launch, its bits, its upload block
        return enroll_fit_launch(h, nn_outputs, logits1, seq_len, labels_or_null, label_len_or_null, T, S_max, nullptr, lr, iterations,
                                 loss_trace_or_null, stream);
    const bool ctc = ft->ctc_weight > 0.f;
    return enroll_fit_launch(h, nn_outputs, logits1, seq_len, ctc ? labels_or_null : nullptr, ctc ? label_len_or_null : nullptr, T,
                             ctc ? S_max : 0, ft, lr, iterations, loss_trace_or_null, stream);
}

int kws_enroll_get(kws_enroll_handle h, float* Wn, float* bn, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!Wn || !bn) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this enrolment handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nw = (size_t)h->E * h->H * h->n, nb = (size_t)h->E * h->n;
    KWS_TRY(h->order.enter(st));
    return h->order.finish(st, [&]() -> int {
        KWS_HIP(hipMemcpyAsync(Wn, h->W, nw * sizeof(float), hipMemcpyDeviceToDevice, st));
        KWS_HIP(hipMemcpyAsync(bn, h->b, nb * sizeof(float), hipMemcpyDeviceToDevice, st));
        return KWS_OK;
    }());
}

int kws_enroll_moments(kws_enroll_handle h, float* m, float* v, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!m || !v) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this enrolment handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nm = (size_t)h->E * (h->H + 1) * h->n;
    KWS_TRY(h->order.enter(st));
    return h->order.finish(st, [&]() -> int {
        KWS_HIP(hipMemcpyAsync(m, h->mW, nm * sizeof(float), hipMemcpyDeviceToDevice, st));
        KWS_HIP(hipMemcpyAsync(v, h->vW, nm * sizeof(float), hipMemcpyDeviceToDevice, st));
        return KWS_OK;
    }());
}

int kws_enroll_stats(kws_enroll_handle h, size_t* device_bytes, int32_t* allocs, int32_t* steps) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (device_bytes) *device_bytes = 3 * (size_t)h->E * (h->H + 1) * h->n * sizeof(float) + h->ints_cap * sizeof(int32_t);
    if (allocs) *allocs = h->allocs;
    if (steps) *steps = h->steps;
    return KWS_OK;
}

}  // extern "C"
