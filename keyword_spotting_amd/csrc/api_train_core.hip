// The host-side core of the train handles (train_core.h): nothing here knows a model.
#include "train_core.h"

namespace kws_host {

int CallOrder::enter(hipStream_t st) {
    if (valid && last_stream != st) KWS_HIP(hipStreamWaitEvent(st, last_done, 0));
    return KWS_OK;
}
int CallOrder::finish(hipStream_t st, int rc) {
    const hipError_t e = hipEventRecord(last_done, st);
    if (e == hipSuccess) { last_stream = st; valid = true; }
    if (rc != KWS_OK) return rc;
    return hip_done(e, "hipEventRecord");
}

void TrainCore::add_job(int src, const float* a, int lda, int K, const float* d, int ldd, int N, size_t out, int ldo) {
    kws::TrainWgradJob j = {};
    j.a = a; j.d = d; j.out = out; j.src = src; j.lda = lda; j.K = K; j.ldd = ldd; j.N = N; j.ldo = ldo; j.unit0 = units;
    units += ((K + 15) / 16) * ((N + 63) / 64);
    jobs_host.push_back(j);
}

int train_core_create(TrainCore* c, size_t P, size_t tail_floats, const float* tail_init, const char* who) {
    c->P = P;
    c->nred = kws::train_reduce_blocks(P);
    const size_t floats = (4 * P + tail_floats + 1) & ~(size_t)1;          // the doubles behind it
    c->state_bytes = floats * sizeof(float) + (size_t)c->nred * sizeof(double);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&c->state), c->state_bytes);
    if (e == hipSuccess) e = hipMemset(c->state, 0, c->state_bytes);
    if (e == hipSuccess && tail_init) e = hipMemcpy(c->state + 4 * P, tail_init, tail_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->order.last_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { train_core_destroy(c); return hip_fail(e, who); }
    c->theta = c->state; c->m = c->theta + P; c->v = c->m + P; c->grad = c->v + P; c->tail = c->grad + P;
    c->sumsq = reinterpret_cast<double*>(c->state + floats);
    return KWS_OK;
}

void train_core_destroy(TrainCore* c) {
    hipDeviceSynchronize();
    if (c->state) hipFree(c->state);
    if (c->arena) hipFree(c->arena);
    if (c->order.last_done) hipEventDestroy(c->order.last_done);
}

int train_arena_reserve(TrainCore* c, size_t need, int B, int T, int layers) {
    if (need > c->arena_bytes) {
        size_t free_b = 0, total_b = 0;
        KWS_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + c->arena_bytes)
            return fail(KWS_ERR_OUT_OF_MEMORY, "the tape of B=%d utterances x T=%d frames x %d layers takes %zu bytes: the device has %zu free "
                        "(%zu in all; fewer utterances per step or shorter ones)", B, T, layers, need, free_b + c->arena_bytes, total_b);
        KWS_HIP(hipDeviceSynchronize());
        if (c->arena) (void)hipFree(c->arena);
        c->arena = nullptr; c->arena_bytes = 0; c->ints_host.clear();
        KWS_HIP(hipMalloc(reinterpret_cast<void**>(&c->arena), need));
        c->arena_bytes = need;
        ++c->allocs;
    }
    c->ints_host.clear();
    c->jobs_host.clear();
    c->units = 0;
    c->jobs_dirty = true;
    return KWS_OK;
}

int train_upload(TrainCore* c, kws::TrainWgradJob* d_jobs, int32_t* d_ints, std::vector<int32_t>* ints, hipStream_t st) {
    if (c->jobs_dirty) {
        KWS_HIP(hipMemcpyAsync(d_jobs, c->jobs_host.data(), c->jobs_host.size() * sizeof(kws::TrainWgradJob), hipMemcpyHostToDevice, st));
        c->jobs_dirty = false;
    }
    // lengths or labels other than the last call's: one upload from pageable memory, which the runtime completes on the host (the
    // header says so); a repeated batch uploads nothing
    if (*ints != c->ints_host) {
        KWS_HIP(hipMemcpyAsync(d_ints, ints->data(), ints->size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        c->ints_host.swap(*ints);
    }
    return KWS_OK;
}

int train_update(TrainCore* c, float lr, float* grad_norm_or_null, hipStream_t st) {
    const bool adam = c->optimizer == KWS_OPT_ADAM;
    const double step = (double)(c->steps + 1);
    const float lr_t = adam ? (float)((double)lr * sqrt(1.0 - pow(0.999, step)) / (1.0 - pow(0.9, step))) : lr;
    KWS_LAUNCH(c, kws::launch_train_update(c->theta, c->m, c->v, c->grad, c->sumsq, c->nred, c->P, adam ? 1 : 0, lr_t, c->max_grad_norm,
                                           grad_norm_or_null, st), "launch train_update");
    ++c->steps;
    return KWS_OK;
}

int train_call(TrainCore* c, void* stream, const std::function<int(hipStream_t)>& body, bool sync) {
    BusyGuard guard(c->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(c->order.enter(st));
    KWS_TRY(c->order.finish(st, body(st)));
    if (sync) KWS_HIP(hipStreamSynchronize(st));
    return KWS_OK;
}

int train_set_weights(TrainCore* c, const void* blob, size_t nbytes, void* stream, const std::function<int(hipStream_t)>& then) {
    if (!c) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (nbytes != c->P * sizeof(float)) return fail(KWS_ERR_INVALID_ARGUMENT, "the weight blob has %zu bytes, the config needs %zu", nbytes, c->P * sizeof(float));
    return train_call(c, stream, [&](hipStream_t st) -> int {
        KWS_HIP(hipMemcpyAsync(c->theta, blob, nbytes, hipMemcpyHostToDevice, st));
        KWS_HIP(hipMemsetAsync(c->m, 0, 2 * c->P * sizeof(float), st));
        if (then) KWS_TRY(then(st));
        c->steps = 0;
        return KWS_OK;
    }, true);
}

int train_get_weights(TrainCore* c, void* blob, size_t nbytes, void* stream) {
    if (!c) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (nbytes != c->P * sizeof(float)) return fail(KWS_ERR_INVALID_ARGUMENT, "the weight blob has %zu bytes, the config needs %zu", nbytes, c->P * sizeof(float));
    return train_call(c, stream, [&](hipStream_t st) { return hip_done(hipMemcpyAsync(blob, c->theta, nbytes, hipMemcpyDeviceToHost, st), "copy of the weights"); },
                      true);
}

int train_moments(TrainCore* c, float* m, float* v, void* stream) {
    if (!c) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!m || !v) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    return train_call(c, stream, [&](hipStream_t st) -> int {
        KWS_HIP(hipMemcpyAsync(m, c->m, c->P * sizeof(float), hipMemcpyDeviceToHost, st));
        KWS_HIP(hipMemcpyAsync(v, c->v, c->P * sizeof(float), hipMemcpyDeviceToHost, st));
        return KWS_OK;
    }, true);
}

int train_stats(const TrainCore* c, int cv_chunk_rows, size_t* device_bytes, int32_t* allocs, int32_t* steps, int32_t* launches, int32_t* chunk_rows) {
    if (!c) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (device_bytes) *device_bytes = c->state_bytes + c->arena_bytes;
    if (allocs) *allocs = c->allocs;
    if (steps) *steps = c->steps;
    if (launches) *launches = c->launches;
    if (chunk_rows) *chunk_rows = cv_chunk_rows;
    return KWS_OK;
}

int check_optimizer(float keep_prob, int optimizer, float max_grad_norm) {
    if (!(keep_prob > 0.f && keep_prob <= 1.f)) return fail(KWS_ERR_UNSUPPORTED, "keep_prob=%g outside (0, 1]", (double)keep_prob);
    if (optimizer != KWS_OPT_ADAM && optimizer != KWS_OPT_NESTEROV)
        return fail(KWS_ERR_INVALID_ARGUMENT, "optimizer=%d: KWS_OPT_ADAM (0) or KWS_OPT_NESTEROV (1)", optimizer);
    if (!std::isfinite(max_grad_norm)) return fail(KWS_ERR_INVALID_ARGUMENT, "max_grad_norm=%g is not finite", (double)max_grad_norm);
    return KWS_OK;
}

int check_s_max(int S_max) {
    if (S_max < 0 || S_max > 31)
        return fail(KWS_ERR_INVALID_ARGUMENT, "S_max=%d out of range [0,31]: one lane of a wave per state of the extended label", S_max);
    return KWS_OK;
}

int check_ctc_lds(int rows, int S_max, const char* rows_text) {
    const size_t lds = kws::ctc_loss_lds_bytes(rows, S_max);
    if (lds <= kWindowIncLdsMax) return KWS_OK;
    char what[48];
    snprintf(what, sizeof(what), rows_text, rows);
    return fail(KWS_ERR_UNSUPPORTED, "the CTC loss keeps %s x (8 log-probabilities + %d states) in LDS: %zu bytes exceed the %zu a workgroup may hold",
                what, 2 * S_max + 1, lds, kWindowIncLdsMax);
}

}  // namespace kws_host
