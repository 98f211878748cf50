// C ABI of the self-attention model's sliding-window stream manager (include/kws_amd.h, kws_attention_stream_*): per chunk the
// front-end with the per-stream gate, the window update, the model over every stream's whole window, the decision
// (attention_stream_kernels.hip).  The handle borrows the attention and front-end handles and owns, per stream, the sample carry, the
// mel window and the slot lengths; one chunk's intermediates are carved out of the attention handle's staging block.
#include <new>

#include "api_internal.h"

using namespace kws_host;

struct kws_attention_stream {
    kws_attention* model = nullptr;
    kws_frontend* fe = nullptr;
    unsigned long long model_serial = 0, fe_serial = 0;      // live_serial() of the borrowed handles at create
    int B = 0, max_chunk = 0, tmax = 0, nq = 0, W = 0, T1max = 0, n_label = 0, cur = 0;
    float vad_thres = 0.f, thres = 0.f;
    uint8_t delta[256] = {0};         // the label's matcher over emitted words (window_label_delta)
    // owned, one allocation: the carried samples and their lengths (they ping-pong, as in the ragged GRU manager: rows of fft - 1
    // floats), the window [B][W][n_mel], its slots' frame counts [B][nq], and per stream the slots held and the frames held
    char* owned = nullptr;
    size_t owned_bytes = 0;
    float* carry[2] = {nullptr, nullptr};
    int32_t* carry_len[2] = {nullptr, nullptr};
    float* win = nullptr;
    int32_t *slot_frames = nullptr, *count = nullptr, *len = nullptr;
    int launches_last = 0;
    // one chunk's intermediates, carved out of kws_attention::stage at every feed (stream_carve)
    size_t stage_bytes = 0;
    float *mel = nullptr, *softmax = nullptr;      // [B][tmax][n_mel], [B][T1max][C]
    uint8_t *silent = nullptr, *reset = nullptr, *skip = nullptr;
    int32_t *frames = nullptr, *run_len = nullptr;
};

namespace {

int frames_out(const kws_attention_config& c, int T) { return c.combine_frame > 1 ? T / c.combine_frame + 1 : T; }

template <typename P>
void take(P*& p, uintptr_t base, size_t& at, size_t count) {
    p = reinterpret_cast<P*>(base + at);
    at += (count * sizeof(P) + 255) & ~size_t(255);
}
size_t stream_carve(kws_attention_stream* s, uintptr_t base) {
    size_t at = 0;
    const size_t B = s->B;
    take(s->mel, base, at, B * s->tmax * s->model->cfg.n_mel);
    take(s->softmax, base, at, B * s->T1max * s->model->cfg.num_classes);
    take(s->silent, base, at, B);
    take(s->reset, base, at, B);
    take(s->skip, base, at, B);
    take(s->frames, base, at, B);
    take(s->run_len, base, at, B);
    return at;
}
size_t owned_carve(kws_attention_stream* s, uintptr_t base) {
    size_t at = 0;
    const size_t B = s->B, row = s->fe->cfg.fft_size - 1;
    take(s->carry[0], base, at, B * row);
    take(s->carry[1], base, at, B * row);
    take(s->carry_len[0], base, at, B);
    take(s->carry_len[1], base, at, B);
    take(s->win, base, at, B * s->W * s->model->cfg.n_mel);
    take(s->slot_frames, base, at, B * s->nq);
    take(s->count, base, at, B);
    take(s->len, base, at, B);
    return at;
}

int stream_check(kws_attention_stream* h) {
    if (live_serial(h->model) != h->model_serial || live_serial(h->fe) != h->fe_serial)
        return fail(KWS_ERR_INVALID_ARGUMENT, "the attention model or front-end this stream manager was created on has been destroyed");
    return KWS_OK;
}

// body(stream) with the attention handle held, `stream` ordered behind the handle's previous call and the staging pointers set
template <typename F>
int with_model_held(kws_attention_stream* h, void* stream, const char* what, F&& body) {
    kws_attention* model = h->model;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    BusyGuard busy(model->in_call);
    if (!busy.owned)
        return fail(KWS_ERR_BUSY, "%s: another host thread is inside a call on the attention handle (one thread at a time per handle)", what);
    if (h->stage_bytes > model->stage_bytes) return fail(KWS_ERR_INVALID_ARGUMENT, "internal: the attention handle's staging block is smaller than this stream's");
    KWS_TRY(attn_call_enter(model, st));
    stream_carve(h, reinterpret_cast<uintptr_t>(model->stage));
    const int rc = body(st);
    const int rl = attn_call_leave(model, st);
    return rc != KWS_OK ? rc : rl;
}

}  // namespace

extern "C" {

int kws_attention_stream_create(kws_attention_handle model, kws_frontend_handle frontend, int B, int max_chunk_samples, int window_chunks,
                                float vad_thres, float decode_thres, const char* label, kws_attention_stream_handle* out) {
    // every refusal in front of the first device call; those that need no handle first
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!model) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument: model");
    if (!frontend) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument: frontend");
    if (!label) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument: label");
    if (B < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "B=%d must be at least 1", B);
    if (window_chunks < 1 || window_chunks > 64)
        return fail(KWS_ERR_UNSUPPORTED, "window_chunks=%d unsupported (1..64)", window_chunks);
    if (max_chunk_samples < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "max_chunk_samples=%d must be at least 1", max_chunk_samples);
    const int n = (int)strlen(label);
    if (n == 0) return fail(KWS_ERR_INVALID_ARGUMENT, "label is empty (every window would fire)");
    if (n > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "label longer than 15 digits (the matcher has 16 states)");
    KWS_TRY(label_digits(label, n, nullptr));
    const unsigned long long ms = live_serial(model), fs = live_serial(frontend);
    if (!ms || !fs) return fail(KWS_ERR_INVALID_ARGUMENT, "attention model or front-end handle is not alive (destroyed, or not a handle)");
    const kws_attention_config& c = model->cfg;
    if (frontend->framing != KWS_FRAMES_DEPLOY) return frontend_needs_deploy_frames("kws_attention_stream_create");
    if (!frontend->plain())
        return fail(KWS_ERR_UNSUPPORTED, "kws_attention_stream_create takes a magnitude-mel front-end only: this one has %s (a whole-utterance "
                    "transform)", frontend->kind == KWS_FEAT_MFCC ? "kind=KWS_FEAT_MFCC" : "power=2");
    if (!frontend->use_fft) return frontend_needs_fft400(frontend, "the attention stream manager's per-stream chunks");
    if (frontend->cfg.n_mel != c.n_mel)
        return fail(KWS_ERR_INVALID_ARGUMENT, "front-end produces n_mel=%d mel bins, the model takes n_mel=%d", frontend->cfg.n_mel, c.n_mel);
    for (int i = 0; i < n; ++i)
        if (label[i] - '0' > c.num_classes - 2)
            return fail(KWS_ERR_INVALID_ARGUMENT, "label digit %c outside 1..%d (num_classes=%d: classes 1..C-2 are words)", label[i],
                        c.num_classes - 2, c.num_classes);
    const int fft = frontend->cfg.fft_size;
    const int tmax = kws_frontend_frames(&frontend->cfg, fft - 1 + max_chunk_samples);
    const long long W = (long long)window_chunks * tmax;
    if (W > c.max_frames)
        return fail(KWS_ERR_UNSUPPORTED, "window_chunks=%d x %d frames per chunk of max_chunk_samples=%d = %lld frames exceed the model's "
                    "max_frames=%d", window_chunks, tmax, max_chunk_samples, W, c.max_frames);
    if (W < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "max_chunk_samples=%d completes no frame", max_chunk_samples);
    if (B > 65535) return fail(KWS_ERR_UNSUPPORTED, "B=%d unsupported (<= 65535)", B);
    if (!frontend_takes_fft400(frontend, B, tmax))
        return fail(KWS_ERR_UNSUPPORTED, "B*T=%lld frames exceed the front-end's grid", (long long)B * tmax);

    kws_attention_stream* s = new (std::nothrow) kws_attention_stream();
    if (!s) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->model = model; s->fe = frontend; s->model_serial = ms; s->fe_serial = fs;
    s->B = B; s->max_chunk = max_chunk_samples; s->tmax = tmax; s->nq = window_chunks; s->W = (int)W;
    s->T1max = frames_out(c, (int)W); s->n_label = n; s->vad_thres = vad_thres; s->thres = decode_thres;
    window_label_delta(label, n, s->delta);
    s->owned_bytes = owned_carve(s, 0);
    s->stage_bytes = stream_carve(s, 0);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->owned), s->owned_bytes);
    if (e == hipSuccess) e = hipMemset(s->owned, 0, s->owned_bytes);      // no carry, empty windows
    if (e != hipSuccess) { kws_attention_stream_destroy(s); return hip_fail(e, "hipMalloc(attention stream buffers)"); }
    owned_carve(s, reinterpret_cast<uintptr_t>(s->owned));
    int rc = KWS_OK;
    {
        BusyGuard busy(model->in_call);
        if (!busy.owned) rc = fail(KWS_ERR_BUSY, "kws_attention_stream_create: another host thread is inside a call on the attention handle");
        else rc = attn_stage_reserve_locked(model, s->stage_bytes);
        if (rc == KWS_OK) rc = attn_reserve_locked(model, B, s->W);      // a feed never allocates afterwards
    }
    if (rc == KWS_OK) rc = hip_done(hipDeviceSynchronize(), "hipDeviceSynchronize");      // the zeros have landed before any stream launches
    if (rc != KWS_OK) { kws_attention_stream_destroy(s); return rc; }
    *out = s;
    return KWS_OK;
}

int kws_attention_stream_destroy(kws_attention_stream_handle h) {
    if (!h) return KWS_OK;
    hipDeviceSynchronize();
    if (h->owned) hipFree(h->owned);
    delete h;
    return KWS_OK;
}

int kws_attention_stream_feed(kws_attention_stream_handle h, const void* pcm, int n_max, const int32_t* n_per_stream, int pcm_int16,
                              int32_t* hit, float* softmax, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (n_max < 0 || n_max > h->max_chunk)
        return fail(KWS_ERR_INVALID_ARGUMENT, "rows of n_max=%d samples outside [0,%d] (max_chunk_samples)", n_max, h->max_chunk);
    if (!hit) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument: hit");
    if (!pcm && n_max > 0) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument: pcm");
    KWS_TRY(stream_check(h));
    const kws_attention_config& c = h->model->cfg;
    const int B = h->B;
    if (n_max == 0) {          // every stream's chunk is empty: every iteration is skipped, nothing is read or written but the outputs
        const hipStream_t st = static_cast<hipStream_t>(stream);
        KWS_HIP(hipMemsetAsync(hit, 0, (size_t)B * sizeof(int32_t), st));
        if (softmax) KWS_HIP(hipMemsetAsync(softmax, 0, (size_t)B * h->T1max * c.num_classes * sizeof(float), st));
        h->launches_last = 0;
        return KWS_OK;
    }
    return with_model_held(h, stream, "kws_attention_stream_feed", [&](hipStream_t st) -> int {
        const kws_frontend_config& fc = h->fe->cfg;
        const int fft = fc.fft_size, T = kws_frontend_frames(&fc, fft - 1 + n_max);
        int launches = 0;
        // 1: the FFT front-end with the per-stream gate -- vad and the silent mask, the chunk's frames of [carry | chunk], the next carry
        // and its length, the frame count and the skip flag of every stream (fft_frontend.hip, stream_gate)
        kws::FrontendParams p = frontend_params(h->fe, true, B, T);
        p.gate = 1; p.vad_thres = h->vad_thres; p.restart = nullptr; p.silent = h->silent; p.reset = h->reset;
        if (pcm_int16) p.pcm_i16 = static_cast<const int16_t*>(pcm);
        else p.pcm = static_cast<const float*>(pcm);
        p.carry = h->carry[h->cur]; p.next = h->carry[h->cur ^ 1]; p.n_next = fft - 1;
        p.n_carry = 0; p.carry_stride = fft - 1;
        p.carry_len = h->carry_len[h->cur]; p.next_len = h->carry_len[h->cur ^ 1];
        p.lens = n_per_stream; p.n_max = n_max; p.frames = h->frames; p.skip = h->skip;
        p.mel = h->mel; p.n_samples = n_max;
        KWS_TRY(hip_done(kws::launch_mel_fft400(p, B, st), "launch mel_fft400 (attention stream)"));
        h->cur ^= 1;          // the samples and lengths are in the other buffer now
        ++launches;
        // 2: the window
        kws::AttnStreamWindowParams wp = {};
        wp.mel = h->mel; wp.frames = h->frames; wp.skip = h->skip; wp.silent = h->silent;
        wp.win = h->win; wp.slot_frames = h->slot_frames; wp.count = h->count; wp.len = h->len; wp.run_len = h->run_len;
        wp.B = B; wp.T = T; wp.W = h->W; wp.F = c.n_mel; wp.nq = h->nq;
        KWS_TRY(hip_done(kws::launch_attn_stream_window(wp, st), "launch attn_stream_window"));
        ++launches;
        // 3: the model over every stream's window: kws_attention_run(win, run_len, B, W)
        float* sm = softmax ? softmax : h->softmax;
        KWS_TRY(attn_run_locked(h->model, h->win, h->run_len, B, h->W, nullptr, sm, st));
        launches += 2 + 3 * c.num_layers;
        // 4: the decision
        kws::AttnStreamDecideParams dp = {};
        dp.softmax = sm; dp.run_len = h->run_len; dp.count = h->count; dp.len = h->len; dp.hit = hit;
        dp.B = B; dp.T1max = h->T1max; dp.C = c.num_classes; dp.c = c.combine_frame; dp.n_label = h->n_label; dp.thres = h->thres;
        memcpy(dp.delta, h->delta, 256);
        KWS_TRY(hip_done(kws::launch_attn_stream_decide(dp, st), "launch attn_stream_decide"));
        h->launches_last = launches + 1;
        return KWS_OK;
    });
}

int kws_attention_stream_recycle(kws_attention_stream_handle h, const uint8_t* slots, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!slots) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument: slots");
    KWS_TRY(stream_check(h));
    return with_model_held(h, stream, "kws_attention_stream_recycle", [&](hipStream_t st) -> int {
        kws::AttnStreamRecycleParams p = {};
        p.slots = slots; p.carry_len = h->carry_len[h->cur]; p.count = h->count; p.len = h->len; p.B = h->B;
        return hip_done(kws::launch_attn_stream_recycle(p, st), "launch attn_stream_recycle");
    });
}

int kws_attention_stream_window(kws_attention_stream_handle h, float* mel, int32_t* frames, int32_t* chunks, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!frames) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument: frames");
    if (!chunks) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument: chunks");
    KWS_TRY(stream_check(h));
    return with_model_held(h, stream, "kws_attention_stream_window", [&](hipStream_t st) -> int {
        const size_t B = (size_t)h->B;
        if (mel) KWS_HIP(hipMemcpyAsync(mel, h->win, B * h->W * h->model->cfg.n_mel * sizeof(float), hipMemcpyDeviceToDevice, st));
        KWS_HIP(hipMemcpyAsync(frames, h->len, B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        KWS_HIP(hipMemcpyAsync(chunks, h->count, B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        return KWS_OK;
    });
}

int kws_attention_stream_carry(kws_attention_stream_handle h, float* samples, int32_t* lengths, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!samples) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument: samples");
    if (!lengths) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument: lengths");
    KWS_TRY(stream_check(h));
    return with_model_held(h, stream, "kws_attention_stream_carry", [&](hipStream_t st) -> int {
        const size_t B = (size_t)h->B, row = (size_t)(h->fe->cfg.fft_size - 1) * sizeof(float);
        KWS_HIP(hipMemcpyAsync(samples, h->carry[h->cur], B * row, hipMemcpyDeviceToDevice, st));
        KWS_HIP(hipMemcpyAsync(lengths, h->carry_len[h->cur], B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        return KWS_OK;
    });
}

int kws_attention_stream_stats(kws_attention_stream_handle h, size_t* device_bytes, int32_t* launches_last_feed) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (device_bytes) *device_bytes = h->owned_bytes;
    if (launches_last_feed) *launches_last_feed = h->launches_last;
    return KWS_OK;
}

}  // extern "C"
