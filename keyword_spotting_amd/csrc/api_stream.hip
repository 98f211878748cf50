// C ABI of libkws_amd.so (include/kws_amd.h): the stream manager -- gate, front-end, GRU step and decode window of one chunk per call.
// A manager created by kws_stream_create_heads (kws_stream::win2 set) decodes BOTH heads of a customised-keyword model per chunk: the
// same gate and front-end, the stack planned as a heads step (every layer to a seam), then heads_window_kernel -- both heads' rows,
// both windows and the coupled clear + restart in one launch (heads_window.hip) -- in lock-step and ragged feeds alike; recycling
// empties both windows.  Every other entry point takes such a handle unchanged.
#include <new>

#include "api_internal.h"

using namespace kws_host;

namespace {

// The decode half of an iteration, behind the gate and the front-end: the GRU step of the chunk's T frames on the manager's state in
// place (reset where the gate found silence) and the window step, in the one form the chunk allows.  frames / skip: the ragged
// feed's per-stream frame counts and skip flags (the step's seq_len: copy-through past them; a skipped stream has reset 0 and 0
// frames, its state comes back unchanged), or null.
int stream_decode(kws_stream_handle h, int T, const int32_t* frames, const uint8_t* skip, int32_t* hit, hipStream_t st) {
    StepArgs step;
    step.state_in = h->state; step.state_out = h->state; step.reset_mask = h->reset; step.seq_len = frames;
    step.B = h->B; step.T = T; step.stream = st; step.locked = true;
    if (T) step.mel = h->mel;
    KWS_TRY(window_bind_label(h->win, h->label));      // (bound at kws_stream_create; refuses a window that went on with another label)
    if (h->win2) {
        // a two-head manager: front-end + L layers + 1 launches -- the stack once, every layer to a seam as a heads step plans it, then
        // heads_window_kernel: both heads' rows -> words -> their own windows, and the coupled clear + restart (heads_window.hip)
        KWS_TRY(window_bind_label(h->win2, h->label2));
        HeadsArgs ha = heads_window_args(h->win, h->win2, h->silent, hit, h->restart);
        ha.frames = frames; ha.skip = skip;
        const kws::BankRef bank = h->bank ? bank_ref(h->bank, h->user) : kws::BankRef{};
        if (h->bank) ha.bank = &bank;            // head 2 of every stream from its own bank slot (bank_heads_window_kernel)
        if (h->bank) ha.bank_slots = bank_slots(h->bank);      // ... over its slot's own keyword where the bank has any
        step.heads = &ha;
        return step_impl(h->model, step);
    }
    const kws::WindowTail wt = window_tail_params(h->win, h->silent, hit, h->restart);
    StepArgs fused = step;
    fused.wt = &wt; fused.decode2_thres = h->win->thres;
    // THREE launches per chunk (two for the bf16 stack): the decode-window step (prob_queue.add, ctc_decode2 over the window,
    // ctc_predict, clear + restart on a hit: detector.py:195-209) rides at the end of the last layer's launch, on the frame words its
    // flush has just produced -- no softmax round trip, no fourth launch.  The window's threshold is the fused decoder's (ctc_decode2's
    // frame rule, utils/prediction.py:74).  Not on a ragged chunk: the tail instantiations take no lengths
    if (T && !frames && step_takes_window(h->model, fused)) return step_impl(h->model, fused);
    if (T) step.softmax = h->softmax;
    KWS_TRY(step_impl(h->model, step));
    kws::WindowIncParams wp = {};      // window_inc_kernel behind the stack, over each stream's own frames
    wp.win = wt;
    memcpy(wp.delta, h->win->inc_delta, 256);
    wp.softmax = step.softmax; wp.thres = h->win->thres; wp.B = h->B; wp.T = T; wp.C = h->win->C;
    wp.frames = frames; wp.skip = skip;
    return hip_done(kws::launch_window_inc(wp, st), "launch window_inc");
}

// One iteration with the model handle held and `st` ordered (kws_stream_feed below).  A chunk that completes no frame is the same
// iteration over T = 0 frames, as in the reference (detector.py:168-209): vad -> clean_state() + prob_queue.clear() when silent, the
// samples are carried (:179-183 keeps all of them), sess.run over zero frames returns the state unchanged and an empty softmax,
// which takes a slot of the window (:195) before the windowed decode (:197-201).
int stream_feed_locked(kws_stream_handle h, const void* pcm, int n, int pcm_int16, int32_t* hit, hipStream_t st) {
    const kws_frontend_config& fc = h->fe->cfg;
    const int fft = fc.fft_size, hop = fc.hop_size, B = h->B;
    const int total = h->n_carry + n, T = kws_frontend_frames(&fc, total);
    const int keep = T ? (total - fft) % hop + (fft - hop) : total;                      // detector.py:181-182
    const float* chunk = pcm_int16 ? h->pcm_f32 : static_cast<const float*>(pcm);
    const float* carry = h->n_carry ? h->carry[h->cur] : nullptr;
    float* next = h->carry[h->cur ^ 1];
    if (T && frontend_takes_fft400(h->fe, B, T)) {
        // ONE launch: vad + masks and the next carry ride on the FFT front-end, which reads the PCM -- int16 as it is -- in place
        kws::FrontendParams gate = {};
        gate.gate = 1; gate.pcm_i16 = pcm_int16 ? static_cast<const int16_t*>(pcm) : nullptr; gate.vad_thres = h->vad_thres;
        gate.restart = h->restart; gate.silent = h->silent; gate.reset = h->reset; gate.next = next; gate.n_next = keep;
        KWS_TRY(frontend_run_impl(h->fe, carry, h->n_carry, pcm_int16 ? nullptr : chunk, n, B, h->mel, st, &gate));
    } else {
        // other frame lengths: one pass over the new chunk (int16 -> float, vad + masks, next carry), then the dense-DFT kernel
        KWS_TRY(hip_done(kws::launch_vad_gate(pcm, pcm_int16, B, n, h->vad_thres, h->pcm_f32, h->restart, h->silent, h->reset, carry,
                                              h->n_carry, next, keep, st), "launch vad_gate"));
        if (T) KWS_TRY(kws_frontend_run_carry(h->fe, carry, h->n_carry, chunk, n, B, h->mel, nullptr, 0, st));
    }
    KWS_TRY(stream_decode(h, T, nullptr, nullptr, hit, st));
    h->n_carry = keep; h->cur ^= 1;
    return KWS_OK;
}

// One ragged iteration (kws_stream_feed_ragged; kws_stream_feed once the handle is ragged, lens == null: n_max for every stream),
// with the model handle held and `st` ordered.  Three or four launches whatever the lengths: the FFT front-end with the per-stream
// gate (vad, masks, next carry and its length, frame count, skip flag), then stream_decode over T = frames of n_max samples after a
// full carry, each stream on its own frames.
int stream_feed_ragged_locked(kws_stream_handle h, const void* pcm, int n_max, const int32_t* lens, int pcm_int16, int32_t* hit,
                              hipStream_t st) {
    const kws_frontend_config& fc = h->fe->cfg;
    const int fft = fc.fft_size, B = h->B;
    if (n_max == 0) {           // every stream's chunk is empty: every iteration is skipped (nothing is read or written,
                                // the carry layout -- and so the handle's mode -- stays as it is; kws_amd.h)
        KWS_HIP(hipMemsetAsync(hit, 0, (size_t)B * sizeof(int32_t), st));
        return KWS_OK;
    }
    const int T = kws_frontend_frames(&fc, fft - 1 + n_max);
    kws::FrontendParams p = frontend_params(h->fe, true, B, T);      // (stream_check: the FFT kernel takes B x tmax frames)
    p.gate = 1; p.vad_thres = h->vad_thres; p.restart = h->restart; p.silent = h->silent; p.reset = h->reset;
    if (pcm_int16) p.pcm_i16 = static_cast<const int16_t*>(pcm);
    else p.pcm = static_cast<const float*>(pcm);
    // lock-step layout on the first ragged call: rows of n_carry samples, one length for all; the output is in the ragged layout
    p.carry = h->carry[h->cur]; p.next = h->carry[h->cur ^ 1]; p.n_next = fft - 1;
    p.n_carry = h->ragged ? 0 : h->n_carry;
    p.carry_stride = h->ragged ? fft - 1 : h->n_carry;
    p.carry_len = h->ragged ? h->carry_len[h->cur] : nullptr;
    p.next_len = h->carry_len[h->cur ^ 1];
    p.lens = lens; p.n_max = n_max; p.frames = h->frames; p.skip = h->skip;
    p.mel = h->mel; p.n_samples = p.n_carry + n_max;
    KWS_TRY(hip_done(kws::launch_mel_fft400(p, B, st), "launch mel_fft400 (ragged)"));
    h->ragged = true; h->n_carry = 0; h->cur ^= 1;          // the samples and lengths are in the other buffer now
    return stream_decode(h, T, h->frames, h->skip, hit, st);
}

// The checks every stream-handle call shares: the borrowed handles are alive; the per-stream paths need the FFT front-end.
int stream_check(kws_stream_handle h, bool ragged_call) {
    if (live_serial(h->model) != h->model_serial || live_serial(h->fe) != h->fe_serial || live_serial(h->win) != h->win_serial ||
        (h->win2 && live_serial(h->win2) != h->win2_serial) || (h->bank && live_serial(h->bank) != h->bank_serial))
        return fail(KWS_ERR_INVALID_ARGUMENT, "the model, front-end, window or bank this stream was created on has been destroyed");
    if (ragged_call && !h->fe->use_fft) return frontend_needs_fft400(h->fe, "per-stream chunk lengths");
    if (ragged_call && !frontend_takes_fft400(h->fe, h->B, h->tmax))
        return fail(KWS_ERR_UNSUPPORTED, "B*T=%lld frames exceed the ragged front-end's grid", (long long)h->B * h->tmax);
    return KWS_OK;
}

// One chunk's intermediates, carved out of a staging block at `base`; returns their size.  kws_stream_create sizes the model handle's
// block with it, so a feed never allocates.  The widened copy of int16 PCM is read by the dense-DFT front-end only (the 400-point FFT
// reads int16 in place); with the FFT front-end it is written just by the gate of a chunk that completes no frame (< fft samples in total).
size_t stream_carve(kws_stream* s, uintptr_t base) {
    size_t at = 0;
    auto take = [&](auto*& p, size_t count) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + at);
        at += (count * sizeof(*p) + 255) & ~size_t(255);
    };
    const size_t B = s->B, tm = s->tmax > 0 ? s->tmax : 1;
    const bool fused_gate = frontend_takes_fft400(s->fe, s->B, (int)tm);       // then for every chunk with a frame
    take(s->pcm_f32, B * (fused_gate ? std::min(s->max_chunk, s->fe->cfg.fft_size - 1) : s->max_chunk));
    take(s->mel, B * tm * s->model->cfg.n_mel);
    take(s->softmax, s->win2 ? 0 : B * tm * s->model->cfg.num_classes);
    take(s->silent, B);
    take(s->reset, B);
    take(s->frames, B);
    take(s->skip, B);
    return at;
}

// Runs `body(stream)` with the model handle held (its staging and seams are the handle's) and `stream` ordered behind the handle's
// previous call when that ran on another stream; the chunk's staging pointers are set for it.
template <typename F>
int with_model_held(kws_stream_handle h, void* stream, const char* what, F&& body) {
    kws_model* model = h->model;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    BusyGuard busy(model->in_call);
    if (!busy.owned)
        return fail(KWS_ERR_BUSY, "%s: another host thread is inside a call on the model handle (one thread at a time per "
                    "handle; stream managers that run concurrently need a model handle each)", what);
    if (h->stage_bytes > model->stage.bytes) return fail(KWS_ERR_INVALID_ARGUMENT, "internal: the model handle's staging block is smaller than this stream's");
    KWS_TRY(call_enter(model, st));
    stream_carve(h, reinterpret_cast<uintptr_t>(model->stage.base));
    const int rc = body(st);
    const int rl = call_leave(model, st);
    return rc != KWS_OK ? rc : rl;
}

}  // namespace

// kws_stream_create (window2 == null), kws_stream_create_heads and kws_stream_create_bank (`who` names the entry point in the refusals)
int kws_host::stream_create_impl(const char* who, kws_handle model, kws_frontend_handle frontend, kws_window_handle window,
                                 kws_window_handle window2, int B, int max_chunk_samples, float vad_thres, const char* label, const char* label2,
                                 float* state, uint8_t* restart, kws_stream_handle* out, kws_bank* bank, const int32_t* user) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!model || !frontend || !window || !state || !restart || !label) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument");
    const unsigned long long ms = live_serial(model), fs = live_serial(frontend), ws = live_serial(window);
    const unsigned long long ws2 = window2 ? live_serial(window2) : 0;
    if (!ms || !fs || !ws || (window2 && !ws2))
        return fail(KWS_ERR_INVALID_ARGUMENT, "model, front-end or window handle is not alive (destroyed, or not a handle)");
    if (window2 && model->num_classes2 <= 0)
        return fail(KWS_ERR_INVALID_ARGUMENT, "%s needs a model handle with a second class head (kws_create_heads)", who);
    if (frontend->framing != KWS_FRAMES_DEPLOY) return frontend_needs_deploy_frames(who);
    if (!frontend->plain())
        return fail(KWS_ERR_UNSUPPORTED, "%s takes a magnitude-mel front-end only: this one has %s (the reference's streaming "
                    "detector has no MFCC branch)", who, frontend->kind == KWS_FEAT_MFCC ? "kind=KWS_FEAT_MFCC" : "power=2");
    if (B < 1 || max_chunk_samples < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "bad stream shape B=%d max_chunk_samples=%d", B, max_chunk_samples);
    const int n = (int)strlen(label);
    if (n > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "label longer than 15 digits (the incremental window's matcher has 16 states)");
    KWS_TRY(label_digits(label, n, nullptr));
    const int n2 = window2 ? (int)strlen(label2) : 0;
    if (n2 > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "label2 longer than 15 digits (the incremental window's matcher has 16 states)");
    if (window2) KWS_TRY(label_digits(label2, n2, nullptr));
    if (frontend->cfg.n_mel != model->cfg.n_mel)
        return fail(KWS_ERR_INVALID_ARGUMENT, "front-end produces %d mel bins, the model takes %d", frontend->cfg.n_mel, model->cfg.n_mel);
    if (window->B != B || window->C != model->cfg.num_classes)
        return fail(KWS_ERR_INVALID_ARGUMENT, "window was created for B=%d C=%d, stream needs B=%d C=%d", window->B, window->C, B,
                    model->cfg.num_classes);
    const int fft = frontend->cfg.fft_size;
    const int tmax = kws_frontend_frames(&frontend->cfg, max_chunk_samples + fft - 1);
    if (tmax > window->tmax)
        return fail(KWS_ERR_INVALID_ARGUMENT, "chunks of %d samples give up to %d frames, the window holds %d per chunk", max_chunk_samples,
                    tmax, window->tmax);
    if (window2) KWS_TRY(heads_window_check(model, window, window2, B, tmax, bank));      // both windows' class counts, batch, frames; the LDS of the launch
    if (!window2 && window_inc_lds_bytes(tmax, window->nq) > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "chunks of up to %d frames with a %d-chunk window need %zu bytes of LDS in the incremental window step "
                    "(limit %zu): use shorter chunks", tmax, window->nq, window_inc_lds_bytes(tmax, window->nq), kWindowIncLdsMax);
    kws_stream* s = new (std::nothrow) kws_stream();
    if (!s) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->model_serial = ms; s->fe_serial = fs; s->win_serial = ws;
    s->win2 = window2; s->win2_serial = ws2;
    s->bank = bank; s->bank_serial = bank ? live_serial(bank) : 0; s->user = user;
    if (window2) memcpy(s->label2, label2, n2);
    s->model = model; s->fe = frontend; s->win = window; s->B = B; s->max_chunk = max_chunk_samples; s->tmax = tmax;
    s->vad_thres = vad_thres; s->state = state; s->restart = restart;
    memcpy(s->label, label, n);
    const size_t carry_bytes = (size_t)B * (fft - 1) * sizeof(float);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->carry[0]), carry_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->carry[1]), carry_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->carry_len[0]), (size_t)B * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->carry_len[1]), (size_t)B * sizeof(int32_t));
    if (e != hipSuccess) { kws_stream_destroy(s); return hip_fail(e, "hipMalloc(stream buffers)"); }
    s->stage_bytes = stream_carve(s, 0);
    int rc = KWS_OK;
    {
        BusyGuard busy(model->in_call);
        if (!busy.owned) rc = fail(KWS_ERR_BUSY, "kws_stream_create: another host thread is inside a call on the model handle");
        else      // grows only here; the old block may still be read by a feed in flight
            rc = grow_device(model, &model->stage.bytes, s->stage_bytes, false, {{reinterpret_cast<void**>(&model->stage.base), s->stage_bytes}},
                             "hipMalloc(stream staging)");
    }
    if (rc == KWS_OK) rc = kws_reserve(model, B, tmax);            // the GRU step of a chunk never allocates afterwards
    if (rc == KWS_OK) rc = window_bind_label(window, s->label);      // the window's summaries are built for this label
    if (rc == KWS_OK && window2) rc = window_bind_label(window2, s->label2);      // ... each window for its own
    if (rc != KWS_OK) { kws_stream_destroy(s); return rc; }
    *out = s;
    return KWS_OK;
}

extern "C" {

int kws_stream_create(kws_handle model, kws_frontend_handle frontend, kws_window_handle window, int B, int max_chunk_samples,
                      float vad_thres, const char* label, float* state, uint8_t* restart, kws_stream_handle* out) {
    return stream_create_impl("kws_stream_create", model, frontend, window, nullptr, B, max_chunk_samples, vad_thres, label, nullptr, state,
                              restart, out);
}

int kws_stream_create_heads(kws_handle model, kws_frontend_handle frontend, kws_window_handle window1, kws_window_handle window2, int B,
                            int max_chunk_samples, float vad_thres, const char* label1, const char* label2, float* state, uint8_t* restart,
                            kws_stream_handle* out) {
    if (out) *out = nullptr;
    if (!window2 || !label2) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument");
    return stream_create_impl("kws_stream_create_heads", model, frontend, window1, window2, B, max_chunk_samples, vad_thres, label1, label2,
                              state, restart, out);
}

int kws_stream_destroy(kws_stream_handle h) {
    if (!h) return KWS_OK;
    hipDeviceSynchronize();
    for (void* p : {(void*)h->carry[0], (void*)h->carry[1], (void*)h->carry_len[0], (void*)h->carry_len[1]}) if (p) hipFree(p);
    delete h;
    return KWS_OK;
}

int kws_stream_reset(kws_stream_handle h) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    h->n_carry = 0;
    h->ragged = false;        // lock-step with no carry: the per-stream lengths are forgotten with the samples
    return KWS_OK;
}

int kws_stream_feed(kws_stream_handle h, const void* pcm, int n, int pcm_int16, int32_t* hit, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (n < 0 || n > h->max_chunk) return fail(KWS_ERR_INVALID_ARGUMENT, "chunk of %d samples outside [0,%d]", n, h->max_chunk);
    if (!hit || (!pcm && n > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    KWS_TRY(stream_check(h, false));
    if (n == 0) {            // detector.py:164-166: an empty read is skipped before anything else happens
        KWS_HIP(hipMemsetAsync(hit, 0, (size_t)h->B * sizeof(int32_t), static_cast<hipStream_t>(stream)));
        return KWS_OK;
    }
    return with_model_held(h, stream, "kws_stream_feed", [&](hipStream_t st) {     // (per-stream carry layout: the ragged iteration, every length n)
        return h->ragged ? stream_feed_ragged_locked(h, pcm, n, nullptr, pcm_int16, hit, st) : stream_feed_locked(h, pcm, n, pcm_int16, hit, st);
    });
}

int kws_stream_feed_ragged(kws_stream_handle h, const void* pcm, int n_max, const int32_t* n_per_stream, int pcm_int16, int32_t* hit,
                           void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (n_max < 0 || n_max > h->max_chunk) return fail(KWS_ERR_INVALID_ARGUMENT, "rows of %d samples outside [0,%d]", n_max, h->max_chunk);
    if (!hit || !n_per_stream || (!pcm && n_max > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    KWS_TRY(stream_check(h, true));
    return with_model_held(h, stream, "kws_stream_feed_ragged",
                           [&](hipStream_t st) { return stream_feed_ragged_locked(h, pcm, n_max, n_per_stream, pcm_int16, hit, st); });
}

int kws_stream_recycle(kws_stream_handle h, const uint8_t* slots, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!slots) return fail(KWS_ERR_INVALID_ARGUMENT, "slots is null");
    KWS_TRY(stream_check(h, true));
    return with_model_held(h, stream, "kws_stream_recycle", [&](hipStream_t st) -> int {
        const kws_config& c = h->model->cfg;
        kws::StreamRecycleParams p = {};
        p.slots = slots; p.state = h->state; p.restart = h->restart; p.head = h->win->inc_head; p.count = h->win->inc_count;
        p.L = c.num_layers; p.B = h->B; p.H = c.hidden;
        if (h->ragged) {
            p.len_out = h->carry_len[h->cur];                     // in place: only the recycled streams' lengths change
        } else {
            // leaves the lock-step layout: the other streams' carries move to rows of fft - 1 samples with their length
            p.carry_in = h->carry[h->cur]; p.n_carry = h->n_carry;
            p.carry_out = h->carry[h->cur ^ 1]; p.carry_out_stride = h->fe->cfg.fft_size - 1; p.len_out = h->carry_len[h->cur ^ 1];
        }
        KWS_TRY(hip_done(kws::launch_stream_recycle(p, st), "launch stream_recycle"));
        if (!h->ragged) { h->ragged = true; h->n_carry = 0; h->cur ^= 1; }
        if (h->win2)      // a two-head manager: head 2's window of the same streams (two stores per recycled stream)
            KWS_TRY(hip_done(kws::launch_window_reset_masked(slots, h->B, h->win2->inc_head, h->win2->inc_count, st), "launch window_reset (window 2)"));
        return KWS_OK;
    });
}

int kws_stream_carry(kws_stream_handle h, float* samples, int32_t* lengths, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!samples || !lengths) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    KWS_TRY(stream_check(h, false));
    return with_model_held(h, stream, "kws_stream_carry", [&](hipStream_t st) -> int {
        const size_t B = (size_t)h->B, row = (size_t)(h->fe->cfg.fft_size - 1) * sizeof(float);
        if (h->ragged) {                       // already the layout handed out
            KWS_HIP(hipMemcpyAsync(samples, h->carry[h->cur], B * row, hipMemcpyDeviceToDevice, st));
            KWS_HIP(hipMemcpyAsync(lengths, h->carry_len[h->cur], B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        } else {                               // lock-step: rows of n_carry samples, one length for all
            if (h->n_carry > 0)
                KWS_HIP(hipMemcpy2DAsync(samples, row, h->carry[h->cur], (size_t)h->n_carry * sizeof(float), (size_t)h->n_carry * sizeof(float),
                                         B, hipMemcpyDeviceToDevice, st));
            KWS_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lengths), h->n_carry, B, st));
        }
        return KWS_OK;
    });
}

}  // extern "C"
