// C ABI of libkws_amd.so (include/kws_amd.h): the serving surface -- decode windows, PCM front-ends, stream managers.
#include <new>

#include "api_internal.h"

using namespace kws_host;

namespace {

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm=1) restated (the reference calls it at
// models/rnn_ctc.py:139-144; librosa itself is not available offline): Slaney mel scale -- linear below 1 kHz
// (200/3 Hz per mel), logarithmic above (step ln(6.4)/27) -- triangular filters, each scaled by 2/(f_hi - f_lo).
double hz_to_mel_slaney(double f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
double mel_to_hz_slaney(double m) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}
std::vector<float> slaney_mel_basis(int sr, int n_fft, int n_mels, double fmin, double fmax) {
    const int nf = n_fft / 2 + 1;
    std::vector<double> mel_f(n_mels + 2);
    const double m_lo = hz_to_mel_slaney(fmin), m_hi = hz_to_mel_slaney(fmax);
    for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz_slaney(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    std::vector<float> w((size_t)n_mels * nf, 0.f);
    for (int i = 0; i < n_mels; ++i) {
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int k = 0; k < nf; ++k) {
            const double fk = (double)sr / 2.0 * k / (nf - 1);
            const double lower = (fk - mel_f[i]) / (mel_f[i + 1] - mel_f[i]);
            const double upper = (mel_f[i + 2] - fk) / (mel_f[i + 2] - mel_f[i + 1]);
            const double v = std::max(0.0, std::min(lower, upper));
            w[(size_t)i * nf + k] = (float)(v * enorm);
        }
    }
    return w;
}

// dct(n_filters, n_input) of utils/mfcc.py:33-42, already transposed as :42 returns it and cast as :93 does: the orthonormal
// DCT-II basis [n_mel][n_mfcc] in float32
std::vector<float> dct_basis_f32(int n_mfcc, int n_mel) {
    const double pi = 3.14159265358979323846;
    std::vector<float> d((size_t)n_mel * n_mfcc);
    for (int j = 0; j < n_mel; ++j) {
        const double sample = (2 * j + 1) * pi / (2.0 * n_mel);
        d[(size_t)j * n_mfcc] = (float)(1.0 / std::sqrt((double)n_mel));
        for (int i = 1; i < n_mfcc; ++i) d[(size_t)j * n_mfcc + i] = (float)(std::cos(i * sample) * std::sqrt(2.0 / n_mel));
    }
    return d;
}

// The label matcher of the incremental window: KMP automaton over emitted words, delta[q * 16 + w] = digits of the label
// matched after reading word w (1..15) with q matched before (q < len); words the label does not contain lead to 0.
void window_label_delta(const char* label, int n, uint8_t* delta) {
    memset(delta, 0, 256);
    for (int q = 0; q < n; ++q)
        for (int w = 1; w < 16; ++w) {
            int k = q + 1;                       // longest k with label[0..k) a suffix of label[0..q) + w
            for (; k > 0; --k) {
                if (label[k - 1] - '0' != w) continue;
                bool ok = true;
                for (int i = 0; i < k - 1 && ok; ++i) ok = label[i] == label[q - (k - 1) + i];
                if (ok) break;
            }
            delta[q * 16 + w] = (uint8_t)k;
        }
}

// LDS of window_inc_kernel for chunks of T frames (launch_window_inc, stream_kernels.hip): the 16 streams' frame words, the label
// matcher, the rings.  kws_window_create only sizes the re-scanning kernel; the incremental entry points check this one.
size_t window_inc_lds_bytes(int T, int nq) {
    const int stride = (T + 15) & ~15;
    return (size_t)16 * (stride > 0 ? stride : 16) + 256 + kws::window_tail_scratch_bytes(nq);
}
constexpr size_t kWindowIncLdsMax = 160 * 1024;

// Binds `label` to the window's incremental state (the queued summaries are label-specific).  The first binding uploads the
// matcher (synchronises); the same label again is free; another label while chunks may be queued is refused.
int window_bind_label(kws_window* w, const char* label) {
    const int n = (int)strlen(label);
    if (n > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "the incremental window takes labels of up to 15 digits (its matcher has 16 states); "
                            "kws_window_step re-scans the frames for longer ones");
    for (int i = 0; i < n; ++i)
        if (label[i] < '1' || label[i] > '9') return fail(KWS_ERR_INVALID_ARGUMENT, "label must be digits 1..9, got '%s'", label);
    if (w->inc_bound) {
        if (strcmp(w->inc_label, label) == 0) return KWS_OK;
        return fail(KWS_ERR_INVALID_ARGUMENT, "the window's incremental state was built for label '%s'; it cannot continue with '%s' "
                    "(create another window, or use kws_window_step, which re-scans the frames)", w->inc_label, label);
    }
    window_label_delta(label, n, w->inc_delta);
    KWS_HIP(hipMemcpy(w->inc_delta_dev, w->inc_delta, 256, hipMemcpyHostToDevice));
    memcpy(w->inc_label, label, n + 1);
    w->inc_bound = true;
    return KWS_OK;
}

kws::WindowTail window_tail_params(kws_window* w, const uint8_t* clear_before, int32_t* hit, uint8_t* restart) {
    kws::WindowTail t;
    memset(&t, 0, sizeof(t));
    t.tab = w->inc_tab; t.meta = w->inc_meta; t.head = w->inc_head; t.count = w->inc_count; t.delta = w->inc_delta_dev;
    t.clear_before = clear_before; t.hit = hit; t.restart = restart; t.nq = w->nq; t.n_label = (int)strlen(w->inc_label);
    return t;
}

// the head of a stream-manager iteration that the FFT front-end can take along in its own launch (kws_stream_feed)
struct FrontGate {
    const int16_t* pcm_i16;        // int16 input read in place (chunk is then ignored), or null
    float vad_thres;
    const uint8_t* restart;
    uint8_t *silent, *reset;
    float* next;
    int n_next;
};
bool frontend_fuses_gate(kws_frontend_handle h, int B, int T) { return h->use_fft && T > 0 && (long long)B * T < (1LL << 31); }

int frontend_run_impl(kws_frontend_handle h, const float* carry, int n_carry, const float* chunk, int n_chunk, int B,
                             float* mel, void* stream, const FrontGate* gate = nullptr) {
    const int n_samples = n_carry + n_chunk;
    const int T = kws_frontend_frames(&h->cfg, n_samples);
    if (B == 0 || T == 0) return KWS_OK;
    if ((!chunk && !(gate && gate->pcm_i16)) || !mel || (n_carry > 0 && !carry)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if ((long long)B * T > (1LL << 36)) return fail(KWS_ERR_UNSUPPORTED, "B*T=%lld frames exceed the grid limit", (long long)B * T);
    kws::FrontendParams p = {};
    p.pcm = chunk; p.carry = n_carry > 0 ? carry : chunk; p.mel = mel;
    if (gate) {
        if (!frontend_fuses_gate(h, B, T)) return fail(KWS_ERR_UNSUPPORTED, "internal: the gate rides only on the FFT front-end");
        p.gate = 1; p.pcm_i16 = gate->pcm_i16; p.vad_thres = gate->vad_thres; p.restart = gate->restart;
        p.silent = gate->silent; p.reset = gate->reset; p.next = gate->next; p.n_next = gate->n_next;
        if (n_carry == 0) p.carry = gate->next;     // never dereferenced (n_carry == 0), only has to be a float pointer
    }
    p.dft = h->d_tables + h->dft_off; p.melw = h->d_tables + h->melw_off;
    p.n_samples = n_samples; p.n_carry = n_carry; p.T = T; p.fft = h->cfg.fft_size; p.hop = h->cfg.hop_size; p.n_mel = h->cfg.n_mel;
    p.nf_tiles = h->nf_tiles; p.mel_tiles = h->mel_tiles; p.kc4 = h->kc4; p.B = B;
    hipError_t e;
    if (h->use_fft && (long long)B * T < (1LL << 31)) {
        p.dft = h->d_tables + h->fft_tw_off; p.melw = h->d_tables + h->fft_mel_off;
        for (int m = 0; m < 4; ++m) { p.mel_lo[m] = h->mel_lo[m]; p.mel_cnt[m] = h->mel_cnt[m]; p.mel_off[m] = h->mel_off[m]; }
        e = kws::launch_mel_fft400(p, B, static_cast<hipStream_t>(stream));
    } else {
        e = kws::launch_mel_frontend(p, B, static_cast<hipStream_t>(stream));
    }
    if (e != hipSuccess) return hip_fail(e, "launch mel_frontend");
    return KWS_OK;
}

// one iteration with the model handle held and `st` ordered (kws_stream_feed below)
int stream_feed_locked(kws_stream_handle h, const void* pcm, int n, int pcm_int16, int32_t* hit, hipStream_t st) {
    const kws_frontend_config& fc = h->fe->cfg;
    const int fft = fc.fft_size, hop = fc.hop_size, B = h->B;
    const int total = h->n_carry + n;
    const float* chunk = pcm_int16 ? h->pcm_f32 : static_cast<const float*>(pcm);
    const float* carry = h->carry[h->cur];
    float* next = h->carry[h->cur ^ 1];
    // the GRU step of the chunk: the manager's state in place, reset where the gate found silence
    StepArgs step;
    step.state_in = h->state; step.state_out = h->state; step.reset_mask = h->reset;
    step.B = B; step.stream = st; step.locked = true;
    if (total < fft) {
        // Not a full frame yet.  The reference still runs the whole iteration on such a chunk (detector.py:168-209): vad ->
        // clean_state() + prob_queue.clear() when silent, the samples are carried (:179-183 keeps all of them), sess.run over
        // zero frames returns the state unchanged and an empty softmax, which takes a slot of the window (:195) before the
        // windowed decode (:197-201).
        hipError_t e = kws::launch_vad_gate(pcm, pcm_int16, B, n, h->vad_thres, h->pcm_f32, h->restart, h->silent, h->reset,
                                            h->n_carry ? carry : nullptr, h->n_carry, next, total, st);
        if (e != hipSuccess) return hip_fail(e, "launch vad_gate");
        int rc = step_impl(h->model, step);
        if (rc != KWS_OK) return rc;
        rc = kws_window_step_incremental(h->win, nullptr, 0, h->silent, h->label, hit, h->restart, st);
        if (rc != KWS_OK) return rc;
        h->n_carry = total; h->cur ^= 1;
        return KWS_OK;
    }
    const int keep = (total - fft) % hop + (fft - hop);                                  // detector.py:181-182
    const int T = kws_frontend_frames(&fc, total);
    step.mel = h->mel;
    step.T = T;
    int rc;
    if (frontend_fuses_gate(h->fe, B, T)) {
        // ONE launch: vad + masks and the next carry ride on the FFT front-end, which reads the PCM -- int16 as it is -- in place
        FrontGate gate = {pcm_int16 ? static_cast<const int16_t*>(pcm) : nullptr, h->vad_thres, h->restart, h->silent, h->reset, next, keep};
        rc = frontend_run_impl(h->fe, h->n_carry ? carry : nullptr, h->n_carry, pcm_int16 ? nullptr : chunk, n, B, h->mel, st, &gate);
        if (rc != KWS_OK) return rc;
    } else {
        // other frame lengths: one pass over the new chunk (int16 -> float, vad + masks, next carry), then the dense-DFT kernel
        hipError_t e = kws::launch_vad_gate(pcm, pcm_int16, B, n, h->vad_thres, h->pcm_f32, h->restart, h->silent, h->reset,
                                            h->n_carry ? carry : nullptr, h->n_carry, next, keep, st);
        if (e != hipSuccess) return hip_fail(e, "launch vad_gate");
        rc = kws_frontend_run_carry(h->fe, h->n_carry ? carry : nullptr, h->n_carry, chunk, n, B, h->mel, nullptr, 0, st);
        if (rc != KWS_OK) return rc;
    }
    rc = window_bind_label(h->win, h->label);          // (bound at kws_stream_create; refuses a window that went on with another label)
    if (rc != KWS_OK) return rc;
    if (step_takes_window(h->model, B, T, h->win->nq)) {
        // THREE launches per chunk (two for the bf16 stack): the decode-window step (prob_queue.add, ctc_decode2 over the
        // window, ctc_predict, clear + restart on a hit: detector.py:195-209) rides at the end of the last layer's launch, on
        // the frame words its flush has just produced -- no softmax round trip, no fourth launch.  The window's threshold
        // is the fused decoder's (ctc_decode2's frame rule, utils/prediction.py:74)
        const kws::WindowTail wt = window_tail_params(h->win, h->silent, hit, h->restart);
        step.decode2_thres = h->win->thres;
        step.wt = &wt;
        rc = step_impl(h->model, step);
        if (rc != KWS_OK) return rc;
    } else {
        step.softmax = h->softmax;
        rc = step_impl(h->model, step);
        if (rc != KWS_OK) return rc;
        rc = kws_window_step_incremental(h->win, h->softmax, T, h->silent, h->label, hit, h->restart, st);
        if (rc != KWS_OK) return rc;
    }
    h->n_carry = keep; h->cur ^= 1;
    return KWS_OK;
}

// One ragged iteration (kws_stream_feed_ragged; kws_stream_feed once the handle is ragged, lens == null: n_max for every stream),
// with the model handle held and `st` ordered.  Three or four launches whatever the lengths: the FFT front-end with the per-stream
// gate (vad, masks, next carry and its length, frame count, skip flag), the GRU layers over T = frames of n_max samples after a
// full carry with seq_len = the per-stream frame counts (copy-through past them; a skipped stream has reset 0 and 0 frames: its
// state comes back unchanged), and window_inc_kernel over each stream's own frames.  The window step cannot ride in the last GRU
// launch here: the tail instantiations take no lengths.
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
    kws::FrontendParams p = {};
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
    p.dft = h->fe->d_tables + h->fe->fft_tw_off; p.melw = h->fe->d_tables + h->fe->fft_mel_off;
    p.T = T; p.fft = fft; p.hop = fc.hop_size; p.n_mel = fc.n_mel;
    p.nf_tiles = h->fe->nf_tiles; p.mel_tiles = h->fe->mel_tiles; p.kc4 = h->fe->kc4; p.B = B;
    for (int m = 0; m < 4; ++m) { p.mel_lo[m] = h->fe->mel_lo[m]; p.mel_cnt[m] = h->fe->mel_cnt[m]; p.mel_off[m] = h->fe->mel_off[m]; }
    hipError_t e = kws::launch_mel_fft400(p, B, st);
    if (e != hipSuccess) return hip_fail(e, "launch mel_fft400 (ragged)");
    h->ragged = true; h->n_carry = 0; h->cur ^= 1;          // the samples and lengths are in the other buffer now
    StepArgs step;
    step.mel = h->mel; step.softmax = h->softmax;
    step.state_in = h->state; step.state_out = h->state; step.reset_mask = h->reset; step.seq_len = h->frames;
    step.B = B; step.T = T; step.stream = st; step.locked = true;
    int rc = step_impl(h->model, step);
    if (rc != KWS_OK) return rc;
    rc = window_bind_label(h->win, h->label);
    if (rc != KWS_OK) return rc;
    kws::WindowIncParams wp;
    memset(&wp, 0, sizeof(wp));
    wp.win = window_tail_params(h->win, h->silent, hit, h->restart);
    memcpy(wp.delta, h->win->inc_delta, 256);
    wp.softmax = h->softmax; wp.thres = h->win->thres; wp.B = B; wp.T = T; wp.C = h->win->C;
    wp.frames = h->frames; wp.skip = h->skip;
    e = kws::launch_window_inc(wp, st);
    if (e != hipSuccess) return hip_fail(e, "launch window_inc (ragged)");
    return KWS_OK;
}

// The checks every stream-handle call shares: the borrowed handles are alive; the per-stream paths need the FFT front-end.
int stream_check(kws_stream_handle h, bool ragged_call) {
    if (live_serial(h->model) != h->model_serial || live_serial(h->fe) != h->fe_serial || live_serial(h->win) != h->win_serial)
        return fail(KWS_ERR_INVALID_ARGUMENT, "the model, front-end or window this stream was created on has been destroyed");
    if (ragged_call && !(h->fe->use_fft && h->fe->cfg.fft_size == 400))
        return fail(KWS_ERR_UNSUPPORTED, "per-stream chunk lengths need the 400-point FFT front-end (fft_size=%d%s)", h->fe->cfg.fft_size,
                    h->fe->cfg.fft_size == 400 ? ", KWS_FRONTEND_DENSE=1" : "");
    if (ragged_call && (long long)h->B * h->tmax >= (1LL << 31))
        return fail(KWS_ERR_UNSUPPORTED, "B*T=%lld frames exceed the ragged front-end's grid", (long long)h->B * h->tmax);
    return KWS_OK;
}

// Runs `body` with the model handle held (its staging and seams are the handle's) and `stream` ordered behind the handle's
// previous call when that ran on another stream; the chunk's staging pointers are set for it.
template <typename F>
int with_model_held(kws_stream_handle h, hipStream_t st, const char* what, F&& body) {
    kws_model* model = h->model;
    BusyGuard busy(model->in_call);
    if (!busy.owned)
        return fail(KWS_ERR_BUSY, "%s: another host thread is inside a call on the model handle (one thread at a time per "
                    "handle; stream managers that run concurrently need a model handle each)", what);
    if (h->stage_bytes > model->stage.bytes) return fail(KWS_ERR_INVALID_ARGUMENT, "internal: the model handle's staging block is smaller than this stream's");
    int rc = call_enter(model, st);
    if (rc != KWS_OK) return rc;
    h->pcm_f32 = reinterpret_cast<float*>(model->stage.base + h->off_pcm_f32);
    h->mel = reinterpret_cast<float*>(model->stage.base + h->off_mel);
    h->softmax = reinterpret_cast<float*>(model->stage.base + h->off_softmax);
    h->silent = reinterpret_cast<uint8_t*>(model->stage.base + h->off_silent);
    h->reset = reinterpret_cast<uint8_t*>(model->stage.base + h->off_reset);
    h->frames = reinterpret_cast<int32_t*>(model->stage.base + h->off_frames);
    h->skip = reinterpret_cast<uint8_t*>(model->stage.base + h->off_skip);
    rc = body();
    const int rl = call_leave(model, st);
    return rc != KWS_OK ? rc : rl;
}

}  // namespace

extern "C" {

int kws_window_create(int B, int max_chunks, int max_frames, int C, float thres, kws_window_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (B < 1 || max_chunks < 1 || max_frames < 1 || C < 3 || C > 64)
        return fail(KWS_ERR_INVALID_ARGUMENT, "bad window shape B=%d chunks=%d frames=%d C=%d", B, max_chunks, max_frames, C);
    // window_step_kernel: one lane per queued chunk and two byte images of the window (ring, emitted words) in LDS
    if (max_chunks > 64)
        return fail(KWS_ERR_UNSUPPORTED, "max_chunks=%d unsupported (1..64; the reference uses SimpleQueue(15), detector.py:122)", max_chunks);
    if ((size_t)2 * max_chunks * ((max_frames + 15) & ~15) > 48 * 1024)
        return fail(KWS_ERR_UNSUPPORTED, "window of %d chunks x %d frames exceeds the 48 KiB of LDS the kernel stages it in", max_chunks, max_frames);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    kws_window* wnd = new (std::nothrow) kws_window();
    if (!wnd) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    wnd->B = B; wnd->nq = max_chunks; wnd->tmax = max_frames; wnd->tmax_pad = (max_frames + 15) & ~15; wnd->C = C;
    wnd->thres = thres;
    // the summaries of the incremental form (what kws_stream_feed drives: 32 + 4 bytes per queued chunk and stream); the frame
    // ring of the re-scanning kws_window_step (tmax_pad + 4 bytes per queued chunk) is allocated by its first call
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&wnd->inc_tab), (size_t)B * max_chunks * 32);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&wnd->inc_meta), (size_t)B * max_chunks * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&wnd->inc_head), (size_t)B * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&wnd->inc_count), (size_t)B * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&wnd->inc_delta_dev), 256);
    if (e == hipSuccess) e = hipMemset(wnd->inc_tab, 0, (size_t)B * max_chunks * 32);
    if (e == hipSuccess) e = hipMemset(wnd->inc_meta, 0, (size_t)B * max_chunks * sizeof(uint32_t));
    if (e == hipSuccess) e = kws::launch_window_reset(B, wnd->inc_head, wnd->inc_count, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { kws_window_destroy(wnd); return hip_fail(e, "kws_window_create"); }
    live_register(wnd);
    *out = wnd;
    return KWS_OK;
}

int kws_window_destroy(kws_window_handle h) {
    if (!h) return KWS_OK;
    live_unregister(h);
    hipDeviceSynchronize();
    for (void* q : {(void*)h->words, (void*)h->lens, (void*)h->head, (void*)h->count, (void*)h->inc_tab, (void*)h->inc_meta,
                    (void*)h->inc_head, (void*)h->inc_count, (void*)h->inc_delta_dev})
        if (q) hipFree(q);
    delete h;
    return KWS_OK;
}

int kws_window_step(kws_window_handle h, const float* softmax, int T, const uint8_t* clear_before, const char* label,
                    int32_t* hit, uint8_t* restart, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (T < 0 || T > h->tmax) return fail(KWS_ERR_INVALID_ARGUMENT, "T=%d outside [0,%d]", T, h->tmax);
    if (!hit || (!softmax && T > 0) || !label) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    const int n = (int)strlen(label);
    if (n > 16) return fail(KWS_ERR_INVALID_ARGUMENT, "label longer than 16 digits");
    kws::WindowParams p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < n; ++i) {
        if (label[i] < '1' || label[i] > '9') return fail(KWS_ERR_INVALID_ARGUMENT, "label must be digits 1..9, got '%s'", label);
        p.label[i] = label[i] - '0';
    }
    p.label_len = n;
    if (!h->words) {          // first re-scanning step of this window: its frame ring (synchronises once)
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->words), (size_t)h->B * h->nq * h->tmax_pad);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->lens), (size_t)h->B * h->nq * sizeof(int));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->head), (size_t)h->B * sizeof(int));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->count), (size_t)h->B * sizeof(int));
        if (e == hipSuccess) e = kws::launch_window_reset(h->B, h->head, h->count, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            for (void* q : {(void*)h->words, (void*)h->lens, (void*)h->head, (void*)h->count}) if (q) hipFree(q);
            h->words = nullptr; h->lens = nullptr; h->head = nullptr; h->count = nullptr;
            return hip_fail(e, "hipMalloc(window frame ring)");
        }
    }
    p.words = h->words; p.lens = h->lens; p.head = h->head; p.count = h->count;
    p.softmax = softmax; p.clear_before = clear_before; p.hit = hit; p.restart = restart;
    p.thres = h->thres; p.B = h->B; p.T = T; p.C = h->C; p.nq = h->nq; p.tmax = h->tmax_pad;
    hipError_t e = kws::launch_window_step(p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "launch window_step");
    return KWS_OK;
}

int kws_window_step_incremental(kws_window_handle h, const float* softmax, int T, const uint8_t* clear_before, const char* label,
                                int32_t* hit, uint8_t* restart, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (T < 0 || T > h->tmax) return fail(KWS_ERR_INVALID_ARGUMENT, "T=%d outside [0,%d]", T, h->tmax);
    if (!hit || (!softmax && T > 0) || !label) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (window_inc_lds_bytes(T, h->nq) > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "the incremental window step stages 16 streams x %d frame words and their %d-chunk rings in LDS: %zu bytes "
                    "exceed the %zu a workgroup may hold (shorter chunks, or kws_window_step, which re-scans the frames)", T, h->nq,
                    window_inc_lds_bytes(T, h->nq), kWindowIncLdsMax);
    const int rc = window_bind_label(h, label);
    if (rc != KWS_OK) return rc;
    kws::WindowIncParams p;
    memset(&p, 0, sizeof(p));
    p.win = window_tail_params(h, clear_before, hit, restart);
    memcpy(p.delta, h->inc_delta, 256);
    p.softmax = softmax; p.thres = h->thres; p.B = h->B; p.T = T; p.C = h->C;
    hipError_t e = kws::launch_window_inc(p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "launch window_inc");
    return KWS_OK;
}

int kws_frontend_frames(const kws_frontend_config* cfg, int n_samples) {
    if (!cfg || cfg->fft_size <= 0 || cfg->hop_size <= 0 || n_samples < cfg->fft_size) return 0;
    return 1 + (n_samples - cfg->fft_size) / cfg->hop_size;
}

int kws_frontend_create(const kws_frontend_config* cfg, kws_frontend_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    const kws_feature_config fc = {*cfg, KWS_FEAT_MEL, 1, 0};
    return kws_frontend_create_features(&fc, out);
}

size_t kws_sizeof_feature_config(void) { return sizeof(kws_feature_config); }

int kws_frontend_create_features(const kws_feature_config* fcfg, kws_frontend_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!fcfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    const kws_frontend_config* cfg = &fcfg->base;
    if (cfg->fft_size < 16 || cfg->fft_size > 496 || cfg->fft_size % 16 != 0)
        return fail(KWS_ERR_UNSUPPORTED, "fft_size=%d must be a multiple of 16 in [16,496] (the reference uses 400)", cfg->fft_size);
    if (cfg->hop_size < 1 || cfg->n_mel < 1 || cfg->n_mel > 64 || cfg->samplerate < 1)
        return fail(KWS_ERR_INVALID_ARGUMENT, "bad hop_size/n_mel/samplerate (%d/%d/%d)", cfg->hop_size, cfg->n_mel, cfg->samplerate);
    if (!(cfg->fmin >= 0.f) || !(cfg->fmax > cfg->fmin) || cfg->fmax > cfg->samplerate / 2.0f + 1e-3f)
        return fail(KWS_ERR_INVALID_ARGUMENT, "need 0 <= fmin < fmax <= sr/2");
    const bool mfcc = fcfg->kind == KWS_FEAT_MFCC;
    if (fcfg->kind != KWS_FEAT_MEL && !mfcc) return fail(KWS_ERR_INVALID_ARGUMENT, "kind=%d is neither KWS_FEAT_MEL nor KWS_FEAT_MFCC", fcfg->kind);
    if (!mfcc && fcfg->power != 1 && fcfg->power != 2) return fail(KWS_ERR_INVALID_ARGUMENT, "power=%d must be 1 (|X|) or 2 (|X|^2)", fcfg->power);
    if (mfcc && (fcfg->n_mfcc < 1 || fcfg->n_mfcc > std::min(cfg->n_mel, 32)))
        return fail(KWS_ERR_INVALID_ARGUMENT, "n_mfcc=%d outside 1..min(n_mel, 32) = %d", fcfg->n_mfcc, std::min(cfg->n_mel, 32));
    const char* dense_env = getenv("KWS_FRONTEND_DENSE");      // A/B switch: the dense-DFT kernel also handles 400
    const bool dense400 = dense_env && dense_env[0] == '1';
    if ((mfcc || fcfg->power == 2) && (cfg->fft_size != 400 || dense400))
        return fail(KWS_ERR_UNSUPPORTED, "%s needs the 400-point FFT front-end: fft_size=%d%s unsupported (the dense-DFT kernel produces "
                    "magnitude mel only)", mfcc ? "kind=KWS_FEAT_MFCC" : "power=2", cfg->fft_size, dense400 ? " with KWS_FRONTEND_DENSE=1" : "");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    kws_frontend* f = new (std::nothrow) kws_frontend();
    if (!f) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    f->cfg = *cfg;
    f->kind = fcfg->kind; f->power = mfcc ? 2 : fcfg->power; f->n_mfcc = mfcc ? fcfg->n_mfcc : 0;
    // frontend_kernels.hip: bins k = 0..N/4 are contracted, each over the even and the odd folded samples
    const int N = cfg->fft_size, NF = N / 2 + 1, NH = N / 2, NQ = N / 4, TILES = (NQ + 1 + 15) / 16, KC4 = TILES;
    f->kc4 = KC4;
    f->nf_tiles = TILES;
    f->mel_tiles = (cfg->n_mel + 15) / 16;
    f->basis = slaney_mel_basis(cfg->samplerate, N, cfg->n_mel, cfg->fmin, cfg->fmax);
    std::vector<float> host;
    f->dft_off = 0;
    host.resize((size_t)4 * TILES * KC4 * 64 * 4, 0.f);
    const double two_pi = 6.283185307179586476925286766559;
    for (int tile = 0; tile < TILES; ++tile)
        for (int a = 0; a < 4; ++a)                      // a = 2 * (cos|sin) + parity of n
            for (int k4 = 0; k4 < KC4; ++k4)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int g = lane >> 4, i = lane & 15, cs = a >> 1, par = a & 1;
                        const int bin = 16 * tile + i, m = 4 * (4 * k4 + e) + g, n = 2 * m + par;
                        float v = 0.f;
                        // cos rows use folded samples 0..N/2, sin rows 1..N/2-1 (sin vanishes at 0 and N/2)
                        if (bin <= NQ && n <= NH && !(cs == 1 && (n == 0 || n == NH))) {
                            const double ang = two_pi * (double)(((long long)bin * n) % N) / N;
                            v = (float)(cs == 0 ? std::cos(ang) : std::sin(ang));
                        }
                        host[((((size_t)(4 * tile + a) * KC4 + k4) * 64 + lane) * 4) + e] = v;
                    }
    // mel basis fragments, xl k map over k = 0..N/4: direct set basis[m][k], mirrored set basis[m][N/2 - k] (k < N/4)
    f->melw_off = host.size();
    host.resize(host.size() + (size_t)f->mel_tiles * TILES * 8 * 64, 0.f);
    for (int mt = 0; mt < f->mel_tiles; ++mt)
        for (int t = 0; t < TILES; ++t)
            for (int mir = 0; mir < 2; ++mir)
                for (int e = 0; e < 4; ++e)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int g = lane >> 4, i = lane & 15;
                        const int k = 16 * t + 4 * g + e, m = 16 * mt + i;
                        float v = 0.f;
                        if (m < cfg->n_mel) {
                            if (mir == 0 && k <= NQ) v = f->basis[(size_t)m * NF + k];
                            if (mir == 1 && k < NQ) v = f->basis[(size_t)m * NF + (NH - k)];
                        }
                        host[f->melw_off + ((((size_t)mt * TILES + t) * 2 + mir) * 4 + e) * 64 + lane] = v;
                    }
    if (N == 400) {
        // fft_frontend.hip: the 16 x 25 real FFT.  Twiddles W400^{n2 k1} as (cos, sin) [k1 = 1..12][n2 = 0..15].  Mel basis as MFMA
        // A fragments over 4-bin groups (k = g <-> bin 4 group + g): per tile of 16 filters only the contiguous run of groups that
        // carry a non-zero weight, padded to a multiple of four; bins > 200 are zero rows.
        f->fft_tw_off = host.size();                        // [6 pairs (k1 = 2i+1, 2i+2)][16 n2][cos, sin, cos, sin]
        host.resize(host.size() + 12 * 16 * 2, 0.f);
        for (int k1 = 1; k1 <= 12; ++k1)
            for (int n2 = 0; n2 < 16; ++n2) {
                const double ang = two_pi * (double)(n2 * k1) / 400.0;
                const size_t at = f->fft_tw_off + ((size_t)((k1 - 1) / 2) * 16 + n2) * 4 + 2 * ((k1 - 1) & 1);
                host[at + 0] = (float)std::cos(ang);
                host[at + 1] = (float)std::sin(ang);
            }
        f->fft_mel_off = host.size();
        int groups_total = 0;
        for (int mt = 0; mt < f->mel_tiles; ++mt) {
            int lo = 51, hi = -1;                       // 51 groups cover bins 0..203
            for (int grp = 0; grp < 51; ++grp)
                for (int b = 4 * grp; b < 4 * grp + 4 && b <= 200; ++b)
                    for (int m = 16 * mt; m < 16 * mt + 16 && m < cfg->n_mel; ++m)
                        if (f->basis[(size_t)m * NF + b] != 0.f) { lo = std::min(lo, grp); hi = std::max(hi, grp); }
            int cnt = hi >= lo ? hi - lo + 1 : 0;
            if (cnt == 0) lo = 0;
            cnt = (cnt + 3) & ~3;                       // the kernel works in fours: the extra groups carry zero weights and stay
            if (lo + cnt > 52) lo = 52 - cnt;           // inside the 52 groups (208 rows) of the spectrum block
            f->mel_lo[mt] = lo; f->mel_cnt[mt] = cnt; f->mel_off[mt] = groups_total;
            const int stored = std::max(cnt, 24);       // the kernel preloads 24 groups per tile unconditionally (kMelRegs): zero padded
            host.resize(host.size() + (size_t)stored * 64, 0.f);
            for (int e = 0; e < cnt; ++e)                 // [tile][e / 4][lane][e % 4]: four groups' fragments per 16-byte load
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, m = 16 * mt + (lane & 15), b = 4 * (lo + e) + g;
                    if (m < cfg->n_mel && b <= 200)
                        host[f->fft_mel_off + (((size_t)(groups_total + e) / 4 * 64) + lane) * 4 + (e & 3)] = f->basis[(size_t)m * NF + b];
                }
            groups_total += stored;
        }
        f->use_fft = !dense400;
        if (mfcc) {
            // D^T as the A operand of the DCT behind the mel MFMAs: the B operand is the mel tile's own C image, whose lane (g, f)
            // holds filters 16 tile + 4g + e, so k-chunk e carries filters {4g + e}.  [tile][coefficient tile][64 lanes][e];
            // rows of the padding filters >= n_mel stay zero (those lanes hold -100 dB)
            f->dct = dct_basis_f32(f->n_mfcc, cfg->n_mel);
            f->dct_tiles = (f->n_mfcc + 15) / 16;
            f->dct_off = host.size();
            host.resize(host.size() + (size_t)f->mel_tiles * f->dct_tiles * 64 * 4, 0.f);
            for (int mt = 0; mt < f->mel_tiles; ++mt)
                for (int ct = 0; ct < f->dct_tiles; ++ct)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int filt = 16 * mt + 4 * (lane >> 4) + e, c = 16 * ct + (lane & 15);
                            if (filt < cfg->n_mel && c < f->n_mfcc)
                                host[f->dct_off + (((size_t)mt * f->dct_tiles + ct) * 64 + lane) * 4 + e] = f->dct[(size_t)filt * f->n_mfcc + c];
                        }
        }
    }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&f->d_tables), host.size() * sizeof(float));
    if (e != hipSuccess) { delete f; return hip_fail(e, "hipMalloc(frontend tables)"); }
    e = hipMemcpy(f->d_tables, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { hipFree(f->d_tables); delete f; return hip_fail(e, "hipMemcpy(frontend tables)"); }
    live_register(f);
    *out = f;
    return KWS_OK;
}

int kws_frontend_destroy(kws_frontend_handle h) {
    if (!h) return KWS_OK;
    live_unregister(h);
    hipDeviceSynchronize();
    if (h->d_tables) hipFree(h->d_tables);
    delete h;
    return KWS_OK;
}

int kws_frontend_mel_basis(kws_frontend_handle h, float* basis_host) {
    if (!h || !basis_host) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument");
    memcpy(basis_host, h->basis.data(), h->basis.size() * sizeof(float));
    return KWS_OK;
}

int kws_frontend_run(kws_frontend_handle h, const float* pcm, int B, int n_samples, float* mel, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (B < 0 || n_samples < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative dimension");
    if (!h->plain()) return kws_frontend_run_lengths(h, pcm, nullptr, B, n_samples, mel, stream);
    return frontend_run_impl(h, nullptr, 0, pcm, n_samples, B, mel, stream);
}

int kws_frontend_feature_size(kws_frontend_handle h) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    return h->kind == KWS_FEAT_MFCC ? 3 * h->n_mfcc : h->cfg.n_mel;
}

int kws_frontend_dct_basis(kws_frontend_handle h, float* basis_host) {
    if (!h || !basis_host) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument");
    if (h->kind != KWS_FEAT_MFCC) return fail(KWS_ERR_INVALID_ARGUMENT, "the front-end has no DCT basis: its kind is KWS_FEAT_MEL");
    memcpy(basis_host, h->dct.data(), h->dct.size() * sizeof(float));
    return KWS_OK;
}

int kws_frontend_run_lengths(kws_frontend_handle h, const float* pcm, const int32_t* n_samples, int B, int n_max, float* out, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (B < 0 || n_max < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative dimension");
    const int T = kws_frontend_frames(&h->cfg, n_max);
    if (B == 0 || T == 0) return KWS_OK;
    if (!pcm || !out) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (!(h->use_fft && h->cfg.fft_size == 400)) {
        // (only a magnitude-mel handle gets here: the other kinds are refused at create)
        if (!n_samples) return frontend_run_impl(h, nullptr, 0, pcm, n_max, B, out, stream);
        return fail(KWS_ERR_UNSUPPORTED, "per-utterance n_samples need the 400-point FFT front-end (fft_size=%d%s)", h->cfg.fft_size,
                    h->cfg.fft_size == 400 ? ", KWS_FRONTEND_DENSE=1" : "");
    }
    if ((long long)B * T >= (1LL << 31)) return fail(KWS_ERR_UNSUPPORTED, "B*T_max=%lld frames exceed the grid limit", (long long)B * T);
    kws::FrontendParams p = {};
    p.pcm = pcm; p.carry = pcm; p.mel = out;
    p.dft = h->d_tables + h->fft_tw_off; p.melw = h->d_tables + h->fft_mel_off;
    p.n_samples = n_max; p.T = T; p.fft = h->cfg.fft_size; p.hop = h->cfg.hop_size; p.n_mel = h->cfg.n_mel;
    p.nf_tiles = h->nf_tiles; p.mel_tiles = h->mel_tiles; p.kc4 = h->kc4; p.B = B;
    for (int m = 0; m < 4; ++m) { p.mel_lo[m] = h->mel_lo[m]; p.mel_cnt[m] = h->mel_cnt[m]; p.mel_off[m] = h->mel_off[m]; }
    p.lens = n_samples; p.n_max = n_max;
    p.power = h->power; p.n_mfcc = h->n_mfcc; p.dct_tiles = h->dct_tiles; p.dct = h->n_mfcc ? h->d_tables + h->dct_off : nullptr;
    const hipError_t e = kws::launch_features_fft400(p, B, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "launch features_fft400");
    return KWS_OK;
}

int kws_frontend_run_carry(kws_frontend_handle h, const float* carry, int n_carry, const float* chunk, int n_chunk, int B,
                           float* mel, float* next_carry, int n_next, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!h->plain())
        return fail(KWS_ERR_UNSUPPORTED, "kws_frontend_run_carry streams magnitude mel only: this front-end has %s (MFCC deltas need the whole "
                    "utterance; use kws_frontend_run_lengths)", h->kind == KWS_FEAT_MFCC ? "kind=KWS_FEAT_MFCC" : "power=2");
    if (B < 0 || n_carry < 0 || n_chunk < 0 || n_next < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative dimension");
    if (n_next > n_carry + n_chunk) return fail(KWS_ERR_INVALID_ARGUMENT, "n_next=%d exceeds the %d available samples", n_next, n_carry + n_chunk);
    if (n_next > 0 && !next_carry) return fail(KWS_ERR_INVALID_ARGUMENT, "next_carry is null");
    if (B == 0) return KWS_OK;
    if (n_chunk > 0 && !chunk) return fail(KWS_ERR_INVALID_ARGUMENT, "chunk is null");
    if (n_carry > 0 && !carry) return fail(KWS_ERR_INVALID_ARGUMENT, "carry is null");
    if (n_carry + n_chunk >= h->cfg.fft_size) {
        if (!mel) return fail(KWS_ERR_INVALID_ARGUMENT, "mel is null");
        const int rc = frontend_run_impl(h, carry, n_carry, chunk, n_chunk, B, mel, stream);
        if (rc != KWS_OK) return rc;
    }
    if (n_next > 0) {
        hipError_t e = kws::launch_carry_tail(carry ? carry : chunk, n_carry, chunk ? chunk : carry, n_chunk, next_carry, n_next, B,
                                              static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return hip_fail(e, "launch carry_tail");
    }
    return KWS_OK;
}

int kws_stream_create(kws_handle model, kws_frontend_handle frontend, kws_window_handle window, int B, int max_chunk_samples,
                      float vad_thres, const char* label, float* state, uint8_t* restart, kws_stream_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!model || !frontend || !window || !state || !restart || !label) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument");
    const unsigned long long ms = live_serial(model), fs = live_serial(frontend), ws = live_serial(window);
    if (!ms || !fs || !ws) return fail(KWS_ERR_INVALID_ARGUMENT, "model, front-end or window handle is not alive (destroyed, or not a handle)");
    if (!frontend->plain())
        return fail(KWS_ERR_UNSUPPORTED, "kws_stream_create takes a magnitude-mel front-end only: this one has %s (the reference's streaming "
                    "detector has no MFCC branch)", frontend->kind == KWS_FEAT_MFCC ? "kind=KWS_FEAT_MFCC" : "power=2");
    if (B < 1 || max_chunk_samples < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "bad stream shape B=%d max_chunk_samples=%d", B, max_chunk_samples);
    const int n = (int)strlen(label);
    if (n > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "label longer than 15 digits (the incremental window's matcher has 16 states)");
    for (int i = 0; i < n; ++i)
        if (label[i] < '1' || label[i] > '9') return fail(KWS_ERR_INVALID_ARGUMENT, "label must be digits 1..9, got '%s'", label);
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
    if (window_inc_lds_bytes(tmax, window->nq) > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "chunks of up to %d frames with a %d-chunk window need %zu bytes of LDS in the incremental window step "
                    "(limit %zu): use shorter chunks", tmax, window->nq, window_inc_lds_bytes(tmax, window->nq), kWindowIncLdsMax);
    kws_stream* s = new (std::nothrow) kws_stream();
    if (!s) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    s->model_serial = ms; s->fe_serial = fs; s->win_serial = ws;
    s->model = model; s->fe = frontend; s->win = window; s->B = B; s->max_chunk = max_chunk_samples; s->tmax = tmax;
    s->vad_thres = vad_thres; s->state = state; s->restart = restart;
    memcpy(s->label, label, n);
    const size_t carry_bytes = (size_t)B * (fft - 1) * sizeof(float);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->carry[0]), carry_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->carry[1]), carry_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->carry_len[0]), (size_t)B * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->carry_len[1]), (size_t)B * sizeof(int32_t));
    if (e != hipSuccess) { kws_stream_destroy(s); return hip_fail(e, "hipMalloc(stream buffers)"); }
    // One chunk's intermediates come out of the model handle's staging block: sized here, so a feed never allocates.  The
    // widened copy of int16 PCM is read by the dense-DFT front-end only (the 400-point FFT reads int16 in place); with the
    // FFT front-end it is written just by the gate of a chunk that completes no frame (< fft samples in total).
    {
        auto take = [&](size_t bytes) { const size_t at = s->stage_bytes; s->stage_bytes += (bytes + 255) & ~size_t(255); return at; };
        const size_t tm = (size_t)(tmax > 0 ? tmax : 1);
        const bool fused_gate = frontend->use_fft && (long long)B * tm < (1LL << 31);        // frontend_fuses_gate for every chunk with a frame
        s->off_pcm_f32 = take((size_t)B * (fused_gate ? std::min(max_chunk_samples, fft - 1) : max_chunk_samples) * sizeof(float));
        s->off_mel = take((size_t)B * tm * model->cfg.n_mel * sizeof(float));
        s->off_softmax = take((size_t)B * tm * model->cfg.num_classes * sizeof(float));
        s->off_silent = take((size_t)B);
        s->off_reset = take((size_t)B);
        s->off_frames = take((size_t)B * sizeof(int32_t));
        s->off_skip = take((size_t)B);
    }
    int rc = KWS_OK;
    {
        BusyGuard busy(model->in_call);
        if (!busy.owned) rc = fail(KWS_ERR_BUSY, "kws_stream_create: another host thread is inside a call on the model handle");
        else if (s->stage_bytes > model->stage.bytes) {
            // grows only here; the old block may still be read by a feed in flight
            hipError_t es = hipDeviceSynchronize();
            if (es == hipSuccess && model->stage.base) { hipFree(model->stage.base); model->stage.base = nullptr; model->stage.bytes = 0; }
            if (es == hipSuccess) es = hipMalloc(reinterpret_cast<void**>(&model->stage.base), s->stage_bytes);
            if (es != hipSuccess) { model->stage.base = nullptr; rc = hip_fail(es, "hipMalloc(stream staging)"); }
            else { model->stage.bytes = s->stage_bytes; ++model->scratch_allocs; }
        }
    }
    if (rc == KWS_OK) rc = kws_reserve(model, B, tmax);            // the GRU step of a chunk never allocates afterwards
    if (rc == KWS_OK) rc = window_bind_label(window, s->label);      // the window's summaries are built for this label
    if (rc != KWS_OK) { kws_stream_destroy(s); return rc; }
    *out = s;
    return KWS_OK;
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
    int rc = stream_check(h, false);
    if (rc != KWS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) {            // detector.py:164-166: an empty read is skipped before anything else happens
        KWS_HIP(hipMemsetAsync(hit, 0, (size_t)h->B * sizeof(int32_t), st));
        return KWS_OK;
    }
    // a handle in the per-stream carry layout runs the ragged iteration with every stream's length n
    if (h->ragged) return with_model_held(h, st, "kws_stream_feed", [&] { return stream_feed_ragged_locked(h, pcm, n, nullptr, pcm_int16, hit, st); });
    return with_model_held(h, st, "kws_stream_feed", [&] { return stream_feed_locked(h, pcm, n, pcm_int16, hit, st); });
}

int kws_stream_feed_ragged(kws_stream_handle h, const void* pcm, int n_max, const int32_t* n_per_stream, int pcm_int16, int32_t* hit,
                           void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (n_max < 0 || n_max > h->max_chunk) return fail(KWS_ERR_INVALID_ARGUMENT, "rows of %d samples outside [0,%d]", n_max, h->max_chunk);
    if (!hit || !n_per_stream || (!pcm && n_max > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    int rc = stream_check(h, true);
    if (rc != KWS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_model_held(h, st, "kws_stream_feed_ragged", [&] { return stream_feed_ragged_locked(h, pcm, n_max, n_per_stream, pcm_int16, hit, st); });
}

int kws_stream_recycle(kws_stream_handle h, const uint8_t* slots, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!slots) return fail(KWS_ERR_INVALID_ARGUMENT, "slots is null");
    int rc = stream_check(h, true);
    if (rc != KWS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_model_held(h, st, "kws_stream_recycle", [&]() -> int {
        const kws_config& c = h->model->cfg;
        kws::StreamRecycleParams p;
        memset(&p, 0, sizeof(p));
        p.slots = slots; p.state = h->state; p.restart = h->restart; p.head = h->win->inc_head; p.count = h->win->inc_count;
        p.L = c.num_layers; p.B = h->B; p.H = c.hidden;
        if (h->ragged) {
            p.len_out = h->carry_len[h->cur];                     // in place: only the recycled streams' lengths change
        } else {
            // leaves the lock-step layout: the other streams' carries move to rows of fft - 1 samples with their length
            p.carry_in = h->carry[h->cur]; p.n_carry = h->n_carry;
            p.carry_out = h->carry[h->cur ^ 1]; p.carry_out_stride = h->fe->cfg.fft_size - 1; p.len_out = h->carry_len[h->cur ^ 1];
        }
        hipError_t e = kws::launch_stream_recycle(p, st);
        if (e != hipSuccess) return hip_fail(e, "launch stream_recycle");
        if (!h->ragged) { h->ragged = true; h->n_carry = 0; h->cur ^= 1; }
        return KWS_OK;
    });
}

int kws_stream_carry(kws_stream_handle h, float* samples, int32_t* lengths, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!samples || !lengths) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    int rc = stream_check(h, false);
    if (rc != KWS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_model_held(h, st, "kws_stream_carry", [&]() -> int {
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
