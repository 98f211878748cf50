// C ABI of libkws_amd.so (include/kws_amd.h): the decode window, re-scanning (kws_window_step) and incremental.
#include <new>

#include "api_internal.h"

using namespace kws_host;

namespace kws_host {

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

int label_digits(const char* label, int n, int32_t* digits) {
    for (int i = 0; i < n; ++i) {
        if (label[i] < '1' || label[i] > '9') return fail(KWS_ERR_INVALID_ARGUMENT, "label must be digits 1..9, got '%s'", label);
        if (digits) digits[i] = label[i] - '0';
    }
    return KWS_OK;
}

// LDS of window_inc_kernel for chunks of T frames (launch_window_inc, stream_kernels.hip): the 16 streams' frame words, the label
// matcher, the rings.  kws_window_create only sizes the re-scanning kernel; the incremental entry points check this one.
size_t window_inc_lds_bytes(int T, int nq) {
    const int stride = (T + 15) & ~15;
    return (size_t)16 * (stride > 0 ? stride : 16) + 256 + kws::window_tail_scratch_bytes(nq);
}

// The first binding uploads the matcher (synchronises); the same label again is free; another while chunks may be queued is refused.
int window_bind_label(kws_window* w, const char* label) {
    const int n = (int)strlen(label);
    if (n > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "the incremental window takes labels of up to 15 digits (its matcher has 16 states); "
                            "kws_window_step re-scans the frames for longer ones");
    KWS_TRY(label_digits(label, n, nullptr));
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
    kws::WindowTail t = {};
    t.tab = w->inc_tab; t.meta = w->inc_meta; t.head = w->inc_head; t.count = w->inc_count; t.delta = w->inc_delta_dev;
    t.clear_before = clear_before; t.hit = hit; t.restart = restart; t.nq = w->nq; t.n_label = (int)strlen(w->inc_label);
    return t;
}

}  // namespace kws_host

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
    kws::WindowParams p = {};
    KWS_TRY(label_digits(label, n, p.label));
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
    return hip_done(kws::launch_window_step(p, static_cast<hipStream_t>(stream)), "launch window_step");
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
    KWS_TRY(window_bind_label(h, label));
    kws::WindowIncParams p = {};
    p.win = window_tail_params(h, clear_before, hit, restart);
    memcpy(p.delta, h->inc_delta, 256);
    p.softmax = softmax; p.thres = h->thres; p.B = h->B; p.T = T; p.C = h->C;
    return hip_done(kws::launch_window_inc(p, static_cast<hipStream_t>(stream)), "launch window_inc");
}

}  // extern "C"
