// C ABI of libkws_amd.so (include/kws_amd.h): the standalone ops -- CTC decode / predict, vad, OctbitMatMul and its quantiser.
#include <memory>
#include <mutex>
#include <unordered_map>

#include "api_internal.h"

using namespace kws_host;

namespace {

// kws_octbit_matmul's activation-range workspace, one per (device, stream) that has called it (never freed: a few KB each)
struct OctbitWorkspace { std::mutex mutex; float* p = nullptr; size_t floats = 0; };
struct PairHash { size_t operator()(const std::pair<int, const void*>& k) const { return std::hash<const void*>()(k.second) * 31u + (size_t)k.first; } };
std::mutex g_octbit_ws_mutex;
std::unordered_map<std::pair<int, const void*>, std::unique_ptr<OctbitWorkspace>, PairHash> g_octbit_ws;

}  // namespace

extern "C" {

int kws_ctc_decode(int kind, const float* softmax, const int32_t* lengths, int B, int T, int C, int lockout,
                   float thres, float loose_thres, int32_t* words, int32_t* counts, int max_words, void* stream) {
    if (kind != KWS_DECODE && kind != KWS_DECODE2 && kind != KWS_DECODE_STRICT)
        return fail(KWS_ERR_INVALID_ARGUMENT, "unknown decode kind %d", kind);
    if (B < 0 || T < 0 || max_words < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative dimension");
    if (C < 3 || C > 64) return fail(KWS_ERR_INVALID_ARGUMENT, "classnum=%d out of range [3,64]", C);
    if (kind == KWS_DECODE && C < 5) return fail(KWS_ERR_INVALID_ARGUMENT, "ctc_decode slices columns 1:5 and needs classnum >= 5, got %d", C);
    if (lockout < 1 && kind != KWS_DECODE2) return fail(KWS_ERR_INVALID_ARGUMENT, "lockout must be >= 1, got %d", lockout);
    if (B == 0) return KWS_OK;
    if (!counts || (!words && max_words > 0) || (!softmax && T > 0))
        return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    hipError_t e = kws::launch_ctc_decode(kind, softmax, lengths, B, T, C, lockout, thres, loose_thres, words,
                                          counts, max_words, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "launch ctc_decode");
    return KWS_OK;
}

int kws_ctc_predict(const int32_t* words, const int32_t* counts, int B, int max_words, const char* label,
                    int32_t* hit, void* stream) {
    if (!label) return fail(KWS_ERR_INVALID_ARGUMENT, "label is null");
    const int n = (int)strlen(label);
    if (n > 16) return fail(KWS_ERR_INVALID_ARGUMENT, "label longer than 16 digits");
    int32_t digits[16] = {0};
    KWS_TRY(label_digits(label, n, digits));
    if (B < 0 || max_words < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative dimension");
    if (B == 0) return KWS_OK;
    if (!counts || !hit || (!words && max_words > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // digits travel by value inside the launcher (kernel argument), no device allocation
    hipError_t e = kws::launch_ctc_predict(words, counts, B, max_words, digits, n, hit, st);
    if (e != hipSuccess) return hip_fail(e, "launch ctc_predict");
    return KWS_OK;
}

int kws_vad(const float* pcm, int B, int N, float thres, uint8_t* speech, float* abs_sum, void* stream) {
    if (B < 0 || N < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative dimension");
    if (B == 0) return KWS_OK;
    if (!speech || (!pcm && N > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    hipError_t e = kws::launch_vad(pcm, B, N, thres, speech, abs_sum, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "launch vad");
    return KWS_OK;
}

int kws_octbit_matmul(const float* x, const int8_t* Wq, float scale_w, const float* bias, float* out, int A,
                      int K, int N, int per_row_scale, void* stream) {
    // preconditions of octbit/octbit_mat_mul_op.cc:41-46,61-73 as error codes
    if (!(scale_w > 0.f)) return fail(KWS_ERR_INVALID_ARGUMENT, "scale has to be positive");
    if (A < 0 || K < 0 || N < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative dimension");
    if (K % 64 != 0) return fail(KWS_ERR_INVALID_ARGUMENT, "K=%d must be a multiple of 64", K);
    if (A == 0 || N == 0) return KWS_OK;
    if (K == 0) return fail(KWS_ERR_INVALID_ARGUMENT, "K must be positive");
    if (!x || !Wq || !bias || !out) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The 2A+2 floats of activation ranges come from a block cached per (device, stream): the reference's Compute allocates its
    // temporaries per call (octbit_mat_mul_op.cc:49, re-entrant); here a call neither allocates nor frees once its stream has
    // seen a call of this size.  Calls on one stream are ordered by the stream; two host threads that share a stream are
    // serialised on the block's own mutex for the duration of the two launches.
    int dev = 0;
    KWS_HIP(hipGetDevice(&dev));
    OctbitWorkspace* w = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_octbit_ws_mutex);
        std::unique_ptr<OctbitWorkspace>& slot = g_octbit_ws[std::make_pair(dev, (const void*)st)];
        if (!slot) slot.reset(new OctbitWorkspace());
        w = slot.get();
    }
    std::lock_guard<std::mutex> use(w->mutex);
    const size_t need = (size_t)(2 * A + 2);
    if (need > w->floats) {
        // stream-ordered: the old block is released behind the launches that still read it
        float* grown = nullptr;
        KWS_HIP(hipMallocAsync(reinterpret_cast<void**>(&grown), need * sizeof(float), st));
        if (w->p) (void)hipFreeAsync(w->p, st);
        w->p = grown;
        w->floats = need;
    }
    hipError_t e = kws::launch_octbit_matmul(x, Wq, scale_w, bias, out, A, K, N, per_row_scale, w->p, st);
    if (e != hipSuccess) return hip_fail(e, "launch octbit_matmul");
    return KWS_OK;
}

int kws_octbit_quantize(const float* W, int K, int N, int8_t* Wq, float* scale, float* bias) {
    if (!W || !Wq || !scale || !bias) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (K <= 0 || N <= 0) return fail(KWS_ERR_INVALID_ARGUMENT, "K and N must be positive");
    // octbit/octbit_graph.py:196-204: scale = max|W|/127 in double, np.round = half-to-even
    float mx = W[0], mn = W[0];
    for (size_t i = 0; i < (size_t)K * N; ++i) { mx = std::max(mx, W[i]); mn = std::min(mn, W[i]); }
    const double nmax = std::max(std::fabs((double)mx), std::fabs((double)mn));
    if (!(nmax > 0.0)) return fail(KWS_ERR_INVALID_ARGUMENT, "weight matrix is all zero: scale would be 0");
    // numpy: float32 array / python float -> float32 array divided by a float32-cast scalar
    const float sc32 = (float)(nmax / 127.0);
    for (int j = 0; j < N; ++j) bias[j] = 0.f;
    std::vector<double> b(N, 0.0);
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < N; ++j) {
            const float qf = std::nearbyintf(W[(size_t)i * N + j] / sc32);
            Wq[(size_t)j * K + i] = (int8_t)qf;
            b[j] += (double)qf * 127.0;
        }
    for (int j = 0; j < N; ++j) bias[j] = (float)b[j];
    *scale = (float)(nmax / 127.0);
    return KWS_OK;
}

}  // extern "C"
