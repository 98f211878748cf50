// kws_selftest: the library's own known answers, run through kws_step on temporary handles.

#include "api_internal.h"

using namespace kws_host;

// The kernels depend on things the compiler does not check: hand-placed wait states around inline-asm MFMAs (gru_device.h),
// an internal LLVM option for gru_bf16.hip (csrc/Makefile).  A build by another ROCm can therefore be silently wrong; the
// GPU test-suite catches that, a deployment has no test-suite.  So the library carries its own known answers: a plain
// double-precision host loop of the cell (below; the published TF-1.x GRUCell, models/rnn_ctc.py:179-185,228-243) and
// TensorFlow's own unit-test constants for it (rnn_cell_test.py testGRUCell / testMultiRNNCell: all kernels 0.5, gate bias
// 1, candidate bias 0, x = 1, h = 0.1 -> 0.175991, 0.156736 for three inputs, 0.13248 from the second stacked cell).
namespace {

thread_local bool g_in_selftest = false;

// (mel [B,T,I], state [L,B,H]) -> (logits [B,T,C], state'), blob layout of kws_weights_nbytes_wrapped; double throughout.
// With the cell wrappers each layer is ResidualWrapper(LayerNormalizer(GRUCell)) (models/rnn_ctc.py:186-197): the input
// normalised over its features (mean, population variance, eps 1e-5; scale ibeta, shift igamma: custom_wrapper.py:126-158) before
// the cell, and on layers >= 1 the output 0.7071 (h' + x) with x the raw input (:112-116), the state h'.
// seq_len: frames t >= seq_len[b] keep the state and project the zero row (dynamic_rnn).  top: the rows the dense layer reads,
// [B,T,H].  C2 > 0: the second head (Wfc2 [H,C2], bfc2 [C2] behind the blob, kws_weights_nbytes_heads) on the same rows -> logits2.
void host_forward(const kws_config& c, const kws_cell_wrappers& wr, const float* blob, const float* mel, const float* st0, int B, int T,
                  std::vector<double>& logits, std::vector<double>& state, const int32_t* seq_len = nullptr, std::vector<double>* top = nullptr,
                  int C2 = 0, std::vector<double>* logits2 = nullptr) {
    const int H = c.hidden, L = c.num_layers, C = c.num_classes;
    const BlobLayout bl = blob_layout(c);
    const WrapLayout wl = wrap_layout(c, wr);
    state.assign(st0, st0 + (size_t)L * B * H);
    logits.assign((size_t)B * T * C, 0.0);
    if (top) top->assign((size_t)B * T * H, 0.0);
    if (logits2) logits2->assign((size_t)B * T * C2, 0.0);
    std::vector<double> x, g(2 * H), cand(H), hn(H);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            x.assign(mel + ((size_t)b * T + t) * c.n_mel, mel + ((size_t)b * T + t + 1) * c.n_mel);
            const bool live = !seq_len || t < seq_len[b];
            if (!live) x.assign(H, 0.0);
            for (int l = 0; l < L && live; ++l) {
                const int I = bl.layer[l].in;
                const std::vector<double> x_raw = x;
                if (wr.use_layer_norm) {
                    double mu = 0.0, var = 0.0;
                    for (int k = 0; k < I; ++k) mu += x[k];
                    mu /= I;
                    for (int k = 0; k < I; ++k) var += (x[k] - mu) * (x[k] - mu);
                    var /= I;
                    const double scale = blob[wl.ibeta[l]] / std::sqrt(var + 1e-5);
                    for (int k = 0; k < I; ++k) x[k] = (x[k] - mu) * scale + blob[wl.igamma[l] + k];
                }
                const float *Wg = blob + bl.layer[l].wg, *bg = blob + bl.layer[l].bg, *Wc = blob + bl.layer[l].wc, *bc = blob + bl.layer[l].bc;
                double* h = &state[((size_t)l * B + b) * H];
                for (int j = 0; j < 2 * H; ++j) {
                    double a = bg[j];
                    for (int k = 0; k < I; ++k) a += x[k] * Wg[(size_t)k * 2 * H + j];
                    for (int k = 0; k < H; ++k) a += h[k] * Wg[(size_t)(I + k) * 2 * H + j];
                    g[j] = 1.0 / (1.0 + std::exp(-a));                          // [r | u]
                }
                for (int j = 0; j < H; ++j) {
                    double a = bc[j];
                    for (int k = 0; k < I; ++k) a += x[k] * Wc[(size_t)k * H + j];
                    for (int k = 0; k < H; ++k) a += g[k] * h[k] * Wc[(size_t)(I + k) * H + j];   // r (.) h before the matmul
                    cand[j] = std::tanh(a);
                }
                for (int j = 0; j < H; ++j) hn[j] = g[H + j] * h[j] + (1.0 - g[H + j]) * cand[j];
                std::copy(hn.begin(), hn.end(), h);
                x = hn;
                if (wr.use_residual && l > 0)
                    for (int j = 0; j < H; ++j) x[j] = 0.7071067811865475 * (hn[j] + x_raw[j]);
            }
            const float *Wfc = blob + bl.wfc, *bfc = blob + bl.bfc;
            for (int k = 0; k < C; ++k) {
                double a = bfc[k];
                for (int j = 0; j < H; ++j) a += x[j] * Wfc[(size_t)j * C + k];
                if (c.use_relu) { a = std::max(a, 0.0); if (c.value_clip > 0) a = std::min(a, 20.0); }
                logits[((size_t)b * T + t) * C + k] = a;
            }
            if (top) std::copy(x.begin(), x.end(), top->begin() + ((size_t)b * T + t) * H);
            const float *Wfc2 = blob + wl.total, *bfc2 = Wfc2 + (size_t)H * C2;
            for (int k = 0; k < C2 && logits2; ++k) {
                double a = bfc2[k];
                for (int j = 0; j < H; ++j) a += x[j] * Wfc2[(size_t)j * C2 + k];
                if (c.use_relu) { a = std::max(a, 0.0); if (c.value_clip > 0) a = std::min(a, 20.0); }
                (*logits2)[((size_t)b * T + t) * C2 + k] = a;
            }
        }
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 4); }
};

// one case through kws_step on a temporary handle; *err_state / *err_logit = max abs deviation from the host loop
int selftest_case(const kws_config& cfg, const kws_cell_wrappers& wr, int kernel_kind, const std::vector<float>& blob,
                  const std::vector<float>& mel, const std::vector<float>& st0, int B, int T, double* err_logit, double* err_state,
                  std::vector<float>* state_out, std::string* kernels) {
    const int H = cfg.hidden, L = cfg.num_layers, C = cfg.num_classes;
    kws_handle m = nullptr;
    int rc = kws_create_wrapped(&cfg, &wr, blob.data(), blob.size() * sizeof(float), &m);
    if (rc != KWS_OK) return rc;
    rc = kws_set_kernel(m, kernel_kind);
    DevBuf d_mel, d_st, d_lg;
    std::vector<float> lg((size_t)B * T * C), st((size_t)L * B * H);
    auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == KWS_OK) rc = hip_fail(e, what); };
    if (rc == KWS_OK) {
        hip(d_mel.alloc(mel.size() * 4), "selftest hipMalloc");
        hip(d_st.alloc(st.size() * 4), "selftest hipMalloc");
        hip(d_lg.alloc(lg.size() * 4), "selftest hipMalloc");
    }
    if (rc == KWS_OK) {
        hip(hipMemcpy(d_mel.p, mel.data(), mel.size() * 4, hipMemcpyHostToDevice), "selftest upload");
        hip(hipMemcpy(d_st.p, st0.data(), st0.size() * 4, hipMemcpyHostToDevice), "selftest upload");
        hip(hipDeviceSynchronize(), "selftest sync");
    }
    if (rc == KWS_OK)
        rc = kws_step(m, static_cast<const float*>(d_mel.p), static_cast<const float*>(d_st.p), static_cast<float*>(d_lg.p), nullptr,
                      static_cast<float*>(d_st.p), nullptr, nullptr, nullptr, nullptr, 0.4f, B, T, nullptr);
    if (rc == KWS_OK) {
        hip(hipDeviceSynchronize(), "selftest kernels");
        hip(hipMemcpy(lg.data(), d_lg.p, lg.size() * 4, hipMemcpyDeviceToHost), "selftest download");
        hip(hipMemcpy(st.data(), d_st.p, st.size() * 4, hipMemcpyDeviceToHost), "selftest download");
    }
    if (rc == KWS_OK) rc = kws_poll_error(m);
    if (rc == KWS_OK && kernels) {
        kernels->clear();
        for (int l = 0; l < L; ++l)
            if (m->launch_tag[l].family != kws_model::kNone) *kernels += (kernels->empty() ? "" : " + ") + m->launch_name(l);
    }
    const std::string keep = g_last_error;
    kws_destroy(m);
    if (rc != KWS_OK) { g_last_error = keep; return rc; }
    std::vector<double> want_l, want_s;
    host_forward(cfg, wr, blob.data(), mel.data(), st0.data(), B, T, want_l, want_s);
    double el = 0.0, es = 0.0;
    for (size_t i = 0; i < lg.size(); ++i) { const double d = std::fabs(lg[i] - want_l[i]); el = (d > el || d != d) ? d : el; }
    for (size_t i = 0; i < st.size(); ++i) { const double d = std::fabs(st[i] - want_s[i]); es = (d > es || d != d) ? d : es; }
    *err_logit = el; *err_state = es;
    if (state_out) *state_out = st;
    return KWS_OK;
}

// the same case through kws_step_heads on a temporary heads handle (blob: with the second head behind it), stream 1 with a short
// seq_len: max abs deviation of both heads' logits, of nn_outputs and of the state from the host loop
int selftest_heads_case(const kws_config& cfg, int C2, int kernel_kind, const std::vector<float>& blob, const std::vector<float>& mel,
                        const std::vector<float>& st0, int B, int T, double* err_logit, double* err_rows, double* err_state, std::string* kernels) {
    const int H = cfg.hidden, L = cfg.num_layers, C = cfg.num_classes;
    std::vector<int32_t> len(B, T);
    len[1] = T / 2;
    kws_handle m = nullptr;
    int rc = kws_create_heads(&cfg, C2, blob.data(), blob.size() * sizeof(float), &m);
    if (rc != KWS_OK) return rc;
    rc = kws_set_kernel(m, kernel_kind);
    DevBuf d_mel, d_st, d_len, d_l1, d_l2, d_nn;
    std::vector<float> l1((size_t)B * T * C), l2((size_t)B * T * C2), nn((size_t)B * T * H), st((size_t)L * B * H);
    auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == KWS_OK) rc = hip_fail(e, what); };
    if (rc == KWS_OK) {
        hip(d_mel.alloc(mel.size() * 4), "selftest hipMalloc");
        hip(d_st.alloc(st.size() * 4), "selftest hipMalloc");
        hip(d_len.alloc(len.size() * 4), "selftest hipMalloc");
        hip(d_l1.alloc(l1.size() * 4), "selftest hipMalloc");
        hip(d_l2.alloc(l2.size() * 4), "selftest hipMalloc");
        hip(d_nn.alloc(nn.size() * 4), "selftest hipMalloc");
    }
    if (rc == KWS_OK) {
        hip(hipMemcpy(d_mel.p, mel.data(), mel.size() * 4, hipMemcpyHostToDevice), "selftest upload");
        hip(hipMemcpy(d_st.p, st0.data(), st0.size() * 4, hipMemcpyHostToDevice), "selftest upload");
        hip(hipMemcpy(d_len.p, len.data(), len.size() * 4, hipMemcpyHostToDevice), "selftest upload");
        hip(hipDeviceSynchronize(), "selftest sync");
    }
    if (rc == KWS_OK) {
        const kws_head_io h1 = {static_cast<float*>(d_l1.p), nullptr, nullptr, nullptr, 0.4f};
        const kws_head_io h2 = {static_cast<float*>(d_l2.p), nullptr, nullptr, nullptr, 0.4f};
        rc = kws_step_heads(m, static_cast<const float*>(d_mel.p), static_cast<const float*>(d_st.p), static_cast<float*>(d_st.p),
                            static_cast<const int32_t*>(d_len.p), nullptr, static_cast<float*>(d_nn.p), &h1, &h2, B, T, nullptr);
    }
    if (rc == KWS_OK) {
        hip(hipDeviceSynchronize(), "selftest kernels");
        hip(hipMemcpy(l1.data(), d_l1.p, l1.size() * 4, hipMemcpyDeviceToHost), "selftest download");
        hip(hipMemcpy(l2.data(), d_l2.p, l2.size() * 4, hipMemcpyDeviceToHost), "selftest download");
        hip(hipMemcpy(nn.data(), d_nn.p, nn.size() * 4, hipMemcpyDeviceToHost), "selftest download");
        hip(hipMemcpy(st.data(), d_st.p, st.size() * 4, hipMemcpyDeviceToHost), "selftest download");
    }
    if (rc == KWS_OK && kernels) {
        kernels->clear();
        for (int l = 0; l < L; ++l)
            if (m->launch_tag[l].family != kws_model::kNone) *kernels += (kernels->empty() ? "" : " + ") + m->launch_name(l);
    }
    const std::string keep = g_last_error;
    kws_destroy(m);
    if (rc != KWS_OK) { g_last_error = keep; return rc; }
    std::vector<double> want_1, want_2, want_rows, want_s;
    host_forward(cfg, kws_cell_wrappers{0, 0}, blob.data(), mel.data(), st0.data(), B, T, want_1, want_s, len.data(), &want_rows, C2, &want_2);
    auto worst = [](const std::vector<float>& got, const std::vector<double>& want, double e) {
        for (size_t i = 0; i < got.size(); ++i) { const double d = std::fabs(got[i] - want[i]); e = (d > e || d != d) ? d : e; }
        return e;
    };
    *err_logit = worst(l2, want_2, worst(l1, want_1, 0.0));
    *err_rows = worst(nn, want_rows, 0.0);
    *err_state = worst(st, want_s, 0.0);
    return KWS_OK;
}

// deterministic pseudo-random floats in [-1, 1) (no <random>: identical on every libstdc++)
struct Lcg {
    uint64_t s;
    float next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (float)((double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0); }
};

}  // namespace

bool kws_host::in_selftest() { return g_in_selftest; }

extern "C" int kws_selftest(kws_handle h) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (g_in_selftest) return KWS_OK;
    struct Guard { Guard() { g_in_selftest = true; } ~Guard() { g_in_selftest = false; } } guard;
    const kws_config cfg = h->cfg;
    const kws_cell_wrappers wr = h->wrap;
    const kws_cell_wrappers plain = {0, 0};
    const int H = cfg.hidden, L = cfg.num_layers, C = cfg.num_classes, I0 = cfg.n_mel;
    const BlobLayout bl = blob_layout(cfg);
    const WrapLayout wl = wrap_layout(cfg, wr);
    // tolerances: what the arithmetic of each precision leaves on these two cases (fp32: observed <= 4e-6 / 1e-7)
    double tol_rand_logit, tol_rand_state, tol_kat;
    switch (cfg.precision) {
        case KWS_BF16: tol_rand_logit = 6e-2; tol_rand_state = 2e-2; tol_kat = 2e-3; break;
        case KWS_INT8: tol_rand_logit = -1.0; tol_rand_state = -1.0; tol_kat = 2e-2; break;   // int8: known answers only
        default:       tol_rand_logit = 5e-5; tol_rand_state = 2e-5; tol_kat = 1e-6; break;   // fp32 and the f16x3 split
    }
    std::vector<int> kinds;
    if (cfg.precision == KWS_FP32) {
        bool res_ok = true;
        for (const auto& Ld : h->pk.layers) res_ok &= Ld.resident_ok && !h->wrapped;
        if (res_ok) kinds.push_back(KWS_KERNEL_RESIDENT);
        kinds.push_back(KWS_KERNEL_GENERIC);
    } else {
        kinds.push_back(KWS_KERNEL_AUTO);
    }
    for (int kind : kinds) {
        std::string kernels;
        // (1) TensorFlow's published constants, the 2-unit test cell embedded in this shape: units 0,1 and inputs 0..n_in-1 live.
        // They are constants of the plain cell: a wrapped handle skips them (its kernels are proven by (2) alone).
        for (int n_in = 2; n_in <= 3 && n_in <= I0 && !h->wrapped; ++n_in) {
            std::vector<float> blob(bl.total, 0.f);
            for (int l = 0; l < L; ++l) {
                const int in = bl.layer[l].in, live = l == 0 ? n_in : 2;
                float* Wg = blob.data() + bl.layer[l].wg;
                float* bg = blob.data() + bl.layer[l].bg;
                float* Wc = blob.data() + bl.layer[l].wc;
                for (int j = 0; j < 2 * H; ++j) bg[j] = 1.f;
                for (int r = 0; r < live + 2; ++r) {
                    const int row = r < live ? r : in + (r - live);
                    for (int u = 0; u < 2; ++u) {
                        Wg[(size_t)row * 2 * H + u] = 0.5f; Wg[(size_t)row * 2 * H + H + u] = 0.5f; Wc[(size_t)row * H + u] = 0.5f;
                    }
                }
            }
            float* Wfc = blob.data() + bl.wfc;
            Wfc[0 * C + 0] = 1.f; Wfc[1 * C + 1] = 1.f;
            const int B = 19, T = 1;
            std::vector<float> mel((size_t)B * T * I0, 0.f), st0((size_t)L * B * H, 0.f), st;
            for (int b = 0; b < B; ++b) {
                for (int k = 0; k < n_in; ++k) mel[(size_t)b * I0 + k] = 1.f;
                for (int l = 0; l < L; ++l) st0[((size_t)l * B + b) * H + 0] = st0[((size_t)l * B + b) * H + 1] = 0.1f;
            }
            double el, es;
            const int rc = selftest_case(cfg, plain, kind, blob, mel, st0, B, T, &el, &es, &st, &kernels);
            if (rc != KWS_OK) return rc;
            const double first = n_in == 2 ? 0.175991 : 0.156736;
            double worst = 0.0;
            for (int b = 0; b < B; ++b) {
                for (int u = 0; u < 2; ++u) worst = std::max(worst, std::fabs(st[(size_t)b * H + u] - first));
                if (L >= 2 && n_in == 2) for (int u = 0; u < 2; ++u) worst = std::max(worst, std::fabs(st[((size_t)B + b) * H + u] - 0.13248));
                if (cfg.precision != KWS_INT8)
                    for (int j = 2; j < H; ++j) if (st[(size_t)b * H + j] != 0.f) worst = 1.0;     // dead units stay exactly 0
            }
            if (!(worst <= tol_kat + 1e-6))
                return fail(KWS_ERR_HIP, "kws_selftest: %s returns TensorFlow's published GRUCell constant (%g) with error %.3g (tolerance %.1g). "
                            "This build (%s) computes wrong results on this device: rebuild with the ROCm release it was validated on, "
                            "or run the repository's GPU tests.", kernels.c_str(), first, worst, tol_kat, kws_version());
        }
        // (2) 8 random frames of 19 streams against the host double-precision loop
        if (tol_rand_logit > 0) {
            Lcg rng{0x9e3779b97f4a7c15ull + (uint64_t)kind};
            std::vector<float> blob(wl.total);
            for (int l = 0; l < L; ++l) {
                const int in = bl.layer[l].in;
                float* Wg = blob.data() + bl.layer[l].wg;
                float* bg = blob.data() + bl.layer[l].bg;
                float* Wc = blob.data() + bl.layer[l].wc;
                float* bc = blob.data() + bl.layer[l].bc;
                const float ag = std::sqrt(6.f / (in + H + 2 * H)), ac = std::sqrt(6.f / (in + H + H));
                for (size_t i = 0; i < (size_t)(in + H) * 2 * H; ++i) Wg[i] = ag * rng.next();
                for (int j = 0; j < 2 * H; ++j) bg[j] = 1.f + 0.3f * rng.next();
                for (size_t i = 0; i < (size_t)(in + H) * H; ++i) Wc[i] = ac * rng.next();
                for (int j = 0; j < H; ++j) bc[j] = 0.3f * rng.next();
            }
            float* Wfc = blob.data() + bl.wfc;
            for (int i = 0; i < H * C + C; ++i) Wfc[i] = rng.next();
            // the layer norm's tables, random: with TF's initial values (ibeta = 0) its output would not depend on the input
            if (wr.use_layer_norm)
                for (int l = 0; l < L; ++l) {
                    const float r = rng.next();
                    blob[wl.ibeta[l]] = (r < 0.f ? -1.f : 1.f) * (0.5f + 1.5f * std::fabs(r));
                    for (int k = 0; k < bl.layer[l].in; ++k) blob[wl.igamma[l] + k] = 0.5f * rng.next();
                }
            const int B = 19, T = 8;
            std::vector<float> mel((size_t)B * T * I0), st0((size_t)L * B * H);
            for (auto& v : mel) v = 2.f * std::fabs(rng.next());
            for (auto& v : st0) v = 0.5f * rng.next();
            double el, es;
            const int rc = selftest_case(cfg, wr, kind, blob, mel, st0, B, T, &el, &es, nullptr, &kernels);
            if (rc != KWS_OK) return rc;
            if (!(el <= tol_rand_logit && es <= tol_rand_state))
                return fail(KWS_ERR_HIP, "kws_selftest: %s differs from the host double-precision loop on 19 streams x 8 frames: max |dlogit| "
                            "%.3g (tolerance %.1g), max |dstate| %.3g (tolerance %.1g). This build (%s) computes wrong results on this "
                            "device: rebuild with the ROCm release it was validated on, or run the repository's GPU tests.",
                            kernels.c_str(), el, tol_rand_logit, es, tol_rand_state, kws_version());
            // a heads handle (kws_create_heads, fp32): the same case through kws_step_heads, a random second head behind the blob
            if (h->num_classes2 > 0) {
                const int C2 = h->num_classes2;
                for (int i = 0; i < H * C2 + C2; ++i) blob.push_back(rng.next());
                double er;
                const int rh = selftest_heads_case(cfg, C2, kind, blob, mel, st0, B, T, &el, &er, &es, &kernels);
                if (rh != KWS_OK) return rh;
                if (!(el <= tol_rand_logit && er <= tol_rand_state && es <= tol_rand_state))
                    return fail(KWS_ERR_HIP, "kws_selftest: kws_step_heads (%s) differs from the host double-precision loop on 19 streams x 8 frames, "
                                "one of them 4 frames long: max |dlogit| %.3g over both heads (tolerance %.1g), max |dnn_outputs| %.3g, max |dstate| "
                                "%.3g (tolerance %.1g). This build (%s) computes wrong results on this device: rebuild with the ROCm release it was "
                                "validated on, or run the repository's GPU tests.",
                                kernels.c_str(), el, tol_rand_logit, er, es, tol_rand_state, kws_version());
            }
        }
    }
    return KWS_OK;
}
