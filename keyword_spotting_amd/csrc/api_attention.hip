// C ABI of the self-attention CTC model (include/kws_amd.h, kws_attention_*): validation, the blob layout, the packed device
// image of the handle's precision (fp32 MFMA operands, or the split fp16 ones of attention_f16x3.hip) and positional table, the
// launch sequence (attention_kernels.hip, attention_f16x3.hip) and the self-test against a double host loop.
#include <new>
#include <random>

#include "api_internal.h"
#include "attention_internal.h"

using namespace kws_host;

namespace kws_host {

AttnLayout attn_layout(const kws_attention_config& c) {
    AttnLayout o{};
    const size_t H = c.hidden, Fi = c.ffn_inner, K = (size_t)c.n_mel * c.combine_frame;
    size_t at = 0;
    o.w_in = at, at += K * H;
    o.b_in = at, at += H;
    const size_t part[kLayerParts] = {H * 3 * H, 3 * H, H, H, H * Fi, Fi, Fi * H, H, H, H};
    for (int l = 0; l < c.num_layers; ++l)
        for (int i = 0; i < kLayerParts; ++i) o.layer[l][i] = at, at += part[i];
    o.w_out = at, at += H * c.num_classes;
    o.b_out = at, at += c.num_classes;
    o.total = at;
    return o;
}

bool attn_config_ok(const kws_attention_config* c, int* code) {
    if (!c) { *code = fail(KWS_ERR_INVALID_ARGUMENT, "config is null"); return false; }
    auto bad = [&](const char* field, int v, const char* want) {
        *code = fail(KWS_ERR_UNSUPPORTED, "%s=%d unsupported (%s)", field, v, want);
        return false;
    };
    if (c->n_mel < 1 || c->n_mel > 512) return bad("n_mel", c->n_mel, "1..512, n_mel * combine_frame <= 512");
    if (c->combine_frame < 1 || c->combine_frame > 4) return bad("combine_frame", c->combine_frame, "1..4");
    if (c->n_mel * c->combine_frame > 512) return bad("n_mel*combine_frame", c->n_mel * c->combine_frame, "<= 512");
    if (c->hidden != 64 && c->hidden != 128 && c->hidden != 256) return bad("hidden", c->hidden, "64, 128, 256");
    if (c->num_heads < 1 || c->hidden % c->num_heads != 0 || (c->hidden / c->num_heads != 16 && c->hidden / c->num_heads != 32))
        return bad("num_heads", c->num_heads, "hidden / num_heads must be 16 or 32");
    if (c->ffn_inner < 64 || c->ffn_inner > 1024 || c->ffn_inner % 64 != 0) return bad("ffn_inner", c->ffn_inner, "a multiple of 64, 64..1024");
    if (c->num_layers < 1 || c->num_layers > 8) return bad("num_layers", c->num_layers, "1..8");
    if (c->num_classes < 3 || c->num_classes > kws::kMaxClasses) return bad("num_classes", c->num_classes, "3..8");
    if (c->use_relu != 0 && c->use_relu != 1) return bad("use_relu", c->use_relu, "0 or 1");
    if (c->max_frames < 1 || c->max_frames > 8192) return bad("max_frames", c->max_frames, "1..8192");
    return true;
}

}  // namespace kws_host

namespace {

int frames_out(const kws_attention_config& c, int T) { return c.combine_frame > 1 ? T / c.combine_frame + 1 : T; }

// W [K, N] row-major -> v_mfma_f32_16x16x4_f32 B operands [ceil(K/16)][N/16][64][4] (attention_internal.h), appended to img
size_t pack_b(std::vector<float>& img, const float* W, int K, int N) {
    const size_t at = img.size();
    const int KC = (K + 15) / 16, NT = N / 16;
    img.resize(at + (size_t)KC * NT * 256, 0.f);
    float* out = img.data() + at;
    for (int kc = 0; kc < KC; ++kc)
        for (int nt = 0; nt < NT; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int k = 16 * kc + 4 * (lane >> 4) + j;
                    out[(((size_t)kc * NT + nt) * 64 + lane) * 4 + j] = k < K ? W[(size_t)k * N + 16 * nt + (lane & 15)] : 0.f;
                }
    return at;
}
// W [K, N] row-major, times `scale` (a power of two) -> v_mfma_f32_16x16x32_f16 B operands [ceil(K/32)][N/16][hi | lo][64][8 halves]
// (attention_internal.h), rows past K zero, appended to img: 4 bytes per weight, as the fp32 image
size_t pack_b16(std::vector<float>& img, const float* W, int K, int N, float scale) {
    const size_t at = img.size();
    const int KC = (K + 31) / 32, NT = N / 16;
    img.resize(at + (size_t)KC * NT * 2 * 64 * 4, 0.f);
    uint16_t* out = reinterpret_cast<uint16_t*>(img.data() + at);
    for (int kc = 0; kc < KC; ++kc)
        for (int nt = 0; nt < NT; ++nt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * kc + 8 * (lane >> 4) + j;
                    uint16_t hi = 0, lo = 0;
                    if (k < K) f16_split(W[(size_t)k * N + 16 * nt + (lane & 15)] * scale, &hi, &lo);
                    const size_t base = (((size_t)kc * NT + nt) * 2 * 64 + lane) * 8 + j;
                    out[base] = hi;
                    out[base + 64 * 8] = lo;
                }
    return at;
}
// f16x3: only the matrices become fp16 operands (W_in scaled by 256: 256 * 64 < 65504); biases, LN tables and W_out stay fp32
bool f16x3_range_ok(const float* w, size_t off, size_t n, const char* what, int layer, int* code) {
    for (size_t i = off; i < off + n; ++i)
        if (!(std::fabs(w[i]) < 64.0f)) {
            *code = fail(KWS_ERR_UNSUPPORTED, "f16x3 path: %s weight of layer %d (blob index %zu) = %g is outside (-64, 64) (fp16 operands; "
                         "W_in scaled by 256)", what, layer, i, (double)w[i]);
            return false;
        }
    return true;
}
// a plain table, padded so that the next section stays 16-byte aligned
size_t append(std::vector<float>& img, const float* v, size_t n) {
    const size_t at = img.size();
    img.insert(img.end(), v, v + n);
    img.resize((img.size() + 3) & ~(size_t)3, 0.f);
    return at;
}

// The contract (kws_amd.h) for one utterance, in double: logits [T'][C] (post-relu)
void host_forward(const kws_attention_config& c, const float* w, const AttnLayout& o, const std::vector<float>& pe, const float* mel,
                  int Tb, std::vector<double>& logits) {
    const int H = c.hidden, F = c.n_mel, cF = c.combine_frame * F, T1 = frames_out(c, Tb), Fi = c.ffn_inner, C = c.num_classes;
    const int heads = c.num_heads, d = H / heads;
    std::vector<double> x((size_t)T1 * H), qkv((size_t)T1 * 3 * H), y((size_t)T1 * H), inner(Fi), sc(T1);
    for (int t = 0; t < T1; ++t)
        for (int n = 0; n < H; ++n) {
            double s = 0.0;
            for (int k = 0; k < cF; ++k) {
                const size_t flat = (size_t)t * cF + k;
                if (flat < (size_t)Tb * F) s += (double)mel[flat] * w[o.w_in + (size_t)k * H + n];
            }
            x[(size_t)t * H + n] = s + w[o.b_in + n] + pe[(size_t)t * H + n];
        }
    auto layer_norm = [&](std::vector<double>& v, const float* gamma, const float* beta) {
        double mean = 0.0, var = 0.0;
        for (double e : v) mean += e;
        mean /= (double)v.size();
        for (double e : v) var += (e - mean) * (e - mean);
        var /= (double)v.size();
        const double rstd = 1.0 / std::sqrt(var + 1e-12);
        for (size_t i = 0; i < v.size(); ++i) v[i] = (v[i] - mean) * rstd * gamma[i % H] + beta[i % H];
    };
    for (int l = 0; l < c.num_layers; ++l) {
        const size_t* L = o.layer[l];
        for (int t = 0; t < T1; ++t)
            for (int n = 0; n < 3 * H; ++n) {
                double s = 0.0;
                for (int k = 0; k < H; ++k) s += x[(size_t)t * H + k] * w[L[kQkvW] + (size_t)k * 3 * H + n];
                qkv[(size_t)t * 3 * H + n] = s + w[L[kQkvB] + n];
            }
        for (int h = 0; h < heads; ++h)
            for (int t = 0; t < T1; ++t) {
                double mx = -1e300;
                for (int u = 0; u < T1; ++u) {
                    double s = 0.0;
                    for (int e = 0; e < d; ++e) s += qkv[(size_t)t * 3 * H + h * d + e] * qkv[(size_t)u * 3 * H + H + h * d + e];
                    sc[u] = s / std::sqrt((double)d);
                    mx = std::max(mx, sc[u]);
                }
                double den = 0.0;
                for (int u = 0; u < T1; ++u) den += (sc[u] = std::exp(sc[u] - mx));
                for (int e = 0; e < d; ++e) {
                    double s = 0.0;
                    for (int u = 0; u < T1; ++u) s += sc[u] * qkv[(size_t)u * 3 * H + 2 * H + h * d + e];
                    y[(size_t)t * H + h * d + e] = s / den + x[(size_t)t * H + h * d + e];
                }
            }
        layer_norm(y, w + L[kLnaGamma], w + L[kLnaBeta]);
        for (int t = 0; t < T1; ++t) {
            for (int f = 0; f < Fi; ++f) {
                double s = 0.0;
                for (int k = 0; k < H; ++k) s += y[(size_t)t * H + k] * w[L[kW1] + (size_t)k * Fi + f];
                inner[f] = std::max(s + w[L[kB1] + f], 0.0);
            }
            for (int n = 0; n < H; ++n) {
                double s = 0.0;
                for (int f = 0; f < Fi; ++f) s += inner[f] * w[L[kW2] + (size_t)f * H + n];
                x[(size_t)t * H + n] = s + w[L[kB2] + n] + y[(size_t)t * H + n];
            }
        }
        layer_norm(x, w + L[kLnbGamma], w + L[kLnbBeta]);
    }
    logits.assign((size_t)T1 * C, 0.0);
    for (int t = 0; t < T1; ++t)
        for (int cl = 0; cl < C; ++cl) {
            double s = 0.0;
            for (int k = 0; k < H; ++k) s += x[(size_t)t * H + k] * w[o.w_out + (size_t)k * C + cl];
            s += w[o.b_out + cl];
            logits[(size_t)t * C + cl] = c.use_relu ? std::max(s, 0.0) : s;
        }
}

// scratch of a call: S, QKV, U [B][Tp][H | 3H | H] and the two LN partial tables [B][ntile]
size_t scratch_need(const kws_attention_config& c, int B, int T_max, int* Tp_out) {
    const int T1 = frames_out(c, T_max);
    const int Tp = (T1 + kws::kAttnRows - 1) / kws::kAttnRows * kws::kAttnRows;
    if (Tp_out) *Tp_out = Tp;
    return (size_t)B * Tp * 5 * c.hidden * sizeof(float) + 2 * (size_t)B * (Tp / kws::kAttnRows) * sizeof(float4);
}

int ensure_scratch(kws_attention_handle h, size_t need) {
    if (need <= h->scratch_bytes) return KWS_OK;
    KWS_HIP(hipDeviceSynchronize());          // earlier calls may still use the old block
    if (h->scratch) hipFree(h->scratch);
    h->scratch = nullptr;
    h->scratch_bytes = 0;
    KWS_HIP(hipMalloc(reinterpret_cast<void**>(&h->scratch), need));
    h->scratch_bytes = need;
    return KWS_OK;
}

}  // namespace

namespace kws_host {

int attn_reserve_locked(kws_attention* h, int B, int T_max) { return ensure_scratch(h, scratch_need(h->cfg, B, T_max, nullptr)); }

int attn_stage_reserve_locked(kws_attention* h, size_t bytes) {
    if (bytes <= h->stage_bytes) return KWS_OK;
    KWS_HIP(hipDeviceSynchronize());          // a feed in flight may still use the old block
    if (h->stage) hipFree(h->stage);
    h->stage = nullptr;
    h->stage_bytes = 0;
    KWS_HIP(hipMalloc(reinterpret_cast<void**>(&h->stage), bytes));
    h->stage_bytes = bytes;
    return KWS_OK;
}

int attn_call_enter(kws_attention* h, hipStream_t st) {
    if (h->last_stream_valid && st != h->last_stream) KWS_HIP(hipStreamWaitEvent(st, h->last_done, 0));
    h->last_stream = st;
    h->last_stream_valid = true;
    return KWS_OK;
}

int attn_call_leave(kws_attention* h, hipStream_t st) { return hip_done(hipEventRecord(h->last_done, st), "hipEventRecord"); }

// The model's 2 + 3L launches over B utterances of up to T_max frames (validated by the caller, T'_max > 0), the scratch reserved
int attn_run_locked(kws_attention* h, const float* mel, const int32_t* lengths, int B, int T_max, float* logits, float* softmax,
                    hipStream_t st) {
    const kws_attention_config& c = h->cfg;
    int Tp = 0;
    if (scratch_need(c, B, T_max, &Tp) > h->scratch_bytes) return fail(KWS_ERR_INVALID_ARGUMENT, "internal: the attention scratch was not reserved");
    const int H = c.hidden;
    kws::AttnParams p{};
    p.mel = mel;
    p.lengths = lengths;
    p.B = B, p.T_max = T_max, p.F = c.n_mel, p.c = c.combine_frame, p.KE = h->KE;
    p.T1max = frames_out(c, T_max), p.Tp = Tp, p.ntile = Tp / kws::kAttnRows;
    p.Fi = c.ffn_inner, p.C = c.num_classes, p.use_relu = c.use_relu;
    p.w_in = h->w_in, p.b_in = h->b_in, p.pe = h->d_pe, p.w_out = h->w_out, p.b_out = h->b_out;
    float* s = reinterpret_cast<float*>(h->scratch);
    const size_t act = (size_t)B * Tp * H;
    p.S = s, p.QKV = s + act, p.U = s + 4 * act;
    p.st_a = reinterpret_cast<float4*>(s + 5 * act);
    p.st_b = p.st_a + (size_t)B * p.ntile;
    p.logits = logits, p.softmax = softmax;

    // the three GEMM kernels in the handle's precision; the core and the output kernel are fp32 for both
    const bool f16 = h->precision == KWS_F16X3;
    hipError_t e = f16 ? kws::launch_attn_embed_f16x3(p, H, st) : kws::launch_attn_embed(p, H, st);
    for (int l = 0; l < c.num_layers && e == hipSuccess; ++l) {
        const kws::AttnLayerW* prev = l > 0 ? &h->layer[l - 1] : nullptr;
        e = f16 ? kws::launch_attn_qkv_f16x3(p, h->layer[l], prev, H, st) : kws::launch_attn_qkv(p, h->layer[l], prev, H, st);
        if (e == hipSuccess) e = kws::launch_attn_core(p, prev, H, H / c.num_heads, st);
        if (e == hipSuccess) e = f16 ? kws::launch_attn_ffn_f16x3(p, h->layer[l], H, st) : kws::launch_attn_ffn(p, h->layer[l], H, st);
    }
    if (e == hipSuccess) e = kws::launch_attn_out(p, h->layer[c.num_layers - 1], H, st);
    return hip_done(e, "attention kernel launch");
}

}  // namespace kws_host

extern "C" {

size_t kws_sizeof_attention_config(void) { return sizeof(kws_attention_config); }

size_t kws_attention_weights_nbytes(const kws_attention_config* cfg) {
    int code;
    if (!attn_config_ok(cfg, &code)) return 0;
    return attn_layout(*cfg).total * sizeof(float);
}

int kws_attention_frames_out(const kws_attention_config* cfg, int T) {
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    if (T < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative T=%d", T);
    if (cfg->combine_frame < 1 || cfg->combine_frame > 4)
        return fail(KWS_ERR_UNSUPPORTED, "combine_frame=%d unsupported (1..4)", cfg->combine_frame);
    return frames_out(*cfg, T);
}

int kws_attention_create(const kws_attention_config* cfg, const void* weights_blob, size_t nbytes, kws_attention_handle* out) {
    return kws_attention_create_precision(cfg, KWS_FP32, weights_blob, nbytes, out);
}

int kws_attention_create_precision(const kws_attention_config* cfg, int precision, const void* weights_blob, size_t nbytes,
                                   kws_attention_handle* out) {
    int code;
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!attn_config_ok(cfg, &code)) return code;
    if (precision == KWS_BF16 || precision == KWS_INT8)
        return fail(KWS_ERR_UNSUPPORTED, "precision %s is not served for the attention model (KWS_FP32 or KWS_F16X3)",
                    precision == KWS_BF16 ? "KWS_BF16" : "KWS_INT8");
    if (precision != KWS_FP32 && precision != KWS_F16X3)
        return fail(KWS_ERR_UNSUPPORTED, "precision=%d unsupported (KWS_FP32 or KWS_F16X3)", precision);
    if (!weights_blob) return fail(KWS_ERR_INVALID_ARGUMENT, "weights_blob is null");
    const AttnLayout lay = attn_layout(*cfg);
    if (nbytes != lay.total * sizeof(float))
        return fail(KWS_ERR_INVALID_ARGUMENT, "weights_blob has %zu bytes, config needs %zu", nbytes, lay.total * sizeof(float));
    const bool f16 = precision == KWS_F16X3;
    if (f16) {
        const float* wb = static_cast<const float*>(weights_blob);
        const size_t Hh = cfg->hidden, Fii = cfg->ffn_inner;
        bool ok = f16x3_range_ok(wb, lay.w_in, (size_t)cfg->n_mel * cfg->combine_frame * Hh, "W_in", 0, &code);
        for (int l = 0; l < cfg->num_layers && ok; ++l)
            ok = f16x3_range_ok(wb, lay.layer[l][kQkvW], Hh * 3 * Hh, "W_qkv", l, &code) &&
                 f16x3_range_ok(wb, lay.layer[l][kW1], Hh * Fii, "W1", l, &code) && f16x3_range_ok(wb, lay.layer[l][kW2], Fii * Hh, "W2", l, &code);
        if (!ok) return code;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");

    kws_attention* m = new (std::nothrow) kws_attention();
    if (!m) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    m->cfg = *cfg;
    m->precision = precision;
    const float* w = static_cast<const float*>(weights_blob);
    m->blob.assign(w, w + lay.total);
    const int H = cfg->hidden, Fi = cfg->ffn_inner, C = cfg->num_classes, cF = cfg->n_mel * cfg->combine_frame;
    m->KE = f16 ? (cF + 31) / 32 * 32 : (cF + 15) / 16 * 16;
    // positional_encoding_op.cc:44-48: double, stored as float
    m->pe_rows = cfg->max_frames / cfg->combine_frame + 1;
    m->pe.resize((size_t)m->pe_rows * H);
    for (int p = 0; p < m->pe_rows; ++p)
        for (int i = 0; i < H / 2; ++i) {
            const double a = p / std::pow(10000.0, 2.0 * i / H);
            m->pe[(size_t)p * H + 2 * i] = (float)std::sin(a);
            m->pe[(size_t)p * H + 2 * i + 1] = (float)std::cos(a);
        }
    // one GEMM image per handle: the fp32 operands, or the split fp16 ones (W_in times 2^8 against the kernel's mel * 2^-8)
    std::vector<float> img;
    auto pack = [&](const float* W, int K, int N, float scale) { return f16 ? pack_b16(img, W, K, N, scale) : pack_b(img, W, K, N); };
    struct LOff { size_t wqkv, bqkv, ga, ba, w1, b1, w2, b2, gb, bb; } lo[8];
    const size_t o_win = pack(w + lay.w_in, cF, H, 256.f);
    const size_t o_bin = append(img, w + lay.b_in, H);
    for (int l = 0; l < cfg->num_layers; ++l) {
        const size_t* L = lay.layer[l];
        lo[l].wqkv = pack(w + L[kQkvW], H, 3 * H, 1.f);
        lo[l].bqkv = append(img, w + L[kQkvB], 3 * H);
        lo[l].ga = append(img, w + L[kLnaGamma], H);
        lo[l].ba = append(img, w + L[kLnaBeta], H);
        lo[l].w1 = pack(w + L[kW1], H, Fi, 1.f);
        lo[l].b1 = append(img, w + L[kB1], Fi);
        lo[l].w2 = pack(w + L[kW2], Fi, H, 1.f);
        lo[l].b2 = append(img, w + L[kB2], H);
        lo[l].gb = append(img, w + L[kLnbGamma], H);
        lo[l].bb = append(img, w + L[kLnbBeta], H);
    }
    const size_t o_wout = append(img, w + lay.w_out, (size_t)H * C);
    const size_t o_bout = append(img, w + lay.b_out, C);
    const size_t o_pe = append(img, m->pe.data(), m->pe.size());
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->d_w), img.size() * sizeof(float));
    if (e != hipSuccess) { delete m; return hip_fail(e, "hipMalloc(attention weights)"); }
    e = hipMemcpy(m->d_w, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();     // the upload has landed before any stream launches on it
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->last_done, hipEventDisableTiming);
    if (e != hipSuccess) { hipFree(m->d_w); delete m; return hip_fail(e, "attention weight upload"); }
    const float* d = m->d_w;
    m->w_in = reinterpret_cast<const float4*>(d + o_win);
    m->b_in = d + o_bin;
    for (int l = 0; l < cfg->num_layers; ++l)
        m->layer[l] = {reinterpret_cast<const float4*>(d + lo[l].wqkv), d + lo[l].bqkv, d + lo[l].ga, d + lo[l].ba,
                       reinterpret_cast<const float4*>(d + lo[l].w1), d + lo[l].b1, reinterpret_cast<const float4*>(d + lo[l].w2),
                       d + lo[l].b2, d + lo[l].gb, d + lo[l].bb};
    m->w_out = d + o_wout;
    m->b_out = d + o_bout;
    m->d_pe = d + o_pe;
    static const bool selftest_env = [] { const char* s = getenv("KWS_SELFTEST"); return s && s[0] == '1'; }();
    if (selftest_env) {
        const int rc = kws_attention_selftest(m);
        if (rc != KWS_OK) {
            const std::string keep = g_last_error;
            kws_attention_destroy(m);
            g_last_error = keep;
            return rc;
        }
    }
    live_register(m);      // stream managers borrow the handle (kws_attention_stream_create)
    *out = m;
    return KWS_OK;
}

int kws_attention_destroy(kws_attention_handle h) {
    if (!h) return KWS_OK;
    live_unregister(h);
    hipDeviceSynchronize();
    if (h->d_w) hipFree(h->d_w);
    if (h->scratch) hipFree(h->scratch);
    if (h->stage) hipFree(h->stage);
    if (h->last_done) hipEventDestroy(h->last_done);
    delete h;
    return KWS_OK;
}

int kws_attention_reserve(kws_attention_handle h, int B, int T_max) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    BusyGuard busy(h->in_call);
    if (!busy.owned) return fail(KWS_ERR_BUSY, "kws_attention_reserve: another host thread is inside a call on this handle");
    if (B < 0 || T_max < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative B=%d or T_max=%d", B, T_max);
    if (T_max > h->cfg.max_frames) return fail(KWS_ERR_UNSUPPORTED, "T_max=%d exceeds max_frames=%d", T_max, h->cfg.max_frames);
    return attn_reserve_locked(h, B, T_max);
}

int kws_attention_run(kws_attention_handle h, const float* mel, const int32_t* lengths, int B, int T_max, float* logits,
                      float* softmax, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (B < 0 || T_max < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative B=%d or T_max=%d", B, T_max);
    const kws_attention_config& c = h->cfg;
    if (T_max > c.max_frames) return fail(KWS_ERR_UNSUPPORTED, "T_max=%d exceeds max_frames=%d", T_max, c.max_frames);
    if (B > 65535) return fail(KWS_ERR_UNSUPPORTED, "B=%d unsupported (<= 65535)", B);
    if (!logits && !softmax) return fail(KWS_ERR_INVALID_ARGUMENT, "logits and softmax are both null");
    if (B == 0 || frames_out(c, T_max) == 0) return KWS_OK;
    if (!mel && T_max > 0) return fail(KWS_ERR_INVALID_ARGUMENT, "mel is null");
    BusyGuard busy(h->in_call);
    if (!busy.owned)
        return fail(KWS_ERR_BUSY, "kws_attention_run: another host thread is inside a call on this handle (one thread at a time per handle)");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(attn_reserve_locked(h, B, T_max));
    KWS_TRY(attn_call_enter(h, st));
    const int rc = attn_run_locked(h, mel, lengths, B, T_max, logits, softmax, st);
    const int rl = attn_call_leave(h, st);      // also after a failure: what was queued is what the next call waits for
    return rc != KWS_OK ? rc : rl;
}

int kws_attention_pe_table(kws_attention_handle h, float* host_out) {
    if (!h || !host_out) return fail(KWS_ERR_INVALID_ARGUMENT, "null handle / buffer");
    memcpy(host_out, h->pe.data(), h->pe.size() * sizeof(float));
    return KWS_OK;
}

int kws_attention_selftest(kws_attention_handle h) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    const kws_attention_config& c = h->cfg;
    const int B = 3, T = std::min(c.max_frames, 70), F = c.n_mel, C = c.num_classes, T1 = frames_out(c, T);
    const int32_t lens[B] = {T, T / 2 + 1, 1};
    std::mt19937 rng(1234);
    std::uniform_real_distribution<float> uni(-1.f, 1.f);
    std::vector<float> mel((size_t)B * T * F), got((size_t)B * T1 * C);
    for (float& v : mel) v = uni(rng);
    float *d_mel = nullptr, *d_out = nullptr;
    int32_t* d_len = nullptr;
    hipStream_t st = nullptr;
    int rc = KWS_OK;
    auto cleanup = [&] {
        if (st) hipStreamSynchronize(st);
        for (void* q : {(void*)d_mel, (void*)d_out, (void*)d_len}) if (q) hipFree(q);
        if (st) hipStreamDestroy(st);
    };
    hipError_t e = hipStreamCreate(&st);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_mel), mel.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_out), got.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_len), sizeof(lens));
    if (e == hipSuccess) e = hipMemcpy(d_mel, mel.data(), mel.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_len, lens, sizeof(lens), hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); return hip_fail(e, "kws_attention_selftest setup"); }
    rc = kws_attention_run(h, d_mel, d_len, B, T, d_out, nullptr, st);
    if (rc == KWS_OK) {
        e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipMemcpy(got.data(), d_out, got.size() * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = hip_fail(e, "kws_attention_selftest run");
    }
    cleanup();
    if (rc != KWS_OK) return rc;
    const AttnLayout lay = attn_layout(c);
    std::vector<double> want;
    for (int b = 0; b < B; ++b) {
        host_forward(c, h->blob.data(), lay, h->pe, mel.data() + (size_t)b * T * F, lens[b], want);
        const int T1b = frames_out(c, lens[b]);
        for (int t = 0; t < T1; ++t)
            for (int cl = 0; cl < C; ++cl) {
                const double ref = t < T1b ? want[(size_t)t * C + cl] : 0.0;
                const double v = got[((size_t)b * T1 + t) * C + cl];
                if (!(std::fabs(v - ref) <= 2e-4 * (1.0 + std::fabs(ref))))
                    return fail(KWS_ERR_HIP, "kws_attention_selftest: utterance %d (T=%d) row %d class %d: %.7g, host loop %.7g (%s)", b,
                                lens[b], t, cl, v, ref, kws_version());
            }
    }
    return KWS_OK;
}

}  // extern "C"
