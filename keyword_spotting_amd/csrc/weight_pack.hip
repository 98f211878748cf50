// The canonical weight blob read once, re-tiled into the fragment tables of every kernel family (kws_create uploads the image).
// Host code only.

#include "api_internal.h"

namespace kws_host {

BlobLayout blob_layout(const kws_config& c) {
    BlobLayout b;
    const size_t H = c.hidden;
    size_t at = 0;
    int in = c.n_mel;
    for (int l = 0; l < c.num_layers; ++l) {
        BlobLayout::Layer& L = b.layer[l];
        L.in = in;
        L.wg = at;
        L.bg = L.wg + (in + H) * 2 * H;
        L.wc = L.bg + 2 * H;
        L.bc = L.wc + (in + H) * H;
        at = L.bc + H;
        in = c.hidden;
    }
    b.wfc = at;
    b.bfc = b.wfc + H * c.num_classes;
    b.total = b.bfc + c.num_classes;
    return b;
}

WrapLayout wrap_layout(const kws_config& c, const kws_cell_wrappers& w) {
    WrapLayout r;
    size_t at = blob_layout(c).total;
    for (int l = 0; l < c.num_layers; ++l) {
        r.ibeta[l] = at;
        r.igamma[l] = at + 1;
        if (w.use_layer_norm) at += 1 + (size_t)(l == 0 ? c.n_mel : c.hidden);
    }
    r.total = at;
    return r;
}

namespace {

// K-index permutation of the "xl" layout: chunk kc, lane group g -> source row
inline int kmap_grouped(int kc, int g) { return 16 * (kc / 4) + 4 * g + (kc % 4); }
inline int kmap_interleaved(int kc, int g) { return 4 * kc + g; }

// gate q of a layer's canonical weights: q=0 r (Wg[:, :H]), q=1 u (Wg[:, H:]), q=2 c (Wc)
inline float wq(const float* blob, const BlobLayout::Layer& Ly, int H, int q, int row, int unit) {
    return q == 2 ? blob[Ly.wc + (size_t)row * H + unit] : blob[Ly.wg + (size_t)row * 2 * H + q * H + unit];
}

// fp32 -> bf16 bits, round to nearest even (what v_cvt_pk_bf16_f32 does)
inline uint16_t bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// ... and with the lo piece at its own magnitude: v = hi + lo.  Below 2^-14 the piece is an fp16 subnormal (absolute precision
// 2^-25): the value keeps max(2^-23 |v|, 2^-25) -- fp32's own rounding down to |v| = 1/4, a 3e-8 absolute floor below that
inline void f16_split_unscaled(float v, uint16_t* hi, uint16_t* lo) {
    *hi = f16_rne(v);
    *lo = f16_rne(v - f16_value(*hi));
#ifdef KWS_EXP_F16_WLO_ZERO
    *lo = 0;
#endif
}
// unit of a hidden vector addressed by (chunk m, lane group g, element j) in the bf16 exchange layout
inline int bf16_unit(int m, int g, int j) { return 32 * m + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4)); }

// Source row of element j of lane group g in 32-wide K chunk c of a bf16 / f16x3 A operand (gru_bf16's K permutation).  The
// layer's kx input chunks come first: the first layer's mel bins 32c + 8g + j (false: a zero row past the last bin), a higher
// layer's input in the exchange order; then the hidden-state rows, which follow the `in` input rows of the canonical matrix.
inline bool row32(int l, int c, int kx, int in, int g, int j, int* row) {
    if (c >= kx) { *row = in + bf16_unit(c - kx, g, j); return true; }
    if (l > 0) { *row = bf16_unit(c, g, j); return true; }
    *row = 32 * c + 8 * g + j;
    return *row < in;
}

// appends a zeroed table of n floats to the image, starting on a 16-byte boundary; its offset
size_t reserve(std::vector<float>& host, size_t n) {
    const size_t off = host.size();
    host.resize(off + ((n + 3) & ~size_t(3)), 0.f);
    return off;
}

// dense: Wfc [H,C] -> A fragments of Wfc^T padded to 16 rows, [H/4][64]; bias padded to 16
void pack_dense(const float* Wfc, const float* bfc, int H, int C, size_t* wfc_off, size_t* bfc_off, std::vector<float>& host) {
    const int KCH = H / 4;
    *wfc_off = reserve(host, (size_t)KCH * 64);
    for (int kc = 0; kc < KCH; ++kc)
        for (int lane = 0; lane < 64; ++lane) {
            const int g = lane >> 4, i = lane & 15;
            host[*wfc_off + (size_t)kc * 64 + lane] = i < C ? Wfc[(size_t)kmap_grouped(kc, g) * C + i] : 0.f;
        }
    *bfc_off = reserve(host, 16);
    for (int i = 0; i < C; ++i) host[*bfc_off + i] = bfc[i];
}

// fp32 tables: every precision's biases, and the resident / generic kernels' fragments
void pack_fp32(const kws_config& cfg, const float* blob, const BlobLayout& bl, PackedWeights* pk, std::vector<float>& host) {
    const int H = cfg.hidden, NT = H / 16, KCH = H / 4, C = cfg.num_classes;
    for (int l = 0; l < cfg.num_layers; ++l) {
        const bool first = l == 0;
        const BlobLayout::Layer& Ly = bl.layer[l];
        const int in = Ly.in;
        LayerDev L;
        L.in_dim = in;
        L.resident_ok = kws::gru_resident_supported(H, in, first);
        L.kcx_res = kws::gru_resident_kcx(in, first);
        L.kcx_gen = 4 * ((in + 15) / 16);
        // biases [3][H]
        L.bias = reserve(host, 3 * (size_t)H);
        for (int j = 0; j < 2 * H; ++j) host[L.bias + j] = blob[Ly.bg + j];
        for (int j = 0; j < H; ++j) host[L.bias + 2 * H + j] = blob[Ly.bc + j];
        // h-part, group-of-4 fragments [NT][3][NT][64][4] (one dwordx4 = four k-chunks; both kernel families)
        L.wh_gen = reserve(host, (size_t)NT * 3 * KCH * 64);
        for (int n = 0; n < NT; ++n)
            for (int q = 0; q < 3; ++q)
                for (int kc = 0; kc < KCH; ++kc)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int g = lane >> 4, i = lane & 15;
                        const float v = wq(blob, Ly, H, q, in + kmap_grouped(kc, g), n * 16 + i);
                        host[L.wh_gen + ((((size_t)(n * 3 + q) * NT + kc / 4) * 64 + lane) * 4 + kc % 4)] = v;
                    }
        // x-part
        L.wx_res = reserve(host, (size_t)NT * 3 * L.kcx_res * 64);
        L.wx_gen = reserve(host, (size_t)NT * 3 * L.kcx_gen * 64);
        for (int n = 0; n < NT; ++n)
            for (int q = 0; q < 3; ++q)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15;
                    for (int kc = 0; kc < L.kcx_res; ++kc) {
                        const int row = first ? kmap_interleaved(kc, g) : kmap_grouped(kc, g);
                        host[L.wx_res + (((size_t)(n * 3 + q) * L.kcx_res + kc) * 64 + lane)] =
                            row < in ? wq(blob, Ly, H, q, row, n * 16 + i) : 0.f;
                    }
                    for (int kc = 0; kc < L.kcx_gen; ++kc) {
                        const int row = kmap_grouped(kc, g);
                        host[L.wx_gen + ((((size_t)(n * 3 + q) * (L.kcx_gen / 4) + kc / 4) * 64 + lane) * 4 + kc % 4)] =
                            row < in ? wq(blob, Ly, H, q, row, n * 16 + i) : 0.f;
                    }
                }
        pk->layers.push_back(L);
    }
    pack_dense(blob + bl.wfc, blob + bl.bfc, H, C, &pk->wfc_off, &pk->bfc_off, host);
}

// A operands of the 16x16x32 MFMAs, bf16 or f16x3 (gru_bf16.hip, gru_f16x3*.hip): [H/16 tiles][3 gates][kc chunks][pieces][64 lanes]
// x 8 halves, lane (g,i) holding W[row(c,g,j)][16n+i], j = 0..7, rows in gru_bf16's K permutation (row32).  bf16: one piece.
// f16x3: the pieces hi | lo of each weight, the first layer's x-part scaled by 2^8 (the kernel feeds mel * 2^-8: both exact) so
// that mel magnitudes far beyond fp16's 65504 stay representable.
int pack_a32(const kws_config& cfg, const float* blob, const BlobLayout& bl, PackedWeights* pk, std::vector<float>& host) {
    const int H = cfg.hidden, NT = H / 16, C = cfg.num_classes;
    const int HCh = H / 32;                    // 32-wide chunks of a hidden vector
    const bool f16 = cfg.precision == KWS_F16X3;
    const size_t pieces = f16 ? 2 : 1;
    if (f16) {
        // only the matrices become fp16 operands (x-part scaled by 256, candidate by 2 log2 e: 256 * 2.886 * 64 < 65504); the
        // biases and bfc stay fp32 in the kernels and may be of any size
        auto range_ok = [&](size_t off, size_t n, const char* what, int layer) {
            for (size_t i = off; i < off + n; ++i)
                if (!(std::fabs(blob[i]) < 64.0f)) {
                    fail(KWS_ERR_UNSUPPORTED, "f16x3 path: %s weight of layer %d (blob index %zu) = %g is outside (-64, 64) (fp16 operands; "
                         "x-part scaled by 256, candidate by 2 log2 e)", what, layer, i, (double)blob[i]);
                    return false;
                }
            return true;
        };
        bool ok = true;
        for (int l = 0; l < cfg.num_layers && ok; ++l) {
            const size_t K = bl.layer[l].in + H;
            ok = range_ok(bl.layer[l].wg, K * 2 * H, "gate", l) && range_ok(bl.layer[l].wc, K * H, "candidate", l);
        }
        if (!ok || !range_ok(bl.wfc, (size_t)H * C, "projection", cfg.num_layers)) return KWS_ERR_UNSUPPORTED;
        // hidden = 128: the register-resident kernels (gru_f16x3.hip); otherwise the streaming ones (gru_f16x3_generic.hip), whose
        // phases come in row pairs: the first layer's x chunks are padded to an even count (zero operands)
        pk->f16_generic = !kws::gru_f16x3_supported(H, cfg.n_mel);
        pk->f16_kx0 = pk->f16_generic ? 2 * ((cfg.n_mel + 63) / 64) : (cfg.n_mel + 31) / 32;
    } else {
        pk->bf_kx0 = (cfg.n_mel + 31) / 32;
    }
    // one weight -> its pieces.  f16x3: the register-resident kernels (gru_f16x3.hip) keep ONE accumulator per product: lo pieces
    // unscaled, except the first layer's x-part, which meets the mel frame's 2^11-scaled lo piece; the streaming kernels
    // (gru_f16x3_generic.hip) keep main / lo accumulators and scaled lo pieces throughout
    auto put = [&](uint16_t* dst, size_t base, int lane, int j, float v, bool scaled_lo) {
        if (!f16) { dst[(base + lane) * 8 + j] = bf16_rne(v); return; }
        uint16_t hi, lo;
        if (scaled_lo) f16_split(v, &hi, &lo);
        else f16_split_unscaled(v, &hi, &lo);
        dst[(base + lane) * 8 + j] = hi;
        dst[(base + 64 + lane) * 8 + j] = lo;
    };
    for (int l = 0; l < cfg.num_layers; ++l) {
        const BlobLayout::Layer& Ly = bl.layer[l];
        const int kx = l == 0 ? (f16 ? pk->f16_kx0 : pk->bf_kx0) : HCh, kc = kx + HCh;
        const size_t off = reserve(host, (size_t)NT * 3 * kc * pieces * 64 * 4);
        if (f16) pk->f16_w.push_back(off);
        else pk->bf_w[l] = off;
        uint16_t* dst = reinterpret_cast<uint16_t*>(&host[off]);
        for (int n = 0; n < NT; ++n)
            for (int gq = 0; gq < 3; ++gq)
                for (int c = 0; c < kc; ++c)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int g = lane >> 4, i = lane & 15;
                            int row;
                            float v = 0.f;          // a zero row past the last mel bin: +0 in every piece
                            if (row32(l, c, kx, Ly.in, g, j, &row)) {
                                v = wq(blob, Ly, H, gq, row, n * 16 + i);
                                // f16x3: the exponent scale of the gate's activation rides in the weights: sigmoid(a) = 1 / (1 + exp2(-a log2 e)),
                                // tanh(a) = 1 - 2 / (1 + exp2(2 a log2 e)) -- the kernel applies exp2 to the pre-activation as it is
                                const float act = gq == 2 ? 2.0f * 1.4426950408889634f : -1.4426950408889634f;
                                if (f16) v = (l == 0 && c < kx ? 256.f : 1.f) * (act * v);
                            }
                            put(dst, (((size_t)(n * 3 + gq) * kc + c) * pieces) * 64, lane, j, v, pk->f16_generic || (l == 0 && c < kx));
                        }
    }
    // the projection: Wfc^T padded to 16 rows, [HCh chunks][pieces][64 lanes] x 8
    const size_t off = reserve(host, (size_t)HCh * pieces * 64 * 4);
    (f16 ? pk->f16_wfc : pk->bf_wfc) = off;
    uint16_t* dst = reinterpret_cast<uint16_t*>(&host[off]);
    for (int c = 0; c < HCh; ++c)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int g = lane >> 4, i = lane & 15;
                put(dst, (size_t)c * pieces * 64, lane, j, i < C ? blob[bl.wfc + (size_t)bf16_unit(c, g, j) * C + i] : 0.f, pk->f16_generic);
            }
    return KWS_OK;
}

uint32_t pack16(int8_t lo, int8_t hi) { return (uint32_t)(uint16_t)(int16_t)lo | ((uint32_t)(uint16_t)(int16_t)hi << 16); }

// A quantised GRU matrix Wq [units][K] as the int8 layer kernel reads it: K split over `waves` waves, each wave's part
// [unit groups][unit-in-lane 2][K / waves / 2 couples x (even, odd)][64 lanes] (gates: 4 waves x 2 groups, candidate: 8 x 1)
size_t pack_couples(std::vector<float>& host, const std::vector<int8_t>& q, int K, int waves, int groups) {
    const int KW = K / waves;
    const size_t off = reserve(host, (size_t)waves * groups * KW * 64);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&host[off]);
    for (int w = 0; w < waves; ++w)
        for (int ug = 0; ug < groups; ++ug)
            for (int c = 0; c < KW; ++c)
                for (int lane = 0; lane < 64; ++lane) {
                    const int ul = c / (KW / 2), c2 = c % (KW / 2);
                    const int n = 128 * ug + 64 * ul + lane, k0 = KW * w + 4 * (c2 / 2) + (c2 & 1);
                    dst[((size_t)(w * groups + ug) * KW + c) * 64 + lane] = pack16(q[(size_t)n * K + k0], q[(size_t)n * K + k0 + 2]);
                }
    return off;
}

// int8 ("octbit") tables (octbit_graph.py:218-225): every MatMul outside cell_0 is quantised -> layers >= 1 and the projection
int pack_int8(const kws_config& cfg, const float* blob, const BlobLayout& bl, PackedWeights* pk, std::vector<float>& host) {
    const int H = cfg.hidden, C = cfg.num_classes;
    pk->oct.resize(cfg.num_layers);
    for (int l = 1; l < cfg.num_layers; ++l) {
        const int K = bl.layer[l].in + H;
        PackedWeights::OctLayer& O = pk->oct[l];
        O.quantised = true;
        std::vector<int8_t> gq((size_t)2 * H * K), cq((size_t)H * K);
        std::vector<float> gb(2 * H), cb(H);
        int rc = kws_octbit_quantize(blob + bl.layer[l].wg, K, 2 * H, gq.data(), &O.scale_g, gb.data());
        if (rc == KWS_OK) rc = kws_octbit_quantize(blob + bl.layer[l].wc, K, H, cq.data(), &O.scale_c, cb.data());
        if (rc != KWS_OK) return rc;
        O.b127 = reserve(host, 3 * (size_t)H);
        for (int j = 0; j < 2 * H; ++j) host[O.b127 + j] = gb[j];
        for (int j = 0; j < H; ++j) host[O.b127 + 2 * H + j] = cb[j];
        O.wg = pack_couples(host, gq, K, 4, 2);
        O.wc = pack_couples(host, cq, K, 8, 1);
    }
    std::vector<int8_t> fq((size_t)C * H);
    std::vector<float> fb(C);
    const int rc = kws_octbit_quantize(blob + bl.wfc, H, C, fq.data(), &pk->oct_scale_fc, fb.data());
    if (rc != KWS_OK) return rc;
    pk->oct_b127fc = reserve(host, kws::kMaxClasses);
    for (int c = 0; c < C; ++c) host[pk->oct_b127fc + c] = fb[c];
    pk->oct_wfc = reserve(host, (size_t)8 * 4 * 2 * kws::kMaxClasses);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&host[pk->oct_wfc]);
    for (int n = 0; n < 8; ++n)
        for (int g = 0; g < 4; ++g)
            for (int c = 0; c < kws::kMaxClasses; ++c)
                for (int e = 0; e < 2; ++e) {
                    const int k0 = 16 * n + 4 * g + e;
                    dst[((size_t)(n * 4 + g) * kws::kMaxClasses + c) * 2 + e] =
                        c < C ? pack16(fq[(size_t)c * H + k0], fq[(size_t)c * H + k0 + 2]) : 0u;
                }
    return KWS_OK;
}

}  // namespace

int pack_weights(const kws_config& cfg, const kws_cell_wrappers& wrap, const float* blob, PackedWeights* pk, std::vector<float>* image,
                 int num_classes2) {
    const BlobLayout bl = blob_layout(cfg);
    pack_fp32(cfg, blob, bl, pk, *image);
    if (num_classes2 > 0) {      // fp32 handles without wrappers only (kws_create_heads): the second head follows the canonical blob
        const float* Wfc2 = blob + bl.total;
        pack_dense(Wfc2, Wfc2 + (size_t)cfg.hidden * num_classes2, cfg.hidden, num_classes2, &pk->wfc2_off, &pk->bfc2_off, *image);
    }
    if (wrap.use_layer_norm) {
        // igamma in its natural feature order: lane (g, s) of k-group k4 holds features 16 k4 + 4g + e, which is the mel row's
        // order and the seam's "xl" order alike (kws_internal.h), so the kernel reads igamma[16 k4 + 4g ..] as it is
        const WrapLayout wl = wrap_layout(cfg, wrap);
        for (int l = 0; l < cfg.num_layers; ++l) {
            const LayerDev& L = pk->layers[l];
            const size_t off = reserve(*image, (size_t)4 * L.kcx_gen);
            for (int k = 0; k < L.in_dim; ++k) (*image)[off + k] = blob[wl.igamma[l] + k];
            pk->ln_igamma.push_back(off);
            pk->ln_ibeta.push_back(blob[wl.ibeta[l]]);
        }
    }
    switch (cfg.precision) {
        case KWS_BF16:
        case KWS_F16X3: return pack_a32(cfg, blob, bl, pk, *image);
        case KWS_INT8: return pack_int8(cfg, blob, bl, pk, *image);
        default: return KWS_OK;
    }
}

}  // namespace kws_host
