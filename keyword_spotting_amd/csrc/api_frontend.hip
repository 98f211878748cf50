// C ABI of libkws_amd.so (include/kws_amd.h): the PCM front-end -- mel, power mel and MFCC features.
#include <new>

#include "api_internal.h"

using namespace kws_host;

namespace {

// librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm=1) restated (the reference calls it at
// models/rnn_ctc.py:139-144; librosa itself is not available offline): Slaney mel scale -- linear below 1 kHz
// (200/3 Hz per mel), logarithmic above (step ln(6.4)/27) -- triangular filters, each scaled by 2/(f_hi - f_lo).
constexpr double kPi = 3.14159265358979323846, kTwoPi = 6.283185307179586476925286766559;
const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
double hz_to_mel_slaney(double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp; }
double mel_to_hz_slaney(double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m; }
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
    std::vector<float> d((size_t)n_mel * n_mfcc);
    for (int j = 0; j < n_mel; ++j) {
        const double sample = (2 * j + 1) * kPi / (2.0 * n_mel);
        d[(size_t)j * n_mfcc] = (float)(1.0 / std::sqrt((double)n_mel));
        for (int i = 1; i < n_mfcc; ++i) d[(size_t)j * n_mfcc + i] = (float)(std::cos(i * sample) * std::sqrt(2.0 / n_mel));
    }
    return d;
}

// The table packers below each append one kernel table of `f` to the image, zero filled first, and leave its offset in the handle.

// FrontendParams::dft of frontend_kernels.hip: bins k = 0..N/4 are contracted, each over the even and the odd folded samples
void pack_dft(kws_frontend* f, std::vector<float>& img) {
    const int N = f->cfg.fft_size, NH = N / 2, NQ = N / 4, tiles = f->nf_tiles, KC4 = f->kc4;
    const size_t at = f->dft_off = img.size();
    img.resize(at + (size_t)4 * tiles * KC4 * 64 * 4, 0.f);
    for (int tile = 0; tile < tiles; ++tile)
        for (int a = 0; a < 4; ++a)                      // a = 2 * (cos|sin) + parity of n
            for (int k4 = 0; k4 < KC4; ++k4)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int g = lane >> 4, i = lane & 15, cs = a >> 1, par = a & 1;
                        const int bin = 16 * tile + i, m = 4 * (4 * k4 + e) + g, n = 2 * m + par;
                        float v = 0.f;
                        // cos rows use folded samples 0..N/2, sin rows 1..N/2-1 (sin vanishes at 0 and N/2)
                        if (bin <= NQ && n <= NH && !(cs == 1 && (n == 0 || n == NH))) {
                            const double ang = kTwoPi * (double)(((long long)bin * n) % N) / N;
                            v = (float)(cs == 0 ? std::cos(ang) : std::sin(ang));
                        }
                        img[at + ((((size_t)(4 * tile + a) * KC4 + k4) * 64 + lane) * 4) + e] = v;
                    }
}

// FrontendParams::melw of frontend_kernels.hip: mel basis fragments, xl k map over k = 0..N/4: direct set basis[m][k], mirrored
// set basis[m][N/2 - k] (k < N/4)
void pack_melw(kws_frontend* f, std::vector<float>& img) {
    const int N = f->cfg.fft_size, NF = N / 2 + 1, NH = N / 2, NQ = N / 4, tiles = f->nf_tiles;
    const size_t at = f->melw_off = img.size();
    img.resize(at + (size_t)f->mel_tiles * tiles * 8 * 64, 0.f);
    for (int mt = 0; mt < f->mel_tiles; ++mt)
        for (int t = 0; t < tiles; ++t)
            for (int mir = 0; mir < 2; ++mir)
                for (int e = 0; e < 4; ++e)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int g = lane >> 4, i = lane & 15;
                        const int k = 16 * t + 4 * g + e, m = 16 * mt + i;
                        float v = 0.f;
                        if (m < f->cfg.n_mel) {
                            if (mir == 0 && k <= NQ) v = f->basis[(size_t)m * NF + k];
                            if (mir == 1 && k < NQ) v = f->basis[(size_t)m * NF + (NH - k)];
                        }
                        img[at + ((((size_t)mt * tiles + t) * 2 + mir) * 4 + e) * 64 + lane] = v;
                    }
}

// FrontendParams::dft of fft_frontend.hip, the 16 x 25 real FFT: twiddles W400^{n2 k1} as (cos, sin) [k1 = 1..12][n2 = 0..15],
// stored [6 pairs (k1 = 2i+1, 2i+2)][16 n2][cos, sin, cos, sin]
void pack_fft_tw(kws_frontend* f, std::vector<float>& img) {
    const size_t at = f->fft_tw_off = img.size();
    img.resize(at + 12 * 16 * 2, 0.f);
    for (int k1 = 1; k1 <= 12; ++k1)
        for (int n2 = 0; n2 < 16; ++n2) {
            const double ang = kTwoPi * (double)(n2 * k1) / 400.0;
            const size_t o = at + ((size_t)((k1 - 1) / 2) * 16 + n2) * 4 + 2 * ((k1 - 1) & 1);
            img[o + 0] = (float)std::cos(ang);
            img[o + 1] = (float)std::sin(ang);
        }
}

// FrontendParams::melw and mel_lo/cnt/off of fft_frontend.hip: the mel basis as MFMA A fragments over 4-bin groups (k = g <-> bin
// 4 group + g): per tile of 16 filters only the contiguous run of groups that carry a non-zero weight, padded to a multiple of
// four; bins > 200 are zero rows.
void pack_fft_mel(kws_frontend* f, std::vector<float>& img) {
    const int NF = 201, n_mel = f->cfg.n_mel;
    const size_t at = f->fft_mel_off = img.size();
    int groups_total = 0;
    for (int mt = 0; mt < f->mel_tiles; ++mt) {
        int lo = 51, hi = -1;                       // 51 groups cover bins 0..203
        for (int grp = 0; grp < 51; ++grp)
            for (int b = 4 * grp; b < 4 * grp + 4 && b <= 200; ++b)
                for (int m = 16 * mt; m < 16 * mt + 16 && m < n_mel; ++m)
                    if (f->basis[(size_t)m * NF + b] != 0.f) { lo = std::min(lo, grp); hi = std::max(hi, grp); }
        int cnt = hi >= lo ? hi - lo + 1 : 0;
        if (cnt == 0) lo = 0;
        cnt = (cnt + 3) & ~3;                       // the kernel works in fours: the extra groups carry zero weights and stay
        if (lo + cnt > 52) lo = 52 - cnt;           // inside the 52 groups (208 rows) of the spectrum block
        f->mel_lo[mt] = lo; f->mel_cnt[mt] = cnt; f->mel_off[mt] = groups_total;
        const int stored = std::max(cnt, 24);       // the kernel preloads 24 groups per tile unconditionally (kMelRegs): zero padded
        img.resize(img.size() + (size_t)stored * 64, 0.f);
        for (int e = 0; e < cnt; ++e)                 // [tile][e / 4][lane][e % 4]: four groups' fragments per 16-byte load
            for (int lane = 0; lane < 64; ++lane) {
                const int g = lane >> 4, m = 16 * mt + (lane & 15), b = 4 * (lo + e) + g;
                if (m < n_mel && b <= 200)
                    img[at + (((size_t)(groups_total + e) / 4 * 64) + lane) * 4 + (e & 3)] = f->basis[(size_t)m * NF + b];
            }
        groups_total += stored;
    }
}

// FrontendParams::dct of fft_frontend.hip: D^T as the A operand of the DCT behind the mel MFMAs: the B operand is the mel tile's
// own C image, whose lane (g, f) holds filters 16 tile + 4g + e, so k-chunk e carries filters {4g + e}.  [tile][coefficient
// tile][64 lanes][e]; rows of the padding filters >= n_mel stay zero (those lanes hold -100 dB)
void pack_dct(kws_frontend* f, std::vector<float>& img) {
    const size_t at = f->dct_off = img.size();
    img.resize(at + (size_t)f->mel_tiles * f->dct_tiles * 64 * 4, 0.f);
    for (int mt = 0; mt < f->mel_tiles; ++mt)
        for (int ct = 0; ct < f->dct_tiles; ++ct)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 4; ++e) {
                    const int filt = 16 * mt + 4 * (lane >> 4) + e, c = 16 * ct + (lane & 15);
                    if (filt < f->cfg.n_mel && c < f->n_mfcc)
                        img[at + (((size_t)mt * f->dct_tiles + ct) * 64 + lane) * 4 + e] = f->dct[(size_t)filt * f->n_mfcc + c];
                }
}

// FrontendParams::win of fft_frontend.hip: the periodic Hann window of the dataset's frames, scipy.signal.get_window('hann', 400) as
// librosa.stft builds it: in double, stored as float
void pack_window(kws_frontend* f, std::vector<float>& img) {
    const int N = f->cfg.fft_size;
    f->window.resize(N);
    for (int i = 0; i < N; ++i) f->window[i] = (float)(0.5 - 0.5 * std::cos(kTwoPi * i / N));
    f->win_off = img.size();
    img.insert(img.end(), f->window.begin(), f->window.end());
}

// (the handle's validated cfg / kind / n_mfcc / framing, KWS_FRONTEND_DENSE) -> the device image of every table its kernels launch with, and in the
// handle where each one is: the dense-DFT pair for every frame length, behind it the FFT tables of a 400-sample frame.  Host code only.
std::vector<float> pack_frontend_tables(kws_frontend* f, bool dense400) {
    const kws_frontend_config& c = f->cfg;
    std::vector<float> image;
    f->nf_tiles = f->kc4 = (c.fft_size / 4 + 1 + 15) / 16;
    f->mel_tiles = (c.n_mel + 15) / 16;
    f->basis = slaney_mel_basis(c.samplerate, c.fft_size, c.n_mel, c.fmin, c.fmax);
    pack_dft(f, image);
    pack_melw(f, image);
    if (c.fft_size != 400) return image;
    pack_fft_tw(f, image);
    pack_fft_mel(f, image);
    f->use_fft = !dense400;
    if (f->kind == KWS_FEAT_MFCC) {
        f->dct = dct_basis_f32(f->n_mfcc, c.n_mel);
        f->dct_tiles = (f->n_mfcc + 15) / 16;
        pack_dct(f, image);
    }
    if (f->framing == KWS_FRAMES_DATASET) pack_window(f, image);
    return image;
}

// The checks and the handle behind kws_frontend_create_features and kws_frontend_create_dataset (which has validated framing and
// pre_emphasis on their own): every argument check in front of the device check.
int create_frontend(const kws_feature_config* fcfg, int framing, float pre_emphasis, kws_frontend_handle* out) {
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
    if (framing == KWS_FRAMES_DATASET && (cfg->fft_size != 400 || dense400))
        return fail(KWS_ERR_UNSUPPORTED, "framing=KWS_FRAMES_DATASET needs the 400-point FFT front-end: fft_size=%d%s unsupported (the dense-DFT "
                    "kernel frames as the deploy graph only)", cfg->fft_size, dense400 ? " with KWS_FRONTEND_DENSE=1" : "");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    kws_frontend* f = new (std::nothrow) kws_frontend();
    if (!f) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    f->cfg = *cfg;
    f->kind = fcfg->kind; f->power = mfcc ? 2 : fcfg->power; f->n_mfcc = mfcc ? fcfg->n_mfcc : 0;
    f->framing = framing; f->pre_emphasis = pre_emphasis;
    const std::vector<float> host = pack_frontend_tables(f, dense400);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&f->d_tables), host.size() * sizeof(float));
    if (e != hipSuccess) { delete f; return hip_fail(e, "hipMalloc(frontend tables)"); }
    e = hipMemcpy(f->d_tables, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { hipFree(f->d_tables); delete f; return hip_fail(e, "hipMemcpy(frontend tables)"); }
    live_register(f);
    *out = f;
    return KWS_OK;
}

}  // namespace

namespace kws_host {

bool frontend_takes_fft400(const kws_frontend* h, int B, int T) { return h->use_fft && (long long)B * T < (1LL << 31); }

int frontend_needs_deploy_frames(const char* who) {
    return fail(KWS_ERR_UNSUPPORTED, "%s takes deploy framing only: this front-end has framing=KWS_FRAMES_DATASET (centred frames need the "
                "utterance's end; use kws_frontend_run_lengths)", who);
}

int frontend_needs_fft400(const kws_frontend* h, const char* what) {
    return fail(KWS_ERR_UNSUPPORTED, "%s need the 400-point FFT front-end (fft_size=%d%s)", what, h->cfg.fft_size,
                h->cfg.fft_size == 400 ? ", KWS_FRONTEND_DENSE=1" : "");
}

kws::FrontendParams frontend_params(const kws_frontend* h, bool fft400, int B, int T, const kws::FrontendParams* seed) {
    kws::FrontendParams p = seed ? *seed : kws::FrontendParams{};
    p.dft = h->d_tables + (fft400 ? h->fft_tw_off : h->dft_off);
    p.melw = h->d_tables + (fft400 ? h->fft_mel_off : h->melw_off);
    for (int m = 0; m < 4; ++m) { p.mel_lo[m] = h->mel_lo[m]; p.mel_cnt[m] = h->mel_cnt[m]; p.mel_off[m] = h->mel_off[m]; }
    p.fft = h->cfg.fft_size; p.hop = h->cfg.hop_size; p.n_mel = h->cfg.n_mel;
    p.nf_tiles = h->nf_tiles; p.mel_tiles = h->mel_tiles; p.kc4 = h->kc4; p.B = B; p.T = T;
    p.power = h->power; p.n_mfcc = h->n_mfcc; p.dct_tiles = h->dct_tiles; p.dct = h->n_mfcc ? h->d_tables + h->dct_off : nullptr;
    p.centred = h->framing == KWS_FRAMES_DATASET; p.pre_emphasis = h->pre_emphasis; p.win = p.centred ? h->d_tables + h->win_off : nullptr;
    return p;
}

int frontend_run_impl(kws_frontend_handle h, const float* carry, int n_carry, const float* chunk, int n_chunk, int B, float* mel,
                      void* stream, const kws::FrontendParams* gate) {
    const int n_samples = n_carry + n_chunk;
    const int T = kws_frontend_frames(&h->cfg, n_samples);
    if (B == 0 || T == 0) return KWS_OK;
    if ((!chunk && !(gate && gate->pcm_i16)) || !mel || (n_carry > 0 && !carry)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if ((long long)B * T > (1LL << 36)) return fail(KWS_ERR_UNSUPPORTED, "B*T=%lld frames exceed the grid limit", (long long)B * T);
    const bool fft400 = frontend_takes_fft400(h, B, T);        // beyond its grid a 400-sample handle falls back to the dense kernel
    if (gate && !fft400) return fail(KWS_ERR_UNSUPPORTED, "internal: the gate rides only on the FFT front-end");
    kws::FrontendParams p = frontend_params(h, fft400, B, T, gate);
    p.pcm = chunk; p.carry = n_carry > 0 ? carry : chunk; p.mel = mel; p.n_samples = n_samples; p.n_carry = n_carry;
    if (gate && n_carry == 0) p.carry = gate->next;     // never dereferenced (n_carry == 0), only has to be a float pointer
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return hip_done(fft400 ? kws::launch_mel_fft400(p, B, st) : kws::launch_mel_frontend(p, B, st), "launch mel_frontend");
}

}  // namespace kws_host

extern "C" {

int kws_frontend_frames(const kws_frontend_config* cfg, int n_samples) {
    if (!cfg || cfg->fft_size <= 0 || cfg->hop_size <= 0 || n_samples < cfg->fft_size) return 0;
    return 1 + (n_samples - cfg->fft_size) / cfg->hop_size;
}

int kws_frontend_create(const kws_frontend_config* cfg, kws_frontend_handle* out) {
    if (!cfg) return kws_frontend_create_features(nullptr, out);        // (its null checks, in its order)
    const kws_feature_config fc = {*cfg, KWS_FEAT_MEL, 1, 0};
    return kws_frontend_create_features(&fc, out);
}

size_t kws_sizeof_feature_config(void) { return sizeof(kws_feature_config); }

int kws_frontend_create_features(const kws_feature_config* fcfg, kws_frontend_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!fcfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    return create_frontend(fcfg, KWS_FRAMES_DEPLOY, 0.f, out);
}

size_t kws_sizeof_dataset_config(void) { return sizeof(kws_dataset_config); }

int kws_frontend_create_dataset(const kws_dataset_config* dcfg, kws_frontend_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!dcfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    if (dcfg->framing != KWS_FRAMES_DEPLOY && dcfg->framing != KWS_FRAMES_DATASET)
        return fail(KWS_ERR_INVALID_ARGUMENT, "framing=%d is neither KWS_FRAMES_DEPLOY nor KWS_FRAMES_DATASET", dcfg->framing);
    if (!std::isfinite(dcfg->pre_emphasis) || dcfg->pre_emphasis < 0.f || dcfg->pre_emphasis >= 1.f)
        return fail(KWS_ERR_INVALID_ARGUMENT, "pre_emphasis=%g must be finite and in [0, 1)", (double)dcfg->pre_emphasis);
    if (dcfg->framing == KWS_FRAMES_DEPLOY && dcfg->pre_emphasis != 0.f)
        return fail(KWS_ERR_INVALID_ARGUMENT, "pre_emphasis=%g with framing=KWS_FRAMES_DEPLOY: the deploy graph has no pre-emphasis", (double)dcfg->pre_emphasis);
    return create_frontend(&dcfg->feat, dcfg->framing, dcfg->pre_emphasis, out);
}

int kws_frontend_frames_of(kws_frontend_handle h, int n_samples) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (h->framing != KWS_FRAMES_DATASET) return kws_frontend_frames(&h->cfg, n_samples);
    return n_samples > h->cfg.fft_size / 2 ? 1 + n_samples / h->cfg.hop_size : 0;
}

int kws_frontend_window(kws_frontend_handle h, float* window_host) {
    if (!h || !window_host) return fail(KWS_ERR_INVALID_ARGUMENT, "null argument");
    if (h->framing != KWS_FRAMES_DATASET) return fail(KWS_ERR_INVALID_ARGUMENT, "the front-end has no window: its framing is KWS_FRAMES_DEPLOY");
    memcpy(window_host, h->window.data(), h->window.size() * sizeof(float));
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
    const int T = kws_frontend_frames_of(h, n_max);
    if (B == 0 || T == 0) return KWS_OK;
    if (!pcm || !out) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (!h->use_fft) {
        // (only a magnitude-mel handle gets here: the other kinds are refused at create)
        if (!n_samples) return frontend_run_impl(h, nullptr, 0, pcm, n_max, B, out, stream);
        return frontend_needs_fft400(h, "per-utterance n_samples");
    }
    if (!frontend_takes_fft400(h, B, T)) return fail(KWS_ERR_UNSUPPORTED, "B*T_max=%lld frames exceed the grid limit", (long long)B * T);
    kws::FrontendParams p = frontend_params(h, true, B, T);
    p.pcm = pcm; p.carry = pcm; p.mel = out; p.n_samples = n_max; p.lens = n_samples; p.n_max = n_max;
    return hip_done(kws::launch_features_fft400(p, B, static_cast<hipStream_t>(stream)), "launch features_fft400");
}

int kws_frontend_linear_size(kws_frontend_handle h) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!h->use_fft) return frontend_needs_fft400(h, "the linear spectrum and the noise mix");
    return 201;
}

// Both entry points below decide sizes, then pointers, then the handle's kind: all of it host work, in front of any device call.
int kws_frontend_run_linear(kws_frontend_handle h, const float* pcm, const int32_t* n_samples, int B, int n_max, float* spec,
                            int32_t* frames_out, float* energy_out, void* stream) {
    if (B < 1 || n_max < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_run_linear: B=%d n_max=%d must be positive", B, n_max);
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_run_linear: handle is null");
    if (!pcm || !spec || !frames_out || !energy_out)
        return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_run_linear: null pointer argument (pcm, spec, frames_out and energy_out are required)");
    if (!h->use_fft) return frontend_needs_fft400(h, "kws_frontend_run_linear: the linear spectrum and the noise mix");
    const int T = kws_frontend_frames_of(h, n_max);
    if (T < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_run_linear: n_max=%d samples hold no frame", n_max);
    if (!frontend_takes_fft400(h, B, T)) return fail(KWS_ERR_UNSUPPORTED, "B*T_max=%lld frames exceed the grid limit", (long long)B * T);
    kws::FrontendParams p = frontend_params(h, true, B, T);
    p.pcm = pcm; p.carry = pcm; p.mel = spec; p.n_samples = n_max; p.lens = n_samples; p.n_max = n_max;
    return hip_done(kws::launch_linear_fft400(p, B, frames_out, energy_out, static_cast<hipStream_t>(stream)), "launch linear_fft400");
}

int kws_frontend_augment(kws_frontend_handle h, const float* spec, const int32_t* frames, const float* energy, int B, int T_max,
                         const float* noise_spec, const int32_t* noise_frames, const float* noise_energy, int K, int Tn_max,
                         const int32_t* src, const int32_t* noise, const int32_t* start, const float* gain_db, int R, float* out,
                         void* stream) {
    if (B < 1 || T_max < 1 || K < 1 || Tn_max < 1 || R < 1)
        return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_augment: B=%d T_max=%d K=%d Tn_max=%d R=%d must be positive", B, T_max, K, Tn_max, R);
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_augment: handle is null");
    if (!spec || !frames || !energy || !noise_spec || !noise_frames || !noise_energy)
        return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_augment: null pointer argument (the clean and the noise set are spec, frames and energy each)");
    if (!src || !noise || !start || !gain_db || !out)
        return fail(KWS_ERR_INVALID_ARGUMENT, "kws_frontend_augment: null pointer argument (src, noise, start, gain_db and out are required)");
    if (!h->use_fft) return frontend_needs_fft400(h, "kws_frontend_augment: the linear spectrum and the noise mix");
    // every index of the three sets stays below 2^31 elements' worth of frames (the kernels' 32-bit frame index)
    if ((long long)R * T_max >= (1LL << 31) || (long long)B * T_max >= (1LL << 31) || (long long)K * Tn_max >= (1LL << 31))
        return fail(KWS_ERR_UNSUPPORTED, "kws_frontend_augment: R*T_max, B*T_max and K*Tn_max frames must stay below 2^31");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    kws::FrontendParams p = frontend_params(h, true, R, T_max);
    p.mel = out;
    kws::AugmentRows rows = {frames, noise_frames, energy, noise_energy, src, noise, start, gain_db, B, K, R, T_max, Tn_max, nullptr};
    // the plan travels as one stream-ordered block, released behind the launches that read it
    KWS_HIP(hipMallocAsync(reinterpret_cast<void**>(&rows.plan), (size_t)R * (kws::kPlanInts + 1) * sizeof(int32_t), st));
    const hipError_t e = kws::launch_augment_fft400(p, spec, noise_spec, rows, st);
    (void)hipFreeAsync(rows.plan, st);
    return hip_done(e, "launch augment_fft400");
}

int kws_frontend_run_carry(kws_frontend_handle h, const float* carry, int n_carry, const float* chunk, int n_chunk, int B,
                           float* mel, float* next_carry, int n_next, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (h->framing != KWS_FRAMES_DEPLOY) return frontend_needs_deploy_frames("kws_frontend_run_carry");
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
        KWS_TRY(frontend_run_impl(h, carry, n_carry, chunk, n_chunk, B, mel, stream));
    }
    if (n_next == 0) return KWS_OK;
    return hip_done(kws::launch_carry_tail(carry ? carry : chunk, n_carry, chunk ? chunk : carry, n_chunk, next_carry, n_next, B,
                                           static_cast<hipStream_t>(stream)), "launch carry_tail");
}

}  // extern "C"
