// PCM -> mel front-end of the deploy graph for the reference's frame length, as a real mixed-radix FFT.
//   frames = tf_frame(x, 400, 160)            utils/stft.py:27-81  (no padding, NO window function)
//   linearspec = |rfft(frames, 400)|          models/rnn_ctc.py:137
//   melspec = linearspec @ mel_basis^T        models/rnn_ctc.py:139-149
// (frontend_kernels.hip keeps the dense-DFT kernel for every other frame length.)
// The same transform also serves the reference's other features of whole utterances (kws_frontend_run_lengths; the Utterances tag below):
//   power mel        |rfft|^2 @ mel_basis^T                                          reader.py:267-268
//   MFCC + deltas    10 log10(max(1e-10, |rfft|^2 @ mel_basis^T)) @ dct, [c | d/2 | 0.3 d]    utils/mfcc.py:20-99
// with the log and the DCT fused behind the mel MFMAs (the mel C tile is the DCT's B operand) and the deltas in a second small launch.
// ... and the features the reference's models are trained and validated on (kws_frontend_create_dataset; the DatasetFrames tag below):
//   y = pre_emphasis(x)  (optional)                                                  process_wav.py:38-44,72-73
//   |librosa.stft(y, 400, 160)|: centred frames of the reflect-padded utterance, periodic Hann window    process_wav.py:74-78, server_demo.py:59-82
// in front of the same three epilogues: only the sample load of stage 1 differs.
//
// 400 = 16 x 25, n = 16 n1 + n2, k = k1 + 25 k2 (Cooley-Tukey):
//     X[k1 + 25 k2] = sum_{n2<16} W16^{n2 k2} * ( W400^{n2 k1} * Y_{n2}[k1] ),   Y_{n2}[k1] = sum_{n1<25} x[16 n1 + n2] W25^{n1 k1}
// Stage 1: the 25-point DFT of a REAL decimated sequence, one per lane (lane = (frame j of 4, n2)), as 5 x 5 with
//   n1 = 5a + b, k1 = c + 5d:  Z_b[c] = sum_a x[5a+b] W5^{ac} (real input: c = 0,1,2 suffice),
//   Y[c + 5d] = sum_b W5^{bd} (W25^{bc} Z_b[c]).  Y is Hermitian, so only k1 = 0..12 is kept, and those thirteen come
//   from c in {0,1,2} alone: Y3 = conj Y22, Y4 = conj Y21, Y8 = conj Y17, Y9 = conj Y16.
// Stage 2: for k1 = 0..12 a 16-point complex FFT over n2 (radix 4 x 4) gives X[k1 + 25 k2], k2 = 0..15.  Those 208 values
//   hold every bin 0..200 exactly once: k <= 200 directly, k > 200 as the mirror 400 - k (|X[400-k]| = |X[k]|; the bins of
//   residue 13..24 mod 25), and k1 = 0, k2 >= 9 are duplicates that the mel table zeroes.
// Between the stages the 13 x 16 complex values of a frame cross lanes through LDS (one transpose; a workgroup is 16
// frames).  In stage 2 lane = (g, frame f of 16) takes k1 = 4q + g in pass q (= wave q); the magnitudes return to LDS in BIN
// order, where the mel projection (v_mfma_f32_16x16x4_f32 over 4-bin groups) only touches the blocks of the basis that are
// not all zero.  ~9 kflop per frame on the VALU instead of the 100 kflop of the dense contraction.
// Below: the tags of the kernel's variants, its phases as one function each in calling order, the kernel, its small companions, the launchers.
#include <cstdlib>

#include "gru_device.h"
#include "launch.h"
#include "vad_device.h"

#pragma clang fp contract(off)      // only the fmaf() written below fuse: one fixed instruction sequence per frame (lexical: covers every phase below)

namespace kws {

namespace {

struct c32 { float re, im; };
__device__ __forceinline__ c32 operator+(c32 a, c32 b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ c32 operator-(c32 a, c32 b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ c32 cmul(c32 a, float c, float s) {           // a * (c + i s)
    return {fmaf(-a.im, s, a.re * c), fmaf(a.re, s, a.im * c)};
}
__device__ __forceinline__ c32 conj(c32 a) { return {a.re, -a.im}; }

constexpr float kC1 = 0.30901699437494742f, kC2 = -0.80901699437494742f;   // cos(2 pi/5), cos(4 pi/5)
constexpr float kS1 = 0.95105651629515357f, kS2 = 0.58778525229247313f;    // sin(2 pi/5), sin(4 pi/5)

// 5-point DFT of a real sequence: z0 (real), z1, z2 (z3 = conj z2, z4 = conj z1)
__device__ __forceinline__ void rdft5(float x0, float x1, float x2, float x3, float x4, float& z0, c32& z1, c32& z2) {
    const float sa = x1 + x4, da = x1 - x4, sb = x2 + x3, db = x2 - x3;
    z0 = x0 + sa + sb;
    z1.re = fmaf(kC2, sb, fmaf(kC1, sa, x0));
    z2.re = fmaf(kC1, sb, fmaf(kC2, sa, x0));
    z1.im = fmaf(-kS2, db, -kS1 * da);
    z2.im = fmaf(kS1, db, -kS2 * da);
}
// 5-point DFT of a complex sequence
__device__ __forceinline__ void cdft5(c32 t0, c32 t1, c32 t2, c32 t3, c32 t4, c32& y0, c32& y1, c32& y2, c32& y3, c32& y4) {
    const c32 sa = t1 + t4, da = t1 - t4, sb = t2 + t3, db = t2 - t3;
    y0 = t0 + sa + sb;
    const c32 a1 = {fmaf(kC2, sb.re, fmaf(kC1, sa.re, t0.re)), fmaf(kC2, sb.im, fmaf(kC1, sa.im, t0.im))};
    const c32 a2 = {fmaf(kC1, sb.re, fmaf(kC2, sa.re, t0.re)), fmaf(kC1, sb.im, fmaf(kC2, sa.im, t0.im))};
    const c32 b1 = {fmaf(kS2, db.re, kS1 * da.re), fmaf(kS2, db.im, kS1 * da.im)};
    const c32 b2 = {fmaf(-kS1, db.re, kS2 * da.re), fmaf(-kS1, db.im, kS2 * da.im)};
    // y1 = a1 - i b1, y4 = a1 + i b1, y2 = a2 - i b2, y3 = a2 + i b2
    y1 = {a1.re + b1.im, a1.im - b1.re};
    y4 = {a1.re - b1.im, a1.im + b1.re};
    y2 = {a2.re + b2.im, a2.im - b2.re};
    y3 = {a2.re - b2.im, a2.im + b2.re};
}
// radix-4 butterfly, forward transform (W4 = -i)
__device__ __forceinline__ void bfly4(c32 v0, c32 v1, c32 v2, c32 v3, c32& r0, c32& r1, c32& r2, c32& r3) {
    const c32 e0 = v0 + v2, e1 = v0 - v2, o0 = v1 + v3, o1 = v1 - v3;
    r0 = e0 + o0;
    r2 = e0 - o0;
    r1 = {e1.re + o1.im, e1.im - o1.re};
    r3 = {e1.re - o1.im, e1.im + o1.re};
}

// W25^e = cos - i sin, e = b c for b = 1..4, c = 1,2
constexpr float kW25c[9] = {1.f, 0.96858316112863108f, 0.87630668004386358f, 0.72896862742141155f, 0.53582679497899666f,
                            0.f, 0.06279051952931353f, 0.f, -0.42577929156507272f};
constexpr float kW25s[9] = {0.f, 0.24868988716485479f, 0.48175367410171532f, 0.68454710592868873f, 0.84432792550201508f,
                            0.f, 0.99802672842827156f, 0.f, 0.90482705246601958f};
constexpr float kR2 = 0.70710678118654752f;                                     // 1/sqrt 2
constexpr float kW16c1 = 0.92387953251128674f, kW16s1 = 0.38268343236508977f;   // cos, sin (pi/8)

constexpr int kRowBytes = 128;                 // one (k1, frame) row: 16 complex values over n2
constexpr int kPlaneBytes = 16 * kRowBytes;    // one k1: 16 frames
constexpr int kFftLds = 13 * kPlaneBytes;      // 26,624 B per workgroup: six workgroups per CU
constexpr int kMelRegs = 24;                   // basis fragments (4-bin groups) of a mel tile that wait in registers
constexpr int kSpecRows = 208;                 // spectrum rows (bins 0..200 + zero padding) of 16 frames: 13,312 B of the same space
constexpr int kMaxDctTiles = 2;                // MFCC: coefficient tiles of 16 (n_mfcc <= 32, kws_amd.h); the mel tiles' partial
                                               // products [4 tiles][kMaxDctTiles][64 lanes] float4 sit behind the spectrum
constexpr int kDctPartBytes = 4 * kMaxDctTiles * 64 * 16;
static_assert(kSpecRows * 64 + kDctPartBytes <= kFftLds, "the DCT partials must fit behind the spectrum");

}  // namespace

// MT = mel tiles of 16 filters.  One workgroup = 4 waves = 16 frames of the flattened [B*T] frame index: wave w runs
// stage 1 for frames 4w..4w+3, after the barrier stage 2 for k1 = 4w..4w+3 of all sixteen frames, and the magnitudes go
// back to LDS in BIN order (S[bin][frame]) so that the mel projection only touches the 4-bin x 16-filter blocks whose
// weights are not all zero: filters are contiguous in frequency, so tile m needs one contiguous run of 4-bin groups --
// 52 MFMAs per 16 frames for 40 filters where the dense product takes 156.  Wave m = tile m.
// 26 KiB of LDS per workgroup (the spectrum reuses the transpose planes): six workgroups = 24 waves per CU.
// SampleT: float samples, or int16 PCM as the sound card delivers it (detector.py:40-43,74-79: scaled by 2^-15 on load --
// read once, in place, no widened copy).  GATE: the head of a stream-manager iteration rides along in the same launch: the
// workgroup that transforms a stream's FIRST frame also takes the vad sum of its new samples (the masks silent / reset) and writes
// its next sample carry (detector.py:168-183) -- see gate_streams below.
#ifndef KWS_FE_OCC
#define KWS_FE_OCC 6          // workgroups per CU the register allocation aims at (tools/build_variant.sh -DKWS_FE_OCC=n for A/B)
#endif
// The kernel's variants are tags in place of the sample type: every instantiation keeps the name it was first given.
// RaggedRows<S> (with GATE; kws_stream_feed_ragged): every stream has its own chunk length (p.lens) and carry length (p.carry_len, or
// p.n_carry for all); the grid is B x T frames for the longest possible chunk, and frames past a stream's own count load nothing and
// store zeros.  See stream_gate below for what the gate writes.
template <typename S> struct RaggedRows {};
// Utterances<S, EPI> (without GATE; kws_frontend_run_lengths): B whole utterances in rows of p.n_max samples, utterance b with its own
// sample count (p.lens, null: n_max for all) and so its own frame count T_b <= p.T; frames past T_b load nothing.  EPI picks what
// leaves the kernel (kws_feature_config; utils/mfcc.py:72-99, reader.py:267-268):
//   kEpiMel    |X| -> mel, as the plain instantiations
//   kEpiPower  |X|^2 = re^2 + im^2 (no sqrt) -> mel
//   kEpiMfcc   |X|^2 -> mel -> 10 log10(max(1e-10, .)) -> DCT: the static coefficients [c < n_mfcc] of rows of 3 n_mfcc floats;
//              rows past T_b are zero.  mfcc_delta_kernel below fills the other two thirds of every row.
//   kEpiLinear (kws_frontend_run_linear) the magnitudes themselves, bins 0..200 of every frame as rows of p.mel = spec [B, T, 201] --
//              the block's 16 rows are one contiguous run of the flattened frame index, stored straight from the bin-order spectrum;
//              rows past T_b are the transform of zeros: zero.  No mel tile: instantiated with MT = 1.
constexpr int kEpiMel = 0, kEpiPower = 1, kEpiMfcc = 2, kEpiLinear = 3;
constexpr int kLinearBins = 201;
template <typename S, int EPI> struct Utterances {};
// DatasetFrames<S, EPI, PRE>: Utterances<S, EPI> with the dataset's framing (p.centred; kws_amd.h).
// Frame t of utterance b (n samples) is centred on sample t * hop: tap i reads s = t * hop + i - 200, reflected once at either end
// (s < 0: -s; s >= n: 2 (n - 1) - s -- np.pad(mode='reflect') for n >= 201, the shortest utterance that has frames), times the
// Hann window p.win[i]; T_b = 1 + n / hop.  PRE: the samples pass y[0] = x[0], y[i] = x[i] - fl32(p.pre_emphasis * x[i-1]) first, two
// roundings as numpy's float32 arrays take them.  Frames whose 400 taps and their predecessors all lie inside the utterance -- all
// but the first two and the last two or three -- load as the other instantiations do; the others take the index per tap.
template <typename S, int EPI, bool PRE> struct DatasetFrames {};
// Mixed<EPI> (without GATE; kws_frontend_augment): stages 1 and 2 are replaced by "load the 16 frames x 201 magnitudes of the clean
// rows and of their noise slices, mix, store into the S[bin][frame] planes" (reader.py:238-253); the epilogues follow as they stand,
// on mixed (kEpiMel) or mixed^2 (kEpiPower, kEpiMfcc; reader.py:264-268).  The grid is R x p.T frames; row r is described by its
// PlanRow (kws_internal.h), which augment_plan_kernel below wrote.
template <int EPI> struct Mixed {};

namespace {
template <typename T> struct SampleOf {          // what a tag says about the sample type, the framing and the epilogue
    using type = T;
    static constexpr bool ragged = false, lengths = false, centred = false, pre = false, mixed = false;
    static constexpr int epi = kEpiMel;
};
template <typename S> struct SampleOf<RaggedRows<S>> : SampleOf<S> { static constexpr bool ragged = true; };
template <typename S, int EPI> struct SampleOf<Utterances<S, EPI>> : SampleOf<S> { static constexpr bool lengths = true; static constexpr int epi = EPI; };
template <typename S, int EPI, bool PRE> struct SampleOf<DatasetFrames<S, EPI, PRE>> : SampleOf<Utterances<S, EPI>> { static constexpr bool centred = true, pre = PRE; };
template <int EPI> struct SampleOf<Mixed<EPI>> : SampleOf<Utterances<float, EPI>> { static constexpr bool mixed = true; };
template <typename SampleT> constexpr float kPcmScale = sizeof(SampleT) == 2 ? 1.0f / 32768.0f : 1.0f;      // int16 PCM is scaled by 2^-15 on load
template <typename SampleT> __device__ __forceinline__ const SampleT* pcm_rows(const FrontendParams& p) {
    return sizeof(SampleT) == 2 ? reinterpret_cast<const SampleT*>(p.pcm_i16) : reinterpret_cast<const SampleT*>(p.pcm);
}
// the new samples of stream b: rows of n_max samples on the ragged feed, of the chunk's length in lock step
template <bool RAGGED, typename SampleT> __device__ __forceinline__ const SampleT* stream_row(const FrontendParams& p, const SampleT* rows, int n_chunk, unsigned b) {
    return rows + (size_t)b * (RAGGED ? p.n_max : n_chunk);
}
// The mix's arguments: the clean spectra [B, T, 201], the noise spectra [K, noise_stride frames, 201], the plan [R].  FrontendParams, the
// kernarg of every front-end kernel, has no field for them: they travel in fields the Mixed instantiations do not otherwise read.
// These two functions, and nothing else, know which.
struct MixRows { const float *clean, *noise; int noise_stride; const PlanRow* plan; };
void bind_mix_rows(FrontendParams& q, const MixRows& m) {
    q.pcm = m.clean; q.carry = m.noise; q.carry_stride = m.noise_stride; q.carry_len = reinterpret_cast<const int32_t*>(m.plan);
}
__device__ __forceinline__ MixRows mix_rows(const FrontendParams& p) {
    return {p.pcm, p.carry, p.carry_stride, reinterpret_cast<const PlanRow*>(p.carry_len)};
}
__device__ __forceinline__ int ragged_len(const FrontendParams& p, unsigned b) {      // clamped to [0, n_max] (kws_amd.h)
    const int n = p.lens ? p.lens[b] : p.n_max;
    return n < 0 ? 0 : (n > p.n_max ? p.n_max : n);
}
__device__ __forceinline__ int ragged_carry(const FrontendParams& p, unsigned b) { return p.carry_len ? p.carry_len[b] : p.n_carry; }
// frames of n samples: 1 + n / hop centred ones once half a frame fits, else the whole frames of the deploy graph ...
__device__ __forceinline__ int frames_of(const FrontendParams& p, bool centred, int n) {
    return centred ? (n > p.fft / 2 ? 1 + n / p.hop : 0) : (n < p.fft ? 0 : 1 + (n - p.fft) / p.hop);
}
// ... and of row b of the launch: the kernel knows its framing from its tag (Mixed: the plan says), the kernels around it from p.centred
template <typename Tag> __device__ __forceinline__ int row_frames(const FrontendParams& p, unsigned b) {
    if constexpr (SampleOf<Tag>::mixed) return mix_rows(p).plan[b].frames;
    else return frames_of(p, SampleOf<Tag>::centred, ragged_len(p, b));
}
__device__ __forceinline__ int row_frames(const FrontendParams& p, unsigned b) { return frames_of(p, p.centred != 0, ragged_len(p, b)); }
// ---- block map.  XCD-aware block -> frame-block map.  Workgroups go round-robin over the 8 XCDs (blockIdx % 8), each with its own L2;
// a stream's frames span two or three 16-frame blocks, every frame re-reads 240 samples of its predecessor, and with GATE
// the block of a stream's first frame reads its whole row.  Giving XCD x the CONTIGUOUS run of blocks [x F, (x+1) F),
// F = fft_blocks / 8, keeps all readers of a row behind one L2, so the PCM leaves HBM once (the grid is a multiple of 8).
// The block's first frame is 16 x this; one at or past B * T is a padding block of the rounded-up grid.
__device__ __forceinline__ unsigned frame_block(const FrontendParams& p) {
    const unsigned xcd = blockIdx.x & 7u, seq = blockIdx.x >> 3;       // XCD, position in that XCD's sequence
    const unsigned F = (unsigned)p.fft_blocks >> 3;                   // transform blocks per XCD
    return xcd * F + seq;
}
// ---- gate.  GATE: the stream whose FIRST frame lies in this block gets its vad sum, masks and next carry here.  The row is requested
// before the frames' samples and summed while those are in flight; the four wave totals cross at the transform's own first
// barrier.  block_abs_sum's association term by term (thread t owns groups t, t + 256, ...; shuffle tree; the four wave
// totals pairwise), so kws_vad, the stream manager's gate kernel and this one still take the same decision on the same
// samples.  The transform reads the same row right behind: the PCM leaves HBM once (67 MB per 4096 x 3600-sample launch; gate
// workgroups in front of the transforms pulled each XCD's 7 MB of rows through its 4 MB L2 first: 94-100 MB; round 3: 140).
struct GateRow {      // workgroup-uniform: the stream handled the fast way (none), its chunk and carry lengths; this thread's four groups of its row
    unsigned b = 0xffffffffu;
    int n = 0, nc = 0;
    float v[4][4];
    __device__ __forceinline__ bool taken() const { return b != 0xffffffffu; }
};
// fetch the row, four float4 / short4 groups per thread (n <= 4096, a multiple of 4, the row aligned to a group)
template <typename SampleT> __device__ __forceinline__ void gate_row_fetch(const SampleT* row, int n, int tid, float (&v)[4][4]) {
    const int full = n >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k][e] = 0.f;
        if (i < full) {
            if constexpr (sizeof(SampleT) == 2) {
                const short4 q4 = reinterpret_cast<const short4*>(row)[i];
                v[k][0] = (float)q4.x * kPcmScale<SampleT>; v[k][1] = (float)q4.y * kPcmScale<SampleT>;
                v[k][2] = (float)q4.z * kPcmScale<SampleT>; v[k][3] = (float)q4.w * kPcmScale<SampleT>;
            } else {
                const float4 q4 = reinterpret_cast<const float4*>(row)[i];
                v[k][0] = q4.x; v[k][1] = q4.y; v[k][2] = q4.z; v[k][3] = q4.w;
            }
        }
    }
}
// What the gate writes for stream b once the vad sum of its row is known.  In lock step: the masks and the next carry, the same lengths for
// every stream.  On the ragged feed (detector.py:162-183 for this stream alone): n == 0 skips the iteration -- carry copied through,
// reset 0 (the GRU hands the state back over zero frames), skip set; otherwise the vad masks of its n new samples, the next carry (all
// samples while fewer than 400, else what detector.py:181-182 keeps) and its frame count.
template <bool RAGGED, typename SampleT>
__device__ __forceinline__ void stream_gate(const FrontendParams& p, unsigned b, float vad_sum, int n, int nc, const SampleT* row, int tid) {
    if constexpr (RAGGED) {
        const float* crow = p.carry + (size_t)b * p.carry_stride;
        float* nrow = p.next + (size_t)b * (p.fft - 1);
        const int total = nc + n;
        const int keep = n == 0 || total < p.fft ? total : (total - p.fft) % p.hop + (p.fft - p.hop);
        if (tid == 0) {
            if (n > 0) {
                vad_masks(vad_sum, p.vad_thres, b, p.restart, p.silent, p.reset);
            } else {
                p.silent[b] = 0;
                p.reset[b] = 0;
            }
            p.skip[b] = n == 0 ? 1 : 0;
            p.frames[b] = n == 0 ? 0 : frames_of(p, false, total);
            p.next_len[b] = keep;
        }
        carry_tail<SampleT>(crow, nc, row, n, nrow, keep, tid, 256);
    } else {
        if (tid == 0) vad_masks(vad_sum, p.vad_thres, b, p.restart, p.silent, p.reset);
        carry_tail<SampleT>(p.carry + (size_t)b * p.n_carry, p.n_carry, row, n, p.next + (size_t)b * p.n_next, p.n_next, tid, 256);
    }
}
// Every stream whose first frame lies in this block.  The first of them, if its row is short and aligned enough, goes the fast way:
// its row is only requested here (g), summed behind the tap loads (gate_wave_sum) and gated behind barrier 1.  A second stream
// starting in this block (chunks shorter than 16 frames) and long or unaligned rows are gated on the spot, one after the other; an
// empty ragged chunk has nothing to sum.
template <bool RAGGED, typename SampleT>
__device__ __forceinline__ void gate_streams(const FrontendParams& p, unsigned f0, unsigned total, const SampleT* rows, int n_chunk, int tid, GateRow& g) {
    const unsigned T = (unsigned)p.T;
    const unsigned f_end = f0 + 16u < total ? f0 + 16u : total;
    const unsigned sb0 = (f0 + T - 1u) / T;
    for (unsigned sb = sb0; sb < (unsigned)p.B && sb * T < f_end; ++sb) {
        const int n = RAGGED ? __builtin_amdgcn_readfirstlane(ragged_len(p, sb)) : n_chunk;
        const int nc = RAGGED ? __builtin_amdgcn_readfirstlane(ragged_carry(p, sb)) : p.n_carry;
        const SampleT* row = stream_row<RAGGED>(p, rows, n_chunk, sb);
        if (RAGGED && n == 0) {
            stream_gate<RAGGED, SampleT>(p, sb, 0.f, 0, nc, row, tid);
        } else if (sb == sb0 && n <= 4096 && (n & 3) == 0 && (reinterpret_cast<uintptr_t>(row) & (4 * sizeof(SampleT) - 1)) == 0) {
            g.b = sb; g.n = n; g.nc = nc;
            gate_row_fetch<SampleT>(row, n, tid, g.v);
        } else {
            const float tot = block_abs_sum<SampleT>(row, n, nullptr);
            stream_gate<RAGGED, SampleT>(p, sb, tot, n, nc, row, tid);
            __syncthreads();
        }
    }
}
// the fetched row's |samples|, summed per wave into part[w]
__device__ __forceinline__ void gate_wave_sum(const GateRow& g, int w, int lane, float* part) {
    if (!g.taken()) return;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)      // a thread without group k adds +0: the same bits as not adding
        acc += (fabsf(g.v[k][0]) + fabsf(g.v[k][1])) + (fabsf(g.v[k][2]) + fabsf(g.v[k][3]));
    acc = wave_sum_lane0(acc);
    if (lane == 0) part[w] = acc;
}
// ---- tap load: the lane's 25 taps x[n1] = sample 16 n1 + n2 of its frame, one function per framing; false: a dead frame, nothing loaded
// the frame's samples lie in one array: src points at tap 0
template <typename SampleT> __device__ __forceinline__ void taps_from(const SampleT* src, float (&x)[25]) {
#pragma unroll
    for (int n1 = 0; n1 < 25; ++n1) x[n1] = (float)src[16 * n1] * kPcmScale<SampleT>;
}
// the frame may straddle the seam between the nc carried samples and the new ones: per-sample select
template <typename SampleT> __device__ __forceinline__ void taps_across(const float* carry, int nc, const SampleT* chunk, int s0, float (&x)[25]) {
#pragma unroll
    for (int n1 = 0; n1 < 25; ++n1) {
        const int idx = s0 + 16 * n1;
        x[n1] = idx < nc ? carry[idx] : (float)chunk[idx - nc] * kPcmScale<SampleT>;
    }
}
// lock step: the signal of stream sb is carry[sb] (n_carry samples, may be 0) followed by pcm[sb] (detector.py:179)
template <typename SampleT>
__device__ __forceinline__ bool taps_lockstep(const FrontendParams& p, const SampleT* rows, int n_chunk, unsigned sb, int st, int n2, float (&x)[25]) {
    const float* xc_ = p.carry + (size_t)sb * p.n_carry;
    const SampleT* xp_ = stream_row<false>(p, rows, n_chunk, sb);
    const int s0 = st * p.hop + n2;
    const bool seam = s0 - n2 < p.n_carry && s0 - n2 + 400 > p.n_carry;
    const unsigned long long any_seam = __builtin_amdgcn_ballot_w64(seam);
    const unsigned long long any_carry = __builtin_amdgcn_ballot_w64(s0 - n2 < p.n_carry);
    if (!any_carry) {
        // every frame of this wave lies in the new samples (all but the first rounds of a chunk)
        taps_from(xp_ + (s0 - p.n_carry), x);
    } else if (!any_seam && sizeof(SampleT) == 4) {
        // whole frames, some in the carried samples, some in the new ones; one float array each
        taps_from(s0 - n2 >= p.n_carry ? reinterpret_cast<const float*>(xp_) + (s0 - p.n_carry) : xc_ + s0, x);
    } else {
        // some frame of this wave straddles the seam (the first two or three frames of a chunk)
        taps_across(xc_, p.n_carry, xp_, s0, x);
    }
    return true;
}
// ragged feed: stream sb's carry row (nc samples) followed by its n new samples; frames past its own count are dead
template <typename SampleT> __device__ __forceinline__ bool taps_ragged(const FrontendParams& p, const SampleT* rows, unsigned sb, int st, int n2, float (&x)[25]) {
    const int s0 = st * p.hop + n2;
    const int n = ragged_len(p, sb), nc = ragged_carry(p, sb);
    const bool live = n > 0 && st < frames_of(p, false, nc + n);
    const float* xc_ = p.carry + (size_t)sb * p.carry_stride;
    const SampleT* xp_ = stream_row<true>(p, rows, 0, sb);
    const unsigned long long any_carry = __builtin_amdgcn_ballot_w64(live && s0 - n2 < nc);
    if (!live) return false;
    if (!any_carry) taps_from(xp_ + (s0 - nc), x);
    else taps_across(xc_, nc, xp_, s0, x);
    return true;
}
// Centred: frame st of utterance sb spans samples [s0, s0 + 400) of its reflected signal, under the window.  An interior frame (and,
// for PRE, the sample in front of it) lies inside [0, n); a wave of interior frames loads as Utterances does, one with an edge frame
// -- decided by ballot, as the seam path above -- takes the reflected index per tap.  Same operations on the same samples either
// way: a frame's bits do not depend on its neighbours in the wave.
template <typename Tag> __device__ __forceinline__ bool taps_centred(const FrontendParams& p, const float* rows, unsigned sb, int st, int n2, float (&x)[25]) {
    constexpr bool PRE = SampleOf<Tag>::pre;
    const float pre = p.pre_emphasis;
    const int n = ragged_len(p, sb);
    const bool live = st < row_frames<Tag>(p, sb);
    const int s0 = st * p.hop - 200;
    const unsigned long long any_edge = __builtin_amdgcn_ballot_w64(live && (s0 < 1 || s0 + 400 > n));
    const float* row = rows + (size_t)sb * p.n_max;
    if (!live) return false;
    // The window: 25 registers from here on.  PRE multiplies in the path -- its edge path has no registers to spare and takes each value
    // with its tap; without PRE the 25 products stand once behind both paths (as two copies the edge path spills).
    const float* wtab = p.win + n2;
    float win[25];
    if (!PRE || !any_edge) {
#pragma unroll
        for (int n1 = 0; n1 < 25; ++n1) win[n1] = wtab[16 * n1];
    }
    if (!any_edge) {
        const float* src = row + (s0 + n2);
#pragma unroll
        for (int n1 = 0; n1 < 25; ++n1) {
            float t = src[16 * n1];
            if constexpr (PRE) t = t - pre * src[16 * n1 - 1];
            x[n1] = PRE ? t * win[n1] : t;
        }
    } else {
#pragma unroll
        for (int n1 = 0; n1 < 25; ++n1) {
            int s = s0 + n2 + 16 * n1;                  // n >= 201: one reflection at most, then 0 <= s < n
            s = s < 0 ? -s : s;
            s = s >= n ? 2 * (n - 1) - s : s;
            float t = row[s];
            if constexpr (PRE) {
                const float pred = pre * row[s > 0 ? s - 1 : 0];
                t = s > 0 ? t - pred : t;
            }
            x[n1] = PRE ? t * wtab[16 * n1] : t;
            // the rare path: five taps' loads in flight at a time, not 25 addresses (the register budget of six workgroups per CU)
            if (n1 % 5 == 4) __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (!PRE) {
#pragma unroll
        for (int n1 = 0; n1 < 25; ++n1) x[n1] = x[n1] * win[n1];
    }
    return true;
}
// Frame f of the block -> its stream and frame in it, the framing the tag names, zeros for a dead frame.
template <typename Tag, typename SampleT>
__device__ __forceinline__ void frame_taps(const FrontendParams& p, const SampleT* rows, int n_chunk, unsigned f0, unsigned total, int f, int n2, float (&x)[25]) {
    using V = SampleOf<Tag>;
    unsigned fidx = f0 + f;
    fidx = fidx < total ? fidx : total - 1;         // frames past the end redo the last one (finite values, never stored)
    const unsigned sb = fidx / (unsigned)p.T;
    const int st = (int)(fidx - sb * (unsigned)p.T);
    bool live;
    if constexpr (V::centred) {
        static_assert(sizeof(SampleT) == 4, "the dataset's utterances are float PCM");
        live = taps_centred<Tag>(p, rows, sb, st, n2, x);
    } else if constexpr (V::lengths) {        // whole utterance sb: the first n samples of its row; a live frame (st < T_b) ends before sample n
        live = st < row_frames<Tag>(p, sb);
        if (live) taps_from(rows + (size_t)sb * p.n_max + (st * p.hop + n2), x);
    } else if constexpr (V::ragged) {
        live = taps_ragged(p, rows, sb, st, n2, x);
    } else {
        live = taps_lockstep(p, rows, n_chunk, sb, st, n2, x);
    }
    if (!live) {
#pragma unroll
        for (int n1 = 0; n1 < 25; ++n1) x[n1] = 0.f;
    }
}
// ---- transform.  W400^{n2 k1}, k1 = 1..12, for this lane's n2: table [6 pairs of k1][16 n2] float4 = (cos, sin) of k1 = 2i+1 and 2i+2
__device__ __forceinline__ void load_twiddles(const FrontendParams& p, int n2, float2 (&tw)[12]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const f32x4 t = reinterpret_cast<const f32x4*>(p.dft)[k * 16 + n2];
        tw[2 * k] = make_float2(t[0], t[1]);
        tw[2 * k + 1] = make_float2(t[2], t[3]);
    }
}
// Stage 1 of frame f, column n2: the 25-point DFT of the lane's real taps, twiddled and parked in the planes
__device__ __forceinline__ void dft25_to_planes(const float (&x)[25], const float2 (&tw)[12], char* lds, int f, int n2) {
    // Z_b[c] = sum_a x[5a + b] W5^{ac}
    float z0[5];
    c32 z1[5], z2[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) rdft5(x[b], x[5 + b], x[10 + b], x[15 + b], x[20 + b], z0[b], z1[b], z2[b]);
    c32 Y[13];
    {   // c = 0: real inputs again
        float y0;
        rdft5(z0[0], z0[1], z0[2], z0[3], z0[4], y0, Y[5], Y[10]);
        Y[0] = {y0, 0.f};
    }
    {   // c = 1: Y1, Y6, Y11, Y16, Y21
        c32 y16, y21;
        cdft5(z1[0], cmul(z1[1], kW25c[1], -kW25s[1]), cmul(z1[2], kW25c[2], -kW25s[2]), cmul(z1[3], kW25c[3], -kW25s[3]),
              cmul(z1[4], kW25c[4], -kW25s[4]), Y[1], Y[6], Y[11], y16, y21);
        Y[9] = conj(y16);
        Y[4] = conj(y21);
    }
    {   // c = 2: Y2, Y7, Y12, Y17, Y22
        c32 y17, y22;
        cdft5(z2[0], cmul(z2[1], kW25c[2], -kW25s[2]), cmul(z2[2], kW25c[4], -kW25s[4]), cmul(z2[3], kW25c[6], -kW25s[6]),
              cmul(z2[4], kW25c[8], -kW25s[8]), Y[2], Y[7], Y[12], y17, y22);
        Y[8] = conj(y17);
        Y[3] = conj(y22);
    }
    // twiddle W400^{n2 k1} and park the row: plane k1, row f, column n2 ^ (f & 14) (the swizzle that makes the
    // stage-2 ds_read_b128 of sixteen different rows conflict-free)
    char* dst = lds + f * kRowBytes + ((n2 ^ (f & 14)) << 3);
    *reinterpret_cast<float2*>(dst) = make_float2(Y[0].re, Y[0].im);
#pragma unroll
    for (int k1 = 1; k1 < 13; ++k1) {
        const c32 t = cmul(Y[k1], tw[k1 - 1].x, -tw[k1 - 1].y);
        *reinterpret_cast<float2*>(dst + k1 * kPlaneBytes) = make_float2(t.re, t.im);
    }
}
// Stage 2: the 16-point FFT over n2 of row f of plane k1 (n2 = 4a + b, k2 = c + 4d) -> o[k2] = X[k1 + 25 k2]
__device__ __forceinline__ void fft16_plane_row(const char* lds, int k1, int f, c32 (&o)[16]) {
    const int sf = (f >> 1) & 7;
    const char* row = lds + k1 * kPlaneBytes + f * kRowBytes;
    c32 z[16];
#pragma unroll
    for (int pr = 0; pr < 8; ++pr) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + ((pr ^ sf) << 4));
        z[2 * pr] = {v[0], v[1]};
        z[2 * pr + 1] = {v[2], v[3]};
    }
    c32 u[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) bfly4(z[b], z[4 + b], z[8 + b], z[12 + b], u[b][0], u[b][1], u[b][2], u[b][3]);
    bfly4(u[0][0], u[1][0], u[2][0], u[3][0], o[0], o[4], o[8], o[12]);
    {   // c = 1: W16^1, W16^2, W16^3
        const c32 v1 = cmul(u[1][1], kW16c1, -kW16s1);
        const c32 v2 = {(u[2][1].re + u[2][1].im) * kR2, (u[2][1].im - u[2][1].re) * kR2};
        const c32 v3 = cmul(u[3][1], kW16s1, -kW16c1);
        bfly4(u[0][1], v1, v2, v3, o[1], o[5], o[9], o[13]);
    }
    {   // c = 2: W16^2, W16^4 = -i, W16^6
        const c32 v1 = {(u[1][2].re + u[1][2].im) * kR2, (u[1][2].im - u[1][2].re) * kR2};
        const c32 v2 = {u[2][2].im, -u[2][2].re};
        const c32 v3 = {(u[3][2].im - u[3][2].re) * kR2, -(u[3][2].re + u[3][2].im) * kR2};
        bfly4(u[0][2], v1, v2, v3, o[2], o[6], o[10], o[14]);
    }
    {   // c = 3: W16^3, W16^6, W16^9 = -W16^1
        const c32 v1 = cmul(u[1][3], kW16s1, -kW16c1);
        const c32 v2 = {(u[2][3].im - u[2][3].re) * kR2, -(u[2][3].re + u[2][3].im) * kR2};
        const c32 v3 = cmul(u[3][3], -kW16c1, kW16s1);
        bfly4(u[0][3], v1, v2, v3, o[3], o[7], o[11], o[15]);
    }
}
// |X| for the magnitude epilogues, |X|^2 (utils/mfcc.py:77: the power spectrum itself, no sqrt) for the others
template <int EPI> __device__ __forceinline__ void spectrum_values(const c32 (&o)[16], float (&mag)[16]) {
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
        const float pw = fmaf(o[k2].re, o[k2].re, o[k2].im * o[k2].im);
        mag[k2] = EPI == kEpiMel || EPI == kEpiLinear ? __builtin_amdgcn_sqrtf(pw) : pw;
    }
}
// the padding rows of the bin-order spectrum that the last 4-bin group may read
__device__ __forceinline__ void zero_spectrum_padding(float* S, int tid) {
    if (tid < 16 * (kSpecRows - 201)) S[201 * 16 + tid] = 0.f;
}
// The values of (k1, frame f) in bin order: S[bin][frame], 64 B rows.  bin = k1 + 25 k2 folded at 200
__device__ __forceinline__ void spectrum_store(const float (&mag)[16], int k1, int f, int tid, float* S) {
    if (k1 <= 12) {
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) S[(k1 + 25 * k2) * 16 + f] = mag[k2];
        if (k1 == 0) {
            S[200 * 16 + f] = mag[8];
        } else {
#pragma unroll
            for (int k2 = 8; k2 < 16; ++k2) S[(400 - 25 * k2 - k1) * 16 + f] = mag[k2];
        }
    }
    zero_spectrum_padding(S, tid);
}
// ---- mix, the Mixed input stage in place of the transform.  The block's 16 frames lie in one row of the call or straddle several (p.T < 16: up to 16).  Lanes 0..15 of wave 0 read
// their frame's row plan and park where its 201 clean magnitudes and its noise slice's begin (-1: none) behind the
// spectrum and the DCT partials; then element i = 201 f + bin of the block goes to thread i % 256: consecutive lanes read
// consecutive floats of a row (a row is 804 contiguous bytes in both sets), whatever the plan says.
template <int EPI> __device__ __forceinline__ void mix_to_spectrum(const FrontendParams& p, const MixRows rows, unsigned f0, unsigned total, int tid, float* __restrict__ S, char* __restrict__ park) {
    typedef long long i64x2 __attribute__((ext_vector_type(2)));                            // where a frame's clean and noise rows begin (-1: none):
    i64x2* at = reinterpret_cast<i64x2*>(park);                                                        // [16], one 16-byte read per element
    float* fac = reinterpret_cast<float*>(at + 16);                                         // [16]
    if (tid < 16) {
        const unsigned fo = f0 + tid;
        long long ca = -1, na = -1;
        float fc = 0.f;
        if (fo < total) {
            const unsigned r = fo / (unsigned)p.T;
            const int t = (int)(fo - r * (unsigned)p.T);
            const PlanRow& plan = rows.plan[r];
            const int b = plan.src, k = plan.noise;
            if (b >= 0 && t < plan.frames) {
                ca = ((long long)b * p.T + t) * kLinearBins;
                if (k >= 0 && t < plan.noise_avail) {
                    na = ((long long)k * rows.noise_stride + plan.start + t) * kLinearBins;
                    fc = __int_as_float(plan.factor_bits);
                }
            }
        }
        at[tid] = i64x2{ca, na}; fac[tid] = fc;
    }
    zero_spectrum_padding(S, tid);
    lds_barrier();
#pragma unroll
    for (int j = 0; j < (16 * kLinearBins + 255) / 256; ++j) {
        const int i = tid + 256 * j;
        if (i < 16 * kLinearBins) {
            const int fr = i / kLinearBins, bin = i - fr * kLinearBins;
            const i64x2 a = at[fr];
            const long long ca = a[0], na = a[1];
            float v = 0.f;
            if (ca >= 0) {
                v = rows.clean[ca + bin];
                if (na >= 0) v = v + fac[fr] * rows.noise[na + bin];   // reader.py:238,252: two roundings (contraction is off)
            }
            S[bin * 16 + fr] = EPI == kEpiMel ? v : v * v;         // reader.py:267-268, utils/mfcc.py:77
        }
    }
}
// ---- epilogues.  kEpiLinear: the 16 rows of this block are elements [201 f0, 201 (f0 + 16)) of spec: consecutive lanes store consecutive floats
__device__ __forceinline__ void linear_rows_store(const FrontendParams& p, const float* S, unsigned f0, unsigned total, int tid) {
    float* out = p.mel + (size_t)f0 * kLinearBins;
    const unsigned left = total - f0;
    const int count = kLinearBins * (int)(left < 16u ? left : 16u);
    for (int i = tid; i < count; i += 256) {
        const int fr = i / kLinearBins, bin = i - fr * kLinearBins;
        out[i] = S[bin * 16 + fr];
    }
}
// Basis fragments of wave w's mel tile: the first kMelRegs groups of its run wait in registers (the loads fly while the spectrum is
// written and the workgroup meets at the barrier); a longer run streams the rest
struct MelTile {             // first 4-bin group and number of groups (multiple of 4; zero-padded table); the table [tile][group / 4][64 lanes]
    int lo4, n;              // float4 (the fragments of four consecutive groups side by side); the fragments in registers
    const f32x4* A;
    float a[kMelRegs];
};
template <int MT, int EPI> __device__ __forceinline__ void mel_tile_fetch(const FrontendParams& p, int w, int lane, MelTile& t) {
    t.lo4 = w < MT ? p.mel_lo[w] : 0;
    t.n = EPI != kEpiLinear && w < MT ? p.mel_cnt[w] : 0;
    t.A = reinterpret_cast<const f32x4*>(p.melw) + ((size_t)(w < MT ? p.mel_off[w] : 0) / 4 * 64 + lane);
    if (t.n > 0) {         // every tile's table holds at least kMelRegs groups (zero padded): no clamping, one base + immediate offsets
#pragma unroll
        for (int e4 = 0; e4 < kMelRegs / 4; ++e4) {
            const f32x4 v = t.A[e4 * 64];
            t.a[4 * e4] = v[0]; t.a[4 * e4 + 1] = v[1]; t.a[4 * e4 + 2] = v[2]; t.a[4 * e4 + 3] = v[3];
        }
    }
}
// Mel projection: wave m = mel tile m over its contiguous run of 4-bin groups.  A = basis fragments [tile][group][64 lanes],
// B = four spectrum rows (k = g) x 16 frames; two accumulators break the dependent chain.  D[filter 16w + 4g + e][frame f]
__device__ __forceinline__ f32x4 mel_project(const MelTile& t, const float* S, int lane) {
    const float* Sg = S + t.lo4 * 64 + lane;
    f32x4 acc0 = splat4(0.f), acc1 = splat4(0.f);
    // runs are padded to multiples of four groups: four spectrum reads in flight, then four MFMAs
    static_for<0, kMelRegs / 4>([&](auto c) {
        constexpr int e0 = 4 * decltype(c)::value;
        if (e0 < t.n) {
            const float b0 = Sg[e0 * 64], b1 = Sg[(e0 + 1) * 64], b2 = Sg[(e0 + 2) * 64], b3 = Sg[(e0 + 3) * 64];
            acc0 = mfma4(t.a[e0], b0, acc0);
            acc1 = mfma4(t.a[e0 + 1], b1, acc1);
            acc0 = mfma4(t.a[e0 + 2], b2, acc0);
            acc1 = mfma4(t.a[e0 + 3], b3, acc1);
        }
    });
    for (int e = kMelRegs; e < t.n; e += 4) {
        const float b0 = Sg[e * 64], b1 = Sg[(e + 1) * 64], b2 = Sg[(e + 2) * 64], b3 = Sg[(e + 3) * 64];
        const f32x4 v = t.A[(size_t)(e / 4) * 64];
        acc0 = mfma4(v[0], b0, acc0);
        acc1 = mfma4(v[1], b1, acc1);
        acc0 = mfma4(v[2], b2, acc0);
        acc1 = mfma4(v[3], b3, acc1);
    }
    return acc0 + acc1;
}
// filters 16w + 4g .. + 3 of frame fo: one 16-byte store where rows keep that alignment, else filter by filter
__device__ __forceinline__ void mel_row_store(const FrontendParams& p, f32x4 r, unsigned fo, int w, int g) {
    float* out = p.mel + (size_t)fo * p.n_mel;
    const int c0 = 16 * w + 4 * g;
    if ((p.n_mel & 3) == 0 && (reinterpret_cast<uintptr_t>(p.mel) & 15) == 0) {
        if (c0 < p.n_mel) *reinterpret_cast<f32x4*>(out + c0) = r;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + e < p.n_mel) out[c0 + e] = r[e];
    }
}
// kEpiMfcc: the mel C tile r is also the B operand of the DCT (k = g <-> filter 16w + 4g + e in k-chunk e), as the GRU kernels'
// exchange layout: S = 10 log10(max(1e-10, mel)) (utils/mfcc.py:23; v_log_f32 is log2, operands >= 1e-10: no
// denormals) goes straight back into the matrix pipe against D^T packed the same way (p.dct: [tile][coefficient
// tile][64 lanes] float4 over e; rows of filters >= n_mel are zero -- those lanes hold log(floor) = -100 dB, not 0).
// The tiles' partial products meet in the half of LDS the spectrum does not use.
__device__ __forceinline__ void mfcc_partials(const FrontendParams& p, f32x4 r, int w, int lane, char* lds) {
    constexpr float kDbPerLog2 = 3.0102999566398120f;           // 10 log10(2)
    float s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = __builtin_amdgcn_logf(fmaxf(r[e], 1e-10f)) * kDbPerLog2;
    f32x4* part = reinterpret_cast<f32x4*>(lds + kSpecRows * 64);
    for (int ct = 0; ct < p.dct_tiles; ++ct) {
        const f32x4 d = reinterpret_cast<const f32x4*>(p.dct)[(size_t)(w * p.dct_tiles + ct) * 64 + lane];
        f32x4 c0 = splat4(0.f), c1 = splat4(0.f);
        c0 = mfma4(d[0], s[0], c0);
        c1 = mfma4(d[1], s[1], c1);
        c0 = mfma4(d[2], s[2], c0);
        c1 = mfma4(d[3], s[3], c1);
        part[(w * kMaxDctTiles + ct) * 64 + lane] = c0 + c1;
    }
}
// ... and wave ct adds the tiles' partial products, always in tile order, and stores coefficients 16 ct + 4g + e of frame f:
// the static third of the row, zero for a frame past its row's own count
template <int MT, typename Tag> __device__ __forceinline__ void mfcc_reduce_store(const FrontendParams& p, unsigned f0, unsigned total, int w, int lane, const char* lds) {
    if (w >= p.dct_tiles) return;
    const int g = lane >> 4, f = lane & 15;
    const f32x4* part = reinterpret_cast<const f32x4*>(lds + kSpecRows * 64);
    f32x4 c = part[w * 64 + lane];
#pragma unroll
    for (int m = 1; m < MT; ++m) c = c + part[(m * kMaxDctTiles + w) * 64 + lane];
    const unsigned fo = f0 + f;
    if (fo < total) {
        const unsigned sb = fo / (unsigned)p.T;
        const bool live = (int)(fo - sb * (unsigned)p.T) < row_frames<Tag>(p, sb);
        float* out = p.mel + (size_t)fo * (3 * p.n_mfcc);
        const int c0 = 16 * w + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + e < p.n_mfcc) out[c0 + e] = live ? c[e] : 0.f;
    }
}
}  // namespace

// kEpiLinear aims at one workgroup per CU fewer: it is bound by its stores (804 B per frame against 160 B of mel), and with the 96
// registers of five workgroups the pre-emphasis edge path keeps its 25 taps, window values and predecessors without scratch
constexpr int fe_occupancy(int epi) { return epi == kEpiLinear && KWS_FE_OCC > 1 ? KWS_FE_OCC - 1 : KWS_FE_OCC; }
#ifdef KWS_FE_TIMING       // tools/ubench/fe_phases.hip: s_memtime at the phase boundaries of every wave
#define KWS_FE_STAMP(i) do { if (lane == 0) p.timing[((size_t)blk * 4 + w) * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define KWS_FE_STAMP(i) do {} while (0)
#endif
template <int MT, typename SampleTag, bool GATE>
__global__ void __launch_bounds__(256, fe_occupancy(SampleOf<SampleTag>::epi)) mel_fft400_kernel(const FrontendParams p) {
    using V = SampleOf<SampleTag>;
    using SampleT = typename V::type;
    constexpr int EPI = V::epi;
    static_assert(!V::mixed || EPI != kEpiLinear, "the mix feeds the feature epilogues");
    static_assert(GATE || !V::ragged, "the ragged feed always carries the gate");
    static_assert(!(GATE && V::lengths), "whole utterances have no stream gate");
    __shared__ __attribute__((aligned(16))) char lds[kFftLds];
    __shared__ float gate_part[4];
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int hi = lane >> 4, lo = lane & 15;          // stage 1: (frame j of 4, n2); stage 2 / MFMA: (g, frame f of 16)
    const unsigned total = (unsigned)p.B * (unsigned)p.T;
    const SampleT* rows = pcm_rows<SampleT>(p);
    const int n_chunk = p.n_samples - p.n_carry;
    const unsigned blk = frame_block(p), f0 = blk * 16u;
    if (f0 >= total) return;                            // padding block (uniform: before any barrier)
    KWS_FE_STAMP(0);
    GateRow gate;
    if constexpr (GATE) gate_streams<V::ragged>(p, f0, total, rows, n_chunk, tid, gate);
    float mag[16];
    if constexpr (!V::mixed) {          // stage 1: this wave's four frames
        float x[25];
        float2 tw[12];
        frame_taps<SampleTag>(p, rows, n_chunk, f0, total, 4 * w + hi, lo, x);
        load_twiddles(p, lo, tw);
#ifdef KWS_FE_TIMING
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        KWS_FE_STAMP(1);
#endif
        if constexpr (GATE) gate_wave_sum(gate, w, lane, gate_part);
        dft25_to_planes(x, tw, lds, 4 * w + hi, lo);
    }
    KWS_FE_STAMP(2);
    if constexpr (!V::mixed) __syncthreads();
    KWS_FE_STAMP(3);
    if (GATE && gate.taken())           // the four wave totals have met
        stream_gate<V::ragged>(p, gate.b, (gate_part[0] + gate_part[1]) + (gate_part[2] + gate_part[3]), V::ragged ? gate.n : n_chunk, gate.nc,
                               stream_row<V::ragged>(p, rows, n_chunk, gate.b), tid);
    if constexpr (!V::mixed) {          // stage 2: pass q = w, k1 = 4w + g; lanes past k1 = 12 recompute plane 12 and store nothing
        c32 o[16];
        fft16_plane_row(lds, 4 * w + hi < 12 ? 4 * w + hi : 12, lo, o);
        spectrum_values<EPI>(o, mag);
    }
    MelTile tile;
    mel_tile_fetch<MT, EPI>(p, w, lane, tile);
    KWS_FE_STAMP(4);
    if constexpr (!V::mixed) lds_barrier();             // every wave has read its planes: the spectrum takes their place
    KWS_FE_STAMP(5);
    float* S = reinterpret_cast<float*>(lds);
    if constexpr (V::mixed) mix_to_spectrum<EPI>(p, mix_rows(p), f0, total, tid, S, lds + kSpecRows * 64 + kDctPartBytes);   // parked behind the spectrum and the DCT partials
    else spectrum_store(mag, 4 * w + hi, lo, tid, S);
    lds_barrier();
    KWS_FE_STAMP(6);
    if constexpr (EPI == kEpiLinear) {
        linear_rows_store(p, S, f0, total, tid);
        return;
    }
    const bool project = EPI == kEpiMfcc ? w < MT : tile.n > 0;      // kEpiMfcc: every tile takes part in the DCT, one without a weight with mel = 0
#ifdef KWS_ABL_NOMEL          // experiment builds only (tools/build_variant.sh nomel -DKWS_ABL_NOMEL): the kernel without its mel projection
    if (project && p.n_mel < 0) {
#else
    if (project) {
#endif
        const f32x4 r = mel_project(tile, S, lane);
        if constexpr (EPI == kEpiMfcc) mfcc_partials(p, r, w, lane, lds);
        else if (f0 + lo < total) mel_row_store(p, r, f0 + lo, w, hi);
    }
    if constexpr (EPI == kEpiMfcc) {
        lds_barrier();
        mfcc_reduce_store<MT, SampleTag>(p, f0, total, w, lane, lds);
    }
    KWS_FE_STAMP(7);
}

// The energies behind the kEpiLinear launch (kws_frontend_run_linear): energy[b] = sum_{t < T_b} sum_f spec[b, t, f]^2, what the
// reader's compute_db sums (reader.py:325-332).  One workgroup per utterance, so the value cannot depend on the rest of the batch.
// A frame: lane l adds the squares of bins l, l + 64, l + 128, l + 192 in that order, then the xor butterfly over the 64 lanes -- float32,
// one fixed tree.  The frames: wave w adds frames w, w + 4, ... in that order in float64, the four waves meet as (0 + 1) + (2 + 3), and
// the sum is rounded to float32 once.  The spectrum was written by the launch in front and comes back out of L2.
__global__ void __launch_bounds__(256) linear_energy_kernel(const FrontendParams p, int32_t* frames_out, float* energy_out) {
    __shared__ double part[4];
    const unsigned b = blockIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tb = row_frames(p, b);      // <= p.T: n <= n_max
    const float* rows = p.mel + (size_t)b * p.T * kLinearBins;
    double sum = 0.0;
    for (int t = w; t < tb; t += 4) {
        const float* row = rows + (size_t)t * kLinearBins;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int bin = lane + 64 * j;
            const float v = bin < kLinearBins ? row[bin] : 0.f;
            acc = fmaf(v, v, acc);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
        sum += (double)acc;
    }
    if (lane == 0) part[w] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        energy_out[b] = (float)((part[0] + part[1]) + (part[2] + part[3]));
        frames_out[b] = tb;
    }
}

// The rows of kws_frontend_augment -> the plan the Mixed launch reads (kws_internal.h) and the sample counts mfcc_delta_kernel takes
// its edges from.  Every edge case of the device-side arrays is decided here, once per row (kws_amd.h lists them); what leaves is in
// range: b and k index their sets or are -1, start + (frames from start on) <= Tn, T_r <= T.
//   factor = 10^((db_a - db_n + gain) / 20), db(E, n) = 10 log10(E / fft^2 / n)  (reader.py:226-234,325-332)
//          = sqrt((E_a / n_a) / (E_n / n_n)) 10^(gain / 20) in double, rounded to float once
__global__ void __launch_bounds__(256) augment_plan_kernel(const AugmentRows a, int fft, int hop, int centred) {
    const int r = (int)(blockIdx.x * 256u + threadIdx.x);
    if (r >= a.R) return;
    const int b = a.src[r];
    const bool ok = b >= 0 && b < a.B;
    int tr = ok ? a.frames[b] : 0;
    tr = tr < 0 ? 0 : (tr > a.T ? a.T : tr);
    const int k = a.noise[r];
    int st = a.start[r];
    st = st < 0 ? 0 : st;
    int nf = 0;
    float factor = 0.f;
    if (ok && tr > 0 && k >= 0 && k < a.K) {
        nf = a.noise_frames[k];
        nf = nf < 0 ? 0 : (nf > a.Tn ? a.Tn : nf);
        const float ea = a.energy[b], en = a.noise_energy[k];
        if (nf > 0 && ea > 0.f && en > 0.f) {           // (a NaN energy compares false)
            const float f = (float)(sqrt(((double)ea / tr) / ((double)en / nf)) * pow(10.0, (double)a.gain_db[r] / 20.0));
            if (f == f && fabsf(f) <= 3.402823466e38f) factor = f;
        }
    }
    const int avail = nf > st ? nf - st : 0;
    const bool mix = factor != 0.f && avail > 0;
    reinterpret_cast<PlanRow*>(a.plan)[r] = {ok ? b : -1, mix ? k : -1, mix ? st : 0, mix ? avail : 0, __float_as_int(mix ? factor : 0.f), tr, {0, 0}};
    // the fewest samples that hold tr frames: 1 + n / hop centred frames for n > fft / 2, 1 + (n - fft) / hop deploy frames
    int n = 0;
    if (tr > 0) n = centred ? ((tr - 1) * hop > fft / 2 ? (tr - 1) * hop : fft / 2 + 1) : fft + (tr - 1) * hop;
    a.plan[(size_t)a.R * kPlanInts + r] = n;
}

// The delta thirds of the MFCC rows (utils/mfcc.py:45-69,96-99), in place behind the launch above: with
// d[t] = c[min(t + 1, T_b - 1)] - c[max(t - 1, 0)] (_delta_order shifts by one frame whatever its order, and only scales by it),
// columns [n_mfcc, 2 n_mfcc) = d / 2 and [2 n_mfcc, 3 n_mfcc) = (1 d + 2 d) / 10.  The edges are the utterance's own T_b, by the
// framing of the launch in front (p.centred); rows past it are zero.  One thread per (frame, coefficient): n_mfcc reads of
// neighbours in L2, 2 n_mfcc writes per frame.
__global__ void __launch_bounds__(256) mfcc_delta_kernel(const FrontendParams p) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    const unsigned nc = (unsigned)p.n_mfcc;
    const unsigned long long row = i / nc;
    if (row >= (unsigned long long)p.B * (unsigned)p.T) return;
    const unsigned c = (unsigned)(i - row * nc);
    const unsigned b = (unsigned)(row / (unsigned)p.T);
    const int t = (int)(row - (unsigned long long)b * (unsigned)p.T);
    const int tb = row_frames(p, b);
    float* out = p.mel + (size_t)row * (3 * nc);
    float d1 = 0.f, d2 = 0.f;
    if (t < tb) {
        const float* u = p.mel + (size_t)b * p.T * (3 * nc) + c;
        const int tn = t + 1 < tb ? t + 1 : tb - 1, tp = t > 0 ? t - 1 : 0;
        const float d = u[(size_t)tn * (3 * nc)] - u[(size_t)tp * (3 * nc)];
        d1 = d / 2.f;
        d2 = (d + 2.f * d) / 10.f;
    }
    out[nc + c] = d1;
    out[2 * nc + c] = d2;
}
// ---- launchers.  p on the grid of `total` frames: 16 per workgroup, rounded up to a multiple of 8 for the kernel's XCD-aware block map
static FrontendParams on_fft400_grid(FrontendParams q, long long total) {        // total < 2^31 (checked by the callers)
    q.fft_blocks = (int)(((total + 15) / 16 + 7) / 8 * 8);
    return q;
}
template <typename SampleT, bool GATE>
static hipError_t launch_fft400_tiles(const FrontendParams& q, hipStream_t st) {
    return with_int<1, 2, 3, 4>(q.mel_tiles, [&](auto mt) {
        return launch_lds<mel_fft400_kernel<mt(), SampleT, GATE>>(dim3((unsigned)q.fft_blocks), dim3(256), 0, st, q);
    });
}
// whole utterances under the handle's framing: launch(tag) starts the instantiation of that tag
template <int EPI, typename F>
static hipError_t with_utterance_tag(const FrontendParams& q, F&& launch) {
    if (!q.centred) return launch(Utterances<float, EPI>{});
    if (q.pre_emphasis != 0.f) return launch(DatasetFrames<float, EPI, true>{});
    return launch(DatasetFrames<float, EPI, false>{});
}
// The feature q names -- mel, power mel, or MFCC with mfcc_delta_kernel behind it -- of `total` frames; launch(epi) starts the
// transform with that epilogue
template <typename F>
static hipError_t launch_feature(const FrontendParams& q, long long total, hipStream_t st, F&& launch) {
    if (q.n_mfcc == 0) return q.power == 2 ? launch(std::integral_constant<int, kEpiPower>{}) : launch(std::integral_constant<int, kEpiMel>{});
    if (q.n_mfcc > 16 * kMaxDctTiles || q.dct_tiles != (q.n_mfcc + 15) / 16 || !q.dct) return hipErrorInvalidValue;
    const hipError_t e = launch(std::integral_constant<int, kEpiMfcc>{});
    if (e != hipSuccess) return e;
    const unsigned long long cells = (unsigned long long)total * (unsigned)q.n_mfcc;       // < 2^36
    return launch_lds<mfcc_delta_kernel>(dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, q);
}

hipError_t launch_features_fft400(const FrontendParams& p, int B, hipStream_t st) {
    const long long total = (long long)B * p.T;        // 0 < total < 2^31 (checked by the caller)
    if (p.fft != 400 || p.gate || p.pcm_i16 || p.n_carry != 0 || (p.centred && !p.win)) return hipErrorInvalidValue;
    FrontendParams q = on_fft400_grid(p, total);
    q.B = B;
    return launch_feature(q, total, st, [&](auto epi) {
        return with_utterance_tag<epi()>(q, [&](auto tag) { return launch_fft400_tiles<decltype(tag), false>(q, st); });
    });
}

hipError_t launch_linear_fft400(const FrontendParams& p, int B, int32_t* frames_out, float* energy_out, hipStream_t st) {
    const long long total = (long long)B * p.T;        // 0 < total < 2^31 (checked by the caller)
    if (p.fft != 400 || p.gate || p.pcm_i16 || p.n_carry != 0 || (p.centred && !p.win) || total <= 0) return hipErrorInvalidValue;
    FrontendParams q = on_fft400_grid(p, total);
    q.B = B;
    const hipError_t e = with_utterance_tag<kEpiLinear>(q, [&](auto tag) {        // no mel tile: the MT = 1 instantiation
        return launch_lds<mel_fft400_kernel<1, decltype(tag), false>>(dim3((unsigned)q.fft_blocks), dim3(256), 0, st, q);
    });
    if (e != hipSuccess) return e;
    return launch_lds<linear_energy_kernel>(dim3((unsigned)B), dim3(256), 0, st, q, frames_out, energy_out);
}

hipError_t launch_augment_fft400(const FrontendParams& p, const float* spec, const float* noise_spec, const AugmentRows& rows, hipStream_t st) {
    const long long total = (long long)rows.R * rows.T;        // 0 < total < 2^31 (checked by the caller)
    if (p.fft != 400 || total <= 0 || total >= (1LL << 31) || !rows.plan) return hipErrorInvalidValue;
    if ((long long)rows.T * p.hop + p.fft > 0x7fffffffLL) return hipErrorInvalidValue;      // the plan's sample counts are int32
    const hipError_t e = launch_lds<augment_plan_kernel>(dim3((unsigned)((rows.R + 255) / 256)), dim3(256), 0, st, rows, p.fft, p.hop, p.centred);
    if (e != hipSuccess) return e;
    FrontendParams q = on_fft400_grid(p, total);
    q.B = rows.R; q.T = rows.T;
    q.gate = 0; q.pcm_i16 = nullptr; q.n_carry = 0; q.n_samples = 0;
    bind_mix_rows(q, {spec, noise_spec, rows.Tn, reinterpret_cast<const PlanRow*>(rows.plan)});
    // behind the plan, per row a sample count with T_r frames under the handle's framing: mfcc_delta_kernel's edges (nothing clamps it)
    q.lens = rows.plan + (size_t)rows.R * kPlanInts; q.n_max = 0x7fffffff;
    return launch_feature(q, total, st, [&](auto epi) { return launch_fft400_tiles<Mixed<epi()>, false>(q, st); });
}

hipError_t launch_mel_fft400(const FrontendParams& p, int B, hipStream_t st) {
    const FrontendParams q = on_fft400_grid(p, (long long)B * p.T);        // < 2^31 (checked by the caller)
    if (p.frames) {
        if (!p.gate || p.fft != 400) return hipErrorInvalidValue;
        return p.pcm_i16 ? launch_fft400_tiles<RaggedRows<int16_t>, true>(q, st) : launch_fft400_tiles<RaggedRows<float>, true>(q, st);
    }
    if (!p.gate) return p.pcm_i16 ? launch_fft400_tiles<int16_t, false>(q, st) : launch_fft400_tiles<float, false>(q, st);
    return p.pcm_i16 ? launch_fft400_tiles<int16_t, true>(q, st) : launch_fft400_tiles<float, true>(q, st);
}

}  // namespace kws
