// The three plain GEMM kernels of the self-attention CTC model (attention_kernels.hip: embedding, qkv, FFN) on the fp16 matrix
// pipe, "f16x3" as in gru_f16x3_generic.hip: every matmul operand v is split into two fp16 pieces, v = hi + 2^-11 lo
// (hi = fp16(v), lo = fp16((v - hi) 2^11), both round-to-nearest-even: 22 mantissa bits), and a product takes three
// v_mfma_f32_16x16x32_f16 with fp32 accumulation,
//     main += Xh . Wh        lo += Xh . Wl + Xl . Wh        result = main + 2^-11 lo    (once, before the epilogue)
// The lo pieces are scaled so that they never fall into fp16's subnormal range (weights of O(0.1) have lo pieces near 2^-13: the
// scale keeps their full 11 bits), the dropped Xl . Wl term is 2^-22 relative.  Everything else is the fp32 kernels': one
// workgroup = 4 waves on 32 rows of ONE utterance, the same accumulator image (row 16 m + 4 g + j, column lane % 16), the same
// epilogues, the same layer-norm partials and merge (attention_device.h), fp32 activations in HBM.  The attention core and the
// output kernel stay fp32 (attention_kernels.hip): an f16x3 handle launches the same instantiations of them.
//
// Weights: kws_attention_create_precision packs [K/32][N/16][hi | lo][64 lanes] x 8 halves, lane l, element j =
// W[32 kc + 8 (l / 16) + j][16 nt + l % 16] (rows past K zero): one 16-byte load per lane and piece is a B operand.
// Activations: split while they are staged into LDS, AFTER the layer norm, clamped to +-65504 first (an out-of-range value
// saturates instead of becoming inf).  The LDS image is the A operand itself, [K/32][2 row halves][64 lanes] x 8 halves per piece,
// lane l, element j = X[16 m + l % 16][32 kc + 8 (l / 16) + j]: an A read is one ds_read_b128 at lane * 16 bytes, 64 lanes on 1 KiB
// contiguous -- every 16-lane group of the instruction covers all 64 banks once, which no padded row-major image does (its groups mix
// lanes of two k offsets: for any odd 16-byte row stride two of the sixteen reads share a bank quad).
// The embedding stages mel * 2^-8 against W_in * 2^8 (both exact): features up to 2^8 * 65504 stay representable.
#include "attention_device.h"
#include "f16x3_device.h"
#include "launch.h"

namespace kws {
namespace {

constexpr int kPlane = 2 * 64;      // 16-byte units of one 32-wide k chunk of an A plane: [2 row halves][64 lanes]

// position (in halves) of X[r][k] in an A plane
__device__ __forceinline__ int a_half_index(int r, int k) {
    return (((k >> 5) * 2 + (r >> 4)) * 64 + 16 * ((k >> 3) & 3) + (r & 15)) * 8 + (k & 7);
}

// rows [row0, row0 + 32) of src ([rows][H], one utterance) as the hi / lo A planes; rows at or past T1 are 0.  g != null: layer norm
// on the way.  A wave's 64 float4 loads are 8 rows x 128 B; 16 consecutive threads write 128 contiguous bytes of a plane.
template <int H>
__device__ void stage_tile(u32x4* xh, u32x4* xl, const float* src, int row0, int T1, const float* g, const float* bt, float2 ms) {
    uint2* xh2 = reinterpret_cast<uint2*>(xh);
    uint2* xl2 = reinterpret_cast<uint2*>(xl);
    for (int i = threadIdx.x; i < RT * H / 4; i += 256) {
        const int jh = i & 1, gk = (i >> 4) & 3, rest = i >> 6;
        const int r = (rest & 3) * 8 + ((i >> 1) & 7), kc = rest >> 2, c4 = 32 * kc + 8 * gk + 4 * jh;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + r < T1) {
            v = ld4(src + (size_t)(row0 + r) * H + c4);
            if (g)
                for (int j = 0; j < 4; ++j) v[j] = ln1(v[j], ms, g[c4 + j], bt[c4 + j]);
            for (int j = 0; j < 4; ++j) v[j] = clamp_half(v[j]);
        }
        unsigned h0, l0, h1, l1;
        split2((f32x2){v[0], v[1]}, h0, l0);
        split2((f32x2){v[2], v[3]}, h1, l1);
        const int at = ((kc * 2 + (r >> 4)) * 64 + 16 * gk + (r & 15)) * 2 + jh;
        xh2[at] = make_uint2(h0, h1);
        xl2[at] = make_uint2(l0, l1);
    }
}

// acc[m][n] (+ 2^-11 lo[m][n]) += X[16 m + ..][k < 32 KC] . W[k][16 (nt0 + n) + ..] for the 32 rows staged in the planes xh / xl; W
// packed as in the header with ntot tiles per k chunk
template <int NT>
__device__ __forceinline__ void gemm32h(f32x4 (&acc)[2][NT], f32x4 (&lo)[2][NT], const u32x4* xh, const u32x4* xl, int KC, const u32x4* wp,
                                        int ntot, int nt0) {
    const int lane = threadIdx.x & 63;
    for (int kc = 0; kc < KC; ++kc) {
        const u32x4 a0h = xh[kc * kPlane + lane], a1h = xh[kc * kPlane + 64 + lane];
        const u32x4 a0l = xl[kc * kPlane + lane], a1l = xl[kc * kPlane + 64 + lane];
        const u32x4* wk = wp + ((size_t)kc * ntot + nt0) * 128 + lane;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const u32x4 bh = wk[n * 128], bl = wk[n * 128 + 64];
            acc[0][n] = mfma_f16(a0h, bh, acc[0][n]);
            acc[1][n] = mfma_f16(a1h, bh, acc[1][n]);
            lo[0][n] = mfma_f16(a0h, bl, lo[0][n]);
            lo[1][n] = mfma_f16(a1h, bl, lo[1][n]);
            lo[0][n] = mfma_f16(a0l, bh, lo[0][n]);
            lo[1][n] = mfma_f16(a1l, bh, lo[1][n]);
        }
    }
}
template <int NT>
__device__ __forceinline__ void fold_lo(f32x4 (&acc)[2][NT], const f32x4 (&lo)[2][NT]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] += lo[m][n] * kLoInv;
}

}  // namespace

template <int H>
__global__ __launch_bounds__(256) void attn_embed_f16x3_kernel(AttnParams p) {
    extern __shared__ float4 smem4[];
    const int KC = p.KE / 32;
    u32x4* xh = reinterpret_cast<u32x4*>(smem4);     // [KC][2][64]
    u32x4* xl = xh + KC * kPlane;
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int Tb = utt_len(p, b), T1 = frames_out(Tb, p.c);
    if (row0 >= T1) return;
    const int cF = p.c * p.F;
    // as attn_embed_kernel: element k of stacked row t' is mel flat index t' c F + k of the utterance, a real frame iff below Tb * F
    const float* mel_b = p.mel + (size_t)b * p.T_max * p.F;
    const size_t lim = (size_t)Tb * p.F;
    _Float16* xhh = reinterpret_cast<_Float16*>(xh);
    _Float16* xlh = reinterpret_cast<_Float16*>(xl);
    for (int i = threadIdx.x; i < RT * p.KE; i += 256) {
        const int r = i / p.KE, k = i - r * p.KE;
        const size_t flat = (size_t)(row0 + r) * cF + k;
        const float v = (row0 + r < T1 && k < cF && flat < lim) ? clamp_half(mel_b[flat] * kMelScale) : 0.f;
        const int at = a_half_index(r, k);
        split1(v, xhh[at], xlh[at]);
    }
    __syncthreads();
    constexpr int NT = H / 64;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x4 acc[2][NT] = {}, lo[2][NT] = {};
    gemm32h<NT>(acc, lo, xh, xl, KC, reinterpret_cast<const u32x4*>(p.w_in), H / 16, wv * NT);
    fold_lo<NT>(acc, lo);
    float* out = p.S + (size_t)b * p.Tp * H;
    for (int m = 0; m < 2; ++m)
        for (int n = 0; n < NT; ++n) {
            const int col = 16 * (wv * NT + n) + (lane & 15);
            for (int j = 0; j < 4; ++j) {
                const int t = row0 + 16 * m + 4 * (lane >> 4) + j;
                if (t < T1) out[(size_t)t * H + col] = (acc[m][n][j] + p.b_in[col]) + p.pe[(size_t)t * H + col];
            }
        }
}

// main and lo accumulators of a wave's 3H / 64 column tiles: 192 registers at H = 256, no spill (256 in all)
template <int H, bool LN>
__global__ __launch_bounds__(256) void attn_qkv_f16x3_kernel(AttnParams p, AttnLayerW w, const float* gprev, const float* bprev) {
    __shared__ u32x4 xh[(H / 32) * kPlane];
    __shared__ u32x4 xl[(H / 32) * kPlane];
    __shared__ float2 ms_slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = frames_out(utt_len(p, b), p.c);
    if (row0 >= T1) return;
    float2 ms = make_float2(0.f, 1.f);
    if (LN) ms = ln_stats_block(p.st_b + (size_t)b * p.ntile, (T1 + RT - 1) / RT, &ms_slot);
    stage_tile<H>(xh, xl, p.S + (size_t)b * p.Tp * H, row0, T1, LN ? gprev : nullptr, bprev, ms);
    __syncthreads();
    constexpr int NT = 3 * H / 64;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x4 acc[2][NT] = {}, lo[2][NT] = {};
    gemm32h<NT>(acc, lo, xh, xl, H / 32, reinterpret_cast<const u32x4*>(w.wqkv), 3 * H / 16, wv * NT);
    fold_lo<NT>(acc, lo);
    float* out = p.QKV + (size_t)b * p.Tp * 3 * H;
    for (int m = 0; m < 2; ++m)
        for (int n = 0; n < NT; ++n) {
            const int col = 16 * (wv * NT + n) + (lane & 15);
            for (int j = 0; j < 4; ++j) {
                const int t = row0 + 16 * m + 4 * (lane >> 4) + j;
                if (t < T1) out[(size_t)t * 3 * H + col] = acc[m][n][j] + w.bqkv[col];
            }
        }
}

template <int H>
__global__ __launch_bounds__(256) void attn_ffn_f16x3_kernel(AttnParams p, AttnLayerW w) {
    constexpr int NT = H / 64;
    __shared__ u32x4 yh[(H / 32) * kPlane];
    __shared__ u32x4 yl[(H / 32) * kPlane];
    __shared__ u32x4 ih[2][2 * kPlane];            // 64 columns of relu(y W1 + b1), hi; two buffers as in attn_ffn_kernel
    __shared__ u32x4 il[2][2 * kPlane];
    __shared__ float red[4];
    __shared__ float2 ms_slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = frames_out(utt_len(p, b), p.c);
    if (row0 >= T1) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const float2 ms = ln_stats_block(p.st_a + (size_t)b * p.ntile, (T1 + RT - 1) / RT, &ms_slot);
    const float* ub = p.U + (size_t)b * p.Tp * H;
    stage_tile<H>(yh, yl, ub, row0, T1, w.ga, w.ba, ms);   // y = LN_a(att + x)
    __syncthreads();
    f32x4 acc[2][NT] = {}, lo[2][NT] = {};
    const int nf = p.Fi / 64, ntot1 = p.Fi / 16;
    const u32x4* w1 = reinterpret_cast<const u32x4*>(w.w1);
    const u32x4* w2 = reinterpret_cast<const u32x4*>(w.w2);
    for (int fc = 0; fc < nf; ++fc) {
        // 16 of the chunk's 64 columns per wave, split on their way into LDS as the A operand of the W2 product: column 16 wv + r16
        // of the chunk, row 16 m + 4 g + j
        _Float16* ibh = reinterpret_cast<_Float16*>(ih[fc & 1]);
        _Float16* ibl = reinterpret_cast<_Float16*>(il[fc & 1]);
        f32x4 h1[2][1] = {}, h1l[2][1] = {};
        gemm32h<1>(h1, h1l, yh, yl, H / 32, w1, ntot1, fc * 4 + wv);
        fold_lo<1>(h1, h1l);
        const float bias = w.b1[16 * (fc * 4 + wv) + r16];
        for (int m = 0; m < 2; ++m)
            for (int j = 0; j < 4; ++j) {
                const int at = a_half_index(16 * m + 4 * g + j, 16 * wv + r16);
                split1(__builtin_fminf(fmaxf(h1[m][0][j] + bias, 0.f), kHalfMax), ibh[at], ibl[at]);
            }
        __syncthreads();
        gemm32h<NT>(acc, lo, ih[fc & 1], il[fc & 1], 2, w2 + (size_t)fc * 2 * (H / 16) * 128, H / 16, wv * NT);
    }
    fold_lo<NT>(acc, lo);
    // + b2 + y with the fp32 y: LN_a of U again, as attn_core_kernel's epilogue re-derives its x (the planes hold only the pieces)
    float* so = p.S + (size_t)b * p.Tp * H;
    float lsum = 0.f;
    for (int m = 0; m < 2; ++m)
        for (int n = 0; n < NT; ++n) {
            const int col = 16 * (wv * NT + n) + r16;
            for (int j = 0; j < 4; ++j) {
                const int row = 16 * m + 4 * g + j;
                float v = 0.f;
                if (row0 + row < T1) {
                    const float y = ln1(ub[(size_t)(row0 + row) * H + col], ms, w.ga[col], w.ba[col]);
                    v = (acc[m][n][j] + w.b2[col]) + y;
                    so[(size_t)(row0 + row) * H + col] = v;
                    lsum += v;
                }
                acc[m][n][j] = v;
            }
        }
    const int nrows = min(RT, T1 - row0);
    tile_partial(p.st_b + (size_t)b * p.ntile + blockIdx.x, lsum, (float)(nrows * H), red, [&](float mean) {
        float d2 = 0.f;
        for (int m = 0; m < 2; ++m)
            for (int n = 0; n < NT; ++n)
                for (int j = 0; j < 4; ++j)
                    if (row0 + 16 * m + 4 * g + j < T1) d2 += (acc[m][n][j] - mean) * (acc[m][n][j] - mean);
        return d2;
    });
}

hipError_t launch_attn_embed_f16x3(const AttnParams& p, int H, hipStream_t st) {
    return with_int<64, 128, 256>(H, [&](auto h) {
        return launch_lds<attn_embed_f16x3_kernel<h()>>(dim3(p.ntile, p.B), dim3(256), (size_t)(p.KE / 32) * 2 * kPlane * sizeof(u32x4), st, p);
    });
}
hipError_t launch_attn_qkv_f16x3(const AttnParams& p, const AttnLayerW& w, const AttnLayerW* prev, int H, hipStream_t st) {
    const float *gb = prev ? prev->gb : nullptr, *bb = prev ? prev->bb : nullptr;
    return with_int<64, 128, 256>(H, [&](auto h) {
        return with_bool(prev != nullptr, [&](auto ln) {
            return launch_lds<attn_qkv_f16x3_kernel<h(), ln()>>(dim3(p.ntile, p.B), dim3(256), 0, st, p, w, gb, bb);
        });
    });
}
hipError_t launch_attn_ffn_f16x3(const AttnParams& p, const AttnLayerW& w, int H, hipStream_t st) {
    return with_int<64, 128, 256>(H, [&](auto h) { return launch_lds<attn_ffn_f16x3_kernel<h()>>(dim3(p.ntile, p.B), dim3(256), 0, st, p, w); });
}

}  // namespace kws
