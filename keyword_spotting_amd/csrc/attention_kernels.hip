// Self-attention CTC model (models/attention_ctc.py:73-128 inference, DeployModel :215-274), batched over B independent
// utterances.  fp32 storage; every matmul on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).  2 + 3L launches:
//   attn_embed_kernel   stacked rows read straight from mel (pad and out-of-length frames masked to 0) . W_in + b_in + pe
//   per layer
//     attn_qkv_kernel   LN_b of the layer below applied while the operand is staged (layer 0: none) . W_qkv + b_qkv
//     attn_core_kernel  per (utterance, 32-row query tile): every head's softmax(q k^T / sqrt(d)) v over the utterance's T'_b
//                       keys, streamed through LDS 32 keys at a time with a running max and sum; epilogue att + x and the
//                       tile's LN_a partials
//     attn_ffn_kernel   LN_a on load, relu(y . W1 + b1) . W2 in 64-wide chunks of Fi that never leave LDS, + b2 + y, LN_b partials
//   attn_out_kernel     LN_b of the last layer on load, . W_out + b_out, relu, softmax; rows past T'_b written as 0
// Layer norm is tf.contrib.layers.layer_norm of TF 1.x: moments over the utterance's whole [T', H] block.  Each producer tile
// writes (count, mean, M2) of its valid rows (mean first, then the squared deviations, both over registers); every consumer
// merges the utterance's partials in tile order (Chan et al.): no atomics, no E[x^2] - mean^2, bitwise reproducible and a
// function of the utterance's own rows only.
//
// Attention orientation: S^T = K . Q^T (A = K rows from LDS, B = the wave's 16 queries), so a lane holds 4 keys x 1 query of
// each 16x16 score tile -- exactly the B operand of O^T = V^T . P^T (A = V^T from LDS), whose result again has the query on
// the lane.  The running max / sum of a query therefore live in one lane column: no LDS round trip for P, and the rescale of
// O by exp(m_old - m_new) is a per-lane scalar.
#include "attention_device.h"
#include "launch.h"

namespace kws {
namespace {

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// four k-steps: component j of both operands is k = 4 (lane / 16) + j of the chunk
__device__ __forceinline__ f32x4 mfma4(f32x4 a, f32x4 b, f32x4 c) {
    c = mfma(a[0], b[0], c);
    c = mfma(a[1], b[1], c);
    c = mfma(a[2], b[2], c);
    return mfma(a[3], b[3], c);
}
// rows [row0, row0 + 32) of src ([rows][H], one utterance) into xs [32][H + 4]; rows at or past T1 are 0.  g != null: layer
// norm (v - mean) * rstd * g + bt on the way
template <int H>
__device__ void load_tile(float* xs, const float* src, int row0, int T1, const float* g, const float* bt, float2 ms) {
    for (int i = threadIdx.x; i < RT * H / 4; i += 256) {
        const int r = i / (H / 4), c4 = (i % (H / 4)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + r < T1) {
            v = ld4(src + (size_t)(row0 + r) * H + c4);
            if (g)
                for (int j = 0; j < 4; ++j) v[j] = ln1(v[j], ms, g[c4 + j], bt[c4 + j]);
        }
        st4(xs + r * (H + 4) + c4, v);
    }
}

// acc[m][n] += X[16 m + ..][k < 16 KC] . W[k][16 (nt0 + n) + ..] for the 32 rows staged in xs (row stride ldx, == 4 mod 16 floats:
// the float4 A reads of 16 lanes hit 16 distinct bank quads); W packed as in attention_internal.h with ntot tiles per k chunk
template <int NT>
__device__ __forceinline__ void gemm32(f32x4 (&acc)[2][NT], const float* xs, int ldx, int KC, const float4* wp, int ntot, int nt0) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    for (int kc = 0; kc < KC; ++kc) {
        const f32x4 a0 = ld4(xs + r * ldx + 16 * kc + 4 * g);
        const f32x4 a1 = ld4(xs + (16 + r) * ldx + 16 * kc + 4 * g);
        const float* wk = reinterpret_cast<const float*>(wp + ((size_t)kc * ntot + nt0) * 64 + lane);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const f32x4 bv = ld4(wk + n * 256);
            acc[0][n] = mfma4(a0, bv, acc[0][n]);
            acc[1][n] = mfma4(a1, bv, acc[1][n]);
        }
    }
}

}  // namespace

template <int H>
__global__ __launch_bounds__(256) void attn_embed_kernel(AttnParams p) {
    extern __shared__ float4 smem4[];
    float* xs = reinterpret_cast<float*>(smem4);
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int Tb = utt_len(p, b), T1 = frames_out(Tb, p.c);
    if (row0 >= T1) return;
    const int ldx = p.KE + 4, cF = p.c * p.F;
    // stacked row t' = frames c t' .. c t' + c - 1 back to back: element k of it is mel flat index t' c F + k of the utterance,
    // a real frame iff that index lies below Tb * F (the appended pad frames and the caller's padding past Tb read as 0)
    const float* mel_b = p.mel + (size_t)b * p.T_max * p.F;
    const size_t lim = (size_t)Tb * p.F;
    for (int i = threadIdx.x; i < RT * p.KE; i += 256) {
        const int r = i / p.KE, k = i - r * p.KE;
        const size_t flat = (size_t)(row0 + r) * cF + k;
        xs[r * ldx + k] = (row0 + r < T1 && k < cF && flat < lim) ? mel_b[flat] : 0.f;
    }
    __syncthreads();
    constexpr int NT = H / 64;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x4 acc[2][NT] = {};
    gemm32<NT>(acc, xs, ldx, p.KE / 16, p.w_in, H / 16, wv * NT);
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

template <int H, bool LN>
__global__ __launch_bounds__(256) void attn_qkv_kernel(AttnParams p, AttnLayerW w, const float* gprev, const float* bprev) {
    __shared__ float xs[RT * (H + 4)];
    __shared__ float2 ms_slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = frames_out(utt_len(p, b), p.c);
    if (row0 >= T1) return;
    float2 ms = make_float2(0.f, 1.f);
    if (LN) ms = ln_stats_block(p.st_b + (size_t)b * p.ntile, (T1 + RT - 1) / RT, &ms_slot);
    load_tile<H>(xs, p.S + (size_t)b * p.Tp * H, row0, T1, LN ? gprev : nullptr, bprev, ms);
    __syncthreads();
    constexpr int NT = 3 * H / 64;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x4 acc[2][NT] = {};
    gemm32<NT>(acc, xs, H + 4, H / 16, w.wqkv, 3 * H / 16, wv * NT);
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

template <int H, int D, bool LN>
__global__ __launch_bounds__(256) void attn_core_kernel(AttnParams p, const float* gprev, const float* bprev) {
    constexpr int NH = H / D, UPW = NH / 2, DC = D / 16;   // units = 2 query halves x NH heads, UPW per wave
    constexpr int KLD = H + 4, VLD = RT + 4;
    extern __shared__ float4 smem4[];
    float* ks = reinterpret_cast<float*>(smem4);   // [32 keys][KLD]
    float* vt = ks + RT * KLD;                     // [H][VLD]: V transposed
    __shared__ float red[4];
    __shared__ float2 ms_slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = frames_out(utt_len(p, b), p.c);
    if (row0 >= T1) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const float* qkv = p.QKV + (size_t)b * p.Tp * 3 * H;
    const float scale = 1.0f / sqrtf((float)D);
    f32x4 q[UPW][DC], o[UPW][DC];
    float mrun[UPW], lrun[UPW];
#pragma unroll
    for (int u = 0; u < UPW; ++u) {
        const int unit = wv * UPW + u, h = unit >> 1;
        const int tq = row0 + 16 * (unit & 1) + r16;
#pragma unroll
        for (int cc = 0; cc < DC; ++cc) {
            q[u][cc] = tq < T1 ? ld4(qkv + (size_t)tq * 3 * H + h * D + 16 * cc + 4 * g) * scale : f32x4{0.f, 0.f, 0.f, 0.f};
            o[u][cc] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        mrun[u] = -INFINITY;
        lrun[u] = 0.f;
    }
    for (int k0 = 0; k0 < T1; k0 += RT) {
        __syncthreads();                                  // every wave is done with the previous chunk
        for (int i = threadIdx.x; i < RT * H / 4; i += 256) {
            const int kr = i / (H / 4), c4 = (i % (H / 4)) * 4;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (k0 + kr < T1) {                           // keys of this utterance only; past T'_b: zeros, masked below
                const float* row = qkv + (size_t)(k0 + kr) * 3 * H;
                kv = ld4(row + H + c4);
                vv = ld4(row + 2 * H + c4);
            }
            st4(ks + kr * KLD + c4, kv);
            for (int j = 0; j < 4; ++j) vt[(c4 + j) * VLD + kr] = vv[j];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < UPW; ++u) {
            const int h = (wv * UPW + u) >> 1;
            f32x4 s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int cc = 0; cc < DC; ++cc) s[kt] = mfma4(ld4(ks + (16 * kt + r16) * KLD + h * D + 16 * cc + 4 * g), q[u][cc], s[kt]);
            }
            // s[kt][j]: key k0 + 16 kt + 4 g + j, query r16 of the unit
            float cmax = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (k0 + 16 * kt + 4 * g + j >= T1) s[kt][j] = -INFINITY;
                    cmax = fmaxf(cmax, s[kt][j]);
                }
            cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
            cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
            const float mnew = fmaxf(mrun[u], cmax);       // finite: key k0 < T1 is in every chunk
            const float alpha = __expf(mrun[u] - mnew);
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s[kt][j] = __expf(s[kt][j] - mnew);
                    psum += s[kt][j];
                }
            psum += __shfl_xor(psum, 16);
            psum += __shfl_xor(psum, 32);
            lrun[u] = lrun[u] * alpha + psum;
            mrun[u] = mnew;
#pragma unroll
            for (int cc = 0; cc < DC; ++cc) {
                o[u][cc] *= alpha;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) o[u][cc] = mfma4(ld4(vt + (h * D + 16 * cc + r16) * VLD + 16 * kt + 4 * g), s[kt], o[u][cc]);
            }
        }
    }
    // epilogue: o[u][cc][j] = att[query r16][h D + 16 cc + 4 g + j] * l; u = att + x, x = LN_b(S) of the layer below (layer 0: S)
    float2 ms = make_float2(0.f, 1.f);
    if (LN) ms = ln_stats_block(p.st_b + (size_t)b * p.ntile, (T1 + RT - 1) / RT, &ms_slot);
    const float* xin = p.S + (size_t)b * p.Tp * H;
    float* uo = p.U + (size_t)b * p.Tp * H;
    float lsum = 0.f;
#pragma unroll
    for (int u = 0; u < UPW; ++u) {
        const int unit = wv * UPW + u, h = unit >> 1;
        const int tq = row0 + 16 * (unit & 1) + r16;
#pragma unroll
        for (int cc = 0; cc < DC; ++cc) {
            const int col = h * D + 16 * cc + 4 * g;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (tq < T1) {
                f32x4 x = ld4(xin + (size_t)tq * H + col);
                if (LN)
                    for (int j = 0; j < 4; ++j) x[j] = ln1(x[j], ms, gprev[col + j], bprev[col + j]);
                for (int j = 0; j < 4; ++j) v[j] = o[u][cc][j] / lrun[u] + x[j];
                st4(uo + (size_t)tq * H + col, v);
                lsum += (v[0] + v[1]) + (v[2] + v[3]);
            }
            o[u][cc] = v;
        }
    }
    const int nrows = min(RT, T1 - row0);
    tile_partial(p.st_a + (size_t)b * p.ntile + blockIdx.x, lsum, (float)(nrows * H), red, [&](float mean) {
        float d2 = 0.f;
#pragma unroll
        for (int u = 0; u < UPW; ++u) {
            const int tq = row0 + 16 * ((wv * UPW + u) & 1) + r16;
            if (tq < T1)
#pragma unroll
                for (int cc = 0; cc < DC; ++cc)
                    for (int j = 0; j < 4; ++j) d2 += (o[u][cc][j] - mean) * (o[u][cc][j] - mean);
        }
        return d2;
    });
}

template <int H>
__global__ __launch_bounds__(256) void attn_ffn_kernel(AttnParams p, AttnLayerW w) {
    constexpr int YLD = H + 4, ILD = 64 + 4, NT = H / 64;
    __shared__ float ys[RT * YLD];
    __shared__ float is[2][RT * ILD];
    __shared__ float red[4];
    __shared__ float2 ms_slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = frames_out(utt_len(p, b), p.c);
    if (row0 >= T1) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const float2 ms = ln_stats_block(p.st_a + (size_t)b * p.ntile, (T1 + RT - 1) / RT, &ms_slot);
    load_tile<H>(ys, p.U + (size_t)b * p.Tp * H, row0, T1, w.ga, w.ba, ms);   // y = LN_a(att + x)
    __syncthreads();
    f32x4 acc[2][NT] = {};
    const int nf = p.Fi / 64, ntot1 = p.Fi / 16;
    for (int fc = 0; fc < nf; ++fc) {
        // 64 columns of relu(y W1 + b1): 16 per wave, into LDS as the A operand of the W2 product.  Two buffers: the barrier of
        // chunk fc + 1 already orders the rewrite of this one behind every wave's product of chunk fc.
        float* ib = is[fc & 1];
        f32x4 h1[2][1] = {};
        gemm32<1>(h1, ys, YLD, H / 16, w.w1, ntot1, fc * 4 + wv);
        const float bias = w.b1[16 * (fc * 4 + wv) + r16];
        for (int m = 0; m < 2; ++m)
            for (int j = 0; j < 4; ++j) ib[(16 * m + 4 * g + j) * ILD + 16 * wv + r16] = fmaxf(h1[m][0][j] + bias, 0.f);
        __syncthreads();
        gemm32<NT>(acc, ib, ILD, 4, w.w2 + (size_t)fc * 4 * (H / 16) * 64, H / 16, wv * NT);
    }
    float* so = p.S + (size_t)b * p.Tp * H;
    float lsum = 0.f;
    for (int m = 0; m < 2; ++m)
        for (int n = 0; n < NT; ++n) {
            const int col = 16 * (wv * NT + n) + r16;
            for (int j = 0; j < 4; ++j) {
                const int row = 16 * m + 4 * g + j;
                float v = 0.f;
                if (row0 + row < T1) {
                    v = (acc[m][n][j] + w.b2[col]) + ys[row * YLD + col];
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

template <int H>
__global__ __launch_bounds__(256) void attn_out_kernel(AttnParams p, const float* gl, const float* bl) {
    constexpr int YLD = H + 4;
    __shared__ float ys[RT * YLD];
    __shared__ float lg[RT][8];
    __shared__ float2 ms_slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = frames_out(utt_len(p, b), p.c);
    const int rr = threadIdx.x >> 3, cls = threadIdx.x & 7, t = row0 + rr;
    const size_t o = ((size_t)b * p.T1max + t) * p.C + cls;
    if (row0 >= T1) {                                     // rows past T'_b: zeros
        if (cls < p.C && t < p.T1max) {
            if (p.logits) p.logits[o] = 0.f;
            if (p.softmax) p.softmax[o] = 0.f;
        }
        return;
    }
    const float2 ms = ln_stats_block(p.st_b + (size_t)b * p.ntile, (T1 + RT - 1) / RT, &ms_slot);
    load_tile<H>(ys, p.S + (size_t)b * p.Tp * H, row0, T1, gl, bl, ms);
    __syncthreads();
    float v = 0.f;
    if (cls < p.C) {
        float acc = 0.f;
        for (int k = 0; k < H; ++k) acc += ys[rr * YLD + k] * p.w_out[k * p.C + cls];
        v = acc + p.b_out[cls];
        if (p.use_relu) v = fmaxf(v, 0.f);
    }
    lg[rr][cls] = v;
    __syncthreads();
    if (cls < p.C && t < p.T1max) {
        float lo = 0.f, sm = 0.f;
        if (t < T1) {
            float mx = lg[rr][0];
            for (int c = 1; c < p.C; ++c) mx = fmaxf(mx, lg[rr][c]);
            float den = 0.f;
            for (int c = 0; c < p.C; ++c) den += expf(lg[rr][c] - mx);
            lo = v;
            sm = expf(v - mx) / den;
        }
        if (p.logits) p.logits[o] = lo;
        if (p.softmax) p.softmax[o] = sm;
    }
}

hipError_t launch_attn_embed(const AttnParams& p, int H, hipStream_t st) {
    return with_int<64, 128, 256>(H, [&](auto h) {
        return launch_lds<attn_embed_kernel<h()>>(dim3(p.ntile, p.B), dim3(256), (size_t)RT * (p.KE + 4) * sizeof(float), st, p);
    });
}
hipError_t launch_attn_qkv(const AttnParams& p, const AttnLayerW& w, const AttnLayerW* prev, int H, hipStream_t st) {
    const float *gb = prev ? prev->gb : nullptr, *bb = prev ? prev->bb : nullptr;      // the layer norm of the layer below, fused in
    return with_int<64, 128, 256>(H, [&](auto h) {
        return with_bool(prev != nullptr, [&](auto ln) {
            return launch_lds<attn_qkv_kernel<h(), ln()>>(dim3(p.ntile, p.B), dim3(256), 0, st, p, w, gb, bb);
        });
    });
}
hipError_t launch_attn_core(const AttnParams& p, const AttnLayerW* prev, int H, int D, hipStream_t st) {
    const float *gb = prev ? prev->gb : nullptr, *bb = prev ? prev->bb : nullptr;
    return with_int<16, 32>(D, [&](auto d) {
        return with_int<64, 128, 256>(H, [&](auto h) {
            const size_t lds = (size_t)(RT * (h() + 4) + h() * (RT + 4)) * sizeof(float);
            return with_bool(prev != nullptr, [&](auto ln) {
                return launch_lds<attn_core_kernel<h(), d(), ln()>>(dim3(p.ntile, p.B), dim3(256), lds, st, p, gb, bb);
            });
        });
    });
}
hipError_t launch_attn_ffn(const AttnParams& p, const AttnLayerW& w, int H, hipStream_t st) {
    return with_int<64, 128, 256>(H, [&](auto h) { return launch_lds<attn_ffn_kernel<h()>>(dim3(p.ntile, p.B), dim3(256), 0, st, p, w); });
}
hipError_t launch_attn_out(const AttnParams& p, const AttnLayerW& last, int H, hipStream_t st) {
    const dim3 grid((p.T1max + RT - 1) / RT, p.B);
    return with_int<64, 128, 256>(H, [&](auto h) { return launch_lds<attn_out_kernel<h()>>(grid, dim3(256), 0, st, p, last.gb, last.bb); });
}

}  // namespace kws
