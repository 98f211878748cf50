// Training of the self-attention CTC model: the model-specific forward with its tape and the backward (api_attention_train.hip has
// the launch order).  Rows are [B*T1, width], row = b * T1 + t, live iff t < t1[b]; every kernel works on 32-row tiles of ONE
// utterance (grid = tiles x B), so a result depends on the utterance's own rows only.  No float atomics: every sum has a fixed order.
//   attn_train_core_forward_kernel   attn_core_kernel's online softmax (fp32 MFMA, keys streamed through LDS 32 at a time) that also
//                                    writes the log-sum-exp per (query, head) and drops probabilities in front of P . V
//   attn_train_core_dq_kernel        per query tile over the keys: P recomputed from q, k and the log-sum-exp, D = rowsum(dO o O),
//                                    dP = (dO . V^T) o keep / keep_prob, dS = P o (dP - D), dQ = dS . K / sqrt(d)
//   attn_train_core_dkv_kernel       per key tile over the queries: dK = dS^T . Q / sqrt(d), dV = (P o keep / keep_prob)^T . dO
//                                    (both backward kernels: fp32 VALU dot products out of LDS, 8 lanes per row; not on the matrix pipe)
//   attn_train_resid_kernel / attn_train_ln_forward_kernel     residual sum with the row-site dropout and the tile partials; block layer norm
//   attn_train_ln_bwd_sums_kernel / attn_train_ln_bwd_apply_kernel   its backward: the two block scalars per tile, then dx
// No [T', T'] matrix reaches global memory in either direction: the masks are recomputed from the counter hash (kws_internal.h).
#include "attention_device.h"
#include "launch.h"

namespace kws {
namespace {

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma4(f32x4 a, f32x4 b, f32x4 c) {
    c = mfma(a[0], b[0], c);
    c = mfma(a[1], b[1], c);
    c = mfma(a[2], b[2], c);
    return mfma(a[3], b[3], c);
}
// v o keep / keep_prob (a true division) at the site's coordinates; keep_prob == 1: v
__device__ __forceinline__ float dropped(float v, const AttnTrainDrop& d, int site, int b, int head, int row, int col) {
    if (d.keep_prob >= 1.0f) return v;
    return attn_drop_keep(d.seed, site, d.layer, b, head, row, col, d.thr) ? v / d.keep_prob : 0.f;
}
__device__ __forceinline__ int tiles_of(int rows) { return (rows + RT - 1) / RT; }

}  // namespace

__global__ __launch_bounds__(256) void attn_train_stack_kernel(const float* __restrict__ mel, const int32_t* __restrict__ tlen,
                                                               const int32_t* __restrict__ t1, int B, int T, int T1, int F, int c,
                                                               float* __restrict__ xs) {
    const int cF = c * F;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * T1 * cF) return;
    const size_t row = i / cF;
    const int k = (int)(i - row * cF), b = (int)(row / T1), t = (int)(row - (size_t)b * T1);
    const size_t flat = (size_t)t * cF + k;          // a real frame iff below T_b * F (T_b <= T: inside the utterance's block)
    xs[i] = (t < t1[b] && flat < (size_t)tlen[b] * F) ? mel[(size_t)b * T * F + flat] : 0.f;
}

__global__ __launch_bounds__(256) void attn_train_addpe_kernel(float* __restrict__ x, const float* __restrict__ pe,
                                                               const int32_t* __restrict__ t1, int B, int T1, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * T1 * H) return;
    const size_t row = i / H;
    const int col = (int)(i - row * H), b = (int)(row / T1), t = (int)(row - (size_t)b * T1);
    x[i] = t < t1[b] ? x[i] + pe[(size_t)t * H + col] : 0.f;
}

__global__ __launch_bounds__(256) void attn_train_relu_kernel(float* __restrict__ v, const int32_t* __restrict__ t1, int B, int T1, int N,
                                                              int relu) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * T1 * N) return;
    const size_t row = i / N;
    const int b = (int)(row / T1), t = (int)(row - (size_t)b * T1);
    const float a = v[i];
    v[i] = t < t1[b] ? (relu ? fmaxf(a, 0.f) : a) : 0.f;
}

__global__ __launch_bounds__(256) void attn_train_relumask_kernel(float* __restrict__ g, const float* __restrict__ post,
                                                                  const int32_t* __restrict__ t1, int B, int T1, int N) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * T1 * N) return;
    const size_t row = i / N;
    const int b = (int)(row / T1), t = (int)(row - (size_t)b * T1);
    g[i] = (t < t1[b] && post[i] > 0.f) ? g[i] : 0.f;
}

// attn_core_kernel (attention_kernels.hip) with a tape: S^T = K . Q^T, the query on the lane, running max and sum per lane column
template <int H, int D>
__global__ __launch_bounds__(256) void attn_train_core_forward_kernel(AttnTrainCore p) {
    constexpr int NH = H / D, UPW = NH / 2, DC = D / 16;
    constexpr int KLD = H + 4, VLD = RT + 4;
    extern __shared__ float4 smem4[];
    float* ks = reinterpret_cast<float*>(smem4);   // [32 keys][KLD]
    float* vt = ks + RT * KLD;                     // [H][VLD]: V transposed
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = p.t1[b];
    if (row0 >= T1) return;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const float* qkv = p.qkv + (size_t)b * p.T1 * 3 * H;
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
        __syncthreads();
        for (int i = threadIdx.x; i < RT * H / 4; i += 256) {
            const int kr = i / (H / 4), c4 = (i % (H / 4)) * 4;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (k0 + kr < T1) {
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
            const int unit = wv * UPW + u, h = unit >> 1;
            const int tq = row0 + 16 * (unit & 1) + r16;
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
            const float mnew = fmaxf(mrun[u], cmax);
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
            lrun[u] = lrun[u] * alpha + psum;          // the normaliser stays undropped
            mrun[u] = mnew;
            if (p.drop.keep_prob < 1.0f) {
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[kt][j] = dropped(s[kt][j], p.drop, kAttnDropProb, b, h, tq, k0 + 16 * kt + 4 * g + j);
            }
#pragma unroll
            for (int cc = 0; cc < DC; ++cc) {
                o[u][cc] *= alpha;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) o[u][cc] = mfma4(ld4(vt + (h * D + 16 * cc + r16) * VLD + 16 * kt + 4 * g), s[kt], o[u][cc]);
            }
        }
    }
    float* att = p.att + (size_t)b * p.T1 * H;
    float* lse = p.lse + (size_t)b * p.T1 * NH;
#pragma unroll
    for (int u = 0; u < UPW; ++u) {
        const int unit = wv * UPW + u, h = unit >> 1;
        const int tq = row0 + 16 * (unit & 1) + r16;
        if (tq < T1) {
#pragma unroll
            for (int cc = 0; cc < DC; ++cc) {
                f32x4 v;
                for (int j = 0; j < 4; ++j) v[j] = o[u][cc][j] / lrun[u];
                st4(att + (size_t)tq * H + h * D + 16 * cc + 4 * g, v);
            }
            if (g == 0) lse[(size_t)tq * NH + h] = mrun[u] + logf(lrun[u]);
        }
    }
}

// thread = (row of the tile, one of 8 lanes of that row): the lanes split the 32 rows of the other side's chunk, 4 each, and their
// partial sums are added by a butterfly over lane bits 0..2 -- the same order in every call
__device__ __forceinline__ float sum8(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

template <int D>
__global__ __launch_bounds__(256) void attn_train_core_dq_kernel(AttnTrainCore p) {
    __shared__ float ks[RT][D + 1], vs[RT][D + 1];
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = p.t1[b], H = p.H, NH = p.NH;
    if (row0 >= T1) return;
    const int qi = threadIdx.x >> 3, sub = threadIdx.x & 7, tq = row0 + qi;
    const bool qok = tq < T1;
    const size_t base = (size_t)b * p.T1, qrow = base + (qok ? tq : row0);
    const float scale = 1.0f / sqrtf((float)D);
    for (int h = 0; h < NH; ++h) {
        float q[D], dO[D], dq[D];
        float dsum = 0.f;
#pragma unroll
        for (int e = 0; e < D; ++e) {
            q[e] = p.qkv[qrow * 3 * H + h * D + e];
            dO[e] = p.datt[qrow * H + h * D + e];
            dsum += dO[e] * p.att[qrow * H + h * D + e];
            dq[e] = 0.f;
        }
        const float lse = p.lse[qrow * NH + h];
        if (qok && sub == 0) p.dsum[qrow * NH + h] = dsum;
        for (int k0 = 0; k0 < T1; k0 += RT) {
            __syncthreads();
            for (int i = threadIdx.x; i < RT * D; i += 256) {
                const int kr = i / D, e = i - kr * D;
                const bool ok = k0 + kr < T1;
                const float* row = p.qkv + (base + (ok ? k0 + kr : 0)) * 3 * H + h * D + e;
                ks[kr][e] = ok ? row[H] : 0.f;
                vs[kr][e] = ok ? row[2 * H] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kr = sub + 8 * j, key = k0 + kr;
                if (qok && key < T1) {
                    float s = 0.f, dp = 0.f;
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        s += q[e] * ks[kr][e];
                        dp += dO[e] * vs[kr][e];
                    }
                    const float pr = __expf(s * scale - lse);
                    const float ds = pr * (dropped(dp, p.drop, kAttnDropProb, b, h, tq, key) - dsum);
#pragma unroll
                    for (int e = 0; e < D; ++e) dq[e] += ds * ks[kr][e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const float v = sum8(dq[e]) * scale;
            if (qok && (e & 7) == sub) p.dqkv[qrow * 3 * H + h * D + e] = v;
        }
    }
}

template <int D>
__global__ __launch_bounds__(256) void attn_train_core_dkv_kernel(AttnTrainCore p) {
    __shared__ float qs[RT][D + 1], dos[RT][D + 1], lses[RT], dss[RT];
    const int b = blockIdx.y, row0 = blockIdx.x * RT;
    const int T1 = p.t1[b], H = p.H, NH = p.NH;
    if (row0 >= T1) return;
    const int ki = threadIdx.x >> 3, sub = threadIdx.x & 7, key = row0 + ki;
    const bool kok = key < T1;
    const size_t base = (size_t)b * p.T1, krow = base + (kok ? key : row0);
    const float scale = 1.0f / sqrtf((float)D);
    for (int h = 0; h < NH; ++h) {
        float k[D], v[D], dk[D], dv[D];
#pragma unroll
        for (int e = 0; e < D; ++e) {
            k[e] = p.qkv[krow * 3 * H + H + h * D + e];
            v[e] = p.qkv[krow * 3 * H + 2 * H + h * D + e];
            dk[e] = 0.f;
            dv[e] = 0.f;
        }
        for (int q0 = 0; q0 < T1; q0 += RT) {
            __syncthreads();
            for (int i = threadIdx.x; i < RT * D; i += 256) {
                const int qr = i / D, e = i - qr * D;
                const bool ok = q0 + qr < T1;
                const size_t row = base + (ok ? q0 + qr : 0);
                qs[qr][e] = ok ? p.qkv[row * 3 * H + h * D + e] : 0.f;
                dos[qr][e] = ok ? p.datt[row * H + h * D + e] : 0.f;
            }
            if (threadIdx.x < RT) {
                const bool ok = q0 + (int)threadIdx.x < T1;
                const size_t row = base + (ok ? q0 + threadIdx.x : 0);
                lses[threadIdx.x] = ok ? p.lse[row * NH + h] : 0.f;
                dss[threadIdx.x] = ok ? p.dsum[row * NH + h] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int qr = sub + 8 * j, tq = q0 + qr;
                if (kok && tq < T1) {
                    float s = 0.f, dp = 0.f;
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        s += qs[qr][e] * k[e];
                        dp += dos[qr][e] * v[e];
                    }
                    const float pr = __expf(s * scale - lses[qr]);
                    const float pd = dropped(pr, p.drop, kAttnDropProb, b, h, tq, key);
                    const float ds = pr * (dropped(dp, p.drop, kAttnDropProb, b, h, tq, key) - dss[qr]);
#pragma unroll
                    for (int e = 0; e < D; ++e) {
                        dv[e] += pd * dos[qr][e];
                        dk[e] += ds * qs[qr][e];
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < D; ++e) {
            const float a = sum8(dk[e]) * scale, c = sum8(dv[e]);
            if (kok && (e & 7) == sub) {
                p.dqkv[krow * 3 * H + H + h * D + e] = a;
                p.dqkv[krow * 3 * H + 2 * H + h * D + e] = c;
            }
        }
    }
}

__global__ __launch_bounds__(256) void attn_train_resid_kernel(AttnTrainResid p) {
    __shared__ float red[4];
    const int b = blockIdx.y, row0 = blockIdx.x * RT, H = p.H;
    const int T1 = p.t1[b];
    const size_t base = ((size_t)b * p.T1 + row0) * H;
    const int rows = min(RT, p.T1 - row0), live = min(max(T1 - row0, 0), rows);
    float lsum = 0.f;
    for (int i = threadIdx.x; i < rows * H; i += 256) {
        const int r = i / H, col = i - r * H;
        float v = 0.f;
        if (r < live) {
            v = dropped(p.a[base + i], p.drop, p.site, b, 0, row0 + r, col) + p.r[base + i];
            lsum += v;
        }
        p.u[base + i] = v;
    }
    if (live == 0) return;                                  // uniform
    const int ntile = (p.T1 + RT - 1) / RT;
    tile_partial(p.part + (size_t)b * ntile + blockIdx.x, lsum, (float)(live * H), red, [&](float mean) {
        float d2 = 0.f;
        for (int i = threadIdx.x; i < live * H; i += 256) {          // the thread's own stores
            const float d = p.u[base + i] - mean;
            d2 += d * d;
        }
        return d2;
    });
}

__global__ __launch_bounds__(256) void attn_train_ln_forward_kernel(AttnTrainLn p) {
    __shared__ float2 ms_slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT, H = p.H;
    const int T1 = p.t1[b];
    const size_t base = ((size_t)b * p.T1 + row0) * H;
    const int rows = min(RT, p.T1 - row0), live = min(max(T1 - row0, 0), rows);
    const int ntile = (p.T1 + RT - 1) / RT;
    float2 ms = make_float2(0.f, 1.f);
    if (T1 > 0) ms = ln_stats_block(p.part + (size_t)b * ntile, tiles_of(T1), &ms_slot);      // uniform
    if (blockIdx.x == 0 && threadIdx.x == 0) p.rstd[b] = ms.y;
    for (int i = threadIdx.x; i < rows * H; i += 256) {
        const int r = i / H, col = i - r * H;
        float xn = 0.f, y = 0.f;
        if (r < live) {
            xn = (p.u[base + i] - ms.x) * ms.y;
            y = xn * p.g[col] + p.bt[col];
        }
        p.xn[base + i] = xn;
        p.y[base + i] = y;
    }
}

__global__ __launch_bounds__(256) void attn_train_ln_bwd_sums_kernel(AttnTrainLnBwd p) {
    __shared__ float red[4];
    const int b = blockIdx.y, row0 = blockIdx.x * RT, H = p.H;
    const int T1 = p.t1[b];
    const size_t base = ((size_t)b * p.T1 + row0) * H;
    const int rows = min(RT, p.T1 - row0), live = min(max(T1 - row0, 0), rows);
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < rows * H; i += 256) {
        const int r = i / H, col = i - r * H;
        float dy = 0.f, pr = 0.f;
        if (r < live) {
            dy = p.g1[base + i];
            if (p.g2) dy += p.g2[base + i];
            const float xn = p.xn[base + i], dxn = dy * p.gamma[col];
            pr = dy * xn;
            s1 += dxn;
            s2 += dxn * xn;
        }
        p.dy[base + i] = dy;
        p.prod[base + i] = pr;
    }
    const float t1s = block_sum(s1, red), t2s = block_sum(s2, red);
    const int ntile = (p.T1 + RT - 1) / RT;
    if (threadIdx.x == 0) p.sums[(size_t)b * ntile + blockIdx.x] = make_float2(t1s, t2s);
}

__global__ __launch_bounds__(256) void attn_train_ln_bwd_apply_kernel(AttnTrainLnBwd p) {
    __shared__ float2 slot;
    const int b = blockIdx.y, row0 = blockIdx.x * RT, H = p.H;
    const int T1 = p.t1[b];
    const size_t base = ((size_t)b * p.T1 + row0) * H;
    const int rows = min(RT, p.T1 - row0), live = min(max(T1 - row0, 0), rows);
    const int ntile = (p.T1 + RT - 1) / RT;
    if (threadIdx.x == 0) {
        float a = 0.f, c = 0.f;
        for (int i = 0; i < tiles_of(T1); ++i) {          // tile order
            const float2 s = p.sums[(size_t)b * ntile + i];
            a += s.x;
            c += s.y;
        }
        const float n = (float)max(T1, 1) * (float)H;
        slot = make_float2(a / n, c / n);
    }
    __syncthreads();
    const float m1 = slot.x, m2 = slot.y, rstd = p.rstd[b];
    for (int i = threadIdx.x; i < rows * H; i += 256) {
        const int r = i / H, col = i - r * H;
        float dx = 0.f;
        if (r < live) dx = rstd * (p.dy[base + i] * p.gamma[col] - m1 - p.xn[base + i] * m2);
        p.dx[base + i] = dx;
        if (p.ddrop) p.ddrop[base + i] = r < live ? dropped(dx, p.drop, p.site, b, 0, row0 + r, col) : 0.f;
    }
}

namespace {
unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }
dim3 tile_grid(int B, int T1) { return dim3((unsigned)((T1 + RT - 1) / RT), (unsigned)B); }
}  // namespace

hipError_t launch_attn_train_stack(const float* mel, const int32_t* tlen, const int32_t* t1, int B, int T, int T1, int F, int c, float* xs,
                                   hipStream_t st) {
    return launch_lds<attn_train_stack_kernel>(dim3(blocks_of((size_t)B * T1 * c * F)), dim3(256), 0, st, mel, tlen, t1, B, T, T1, F, c, xs);
}
hipError_t launch_attn_train_addpe(float* x, const float* pe, const int32_t* t1, int B, int T1, int H, hipStream_t st) {
    return launch_lds<attn_train_addpe_kernel>(dim3(blocks_of((size_t)B * T1 * H)), dim3(256), 0, st, x, pe, t1, B, T1, H);
}
hipError_t launch_attn_train_relu(float* v, const int32_t* t1, int B, int T1, int N, int relu, hipStream_t st) {
    return launch_lds<attn_train_relu_kernel>(dim3(blocks_of((size_t)B * T1 * N)), dim3(256), 0, st, v, t1, B, T1, N, relu);
}
hipError_t launch_attn_train_relumask(float* g, const float* post, const int32_t* t1, int B, int T1, int N, hipStream_t st) {
    return launch_lds<attn_train_relumask_kernel>(dim3(blocks_of((size_t)B * T1 * N)), dim3(256), 0, st, g, post, t1, B, T1, N);
}
hipError_t launch_attn_train_core_forward(const AttnTrainCore& p, hipStream_t st) {
    return with_int<16, 32>(p.H / p.NH, [&](auto d) {
        return with_int<64, 128, 256>(p.H, [&](auto h) {
            const size_t lds = (size_t)(RT * (h() + 4) + h() * (RT + 4)) * sizeof(float);
            return launch_lds<attn_train_core_forward_kernel<h(), d()>>(tile_grid(p.B, p.T1), dim3(256), lds, st, p);
        });
    });
}
hipError_t launch_attn_train_core_dq(const AttnTrainCore& p, hipStream_t st) {
    return with_int<16, 32>(p.H / p.NH, [&](auto d) { return launch_lds<attn_train_core_dq_kernel<d()>>(tile_grid(p.B, p.T1), dim3(256), 0, st, p); });
}
hipError_t launch_attn_train_core_dkv(const AttnTrainCore& p, hipStream_t st) {
    return with_int<16, 32>(p.H / p.NH, [&](auto d) { return launch_lds<attn_train_core_dkv_kernel<d()>>(tile_grid(p.B, p.T1), dim3(256), 0, st, p); });
}
hipError_t launch_attn_train_resid(const AttnTrainResid& p, hipStream_t st) {
    return launch_lds<attn_train_resid_kernel>(tile_grid(p.B, p.T1), dim3(256), 0, st, p);
}
hipError_t launch_attn_train_ln_forward(const AttnTrainLn& p, hipStream_t st) {
    return launch_lds<attn_train_ln_forward_kernel>(tile_grid(p.B, p.T1), dim3(256), 0, st, p);
}
hipError_t launch_attn_train_ln_bwd_sums(const AttnTrainLnBwd& p, hipStream_t st) {
    return launch_lds<attn_train_ln_bwd_sums_kernel>(tile_grid(p.B, p.T1), dim3(256), 0, st, p);
}
hipError_t launch_attn_train_ln_bwd_apply(const AttnTrainLnBwd& p, hipStream_t st) {
    return launch_lds<attn_train_ln_bwd_apply_kernel>(tile_grid(p.B, p.T1), dim3(256), 0, st, p);
}

}  // namespace kws
