// Training of the GRU stack, everything around the two frame loops of gru_train.hip: the whole-batch GEMMs (x-part products, logits,
// dy of the layer below), the weight-gradient reduction over the B*T rows, its fixed-order sum with the global norm, the optimiser and
// the re-pack of the weights the frame loops and GEMMs read.  No float atomic anywhere: two identical calls give identical bits.
//
// The GEMMs are v_mfma_f32_16x16x4_f32 products on operands read straight from row-major memory.  K is walked in blocks of 16 with the
// "xl" k map of the serving kernels (chunk e of a block has k = 4 g + e on lane group g), so that an activation row is one 16-byte
// load per lane and block where its stride allows it.
#include "gru_device.h"
#include "launch.h"

namespace kws {

// ------------------------------------------------------------------------------------------------
// out [M, N] = bias + a [M, K] . W: a wave owns 16 rows x (16 NJ) columns, D[column][row]
// ------------------------------------------------------------------------------------------------
constexpr int kRowsGemmTiles = 4;      // column tiles per wave
constexpr int kRowsGemmSets = 4;       // accumulators per tile (the sum at the end is written for four)

__global__ void __launch_bounds__(256) train_rows_gemm_kernel(const TrainRowsGemm p) {
    constexpr int NJ = kRowsGemmTiles;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 4, s = lane & 15;
    const long row = ((long)blockIdx.x * 4 + w) * 16 + s;
    const int n0 = blockIdx.y * 16 * NJ;
    const bool rvalid = row < p.M && (p.live == nullptr || p.live[row] != 0);
    const bool vec = (p.lda & 3) == 0 && (reinterpret_cast<uintptr_t>(p.a) & 15u) == 0;
    const float* arow = p.a + (size_t)(rvalid ? row : 0) * p.lda;
    // kRowsGemmSets accumulators per tile, k-block q into set q mod kRowsGemmSets, summed pairwise at the end: the rounding error of a
    // product over K = 3H grows with the length of its chain (a gradient is compared with a float32 reference at a few ulps), and
    // independent chains keep the matrix pipe busy
    constexpr int NS = kRowsGemmSets;
    f32x4 acc[NS][NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int q = 1; q < NS; ++q) acc[q][j] = splat4(0.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = n0 + 16 * j + 4 * g + e;
            acc[0][j][e] = (p.bias != nullptr && n < p.N) ? p.bias[n] : 0.f;
        }
    }
    auto block = [&](int k0, f32x4* set) {
        const int k = k0 + 4 * g;
        f32x4 av = splat4(0.f);
        if (rvalid) {
            if (vec && k + 3 < p.K) {
                av = ld4(arow + k);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) av[e] = (k + e < p.K) ? arow[k + e] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool kin = k + e < p.K;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = n0 + 16 * j + s;
                const float wv = (kin && n < p.N) ? p.w[(size_t)(k + e) * p.swk + (size_t)n * p.swn] : 0.f;
                set[j] = mfma4(wv, av[e], set[j]);
            }
        }
    };
    for (int k0 = 0; k0 < p.K; k0 += 16 * NS) {
#pragma unroll
        for (int q = 0; q < NS; ++q)
            if (k0 + 16 * q < p.K) block(k0 + 16 * q, acc[q]);          // uniform
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[0][j] = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
    if (row < p.M) {
        float* orow = p.out + (size_t)row * p.ldo;
        const bool ovec = (p.ldo & 3) == 0 && (reinterpret_cast<uintptr_t>(p.out) & 15u) == 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = n0 + 16 * j + 4 * g;
            if (ovec && n + 3 < p.N) {
                *reinterpret_cast<f32x4*>(orow + n) = acc[0][j];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (n + e < p.N) orow[n + e] = acc[0][j][e];
            }
        }
    }
}

hipError_t launch_train_rows_gemm(const TrainRowsGemm& p, hipStream_t st) {
    const dim3 grid((unsigned)(((long)p.M + 63) / 64), (unsigned)((p.N + 16 * kRowsGemmTiles - 1) / (16 * kRowsGemmTiles)));
    return launch_lds<train_rows_gemm_kernel>(grid, dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------------
// Weight gradients: out [K, N] = sum over rows of a[row, :]^T d[row, :], the long dimension (rows) on the MFMA's k.  A wave owns
// 16 k x 64 n outputs of one job and one row chunk; D[n][k]: A operand = d (lane (g, i): d[row + g][n + i]), B operand = a (lane
// (g, s): a[row + g][k + s]).  Dead rows (t >= seq_len, empty slots) are masked on BOTH operands: the padding of X may be NaN.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) train_wgrad_kernel(const TrainWgradJob* __restrict__ jobs, int njobs, int units,
                                                          const float* __restrict__ x, const uint8_t* __restrict__ live, int M, int chunk_rows,
                                                          float* __restrict__ partial, size_t P) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 4, s = lane & 15;
    const int unit = blockIdx.x * 4 + w;
    if (unit >= units) return;
    int jb = 0;
    while (jb + 1 < njobs && jobs[jb + 1].unit0 <= unit) ++jb;
    const TrainWgradJob job = jobs[jb];
    const int ngroups = (job.N + 63) / 64, local = unit - job.unit0;
    const int k0 = 16 * (local / ngroups), n0 = 64 * (local % ngroups);
    const long r0 = (long)blockIdx.y * chunk_rows;
    const long r1 = r0 + chunk_rows < M ? r0 + chunk_rows : M;
    const bool kin = k0 + s < job.K;
    const float* a = job.src == kWgradInput ? x : job.a;
    // four accumulators per tile, rows r + 4 q .. r + 4 q + 3 into set q, summed pairwise at the end (shorter chains: see the GEMM)
    f32x4 acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[q][j] = splat4(0.f);
    for (long r = r0; r < r1; r += 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long row = r + 4 * q + g;
            const bool ok = row < r1 && live[row] != 0;
            const float bv = (ok && kin) ? (job.src != kWgradOnes ? a[(size_t)row * job.lda + k0 + s] : 1.0f) : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + 16 * j + s;
                const float av = (ok && n < job.N) ? job.d[(size_t)row * job.ldd + n] : 0.f;
                acc[q][j] = mfma4(av, bv, acc[q][j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[0][j] = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
    if (kin) {
        float* o = partial + (size_t)blockIdx.y * P + job.out + (size_t)(k0 + s) * job.ldo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int n = n0 + 16 * j + 4 * g + e;
                if (n < job.N) o[n] = acc[0][j][e];
            }
        }
    }
}

hipError_t launch_train_wgrad(const TrainWgradJob* jobs, int njobs, int units, const float* x, const uint8_t* live, int M, int chunk_rows,
                              int chunks, float* partial, size_t P, hipStream_t st) {
    return launch_lds<train_wgrad_kernel>(dim3((unsigned)((units + 3) / 4), (unsigned)chunks), dim3(256), 0, st, jobs, njobs, units, x, live, M,
                                          chunk_rows, partial, P);
}

// ------------------------------------------------------------------------------------------------
// grad = the chunks' partial sums in chunk order; per workgroup the sum of grad^2 (double; per thread in index order, then a fixed tree)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) train_reduce_kernel(const float* __restrict__ partial, int chunks, size_t P, float* __restrict__ grad,
                                                           double* __restrict__ sumsq) {
    __shared__ double red[256];
    const size_t base = (size_t)blockIdx.x * kTrainReduceSpan;
    double sq = 0.0;
    for (int i = threadIdx.x; i < kTrainReduceSpan; i += 256) {
        const size_t at = base + i;
        if (at < P) {
            float v = 0.f;
            for (int c = 0; c < chunks; ++c) v += partial[(size_t)c * P + at];
            grad[at] = v;
            sq += (double)v * (double)v;
        }
    }
    red[threadIdx.x] = sq;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) sumsq[blockIdx.x] = red[0];
}

hipError_t launch_train_reduce(const float* partial, int chunks, size_t P, float* grad, double* sumsq, hipStream_t st) {
    return launch_lds<train_reduce_kernel>(dim3((unsigned)train_reduce_blocks(P)), dim3(256), 0, st, partial, chunks, P, grad, sumsq);
}

// ------------------------------------------------------------------------------------------------
// tf.clip_by_global_norm, then tf.train.AdamOptimizer (epsilon outside the root; lr_t carries both bias corrections) or
// tf.train.MomentumOptimizer(momentum = 0.9, use_nesterov = True): a <- 0.9 a + g; theta <- theta - lr g - lr 0.9 a
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) train_update_kernel(float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v,
                                                           const float* __restrict__ grad, const double* __restrict__ sumsq, int nblocks,
                                                           size_t P, int adam, float lr_t, float max_grad_norm, float* __restrict__ grad_norm) {
    __shared__ float norm_s;
    if (threadIdx.x == 0) {          // every workgroup adds the same values in the same order
        double t = 0.0;
        for (int i = 0; i < nblocks; ++i) t += sumsq[i];
        norm_s = (float)sqrt(t);
        if (blockIdx.x == 0 && grad_norm != nullptr) *grad_norm = norm_s;
    }
    __syncthreads();
    const float norm = norm_s;
    const float factor = max_grad_norm > 0.f ? max_grad_norm / fmaxf(norm, max_grad_norm) : 1.0f;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float g = grad[i] * factor;
    if (adam) {
        // m += (g - m) (1 - beta1), v += (g^2 - v) (1 - beta2) as TensorFlow's kernel writes them, with 1 - beta the float nearest to
        // 0.1 / 0.001: 1.0f - 0.999f is 0.00099998713, and v came out 1.29e-5 below Adam's (kws_train_moments against the fp64
        // optimiser, seven times the floor of that comparison); 1 - 0.001f is 0.999 to 5e-11
        const float m1 = m[i] + (g - m[i]) * 0.1f;
        const float v1 = v[i] + (g * g - v[i]) * 0.001f;
        m[i] = m1;
        v[i] = v1;
        theta[i] -= lr_t * m1 / (sqrtf(v1) + 1e-8f);
    } else {
        const float a = 0.9f * m[i] + g;
        m[i] = a;
        theta[i] = theta[i] - lr_t * g - lr_t * 0.9f * a;
    }
}

hipError_t launch_train_update(float* theta, float* m, float* v, const float* grad, const double* sumsq, int nblocks, size_t P, int adam,
                               float lr_t, float max_grad_norm, float* grad_norm_or_null, hipStream_t st) {
    return launch_lds<train_update_kernel>(dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, theta, m, v, grad, sumsq, nblocks, P, adam, lr_t,
                                           max_grad_norm, grad_norm_or_null);
}

// ------------------------------------------------------------------------------------------------
// the copies of a layer's weights the kernels above and the frame loops read (kws_internal.h), from the canonical blob on the device
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) train_pack_kernel(const TrainPackParams p) {
    const TrainPackLayer l = p.layer[blockIdx.y];
    const int H = p.H, H3 = 3 * H;
    const int total = (l.in + H) * H3;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int k = idx / H3, n = idx - k * H3;
        const float v = n < 2 * H ? l.wg[(size_t)k * 2 * H + n] : l.wc[(size_t)k * H + n - 2 * H];
        if (k < l.in) {
            l.wx[idx] = v;
        } else {
            l.wh[(size_t)(k - l.in) * H3 + n] = v;
            l.wht[(size_t)n * H + (k - l.in)] = v;
        }
        if (idx < H3) l.b3[idx] = idx < 2 * H ? l.bg[idx] : l.bc[idx - 2 * H];
    }
}

hipError_t launch_train_pack(const TrainPackParams& p, hipStream_t st) {
    return launch_lds<train_pack_kernel>(dim3(256, (unsigned)p.L), dim3(256), 0, st, p);
}

__global__ void __launch_bounds__(256) train_rowmask_kernel(const int32_t* __restrict__ seq_len, int B, int T, uint8_t* __restrict__ live) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * T) return;
    const int b = (int)(i / T), t = (int)(i - (size_t)b * T);
    live[i] = t < seq_len[b] ? 1 : 0;
}

hipError_t launch_train_rowmask(const int32_t* seq_len, int B, int T, uint8_t* live, hipStream_t st) {
    return launch_lds<train_rowmask_kernel>(dim3((unsigned)(((size_t)B * T + 255) / 256)), dim3(256), 0, st, seq_len, B, T, live);
}

// ------------------------------------------------------------------------------------------------
// grad_logits of ctc_loss_kernel -> the gradient of sum(loss) / B, a thread per frame.  A row of the CTC kernel is softmax - occupancy
// with occupancy = exp(alpha + beta - lp + nll) from the fp32 log-domain recursions: what alpha, beta and nll have drifted by over the
// frames is one factor (1 - delta) on all occupancies of a frame, of one sign for much of an utterance, so it does not average out
// over the rows (T = 250: 1.2e-4 on dbfc, four times the deviation of the float32 reference).  The occupancies of a frame sum to 1,
// so delta = sum_c g[c] -- 0 in exact arithmetic -- measures the factor, and g[c] - occupancy[c] * delta takes it out, with
// occupancy[c] = softmax[c] - g[c] from the logits.  A row of zeros (t >= seq_len, an empty slot, no valid path) stays zeros.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) train_scale_kernel(float* __restrict__ g, const float* __restrict__ logits, size_t rows, int C, float s) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    float v[kMaxClasses], z[kMaxClasses];
    float delta = 0.f, mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
        v[c] = c < C ? g[row * C + c] : 0.f;
        z[c] = c < C ? logits[row * C + c] : -INFINITY;
        delta += v[c];
        mx = fmaxf(mx, z[c]);
    }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
        z[c] = c < C ? expf(z[c] - mx) : 0.f;
        sum += z[c];
    }
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
        if (c < C) g[row * C + c] = (v[c] - (z[c] / sum - v[c]) * delta) * s;
}

hipError_t launch_train_scale(float* g, const float* logits, size_t rows, int C, float s, hipStream_t st) {
    return launch_lds<train_scale_kernel>(dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, g, logits, rows, C, s);
}

}  // namespace kws
