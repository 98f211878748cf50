// Training of the GRU stack under the cell wrappers of get_cell (utils/custom_wrapper.py:95-158): the row kernels around the two frame
// loops of gru_train.hip.  Both wrappers act on whole rows [B*T, width] outside the recurrence:
//
//   train_ln_forward_kernel    LayerNormalizer on a layer's input: m = mean(x), v = mean((x - m)^2), rstd = 1 / sqrt(v + 1e-5),
//                              xn = (x - m) rstd, x^ = xn ibeta + igamma (ibeta the scalar scale, igamma the per-feature shift).
//                              The tape keeps x^ (the cell's x-part reads it), xn and rstd.
//   train_ln_backward_kernel   given g = dx^ of a row: dn = g ibeta, a = mean(dn), c = mean(dn o xn),
//                              d in = rstd (dn - a - xn c) [+ the residual's share], and the row's term of d ibeta: sum_i g_i xn_i.
//                              The sums over the rows (d ibeta from those terms, d igamma from g itself) are column sums of the
//                              weight-gradient launch (train_wgrad_kernel, kWgradOnes): the same row chunks, the same fixed order.
//   train_residual_kernel      out = s (a + b) over whole blocks: the residual's forward 0.7071 (y + in), the scaling of dout in front
//                              of the backward frame loop (b absent) and the sum of the two shares of d in (s = 1).
//
// One wave per row in the two layer-norm kernels: a row has 1 .. 1024 values, lane i holds values i, i + 64, ... (up to 16) in
// registers for both passes -- the variance is taken around the mean, as the serving kernel and the fp64 restatement take it.  Dead
// rows (t >= seq_len[b], empty slots) are written as zeros and never read: the padding of x may be NaN.
#include "gru_device.h"
#include "launch.h"

namespace kws {

namespace {

constexpr int kLnPerLane = 16;          // 1024 values of the widest row over 64 lanes
constexpr float kLnEpsilon = 1e-5f;     // utils/custom_wrapper.py:126

// the sum over the wave in every lane: a butterfly, the same order whatever the row
__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace

__global__ void __launch_bounds__(256) train_ln_forward_kernel(const TrainLnForward p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (row >= p.M) return;
    const int I = p.I, nj = (I + 63) >> 6;
    const size_t at = (size_t)row * I;
    if (p.live[row] == 0) {          // wave-uniform
        for (int i = lane; i < I; i += 64) { p.xhat[at + i] = 0.f; p.xn[at + i] = 0.f; }
        if (lane == 0) p.rstd[row] = 0.f;
        return;
    }
    float v[kLnPerLane];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < kLnPerLane; ++j) {
        const int i = lane + 64 * j;
        v[j] = (j < nj && i < I) ? p.in[at + i] : 0.f;
        sum += v[j];
    }
    const float mean = ln_wave_sum(sum) / (float)I;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < kLnPerLane; ++j) {
        v[j] = (lane + 64 * j < I) ? v[j] - mean : 0.f;
        sq = fmaf(v[j], v[j], sq);
    }
    const float rstd = 1.0f / sqrtf(ln_wave_sum(sq) / (float)I + kLnEpsilon);
    const float scale = *p.ibeta;
#pragma unroll
    for (int j = 0; j < kLnPerLane; ++j) {
        const int i = lane + 64 * j;
        if (j < nj && i < I) {
            const float xn = v[j] * rstd;
            p.xn[at + i] = xn;
            p.xhat[at + i] = fmaf(xn, scale, p.igamma[i]);
        }
    }
    if (lane == 0) p.rstd[row] = rstd;
}

hipError_t launch_train_ln_forward(const TrainLnForward& p, hipStream_t st) {
    return launch_lds<train_ln_forward_kernel>(dim3((unsigned)(((long)p.M + 3) / 4)), dim3(256), 0, st, p);
}

__global__ void __launch_bounds__(256) train_ln_backward_kernel(const TrainLnBackward p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (row >= p.M) return;
    const int I = p.I, nj = (I + 63) >> 6;
    const size_t at = (size_t)row * I;
    if (p.live[row] == 0) {          // wave-uniform
        if (p.din != nullptr)
            for (int i = lane; i < I; i += 64) p.din[at + i] = 0.f;
        if (lane == 0) p.gs[row] = 0.f;
        return;
    }
    const float scale = *p.ibeta;
    float dn[kLnPerLane], xn[kLnPerLane];
    float sa = 0.f, sc = 0.f, ss = 0.f;
#pragma unroll
    for (int j = 0; j < kLnPerLane; ++j) {
        const int i = lane + 64 * j;
        const bool in = j < nj && i < I;
        const float g = in ? p.g[at + i] : 0.f;
        xn[j] = in ? p.xn[at + i] : 0.f;
        dn[j] = g * scale;
        sa += dn[j];
        sc = fmaf(dn[j], xn[j], sc);
        ss = fmaf(g, xn[j], ss);
    }
    ss = ln_wave_sum(ss);
    if (lane == 0) p.gs[row] = ss;
    if (p.din == nullptr) return;          // layer 0: the two parameter gradients only
    const float a = ln_wave_sum(sa) / (float)I, c = ln_wave_sum(sc) / (float)I, rstd = p.rstd[row];
#pragma unroll
    for (int j = 0; j < kLnPerLane; ++j) {
        const int i = lane + 64 * j;
        if (j < nj && i < I) {
            const float d = rstd * (dn[j] - a - xn[j] * c);
            p.din[at + i] = p.resid != nullptr ? d + p.resid[at + i] : d;
        }
    }
}

hipError_t launch_train_ln_backward(const TrainLnBackward& p, hipStream_t st) {
    return launch_lds<train_ln_backward_kernel>(dim3((unsigned)(((long)p.M + 3) / 4)), dim3(256), 0, st, p);
}

__global__ void __launch_bounds__(256) train_residual_kernel(const float* a, const float* b, float s, float* out, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = ld4(a + 4 * i);
    if (b != nullptr) v += ld4(b + 4 * i);
    *reinterpret_cast<f32x4*>(out + 4 * i) = v * s;
}

hipError_t launch_train_residual(const float* a, const float* b_or_null, float s, float* out, size_t n, hipStream_t st) {
    return launch_lds<train_residual_kernel>(dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, a, b_or_null, s, out, n / 4);
}

}  // namespace kws
