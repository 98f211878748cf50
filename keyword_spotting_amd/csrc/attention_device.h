// Device helpers shared by the attention kernel files (attention_kernels.hip: fp32 MFMAs; attention_f16x3.hip: the fp16 matrix
// pipe): utterance geometry, the layer norm's per-tile (count, mean, M2) partials and their Chan merge, fixed-order block sums.
// Everything here is precision-independent: both kernel families produce and consume the same partial tables.
#pragma once
#include "attention_internal.h"

namespace kws {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int RT = kAttnRows;
constexpr float kLnEps = 1e-12f;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

__device__ __forceinline__ int frames_out(int T, int c) { return c > 1 ? T / c + 1 : T; }
__device__ __forceinline__ int utt_len(const AttnParams& p, int b) {
    const int t = p.lengths ? p.lengths[b] : p.T_max;
    return min(max(t, 0), p.T_max);
}
__device__ __forceinline__ float ln1(float v, float2 ms, float g, float bt) { return (v - ms.x) * ms.y * g + bt; }

// Chan's merge of the utterance's per-tile (count, mean, M2), in tile order -> (mean, 1 / sqrt(var + eps)), population variance
__device__ float2 ln_merge(const float4* part, int n) {
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    for (int i = 0; i < n; ++i) {
        const float4 q = part[i];
        const float nab = cnt + q.x;
        const float d = q.y - mean;
        mean += d * (q.x / nab);
        m2 += q.z + d * d * (cnt * q.x / nab);
        cnt = nab;
    }
    return make_float2(mean, 1.0f / sqrtf(m2 / cnt + kLnEps));
}
// the merged statistics of the utterance, broadcast to the block (every thread must call it)
__device__ float2 ln_stats_block(const float4* part, int n, float2* slot) {
    if (threadIdx.x == 0) *slot = ln_merge(part, n);
    __syncthreads();
    return *slot;
}

__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over the block's 4 waves, in a fixed order
__device__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                       // red may still be read by the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// (count, mean, M2) of the tile's n valid elements: s = this thread's sum of them; dev(mean) = its sum of squared deviations
template <class Dev>
__device__ void tile_partial(float4* out, float s, float n, float* red, Dev dev) {
    const float mean = block_sum(s, red) / n;
    const float m2 = block_sum(dev(mean), red);
    if (threadIdx.x == 0) *out = make_float4(n, mean, m2, 0.f);
}

}  // namespace
}  // namespace kws
