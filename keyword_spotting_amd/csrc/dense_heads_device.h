// The per-frame pieces of a class head behind the GRU stack, shared by dense_heads_kernel (dense_heads.hip: kws_step_heads) and
// heads_window_kernel (heads_window.hip: the two-head stream manager), so that both compile the same code and a row's logits,
// softmax and word are the same bits through either: the projection of one frame from the top layer's xl seam, the row's
// relu / clip -> softmax -> ctc_decode2 frame rule, and the row store.
#pragma once
#include "gru_device.h"

namespace kws {
namespace {      // internal linkage, as when these lived in dense_heads.hip

// One frame of one head: v = the lane's xl float4 of every tile (the B operands of the k-chunks 4n..4n+3), wa = the fragments of
// Wfc^T (padded to 16 rows) the fused epilogue of the GRU kernels uses; the 16x16 result `acc` holds class 4g + r of stream s in
// lane (g, s).  The summation order of the fused epilogue (gru_resident.hip, gru_kernels.hip): four partial sums over a quarter of
// the units each -- there one per wave, the first one starting from bfc, the others from zero -- folded ((0 + 1) + 2) + 3
// (epilogue_fold), so that head 1 here and through kws_step is the same sum of the same products.
// A macro, as KWS_MFMA_A (gru_device.h), and not a function: as a function (by value or by reference, force-inlined) the compiler
// canonicalises the fold before it inlines it and dense_heads_kernel comes out with other instruction streams than it had with
// this text in its loop (tools/isa_diff.sh); expanded in place, the kernel is the same machine code.
#define KWS_HEAD_PROJECT(acc, NT, wa, bias4, v)                                                                              \
    f32x4 acc;                                                                                                               \
    {                                                                                                                        \
        f32x4 part[4] = {bias4, splat4(0.f), splat4(0.f), splat4(0.f)};                                                      \
        _Pragma("unroll") for (int n = 0; n < NT; ++n)                                                                       \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) part[n / (NT / 4)] = mfma4(wa[4 * n + e], v[n][e], part[n / (NT / 4)]); \
        acc = ((part[0] + part[1]) + part[2]) + part[3];                                                                     \
    }

// relu / clip, softmax and the ctc_decode2 frame rule of one row: the arithmetic of epilogue_flush (gru_device.h)
__device__ __forceinline__ int head_row(float (&lg)[kMaxClasses], float (&pr)[kMaxClasses], int C, int use_relu, float value_clip, float thres) {
    if (use_relu) {
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c) {
            lg[c] = fmaxf(lg[c], 0.f);
            if (value_clip > 0.f) lg[c] = fminf(lg[c], 20.f);
        }
    }
    float m = lg[0];
#pragma unroll
    for (int c = 1; c < kMaxClasses; ++c) m = (c < C) ? fmaxf(m, lg[c]) : m;
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
        pr[c] = (c < C) ? __expf(lg[c] - m) : 0.f;
        sum += pr[c];
    }
    const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) pr[c] *= inv;
    // classes 1..C-2 (utils/prediction.py:67,74-75): first maximum, strict >
    int word = -1;
    float best = -1.f;
#pragma unroll
    for (int c = 1; c < kMaxClasses - 1; ++c) {
        if (c < C - 1 && pr[c] > best) { best = pr[c]; word = c - 1; }
    }
    return best > thres ? word : -1;
}

// a row of C floats; rows of an even C are 8-byte aligned (the outputs are, as kws_step's)
__device__ __forceinline__ void store_row(float* dst, const float (&v)[kMaxClasses], int C) {
    if ((C & 1) == 0) {
        float2* o = reinterpret_cast<float2*>(dst);
#pragma unroll
        for (int c = 0; c < kMaxClasses / 2; ++c)
            if (2 * c < C) o[c] = make_float2(v[2 * c], v[2 * c + 1]);
    } else {
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c)
            if (c < C) dst[c] = v[c];
    }
}

}  // namespace
}  // namespace kws
