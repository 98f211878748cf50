// The per-stream pieces of a bank of enrolled heads (kws_bank), shared by bank_heads_kernel (kws_step_bank) and bank_heads_window_kernel
// (the bank stream manager) so that both compile the same code and a row's head-2 logits, softmax and word are the same bits
// through either.  Stream b projects its new classes with the columns of bank slot user[b]: sixteen streams of a group have sixteen
// different [H, n_new] matrices, so this is VALU work on the seam values a lane already holds, not a second MFMA projection -- head 2's
// frozen logits ARE head 1's accumulator (weights.extend_head: trained words, new words, blank).
#pragma once
#include "dense_heads_device.h"

namespace kws {
namespace {

constexpr int kBankMaxNew = 5;      // C >= 3 and C + n_new <= 8

// the stream's slot, or -1: no second head (b past the batch, or user[b] outside [0, capacity): nothing is read out of bounds)
__device__ __forceinline__ int bank_user(const BankRef& k, int b, int B) {
    if (b >= B) return -1;
    const int u = k.user[b];
    return (u >= 0 && u < k.capacity) ? u : -1;
}

// The group's columns -> LDS once per workgroup, in the xl lane order of the seam: cols[class j][tile n][lane (g, s)][r] is
// Wn[user[s]][16 n + 4 g + r][j], so that a lane reads the four weights of its float4 of tile n as one b128, consecutive lanes on
// consecutive 16 bytes; bias[s][8] the stream's bn padded.  Sixteen threads per stream: the stream's slot is looked up once, and its
// [H, n_new] block is read front to back, 64 contiguous bytes per step; a stream without a slot stages zeros.  256 threads call this;
// the caller synchronises before bank_project.
template <int NT>
__device__ __forceinline__ void bank_stage(const BankRef& k, int b0, int B, float* cols, float* bias, int tid) {
    const int n_new = k.n_new, per = 16 * NT * n_new;
    const int s = (tid >> 4) & 15, q = tid & 15;
    const int u = bank_user(k, b0 + s, B);
    const float* src = k.Wn + (size_t)(u >= 0 ? u : 0) * per;
    for (int i = q; i < per; i += 16) {
        const int h = i / n_new, j = i - h * n_new;
        const float w = u >= 0 ? src[i] : 0.f;
        const int n = h >> 4, g = (h >> 2) & 3, r = h & 3;
        cols[((j * NT + n) * 64 + 16 * g + s) * 4 + r] = w;
    }
    if (q < 8) bias[s * 8 + q] = (u >= 0 && q < n_new) ? k.bn[(size_t)u * n_new + q] : 0.f;
}

// One frame's new classes of stream s: v = the lane's xl float4 of every tile (units 16 n + 4 g + r).  Per class a lane sums its
// 4 NT products in tile order, then the four g lanes of the stream fold as (g0 + g1) + (g2 + g3) -- two xor exchanges, every lane
// gets the same bits -- and the bias is added last, so a zero row gives exactly bn.  Whole waves call this (the exchanges).
template <int NT>
__device__ __forceinline__ void bank_project(const f32x4 (&v)[NT], const float* cols, const float* bias, int n_new, int lane, float (&out)[8]) {
    const f32x4* c4 = reinterpret_cast<const f32x4*>(cols) + lane;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = 0.f;
#pragma unroll
    for (int j = 0; j < kBankMaxNew; ++j) {
        if (j < n_new) {
            float part = 0.f;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const f32x4 c = c4[(j * NT + n) * 64];
#pragma unroll
                for (int r = 0; r < 4; ++r) part = __builtin_fmaf(v[n][r], c[r], part);
            }
            part = part + __shfl_xor(part, 16);
            part = part + __shfl_xor(part, 32);
            out[j] = part + bias[(lane & 15) * 8 + j];
        }
    }
}

// The keyword form (kws_bank_set_keyword on any slot of the bank): the group's sixteen label matchers -> LDS next to the columns, one
// 16-byte load per thread, and per stream kwn[2 s] = n_label, kwn[2 s + 1] = n_used | own << 8.  A stream whose slot has no keyword of
// its own (or no slot) stages no matcher: it walks window 2's (default_label = that window's n_label) over the bank's full width.
// 256 threads call this; the caller synchronises before bank_keyword_*.
__device__ __forceinline__ void bank_keywords_stage(const BankRef& k, const BankSlotKeyword* slots, int b0, int B, int default_label,
                                                    uint8_t* kwdl, int* kwn, int tid) {
    const int s = (tid >> 4) & 15, q = tid & 15;
    const int u = bank_user(k, b0 + s, B);
    const BankSlotKeyword* slot = slots + (u >= 0 ? u : 0);
    const bool own = u >= 0 && slot->own != 0;
    if (own) *reinterpret_cast<uint4*>(kwdl + s * 256 + 16 * q) = *reinterpret_cast<const uint4*>(slot->delta + 16 * q);
    if (q == 0) {
        kwn[2 * s] = own ? slot->n_label : default_label;
        kwn[2 * s + 1] = own ? (slot->n_used | 256) : k.n_new;
    }
}
__device__ __forceinline__ int bank_keyword_width(const int* kwn, int s) { return kwn[2 * s + 1] & 255; }      // the stream's n_used

// Head 2's row from head 1's raw logits and the stream's new classes: lg1[0..C-2], nw[0..n_new-1], lg1[C-1] (the blank last)
__device__ __forceinline__ void bank_row(const float (&lg1)[kMaxClasses], const float (&nw)[kMaxClasses], int C, int n_new, float (&lg2)[kMaxClasses]) {
    float blank = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) blank = (c == C - 1) ? lg1[c] : blank;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
        float x = (c < C - 1) ? lg1[c] : 0.f;
#pragma unroll
        for (int j = 0; j < kBankMaxNew; ++j) x = (j < n_new && c == C - 1 + j) ? nw[j] : x;
        lg2[c] = (c == C - 1 + n_new) ? blank : x;
    }
}

}  // namespace
}  // namespace kws
