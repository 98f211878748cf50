// The phases of the class-head kernels behind the GRU stack, each defined once: dense_heads_kernel (dense_heads.hip: kws_step_heads),
// heads_window_kernel (heads_window.hip: the two-head stream manager) and the two bank kernels (bank_heads.hip, with bank_device.h
// for what only a bank has) all compile this code, so a row's logits, softmax and word are the same bits through any of them.
//   per frame      head_operands, seam_row / seam_row_step, KWS_HEAD_PROJECT; the row tail (load_row8 / store_row8, head_row,
//                  store_row) is gru_device.h's, shared with the fused epilogues of the GRU kernels
//   a step         heads_tokens (tokens and the carried word of a frame block)
//   a manager      heads_window_carve (the LDS of the launch), heads_window_couple (a hit of either head clears both windows)
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

// A operands of one head (DenseHead or HeadsWindowHead): Wfc^T, k-chunk kc in wa[kc], and the lane's four biases; an absent head
// (on == false) reads nothing and keeps zeros
template <int NT, class Head>
__device__ __forceinline__ void head_operands(const Head& hp, bool on, int lane, int g, float (&wa)[4 * NT], f32x4& bias4) {
#pragma unroll
    for (int kc = 0; kc < 4 * NT; ++kc) wa[kc] = on ? hp.wfc[kc * 64 + lane] : 0.f;
    bias4 = on ? ld4(hp.bfc + 4 * g) : splat4(0.f);
}

// The lane's xl float4 of every tile of frame t; src = the group's seam + lane
template <int NT>
__device__ __forceinline__ void seam_row(const float4* src, int t, f32x4 (&v)[NT]) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const float4 x = src[((size_t)t * NT + n) * 64];
        v[n] = (f32x4){x.x, x.y, x.z, x.w};
    }
}

// ... of a step (dense_heads.hip, "Rows past seq_len"): frames t >= len are dynamic_rnn's zero row whatever the seam holds, and the
// row that is used is the row nn_outputs [B,T,H] gets (store: the frame is the block's own and stream b is in the batch)
template <int NT>
__device__ __forceinline__ void seam_row_step(const float4* src, int t, int len, float* nn_outputs, bool store, int b, int T, int g, f32x4 (&v)[NT]) {
    seam_row<NT>(src, t, v);
    if (t >= len) {
#pragma unroll
        for (int n = 0; n < NT; ++n) v[n] = splat4(0.f);
    }
    if (nn_outputs && store) {
        float4* dst = reinterpret_cast<float4*>(nn_outputs + ((size_t)b * T + t) * (16 * NT) + 4 * g);
#pragma unroll
        for (int n = 0; n < NT; ++n) dst[4 * n] = make_float4(v[n][0], v[n][1], v[n][2], v[n][3]);
    }
}

constexpr int kHeadSlots = kHeadFrames + 1;        // a step's workgroup: slot f <-> frame t0 - 1 + f; slot 0 is the halo

// Tokens (utils/prediction.py:76-80) and the carried word of a step's frame block, from the frame words [head][16 streams][kHeadSlots]
// in LDS (complete and visible: the caller has synchronised).  256 threads call this.
__device__ __forceinline__ void heads_tokens(const DenseHeadsParams& p, const int* words, int G, int t0, int tid) {
    const int T = p.T;
    for (int item = tid; item < 16 * kHeadFrames; item += 256) {
        const int si = item / kHeadFrames, f = 1 + (item - si * kHeadFrames);
        const int t = t0 - 1 + f, bi = G * kStreamsPerGroup + si;
        if (t >= T || bi >= p.B) continue;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            const DenseHead& hp = p.head[hd];
            if (hp.C == 0 || !hp.prev_word) continue;
            const int word = words[(hd * 16 + si) * kHeadSlots + f];
            int prev;
            if (t == 0) prev = (p.reset && p.reset[bi]) ? -1 : hp.prev_in[bi];
            else prev = words[(hd * 16 + si) * kHeadSlots + f - 1];
            if (hp.tokens) hp.tokens[(size_t)bi * T + t] = (int8_t)((word >= 0 && word != prev) ? word + 1 : 0);
            if (t == T - 1) hp.prev_word[bi] = word;
        }
    }
}

// The LDS of a window launch, in the order of heads_window_lds_bytes (kws_internal.h); rest: what a caller asked for beyond it
struct HeadsWindowLds {
    float* lgs;         // [head][stream][frame of the block][8]
    int8_t* cw;         // [head][stream][stride] the chunk's frame words
    uint8_t* dl;        // [head][16 states][16 words] the label matchers
    char* scratch;      // window 1's ring staging | window 2's
    char* rest;
    int stride;
};
__device__ __forceinline__ HeadsWindowLds heads_window_carve(char* lds, int T, int nq1, int nq2) {
    HeadsWindowLds L;
    L.stride = heads_window_stride(T);
    L.lgs = reinterpret_cast<float*>(lds);
    L.cw = reinterpret_cast<int8_t*>(lds + kHeadsWindowLogitsBytes);
    L.dl = reinterpret_cast<uint8_t*>(L.cw) + (size_t)2 * 16 * L.stride;
    L.scratch = reinterpret_cast<char*>(L.dl) + 512;
    L.rest = L.scratch + window_tail_scratch_bytes(nq1) + window_tail_scratch_bytes(nq2);
    return L;
}

// The coupling of the two windows, behind their tails: fired = hit_1 | hit_2, and if fired the q == 0 lane of the stream writes
// head = count = 0 for BOTH windows and restart = 1 -- "the other head fired" is the same state change as "this head fired"
// (tests/test_heads_stream_host.py).  hit[b] = hit_1 | hit_2 << 1.  bt, live: window_tail's stream of this lane and whether it
// writes; hit2w: window 2's own verdict, which counts only where has_head2(bt) -- asked by the writing lane alone.
// (The tails wrote hit / head / count of their own window from this same lane: these stores follow them in program order.)
template <class Gate>
__device__ __forceinline__ void heads_window_couple(const HeadsWindowParams& p, int b0, int tid, int bt, bool live, bool hit1, bool hit2w, Gate has_head2) {
    if ((tid & 15) == 0 && b0 + (tid >> 4) < p.B) {
        if (live) {
            const bool hit2 = hit2w && has_head2(bt);
            const bool fired = hit1 || hit2;
            if (fired) {                                         // detector.py:202-208, whichever head fired
                p.win[0].head[bt] = 0; p.win[0].count[bt] = 0;
                p.win[1].head[bt] = 0; p.win[1].count[bt] = 0;
            }
            if (p.restart) p.restart[bt] = fired ? 1 : 0;
            p.hit[bt] = (hit1 ? 1 : 0) | (hit2 ? 2 : 0);
        } else {
            p.hit[bt] = 0;
        }
    }
}

}  // namespace
}  // namespace kws
