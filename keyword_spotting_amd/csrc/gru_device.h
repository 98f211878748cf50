// Device helpers shared by the GRU kernels (gru_kernels.hip, gru_resident.hip, gru_bf16.hip, gru_f16x3.hip, gru_f16x3_generic.hip, gru_octbit.hip),
// the class-head kernels (through dense_heads_device.h) and the mel front-ends (frontend_kernels.hip, fft_frontend.hip):
//   arithmetic      mfma4, KWS_MFMA_A and its fences, the activations, bitsel, static_for, lds_barrier
//   the row tail    head_row, store_row, load_row8 / store_row8 -- one text for every path that turns 8 logits into a row of outputs --
//                   and carried_word, the word a stream brings into a call
//   the epilogues   epilogue_fold / epilogue_flush (a folded ring) and epilogue_flush_partials (the resident kernels), store_rows
// The f16x3 operand split is f16x3_device.h, the layer-pipelined protocol pipeline_device.h.
#pragma once
#include <type_traits>

#include "kws_internal.h"

namespace kws {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// sigma(x) = 1/(1+e^-x).  v_exp_f32 path: abs error <= 3e-7 on [-30,30]; saturates cleanly.
__device__ __forceinline__ float sigmoid_f(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __expf(-x));
}
// tanh(x) = 1 - 2/(1+e^{2x}); abs error <= 3e-7, exact limits +-1.
__device__ __forceinline__ float tanh_f(float x) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
}
// MFMA whose A operand (a resident weight fragment) is read straight from the AGPR half of the
// unified register file.  hipcc only ever parks such values in AGPRs as spills and re-reads them with
// v_accvgpr_read + s_nop (39 cycles per MFMA instead of 32, tools/ubench/mfma_issue.hip); the "a"
// constraint removes the copy.  The statement is opaque to the hazard recogniser: every chain of these
// ends with mfma_fence() before any non-MFMA instruction touches the accumulators.
// KWS_RESIDENT_VGPR_FORM (gru_resident.hip only, see the Makefile): the accumulators of builtin MFMAs stay in VGPRs there, the
// compiler reads an "+a"-pinned fragment as source A by itself and knows every hazard: the builtin, and no fences.
#if KWS_RESIDENT_VGPR_FORM
#define KWS_MFMA_A(acc, wa, bv) acc = mfma4(wa, bv, acc)
#else
#define KWS_MFMA_A(acc, wa, bv) \
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "a"(wa), "v"(bv))
#endif
// XDL 8-pass write -> VALU read needs 11 wait states (s_nop 15 = 16); the "+v" ties order it after the
// chain and ahead of every consumer
__device__ __forceinline__ void mfma_fence(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
    asm volatile("s_nop 15" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ __forceinline__ void mfma_fence(f32x4& a, f32x4& b) {
    asm volatile("s_nop 15" : "+v"(a), "+v"(b));
}
// ... and every chain STARTS with mfma_prefence(): the compiler may have produced the accumulators (or a B
// operand) with a VALU instruction -- typically v_accvgpr_read copies out of the AGPRs the preceding builtin
// MFMAs used -- immediately before the first asm MFMA, and "VALU write VGPR -> MFMA read" needs wait states
// it cannot know about (observed: intermittent 1e-2 errors in the bf16 stack).
__device__ __forceinline__ void mfma_prefence(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
    asm volatile("s_nop 3" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
__device__ __forceinline__ void mfma_prefence(f32x4& a, f32x4& b) {
    asm volatile("s_nop 3" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ f32x4 splat4(float v) { f32x4 r = {v, v, v, v}; return r; }
// exact, branch-free select: m = all-ones -> a, m = 0 -> b (v_bfi_b32); keeps the h update one
// straight-line block so MFMAs can be scheduled through it
__device__ __forceinline__ float bitsel(unsigned m, float a, float b) {
    return __uint_as_float((__float_as_uint(a) & m) | (__float_as_uint(b) & ~m));
}
template <int I0, int I1, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I0 < I1) {
        f(std::integral_constant<int, I0>{});
        static_for<I0 + 1, I1>(f);
    }
}
constexpr float kLog2e = 1.4426950408889634f;
typedef float f32x2 __attribute__((ext_vector_type(2)));
// Activations on register pairs.  Beside an f32 MFMA stream VALU work is not hidden (f32 MFMA and the
// VALU share the FP32 datapath: tools/ubench/mfma_coissue.hip measures +2..3 cycles per plain op, +8 per
// back-to-back transcendental and +14 for an isolated one), so the ops are clustered, packed
// (v_pk_mul/add/fma_f32) and kept to the minimum count: sigmoid = pk_mul, 2 exp, pk_add, 2 rcp.
__device__ __forceinline__ f32x2 sigmoid2(f32x2 x) {
    const f32x2 t = x * -kLog2e;
    f32x2 e;
    e.x = __builtin_amdgcn_exp2f(t.x);
    e.y = __builtin_amdgcn_exp2f(t.y);
    const f32x2 d = e + 1.0f;
    f32x2 r;
    r.x = __builtin_amdgcn_rcpf(d.x);
    r.y = __builtin_amdgcn_rcpf(d.y);
#ifdef KWS_FAULT_INJECT      // never defined in a product build: tests/test_abi.py builds a deliberately wrong library with it
    r = r * 1.0078125f;      // (tools/build_variant.sh faulty -DKWS_FAULT_INJECT=1) and expects kws_selftest to reject it
#endif
    return r;
}
__device__ __forceinline__ f32x2 tanh2(f32x2 x) {
    const f32x2 t = x * (2.0f * kLog2e);
    f32x2 e;
    e.x = __builtin_amdgcn_exp2f(t.x);
    e.y = __builtin_amdgcn_exp2f(t.y);
    const f32x2 d = e + 1.0f;
    f32x2 r;
    r.x = __builtin_amdgcn_rcpf(d.x);
    r.y = __builtin_amdgcn_rcpf(d.y);
    return r * -2.0f + 1.0f;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// Workgroup barrier that orders LDS traffic only: the inter-layer scratch stores and the x prefetch of the next
// frame, which no other wave of the group ever reads, stay in flight across it.  (hipcc's __syncthreads() is the
// same two instructions on gfx950 -- it does not wait for global memory either; where a store has to be visible
// outside the CU before the barrier, the kernels drain vmcnt(0) explicitly.)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// ------------------------------------------------------------------------------------------------
// The row tail: what every path does with the 8 logits of one frame of one stream (models/rnn_ctc.py:247-284 behind the dense
// product, :165, utils/prediction.py:65-86).  Written ONCE: the epilogues below, the class-head kernels (dense_heads_device.h) and
// the int8 projection (gru_octbit.hip) all call it, so a row is the same bits through any of them.
// ------------------------------------------------------------------------------------------------
// relu / clip, softmax and the ctc_decode2 frame rule of one row; returns the frame's word or -1
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
        pr[c] = (c < C) ? __expf(lg[c] - m) : 0.f;     // arguments <= 0: abs error < 1e-7
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

// the 8 floats of one LDS logit row, as two b128
__device__ __forceinline__ void load_row8(const float* src, float (&lg)[kMaxClasses]) {
    const f32x4* row = reinterpret_cast<const f32x4*>(src);
    const f32x4 lo = row[0], hi = row[1];
#pragma unroll
    for (int c = 0; c < 4; ++c) { lg[c] = lo[c]; lg[4 + c] = hi[c]; }
}
__device__ __forceinline__ void store_row8(float* dst, const float (&v)[kMaxClasses]) {
    f32x4* row = reinterpret_cast<f32x4*>(dst);
    row[0] = (f32x4){v[0], v[1], v[2], v[3]};
    row[1] = (f32x4){v[4], v[5], v[6], v[7]};
}
// The fused epilogues' store of output row `row` ([B, T, C] row-major), logits and softmax each where asked for.  The same bytes as
// two store_row; written apart because the shape matters inside the GRU kernels: the product's C == 6 as three unconditional
// 8-byte stores and every other C scalar-wise costs the last-layer frame loops fewer scalar registers than store_row's four
// predicated pairs (with store_row here, 11 last-layer kernels went past their SGPR-spill bounds in spill_expectations.txt).
__device__ __forceinline__ void store_rows(const GruLayerParams& p, size_t row, const float (&lg)[kMaxClasses], const float (&pr)[kMaxClasses]) {
    const int C = p.C;
    if (C == 6) {       // rows are 24 B
        if (p.logits) {
            float2* o = reinterpret_cast<float2*>(p.logits + row * 6);
            o[0] = make_float2(lg[0], lg[1]); o[1] = make_float2(lg[2], lg[3]); o[2] = make_float2(lg[4], lg[5]);
        }
        if (p.softmax) {
            float2* o = reinterpret_cast<float2*>(p.softmax + row * 6);
            o[0] = make_float2(pr[0], pr[1]); o[1] = make_float2(pr[2], pr[3]); o[2] = make_float2(pr[4], pr[5]);
        }
    } else {
        if (p.logits) {
#pragma unroll
            for (int c = 0; c < kMaxClasses; ++c)
                if (c < C) p.logits[row * C + c] = lg[c];
        }
        if (p.softmax) {
#pragma unroll
            for (int c = 0; c < kMaxClasses; ++c)
                if (c < C) p.softmax[row * C + c] = pr[c];
        }
    }
}
// The word stream b carries into a call: prev_word, or -1 for a reset stream, a stream past the batch, or with no prev_word at all.
// The kernel-argument fields come by REFERENCE and are read where the test needs them: taken by value they are fetched ahead of
// the call and wait in scalar registers, which the last-layer kernels have not got (gru_stack_bf16_ls went past its bounds in
// spill_expectations.txt that way).
__device__ __forceinline__ int carried_word(const int32_t* const& prev_word, const uint8_t* const& reset, int b, const int& B) {
    int pw = -1;
    if (b < B && prev_word && !(reset && reset[b])) pw = prev_word[b];
    return pw;
}
// ------------------------------------------------------------------------------------------------
// Last-layer epilogue.  Each wave leaves the partial logits of its 32 units in `pstage`; after the
// frame's second barrier ONE wave (rotating, w == t & 3) folds the four partials into a 16-frame ring.
// Every kRingFrames frames (and at the end of the call) ALL FOUR waves flush: wave w takes frames
// 4w..4w+3 of the block x 16 streams = 64 items, so the softmax / decode / store work is spread
// over the whole group instead of stalling three waves behind one.
//   pstage [4 waves][16 streams][8]     lring [16 frames][16 streams][8]
//   words  [16 frames][16 streams]      carry [2][16]   (previous block's last word, ping-pong)
// (The fp32 resident kernels have an epilogue of their own without the fold: epilogue_flush_partials, below.)
// ------------------------------------------------------------------------------------------------
constexpr int kRingFrames = 16;
constexpr int xs_stride(int kcx) { return 4 * ((((kcx + 3) / 4) & 1) ? (kcx + 3) / 4 : (kcx + 3) / 4 + 1); }
struct EpilogueLds {
    float* pstage;
    float* lring;
    int* words;
    int* carry;
    int8_t* cwords;     // kernels instantiated with the window tail: [16 streams][kWinTailWordsStride] frame words of the whole call; else nullptr
};
constexpr size_t kEpilogueLdsBytes = (4 * 16 * 8 + kRingFrames * 16 * 8) * 4 + kRingFrames * 16 * 4 + 2 * 16 * 4;
__device__ __forceinline__ EpilogueLds epilogue_carve(char* base) {
    EpilogueLds e;
    e.pstage = reinterpret_cast<float*>(base);
    e.lring = e.pstage + 4 * 16 * 8;
    e.words = reinterpret_cast<int*>(e.lring + kRingFrames * 16 * 8);
    e.carry = e.words + kRingFrames * 16;
    e.cwords = nullptr;
    return e;
}

// top of a group, before its first barrier: the words the group's 16 streams carry in
__device__ __forceinline__ void epilogue_carry_init(const EpilogueLds& e, const int32_t* const& prev_word, const uint8_t* const& reset, int group,
                                                    const int& B, int tid) {
    if (tid < 16) e.carry[tid] = carried_word(prev_word, reset, group * kStreamsPerGroup + tid, B);
}

// fold the 4 partial logit vectors of frame t into the ring: 32 lanes, (stream, half) each
__device__ __forceinline__ void epilogue_fold(const EpilogueLds& e, int t, int lane) {
    if (lane < 32) {
        const int s = lane >> 1, half = lane & 1;
        f32x4 v = *reinterpret_cast<const f32x4*>(e.pstage + (0 * 16 + s) * 8 + 4 * half);
#pragma unroll
        for (int w = 1; w < 4; ++w) v += *reinterpret_cast<const f32x4*>(e.pstage + (w * 16 + s) * 8 + 4 * half);
        *reinterpret_cast<f32x4*>(e.lring + (((t & (kRingFrames - 1)) * 16 + s) * 8 + 4 * half)) = v;
    }
}

// flush frames [t0, t0+n) of the ring; called by all four waves of the group together.
// OPAQUE_LANE: everything the flush derives from the lane index (row pointers, LDS addresses) is computed HERE from an opaque
// copy of it.  Otherwise the compiler hoists those per-lane values out of the frame loop; in gru_layer_f16x3's last-layer
// kernels, which have no register to spare, they get spilled, and every reload (scratch_load + s_waitcnt vmcnt(0)) makes the
// flush wait for the acknowledgement of the stores it has just issued -- several microseconds per call at T = 22.
template <bool OPAQUE_LANE = false>
__device__ __forceinline__ void epilogue_flush(const GruLayerParams& p, const EpilogueLds& e, int group, int t0,
                                               int n, int w, int lane, bool final_flush) {
    if constexpr (OPAQUE_LANE) asm volatile("" : "+v"(lane));
    const int f = 4 * w + (lane & 3);          // frame within the block
    const int s = lane >> 2;
    const int b = group * kStreamsPerGroup + s;
    float lg[kMaxClasses], pr[kMaxClasses];
    load_row8(e.lring + (f * 16 + s) * 8, lg);
    const int word = head_row(lg, pr, p.C, p.use_relu, p.value_clip, p.decode_thres);
    e.words[f * 16 + s] = word;
    if (e.cwords != nullptr) {       // the call's words wait for the window tail (row offset from an opaque copy of the lane, as above)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int f2 = 4 * w + (ln & 3);
        if (f2 < n) e.cwords[(ln >> 2) * kWinTailWordsStride + t0 + f2] = (int8_t)word;
    }
    const bool mine = b < p.B && f < n;
    const size_t row = (size_t)b * (p.t_stride ? p.t_stride : p.T) + (t0 + f);
    if (mine) store_rows(p, row, lg, pr);
    lds_barrier();            // every wave's words are in LDS
    const int blk = (t0 / kRingFrames) & 1;
    const int prev = f == 0 ? e.carry[blk * 16 + s] : e.words[(f - 1) * 16 + s];
    const int token = (word >= 0 && word != prev) ? word + 1 : 0;   // utils/prediction.py:76-80
    if (f == n - 1) {
        // the ping-pong slot is for the NEXT block of this group only: after the final flush nobody reads it, and a persistent
        // workgroup's next group initialises carry[0..15] with no barrier in between (it would race with this store)
        if (!final_flush) e.carry[(blk ^ 1) * 16 + s] = word;
        else if (b < p.B && p.prev_word) p.prev_word[b] = word;
    }
    if (mine && p.tokens) p.tokens[row] = (int8_t)token;
}

// ------------------------------------------------------------------------------------------------
// Last-layer epilogue of the resident kernels (gru_resident.hip): no per-frame fold and no barrier of its own.
//   partials [kRingFrames][4 waves][16 streams][8] (+ 4 floats per frame, below)
// Every wave writes the partial logits of frame t into slot t & 15 ahead of the frame's second barrier.  In the flush wave w
// takes streams 4w..4w+3 x 16 frames, lane = 16 * (stream in wave) + frame: it adds the four partials in the order of
// epilogue_fold, ((p0 + p1) + p2) + p3, and goes on exactly as epilogue_flush does.  A 16-lane row is one stream in frame order,
// so the previous frame's word is the lane below (row_shr:1) and the word carried from the block before is a register of the
// row (`carry`: set from prev_word at the top of a group, refreshed here from the row's last valid frame).
// Why it needs no barrier: the second barrier of frame t has published every partial of the block that the flush behind it
// reads, and a slot is next written behind the FIRST barrier of the following frame, which no wave passes before every wave
// has left this flush; the last block of a group is followed by the group's closing __syncthreads() in the same way.
// The frame slots are 4 floats longer than their contents: the flush reads 16 frames of one stream with one ds_read_b128
// lane group, and whole slots of 2 KiB would put all 16 on the same four banks.
// ------------------------------------------------------------------------------------------------
constexpr int kPartialSlotFloats = 4 * 16 * 8 + 4;
constexpr size_t kPartialRingLdsBytes = (size_t)kRingFrames * kPartialSlotFloats * 4;
__device__ __forceinline__ float* partial_slot(float* ring, int t) { return ring + (t & (kRingFrames - 1)) * kPartialSlotFloats; }

// flush frames [t0, t0+n) of the partial ring; called by all four waves of the group together, every lane active.
// cwords: the window tail's [16 streams][kWinTailWordsStride] frame words of the whole call, or nullptr.
// (Everything derived from the lane index comes from an opaque copy of it, as in epilogue_flush<true>: hoisted out of the frame
// loop those values would take registers the loop has not got.)
__device__ __forceinline__ void epilogue_flush_partials(const GruLayerParams& p, const float* ring, int8_t* cwords, int group,
                                                        int t0, int n, int w, int lane, bool final_flush, int& carry) {
    asm volatile("" : "+v"(lane));
    const int f = lane & 15;                   // frame within the block
    const int s = 4 * w + (lane >> 4);
    const int b = group * kStreamsPerGroup + s;
    float lg[kMaxClasses];
    {
        const f32x4* row = reinterpret_cast<const f32x4*>(ring + f * kPartialSlotFloats + s * 8);
        f32x4 lo = row[0], hi = row[1];
#pragma unroll
        for (int k = 1; k < 4; ++k) { lo += row[k * 32]; hi += row[k * 32 + 1]; }      // wave k's partial: 16 streams x 8 floats on
#pragma unroll
        for (int c = 0; c < 4; ++c) { lg[c] = lo[c]; lg[4 + c] = hi[c]; }
    }
    float pr[kMaxClasses];
    const int word = head_row(lg, pr, p.C, p.use_relu, p.value_clip, p.decode_thres);
    if (cwords != nullptr && f < n) cwords[s * kWinTailWordsStride + t0 + f] = (int8_t)word;
    const bool mine = b < p.B && f < n;
    const size_t row = (size_t)b * (p.t_stride ? p.t_stride : p.T) + (t0 + f);
    if (mine) store_rows(p, row, lg, pr);
    // row_shr:1 -- lane f takes the word of lane f - 1 of its row; the row's first lane has no source and keeps `carry`
    const int prev = __builtin_amdgcn_update_dpp(carry, word, 0x111, 0xf, 0xf, false);
    const int token = (word >= 0 && word != prev) ? word + 1 : 0;   // utils/prediction.py:76-80
    if (mine && p.tokens) p.tokens[row] = (int8_t)token;
    if (final_flush) {
        if (f == n - 1 && b < p.B && p.prev_word) p.prev_word[b] = word;
    } else {
        carry = __builtin_amdgcn_ds_bpermute(((lane & 48) + n - 1) << 2, word);     // the row's last frame, to every lane of the row
    }
}


}  // namespace kws
