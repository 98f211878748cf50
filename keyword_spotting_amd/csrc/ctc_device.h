// CTC loss and its gradient for one utterance on one wave64, fp32, log domain (the arithmetic of tf.nn.ctc_loss as
// models/rnn_ctc.py:59-101 calls it; the blank is the LAST class, config.num_classes - 1).  Shared by ctc_loss_kernel and
// enroll_fit_kernel (enroll_kernels.hip); the forced alignment at the end of the file is ctc_align_kernel's (align_kernels.hip).
//
// The extended label sequence blank, l_1, blank, ..., l_S, blank has L = 2S + 1 <= 63 states: lane s of the wave holds state s and
// reaches states s-1, s-2 (alpha) and s+1, s+2 (beta) by lane shuffles.  lp [len][8] (log-softmax rows) and alpha [len][L] live in
// LDS regions that belong to this wave alone; a wave's LDS operations complete in order, so the hand-offs between lanes need a
// compiler fence, not a workgroup barrier.  expf / logf / log1pf are the accurate library functions.
#pragma once
#include <hip/hip_runtime.h>

namespace kws {

constexpr int kCtcRow = 8;          // floats per lp row: class counts 3..8

// log(exp(a) + exp(b)); an operand (or both) at -inf gives the other one, never NaN
__device__ __forceinline__ float ctc_logaddexp(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1pf(expf(-fabsf(a - b)));
}

__device__ __forceinline__ float ctc_wave_sum(float x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// LDS written by some lanes of this wave is read by others next
__device__ __forceinline__ void ctc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// log-softmax of rows of up to 8 classes held one value per lane in groups of 8 lanes (lane & 7 = class, -inf past the row)
__device__ __forceinline__ float ctc_row_log_softmax(float val) {
    float mx = val;
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
    float sum = val == -INFINITY ? 0.f : expf(val - mx);
#pragma unroll
    for (int d = 4; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    return val - mx - logf(sum);
}

// What lane s knows of the label: its class, whether state s exists, and the two skip transitions
struct CtcLane {
    int L, ext;
    bool live, skip_in, skip_out;      // skip_in: s-2 -> s allowed; skip_out: s -> s+2 allowed
};
__device__ __forceinline__ CtcLane ctc_lane(const int32_t* __restrict__ labels, int S, int blank, int lane) {
    CtcLane c;
    c.L = 2 * S + 1;
    c.live = lane < c.L;
    int ext = blank, before = blank;
    if (c.live && (lane & 1)) {
        ext = labels[lane >> 1];
        ext = ext < 0 ? 0 : (ext > blank - 1 ? blank - 1 : ext);       // the host refused anything else; never index past a row
        if (lane >= 3) before = labels[(lane >> 1) - 1];
    }
    c.ext = ext;
    c.skip_in = c.live && (lane & 1) && lane >= 3 && ext != before;    // ext[s] != blank and ext[s] != ext[s-2]
    c.skip_out = __shfl_down((int)c.skip_in, 2, 64) != 0 && lane + 2 < c.L;
    return c;
}

// alpha [len][L] and -log P(label | rows 0..len-1); len >= 1.  +inf: no valid path.
__device__ __forceinline__ float ctc_alpha(const float* lp, float* alpha, int len, const CtcLane& c, int lane) {
    float a = c.live && lane < 2 ? lp[c.ext] : -INFINITY;
    if (c.live) alpha[lane] = a;
    for (int t = 1; t < len; ++t) {
        float a1 = __shfl_up(a, 1, 64), a2 = __shfl_up(a, 2, 64);
        if (lane < 1) a1 = -INFINITY;
        if (!c.skip_in) a2 = -INFINITY;
        a = ctc_logaddexp(ctc_logaddexp(a, a1), a2) + lp[t * kCtcRow + c.ext];
        if (!c.live) a = -INFINITY;
        if (c.live) alpha[t * c.L + lane] = a;
    }
    const float end1 = __shfl(a, c.L - 1, 64), end2 = c.L > 1 ? __shfl(a, c.L - 2, 64) : -INFINITY;
    return -ctc_logaddexp(end1, end2);
}

// The beta pass, frame len-1 down to 0; per frame emit(t, g) with g on lane c < C the gradient of the loss with respect to logit
// (t, c): softmax - occupancy / P.  nll: ctc_alpha's result, finite.
template <typename F>
__device__ __forceinline__ void ctc_beta_grad(const float* lp, const float* alpha, int len, const CtcLane& c, int lane, int C, float nll,
                                              F&& emit) {
    float b = -INFINITY;
    for (int t = len - 1; t >= 0; --t) {
        const float lpe = lp[t * kCtcRow + c.ext];
        if (t == len - 1) {
            b = c.live && lane >= c.L - 2 ? lpe : -INFINITY;
        } else {
            float b1 = __shfl_down(b, 1, 64), b2 = __shfl_down(b, 2, 64);
            if (lane + 1 >= c.L) b1 = -INFINITY;
            if (!c.skip_out) b2 = -INFINITY;
            b = ctc_logaddexp(ctc_logaddexp(b, b1), b2) + lpe;
            if (!c.live) b = -INFINITY;
        }
        // alpha and beta both carry lp[t][ext]: alpha + beta - lp <= log P, so the occupancy is a plain number in [0, 1]
        float occ = 0.f;
        if (c.live) {
            const float ab = alpha[t * c.L + lane] + b;
            if (ab > -INFINITY) occ = expf(ab - lpe + nll);
        }
        // one butterfly per class, all eight unrolled side by side (independent chains: their shuffle latencies overlap)
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < kCtcRow; ++k) {
            const float s = ctc_wave_sum(c.ext == k ? occ : 0.f);
            if (lane == k) mine = s;
        }
        emit(t, lane < C ? expf(lp[t * kCtcRow + lane]) - mine : 0.f);
    }
}

// ---- forced alignment (align_kernels.hip): the best single path through the extended label, and the states' posteriors

// ctc_alpha's recursion with max in place of log-add-exp: the log-probability of the best path over rows 0..len-1 (len >= 1; -inf: no
// valid path) and in *last the state it ends in.  back [len][2]: for frames 1..len-1 two 64-bit masks, bit s of (back[2t], back[2t+1])
// = (low, high) bit of how far below s the path's state at t-1 lies (0 stay, 1, 2).  Ties, so that one input always gives the same bits:
// a predecessor replaces the choice only when strictly greater, tried in the order stay, s-1, s-2; the path ends in L-1 unless L-2 is
// strictly greater.
__device__ __forceinline__ float ctc_viterbi(const float* lp, unsigned long long* back, int len, const CtcLane& c, int lane, int* last) {
    float v = c.live && lane < 2 ? lp[c.ext] : -INFINITY;
    for (int t = 1; t < len; ++t) {
        float v1 = __shfl_up(v, 1, 64), v2 = __shfl_up(v, 2, 64);
        if (lane < 1) v1 = -INFINITY;
        if (!c.skip_in) v2 = -INFINITY;
        float m = v;
        int from = 0;
        if (v1 > m) { m = v1; from = 1; }
        if (v2 > m) { m = v2; from = 2; }
        v = m + lp[t * kCtcRow + c.ext];
        if (!c.live) v = -INFINITY;
        const unsigned long long lo = __ballot(from & 1), hi = __ballot(from >> 1);
        if (lane == 0) { back[2 * t] = lo; back[2 * t + 1] = hi; }
    }
    const float end1 = __shfl(v, c.L - 1, 64), end2 = c.L > 1 ? __shfl(v, c.L - 2, 64) : -INFINITY;
    const bool second = end2 > end1;
    *last = second ? c.L - 2 : c.L - 1;
    return second ? end2 : end1;
}

// The path ctc_viterbi found, walked from its last frame to its first: row [len] <- its state at every frame.  Every lane walks the
// same chain (the reads are broadcasts), lane 0 writes.  ctc_viterbi never records a step below state 0 (lane 0 has no predecessor, lanes 1
// and 2 no s-2); the clamp keeps the LDS index in bounds whatever the masks hold.
__device__ __forceinline__ void ctc_backtrack(const unsigned long long* back, int32_t* row, int len, int last, int lane) {
    int s = last;
    for (int t = len - 1; t >= 0; --t) {
        if (lane == 0) row[t] = s;
        if (t == 0) break;
        const int from = (int)((back[2 * t] >> s) & 1ull) | ((int)((back[2 * t + 1] >> s) & 1ull) << 1);
        s = s - from < 0 ? 0 : s - from;
    }
}

// ctc_beta_grad's recursion without the per-class butterflies: per frame emit(t, occ) with occ on lane s the posterior occupancy of
// state s at frame t, exp(alpha + beta - lp + nll), at most 1 (0 on the lanes past L).  nll: ctc_alpha's result, finite.
template <typename F>
__device__ __forceinline__ void ctc_beta_post(const float* lp, const float* alpha, int len, const CtcLane& c, int lane, float nll, F&& emit) {
    float b = -INFINITY;
    for (int t = len - 1; t >= 0; --t) {
        const float lpe = lp[t * kCtcRow + c.ext];
        if (t == len - 1) {
            b = c.live && lane >= c.L - 2 ? lpe : -INFINITY;
        } else {
            float b1 = __shfl_down(b, 1, 64), b2 = __shfl_down(b, 2, 64);
            if (lane + 1 >= c.L) b1 = -INFINITY;
            if (!c.skip_out) b2 = -INFINITY;
            b = ctc_logaddexp(ctc_logaddexp(b, b1), b2) + lpe;
            if (!c.live) b = -INFINITY;
        }
        float occ = 0.f;
        if (c.live) {
            const float ab = alpha[t * c.L + lane] + b;
            if (ab > -INFINITY) occ = fminf(expf(ab - lpe + nll), 1.f);
        }
        emit(t, occ);
    }
}

}  // namespace kws
