// Customised-keyword enrolment (the reference README's "Customize keyword"; models/rnn_ctc.py:59-101: tf.nn.ctc_loss + Adam on the
// new columns of the class projection, everything else frozen).
//   ctc_loss_kernel        the whole-batch op: one wave per utterance, loss and optionally the gradient with respect to the logits
//   enroll_fit_kernel<HK>  one workgroup per enrolment, one wave per utterance slot, `iterations` optimiser steps in ONE launch:
//                          projection of the frozen top-layer rows on the enrolment's current [H, n] columns, splice between head
//                          1's columns and its blank, log-softmax, alpha / beta / occupancy, rank-1 accumulation of the gradient,
//                          the K partials summed in slot order through LDS, TensorFlow's Adam.  The parameters and both moments
//                          stay in LDS for the whole launch.
//   enroll_fit_frames_kernel<HK, CTC>  the same fit on frame-wise targets: the frame cross-entropy of the spliced rows in the CTC
//                          loss's place (no alpha / beta, no LDS per frame) or on top of it; the order of accumulation is at the kernel.
// Per step and utterance the arithmetic is [T, H] x [H, n <= 5] and a recurrence over <= 63 states: nothing a 16 x 16 MFMA tile would
// fill, so the projection is plain VALU on coalesced 4 H-byte rows and a wave reduction.
#include "ctc_device.h"
#include "launch.h"

namespace kws {

__global__ void __launch_bounds__(64) ctc_loss_kernel(const float* __restrict__ logits, const int32_t* __restrict__ seq_len,
                                                      const int32_t* __restrict__ labels, const int32_t* __restrict__ label_len, int T, int C,
                                                      int S_max, float* __restrict__ loss, float* __restrict__ grad) {
    extern __shared__ float ctc_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    int len = seq_len[b], S = label_len[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    S = S < 0 ? 0 : (S > S_max ? S_max : S);
    const float* lg = logits + (size_t)b * T * C;
    float* gr = grad ? grad + (size_t)b * T * C : nullptr;
    float* lp = ctc_lds;
    float* alpha = ctc_lds + (size_t)T * kCtcRow;
    const CtcLane c = ctc_lane(labels + (size_t)b * S_max, S, C - 1, lane);
    // 8 frames per pass: lane >> 3 is the frame, lane & 7 the class
    for (int t0 = 0; t0 < len; t0 += 8) {
        const int t = t0 + (lane >> 3), k = lane & 7;
        const bool on = t < len && k < C;
        const float v = ctc_row_log_softmax(on ? lg[(size_t)t * C + k] : -INFINITY);
        if (on) lp[t * kCtcRow + k] = v;
    }
    ctc_wave_sync();
    float nll = 0.f;
    if (len > 0) nll = ctc_alpha(lp, alpha, len, c, lane);
    if (lane == 0) loss[b] = nll;
    if (!gr) return;
    ctc_wave_sync();
    const bool feasible = len > 0 && nll < INFINITY;
    if (feasible)
        ctc_beta_grad(lp, alpha, len, c, lane, C, nll, [&](int t, float g) { if (lane < C) gr[(size_t)t * C + lane] = g; });
    for (int i = (feasible ? len * C : 0) + lane; i < T * C; i += 64) gr[i] = 0.f;      // no path, and the frames past seq_len
}

hipError_t launch_ctc_loss(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C,
                           int S_max, float* loss, float* grad, hipStream_t st) {
    return launch_lds<ctc_loss_kernel>(dim3(B), dim3(64), ctc_loss_lds_bytes(T, S_max), st, logits, seq_len, labels, label_len, T, C, S_max,
                                       loss, grad);
}

constexpr int kNewMax = 5;      // C + n <= 8 with C >= 3

template <int HK>
__global__ void __launch_bounds__(256) enroll_fit_kernel(EnrollFitParams p) {
    constexpr int H = 16 * HK, R = H / 64;
    extern __shared__ float fit_lds[];
    const int e = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tid = threadIdx.x, nthreads = blockDim.x;
    const int K = p.K, n = p.n, C = p.C, C2 = C + n, T = p.T, B = (int)gridDim.x * K;
    const int HN = H * n, P = HN + n;
    const int b = e * K + wave;
    float* theta = fit_lds;                   // [H][n] columns, then [n] bias
    float* mom = theta + P;
    float* vel = mom + P;
    float* red = vel + P;                     // [K][P] the slots' partial gradients
    float* lp = red + (size_t)K * P + (size_t)wave * ctc_wave_lds_floats(T, p.S_max);
    float* alpha = lp + (size_t)T * kCtcRow;

    float* gW = p.W + (size_t)e * HN; float* gB = p.b + (size_t)e * n;
    float* gmW = p.mW + (size_t)e * HN; float* gmB = p.mb + (size_t)e * n;
    float* gvW = p.vW + (size_t)e * HN; float* gvB = p.vb + (size_t)e * n;
    for (int i = tid; i < P; i += nthreads) {
        theta[i] = i < HN ? gW[i] : gB[i - HN];
        mom[i] = i < HN ? gmW[i] : gmB[i - HN];
        vel[i] = i < HN ? gvW[i] : gvB[i - HN];
    }
    __syncthreads();

    int len = p.seq_len[b], S = p.label_len[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    S = S < 0 ? 0 : (S > p.S_max ? p.S_max : S);
    const CtcLane c = ctc_lane(p.labels + (size_t)b * p.S_max, S, C2 - 1, lane);
    const float* nn = p.nn + (size_t)b * T * H;
    const float* l1 = p.logits1 + (size_t)b * T * C;

    for (int it = 0; it < p.iterations; ++it) {
        float w[R][kNewMax], bias[kNewMax];
#pragma unroll
        for (int j = 0; j < kNewMax; ++j) {
            bias[j] = j < n ? theta[HN + j] : 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) w[r][j] = j < n ? theta[(lane + 64 * r) * n + j] : 0.f;
        }
        // rows of the spliced head: head 1's columns 0..C-2, the n new ones, head 1's blank.  The next frame's row and head-1 logit are
        // fetched while this one is reduced (a frame is a chain of dependent shuffles: the fetch latency hides behind it)
        const int k = lane & 7;
        const int col = k < C - 1 ? k : (k == C2 - 1 ? C - 1 : -1);
        float xn[R], ln = -INFINITY;
        if (len > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) xn[r] = nn[lane + 64 * r];
            if (col >= 0) ln = l1[col];
        }
        for (int t = 0; t < len; ++t) {
            float x[R];
#pragma unroll
            for (int r = 0; r < R; ++r) x[r] = xn[r];
            float val = ln;
            if (t + 1 < len) {
#pragma unroll
                for (int r = 0; r < R; ++r) xn[r] = nn[(size_t)(t + 1) * H + lane + 64 * r];
                if (col >= 0) ln = l1[(size_t)(t + 1) * C + col];
            }
#pragma unroll
            for (int j = 0; j < kNewMax; ++j) {
                if (j < n) {          // uniform
                    float z = 0.f;
#pragma unroll
                    for (int r = 0; r < R; ++r) z += x[r] * w[r][j];
                    z = ctc_wave_sum(z) + bias[j];
                    if (k == C - 1 + j) val = z;
                }
            }
            const float v = ctc_row_log_softmax(val);
            if (lane < C2) lp[t * kCtcRow + lane] = v;
        }
        ctc_wave_sync();
        float nll = 0.f;
        if (len > 0) nll = ctc_alpha(lp, alpha, len, c, lane);
        float gw[R][kNewMax], gb[kNewMax];
#pragma unroll
        for (int j = 0; j < kNewMax; ++j) {
            gb[j] = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) gw[r][j] = 0.f;
        }
        ctc_wave_sync();
        if (len > 0 && nll < INFINITY) {
            float xb[R];          // the row of the frame the beta pass reaches next, fetched one frame ahead
#pragma unroll
            for (int r = 0; r < R; ++r) xb[r] = nn[(size_t)(len - 1) * H + lane + 64 * r];
            ctc_beta_grad(lp, alpha, len, c, lane, C2, nll, [&](int t, float g) {
                float x[R];
#pragma unroll
                for (int r = 0; r < R; ++r) x[r] = xb[r];
                if (t > 0) {
#pragma unroll
                    for (int r = 0; r < R; ++r) xb[r] = nn[(size_t)(t - 1) * H + lane + 64 * r];
                }
#pragma unroll
                for (int j = 0; j < kNewMax; ++j) {
                    if (j < n) {
                        const float dz = __shfl(g, C - 1 + j, 64);
                        gb[j] += dz;
#pragma unroll
                        for (int r = 0; r < R; ++r) gw[r][j] += x[r] * dz;
                    }
                }
            });
        }
        if (p.loss_trace && lane == 0) p.loss_trace[(size_t)it * B + b] = nll;
#pragma unroll
        for (int j = 0; j < kNewMax; ++j) {
            if (j < n) {
#pragma unroll
                for (int r = 0; r < R; ++r) red[(size_t)wave * P + (lane + 64 * r) * n + j] = gw[r][j];
                if (lane == 0) red[(size_t)wave * P + HN + j] = gb[j];
            }
        }
        __syncthreads();
        // the slots in order, the reference's division by config.batch_size, then tf.train.AdamOptimizer (epsilon outside the root,
        // the bias corrections folded into the step size)
        const double step = (double)(p.step0 + it + 1);
        const float lr_t = (float)((double)p.lr * sqrt(1.0 - pow(0.999, step)) / (1.0 - pow(0.9, step)));
        for (int i = tid; i < P; i += nthreads) {
            float g = 0.f;
            for (int k = 0; k < K; ++k) g += red[(size_t)k * P + i];
            g = g / (float)K;
            const float m1 = 0.9f * mom[i] + (1.0f - 0.9f) * g;
            const float v1 = 0.999f * vel[i] + (1.0f - 0.999f) * (g * g);
            mom[i] = m1;
            vel[i] = v1;
            theta[i] -= lr_t * m1 / (sqrtf(v1) + 1e-8f);
        }
        __syncthreads();
    }
    for (int i = tid; i < P; i += nthreads) {
        if (i < HN) { gW[i] = theta[i]; gmW[i] = mom[i]; gvW[i] = vel[i]; }
        else { gB[i - HN] = theta[i]; gmB[i - HN] = mom[i]; gvB[i - HN] = vel[i]; }
    }
}

hipError_t launch_enroll_fit(const EnrollFitParams& p, int hidden, int E, hipStream_t st) {
    const size_t lds = enroll_fit_lds_bytes(hidden, p.n, p.K, p.T, p.S_max);
    return with_int<4, 8, 16>(hidden / 16, [&](auto hk) {
        return launch_lds<enroll_fit_kernel<hk()>>(dim3(E), dim3(64 * p.K), lds, st, p);
    });
}

// enroll_fit_kernel's state handling and optimiser step as functions, for the frames kernel below (the kernel above keeps its own text:
// its machine code is pinned).  An enrolment's state in LDS: theta = [H][n] columns then [n] bias, Adam's m
// and v in the same layout, P = (H + 1) n floats each; HN = H n.
__device__ __forceinline__ void enroll_state_load(const EnrollFitParams& p, int e, int HN, int n, float* theta, float* mom, float* vel,
                                                  int tid, int nthreads) {
    const float* gW = p.W + (size_t)e * HN; const float* gB = p.b + (size_t)e * n;
    const float* gmW = p.mW + (size_t)e * HN; const float* gmB = p.mb + (size_t)e * n;
    const float* gvW = p.vW + (size_t)e * HN; const float* gvB = p.vb + (size_t)e * n;
    for (int i = tid; i < HN + n; i += nthreads) {
        theta[i] = i < HN ? gW[i] : gB[i - HN];
        mom[i] = i < HN ? gmW[i] : gmB[i - HN];
        vel[i] = i < HN ? gvW[i] : gvB[i - HN];
    }
}

__device__ __forceinline__ void enroll_state_store(const EnrollFitParams& p, int e, int HN, int n, const float* theta, const float* mom,
                                                   const float* vel, int tid, int nthreads) {
    float* gW = p.W + (size_t)e * HN; float* gB = p.b + (size_t)e * n;
    float* gmW = p.mW + (size_t)e * HN; float* gmB = p.mb + (size_t)e * n;
    float* gvW = p.vW + (size_t)e * HN; float* gvB = p.vb + (size_t)e * n;
    for (int i = tid; i < HN + n; i += nthreads) {
        if (i < HN) { gW[i] = theta[i]; gmW[i] = mom[i]; gvW[i] = vel[i]; }
        else { gB[i - HN] = theta[i]; gmB[i - HN] = mom[i]; gvB[i - HN] = vel[i]; }
    }
}

// red [K][P], the slots' partial gradients, -> one optimiser step: the slots in order, the reference's division by config.batch_size,
// then tf.train.AdamOptimizer (epsilon outside the root, the bias corrections folded into the step size)
__device__ __forceinline__ void enroll_adam_step(const EnrollFitParams& p, int it, const float* red, float* theta, float* mom, float* vel,
                                                 int K, int P, int tid, int nthreads) {
    const double step = (double)(p.step0 + it + 1);
    const float lr_t = (float)((double)p.lr * sqrt(1.0 - pow(0.999, step)) / (1.0 - pow(0.9, step)));
    for (int i = tid; i < P; i += nthreads) {
        float g = 0.f;
        for (int k = 0; k < K; ++k) g += red[(size_t)k * P + i];
        g = g / (float)K;
        const float m1 = 0.9f * mom[i] + (1.0f - 0.9f) * g;
        const float v1 = 0.999f * vel[i] + (1.0f - 0.999f) * (g * g);
        mom[i] = m1;
        vel[i] = v1;
        theta[i] -= lr_t * m1 / (sqrtf(v1) + 1e-8f);
    }
}

// The value lane `src` of the wave holds; src is the same in every lane (it goes through an SGPR)
__device__ __forceinline__ float enroll_lane_value(float x, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), __builtin_amdgcn_readfirstlane(src)));
}

// ctc_alpha / ctc_beta_grad (ctc_device.h) in rescaled form, for the frames kernel.  There every occupancy is exp(alpha + beta - lp + nll)
// with alpha, beta and nll of the size of the loss: one float32 rounding of nll (2^-21 at 15 nats) is a relative error every occupancy of
// the utterance shares, with one sign, and the sum over the frames keeps it.  Here every alpha row and every beta row is stored and carried
// minus its own maximum (the offsets of alpha add up in fp64 for the loss; beta's are never needed), and a frame's occupancies are
// normalised by their own sum -- sum_s alpha_t(s) beta_t(s) / y_t(s) is P at every t --, so the exponentials see numbers near 0.
__device__ __forceinline__ float ctc_wave_max(float x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmaxf(x, __shfl_xor(x, d, 64));
    return x;
}

// alpha [len][L], row t minus its maximum, and -log P(label | rows 0..len-1); len >= 1.  +inf: no valid path.
__device__ __forceinline__ float ctc_alpha_scaled(const float* lp, float* alpha, int len, const CtcLane& c, int lane) {
    float a = c.live && lane < 2 ? lp[c.ext] : -INFINITY;
    double offset = 0.0;
    for (int t = 0; t < len; ++t) {
        if (t > 0) {
            float a1 = __shfl_up(a, 1, 64), a2 = __shfl_up(a, 2, 64);
            if (lane < 1) a1 = -INFINITY;
            if (!c.skip_in) a2 = -INFINITY;
            a = ctc_logaddexp(ctc_logaddexp(a, a1), a2) + lp[t * kCtcRow + c.ext];
            if (!c.live) a = -INFINITY;
        }
        const float m = ctc_wave_max(a);
        if (m > -INFINITY) { a -= m; offset += (double)m; }          // all -inf: no path gets this far, and none will
        if (c.live) alpha[t * c.L + lane] = a;
    }
    const float end1 = __shfl(a, c.L - 1, 64), end2 = c.L > 1 ? __shfl(a, c.L - 2, 64) : -INFINITY;
    const float tail = ctc_logaddexp(end1, end2);
    return tail == -INFINITY ? INFINITY : (float)(-(offset + (double)tail));
}

// ctc_beta_grad on ctc_alpha_scaled's rows: per frame emit(t, g), g on lane c < C the gradient of the loss with respect to logit (t, c).
// Called for an utterance with a valid path only.
template <typename F>
__device__ __forceinline__ void ctc_beta_grad_scaled(const float* lp, const float* alpha, int len, const CtcLane& c, int lane, int C, F&& emit) {
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
        const float mb = ctc_wave_max(b);
        if (mb > -INFINITY) b -= mb;
        float e = -INFINITY;
        if (c.live) {
            const float ab = alpha[t * c.L + lane] + b;
            if (ab > -INFINITY) e = ab - lpe;
        }
        const float me = ctc_wave_max(e);
        const float w = e > -INFINITY ? expf(e - me) : 0.f;
        const float total = ctc_wave_sum(w);
        const float occ = total > 0.f ? w / total : 0.f;
        float mine = 0.f;
#pragma unroll
        for (int k = 0; k < kCtcRow; ++k) {
            const float s = ctc_wave_sum(c.ext == k ? occ : 0.f);
            if (lane == k) mine = s;
        }
        emit(t, lane < C ? expf(lp[t * kCtcRow + lane]) - mine : 0.f);
    }
}

// enroll_fit_kernel with the frame-wise cross-entropy (kws_internal.h, EnrollFitFramesParams) on the spliced rows, alone (CTC false) or
// next to the CTC term (CTC true).  The same workgroup, waves and LDS state; per slot and launch first
//   W_b    the weights of the labelled frames: lane l adds frames l, l + 64, ... in fp64, then one butterfly (and the ballot of the
//          targets outside [-1, C2) at live frames, which count as -1 and make the slot's losses NaN)
// and per step, in this order of accumulation into the slot's partial gradient (registers: gw [H/64][n], gb [n] per lane):
//   1. the forward pass, frames 0 .. len-1: project, splice, log-softmax (ctc_row_log_softmax); at a labelled frame the frame term
//      frame_weight (w[y_t] / W_b) (softmax - onehot) of the new columns goes straight into gw / gb as a rank-1 update with the row
//      that is in registers anyway, and w[y_t] (-log softmax[y_t]) into an fp64 sum.  CTC: the row also goes to lp in LDS.
//   2. CTC only: alpha, then the beta pass, frames len-1 .. 0, adding ctc_weight x (softmax - occupancy) of the new columns, both passes
//      in the rescaled form above.  A slot
//      without a valid path skips this step and keeps step 1.
// Then the K partials in slot order through LDS and Adam, as enroll_fit_kernel.  With CTC false nothing in LDS grows with T, and labels /
// label_len are never read.
template <int HK, bool CTC>
__global__ void __launch_bounds__(256) enroll_fit_frames_kernel(EnrollFitFramesParams q) {
    constexpr int H = 16 * HK, R = H / 64;
    extern __shared__ float fit_lds[];
    const EnrollFitParams& p = q.fit;
    const int e = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tid = threadIdx.x, nthreads = blockDim.x;
    const int K = p.K, n = p.n, C = p.C, C2 = C + n, T = p.T, B = (int)gridDim.x * K;
    const int HN = H * n, P = HN + n;
    const int b = e * K + wave;
    float* theta = fit_lds;
    float* mom = theta + P;
    float* vel = mom + P;
    float* red = vel + P;
    float* lp = red + (size_t)K * P + (CTC ? (size_t)wave * ctc_wave_lds_floats(T, p.S_max) : 0);      // CTC false: never touched
    float* alpha = lp + (size_t)T * kCtcRow;

    enroll_state_load(p, e, HN, n, theta, mom, vel, tid, nthreads);
    __syncthreads();

    int len = p.seq_len[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    CtcLane c = {};
    if constexpr (CTC) {
        int S = p.label_len[b];
        S = S < 0 ? 0 : (S > p.S_max ? p.S_max : S);
        c = ctc_lane(p.labels + (size_t)b * p.S_max, S, C2 - 1, lane);
    }
    const float* nn = p.nn + (size_t)b * T * H;
    const float* l1 = p.logits1 + (size_t)b * T * C;
    const int32_t* tg = q.targets + (size_t)b * T;
    const int k = lane & 7;
    const float wk = k < C2 ? q.weight[k] : 0.f;          // lane y < 8 holds w[y]

    double wsum = 0.0;
    int seen_bad = 0;
    for (int t0 = 0; t0 < len; t0 += 64) {               // every lane runs every pass: the shuffle reads all of them
        const int t = t0 + lane;
        const int y = t < len ? tg[t] : -1;
        const bool labelled = y >= 0 && y < C2;
        if (y < -1 || y >= C2) seen_bad = 1;
        const float wy = __shfl(wk, labelled ? y : 0, 64);
        if (labelled) wsum += (double)wy;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_xor(wsum, d, 64);
    const bool bad = __ballot(seen_bad) != 0ull;
    const float inv_w = wsum > 0.0 ? (float)(1.0 / wsum) : 0.f;

    for (int it = 0; it < p.iterations; ++it) {
        float w[R][kNewMax], bias[kNewMax], gw[R][kNewMax], gb[kNewMax];
#pragma unroll
        for (int j = 0; j < kNewMax; ++j) {
            bias[j] = j < n ? theta[HN + j] : 0.f;
            gb[j] = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                w[r][j] = j < n ? theta[(lane + 64 * r) * n + j] : 0.f;
                gw[r][j] = 0.f;
            }
        }
        const int col = k < C - 1 ? k : (k == C2 - 1 ? C - 1 : -1);
        float xn[R], ln = -INFINITY;
        int yn = -1;
        if (len > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) xn[r] = nn[lane + 64 * r];
            if (col >= 0) ln = l1[col];
            yn = tg[0];
        }
        double ce_sum = 0.0;
        for (int t = 0; t < len; ++t) {
            float x[R];
#pragma unroll
            for (int r = 0; r < R; ++r) x[r] = xn[r];
            float val = ln;
            int y = __builtin_amdgcn_readfirstlane(yn);
            if (t + 1 < len) {
#pragma unroll
                for (int r = 0; r < R; ++r) xn[r] = nn[(size_t)(t + 1) * H + lane + 64 * r];
                if (col >= 0) ln = l1[(size_t)(t + 1) * C + col];
                yn = tg[t + 1];
            }
#pragma unroll
            for (int j = 0; j < kNewMax; ++j) {
                if (j < n) {          // uniform
                    float z = 0.f;
#pragma unroll
                    for (int r = 0; r < R; ++r) z += x[r] * w[r][j];
                    z = ctc_wave_sum(z) + bias[j];
                    if (k == C - 1 + j) val = z;
                }
            }
            const float v = ctc_row_log_softmax(val);
            if constexpr (CTC) {
                if (lane < C2) lp[t * kCtcRow + lane] = v;
            }
            if (y < -1 || y >= C2) y = -1;
            if (y >= 0) {             // uniform
                const float wy = enroll_lane_value(wk, y);
                ce_sum += (double)wy * (double)(-enroll_lane_value(v, y));
                const float g = q.frame_weight * (wy * inv_w) * (expf(v) - (k == y ? 1.0f : 0.f));
#pragma unroll
                for (int j = 0; j < kNewMax; ++j) {
                    if (j < n) {
                        const float dz = __shfl(g, C - 1 + j, 64);
                        gb[j] += dz;
#pragma unroll
                        for (int r = 0; r < R; ++r) gw[r][j] += x[r] * dz;
                    }
                }
            }
        }
        float nll = 0.f;
        if constexpr (CTC) {
            ctc_wave_sync();
            if (len > 0) nll = ctc_alpha_scaled(lp, alpha, len, c, lane);
            ctc_wave_sync();
            if (len > 0 && nll < INFINITY) {
                float xb[R];
#pragma unroll
                for (int r = 0; r < R; ++r) xb[r] = nn[(size_t)(len - 1) * H + lane + 64 * r];
                ctc_beta_grad_scaled(lp, alpha, len, c, lane, C2, [&](int t, float g) {
                    float x[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) x[r] = xb[r];
                    if (t > 0) {
#pragma unroll
                        for (int r = 0; r < R; ++r) xb[r] = nn[(size_t)(t - 1) * H + lane + 64 * r];
                    }
#pragma unroll
                    for (int j = 0; j < kNewMax; ++j) {
                        if (j < n) {
                            const float dz = q.ctc_weight * __shfl(g, C - 1 + j, 64);
                            gb[j] += dz;
#pragma unroll
                            for (int r = 0; r < R; ++r) gw[r][j] += x[r] * dz;
                        }
                    }
                });
            }
        }
        if (lane == 0) {
            const float ce = bad ? NAN : (wsum > 0.0 ? (float)(ce_sum / wsum) : 0.f);
            if (q.frame_loss) q.frame_loss[(size_t)it * B + b] = ce;
            if (p.loss_trace) p.loss_trace[(size_t)it * B + b] = CTC ? q.ctc_weight * nll + q.frame_weight * ce : q.frame_weight * ce;
        }
#pragma unroll
        for (int j = 0; j < kNewMax; ++j) {
            if (j < n) {
#pragma unroll
                for (int r = 0; r < R; ++r) red[(size_t)wave * P + (lane + 64 * r) * n + j] = gw[r][j];
                if (lane == 0) red[(size_t)wave * P + HN + j] = gb[j];
            }
        }
        __syncthreads();
        enroll_adam_step(p, it, red, theta, mom, vel, K, P, tid, nthreads);
        __syncthreads();
    }
    enroll_state_store(p, e, HN, n, theta, mom, vel, tid, nthreads);
}

hipError_t launch_enroll_fit_frames(const EnrollFitFramesParams& q, int hidden, int E, hipStream_t st) {
    const bool ctc = q.ctc_weight > 0.f;
    const size_t lds = enroll_fit_frames_lds_bytes(hidden, q.fit.n, q.fit.K, q.fit.T, q.fit.S_max, ctc);
    return with_int<4, 8, 16>(hidden / 16, [&](auto hk) {
        return with_bool(ctc, [&](auto with_ctc) {
            return launch_lds<enroll_fit_frames_kernel<hk(), with_ctc()>>(dim3(E), dim3(64 * q.fit.K), lds, st, q);
        });
    });
}

}  // namespace kws
