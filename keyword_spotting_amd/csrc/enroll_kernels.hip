// Customised-keyword enrolment (the reference README's "Customize keyword"; models/rnn_ctc.py:59-101: tf.nn.ctc_loss + Adam on the
// new columns of the class projection, everything else frozen).
//   ctc_loss_kernel        the whole-batch op: one wave per utterance, loss and optionally the gradient with respect to the logits
//   enroll_fit_kernel<HK>  one workgroup per enrolment, one wave per utterance slot, `iterations` optimiser steps in ONE launch:
//                          projection of the frozen top-layer rows on the enrolment's current [H, n] columns, splice between head
//                          1's columns and its blank, log-softmax, alpha / beta / occupancy, rank-1 accumulation of the gradient,
//                          the K partials summed in slot order through LDS, TensorFlow's Adam.  The parameters and both moments
//                          stay in LDS for the whole launch.
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

}  // namespace kws
