// Frame-wise softmax cross-entropy on frame-wise targets (include/kws_amd.h, "Frame-wise targets"): the loss of an utterance and its
// gradient with respect to the logits, for the stand-alone op (kws_frame_loss) and between the logits product and the backward pass
// of both train handles (kws_train_*_frames, kws_attention_train_*_frames).
//   frame_loss_kernel   one workgroup of 4 waves per utterance: an utterance's bits do not depend on the batch it is in.  A wave takes
//                       8 consecutive frames per pass, lane >> 3 the frame and lane & 7 the class (ctc_loss_kernel's layout, so the row
//                       log-softmax is ctc_device.h's ctc_row_log_softmax unchanged); the workgroup takes 32 consecutive frames, whose
//                       32 C floats are one contiguous piece of memory: rows of 3..8 floats need no alignment beyond 4 bytes, and
//                       neighbouring lanes touch neighbouring words.  Pass 1 sums the weights of the labelled frames (W_b), pass 2
//                       takes every frame's log-softmax, its share of the loss and its gradient row.  Both sums are per-lane partials
//                       in frame order (fp64: one add per frame, and the sum of 4000 terms rounds once), combined by a wave butterfly
//                       and then over the four waves in wave order through 4 doubles of LDS -- no atomics, no LDS that grows with T.
// Two store modes: write (every row of the utterance, zeros at dead and unlabelled frames) and accumulate (g += on the live labelled
// rows, nothing else touched: the frame term on top of the CTC gradient that ctc_loss_kernel and train_scale_kernel left there).
#include "ctc_device.h"
#include "launch.h"

namespace kws {

namespace {

constexpr int kFrameLossWaves = 4, kFrameLossRows = 8 * kFrameLossWaves;      // frames per pass of the workgroup

__device__ __forceinline__ double frame_wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// the workgroup's sum of one partial per lane: butterfly per wave, then the waves' sums in wave order (every thread the same bits)
__device__ __forceinline__ double frame_block_sum(double x, double* red, int wave, int lane) {
    x = frame_wave_sum(x);
    __syncthreads();          // red may still be read from the sum before
    if (lane == 0) red[wave] = x;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < kFrameLossWaves; ++w) s += red[w];
    return s;
}

}  // namespace

__global__ void __launch_bounds__(64 * kFrameLossWaves) frame_loss_kernel(FrameLossParams p) {
    __shared__ double red[kFrameLossWaves];
    __shared__ float wts[kCtcRow];
    __shared__ int bad[kFrameLossWaves];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int T = p.T, C = p.C, k = lane & 7, row = wave * 8 + (lane >> 3);
    int len = p.seq_len[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    const size_t first = (size_t)b * T;          // the utterance's first frame
    const float* lg = p.logits + first * C;
    const int32_t* tg = p.targets + first;
    float* gr = p.grad ? p.grad + first * C : nullptr;
    if (tid < kCtcRow) wts[tid] = tid < C ? (p.weight ? p.weight[tid] : 1.0f) : 0.f;
    __syncthreads();

    // pass 1: W_b, the weights of the labelled frames; a target outside [-1, C) at a live frame counts as -1 and marks the utterance
    double wsum = 0.0;
    int seen_bad = 0;
    for (int t = row; t < len; t += kFrameLossRows) {
        const int y = tg[t];
        if (y < -1 || y >= C) seen_bad = 1;
        if (k == 0 && y >= 0 && y < C) wsum += (double)wts[y];
    }
    const double W = frame_block_sum(wsum, red, wave, lane);
    const unsigned long long any_bad = __ballot(seen_bad);
    if (lane == 0) bad[wave] = any_bad != 0ull;
    const float inv_w = W > 0.0 ? (float)(1.0 / W) : 0.f;

    // pass 2: the loss and the gradient rows.  Write mode walks all T rows (the dead ones get zeros), accumulate mode the live ones
    const int rows = p.accumulate ? len : T;
    double nll = 0.0;
    for (int t0 = 0; t0 < rows; t0 += kFrameLossRows) {
        const int t = t0 + row;
        const bool live = t < len, on = live && k < C;
        int y = live ? tg[t] : -1;
        if (y < -1 || y >= C) y = -1;
        const float lsm = ctc_row_log_softmax(on ? lg[(size_t)t * C + k] : -INFINITY);
        const bool labelled = on && y >= 0;
        const float w = labelled ? wts[y] : 0.f;
        if (labelled && k == y) nll += (double)w * (double)(-lsm);
        if (!gr || t >= rows || k >= C) continue;
        const float g = labelled ? p.scale * (w * inv_w) * (expf(lsm) - (k == y ? 1.0f : 0.f)) : 0.f;
        float* dst = gr + (size_t)t * C + k;
        if (!p.accumulate) *dst = g;
        else if (labelled) *dst += g;
    }
    const double total = frame_block_sum(nll, red, wave, lane);
    if (tid != 0) return;
    int poisoned = 0;
#pragma unroll
    for (int w = 0; w < kFrameLossWaves; ++w) poisoned |= bad[w];
    const float ce = poisoned ? NAN : (W > 0.0 ? (float)(total / W) : 0.f);
    if (p.ce) p.ce[b] = ce;
    if (p.loss) p.loss[b] = (p.mix_prev != 0.f ? p.mix_prev * p.loss[b] : 0.f) + p.mix_ce * ce;
}

hipError_t launch_frame_loss(const FrameLossParams& p, int B, hipStream_t st) {
    return launch_lds<frame_loss_kernel>(dim3(B), dim3(64 * kFrameLossWaves), 0, st, p);
}

}  // namespace kws
