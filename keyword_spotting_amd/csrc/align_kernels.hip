// CTC forced alignment (kws_ctc_align): given the transcript, where in the utterance each label lies and how sure the model is of it.
//   ctc_align_kernel   one wave per utterance, lane s = state s of the extended label (ctc_loss_kernel's layout).  The log-softmax rows
//                      go into LDS as ctc_loss_kernel loads them; ctc_viterbi runs the max-plus recursion and leaves two bits of
//                      back-pointer per (frame, state); the backtrack walks them from the last frame to the first -- a serial chain of
//                      len dependent LDS reads, the known cost of this kernel -- and leaves the state row in LDS; the whole wave copies
//                      it out coalesced and scatters the spans from it (a label's frames are one run of the row: each end is written by
//                      the one lane that sees it).  Then, if asked for, the unchanged ctc_alpha (the loss, bitwise kws_ctc_loss's) and
//                      ctc_beta_post, which stores each label state's occupancy straight from its lane.
// LDS, all of it this wave's own (hand-offs by ctc_wave_sync): lp [T][8] | back-pointers [T][2] 64-bit masks | states [T] | alpha [T][L]
// (the last only when the loss or the posteriors are asked for) -- ctc_align_lds_bytes.
#include "ctc_device.h"
#include "launch.h"

namespace kws {

__global__ void __launch_bounds__(64) ctc_align_kernel(const float* __restrict__ logits, const int32_t* __restrict__ seq_len,
                                                       const int32_t* __restrict__ labels, const int32_t* __restrict__ label_len, int T, int C,
                                                       int S_max, int32_t* __restrict__ states, int32_t* __restrict__ spans,
                                                       float* __restrict__ score, float* __restrict__ loss, float* __restrict__ post) {
    extern __shared__ float align_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    int len = seq_len[b], S = label_len[b];
    len = len < 0 ? 0 : (len > T ? T : len);
    S = S < 0 ? 0 : (S > S_max ? S_max : S);
    const float* lg = logits + (size_t)b * T * C;
    float* lp = align_lds;
    unsigned long long* back = reinterpret_cast<unsigned long long*>(align_lds + (size_t)T * kCtcRow);      // 32 T bytes in: 8-byte aligned
    int32_t* row = reinterpret_cast<int32_t*>(back + 2 * (size_t)T);
    float* alpha = reinterpret_cast<float*>(row + T);
    const CtcLane c = ctc_lane(labels + (size_t)b * S_max, S, C - 1, lane);
    // 8 frames per pass: lane >> 3 is the frame, lane & 7 the class
    for (int t0 = 0; t0 < len; t0 += 8) {
        const int t = t0 + (lane >> 3), k = lane & 7;
        const bool on = t < len && k < C;
        const float v = ctc_row_log_softmax(on ? lg[(size_t)t * C + k] : -INFINITY);
        if (on) lp[t * kCtcRow + k] = v;
    }
    ctc_wave_sync();
    float best = 0.f;
    int last = 0;
    if (len > 0) best = ctc_viterbi(lp, back, len, c, lane, &last);
    if (lane == 0) score[b] = best;
    const bool path = len > 0 && best > -INFINITY;
    if (states || spans) {
        ctc_wave_sync();
        if (path) ctc_backtrack(back, row, len, last, lane);
        ctc_wave_sync();
        if (states)
            for (int t = lane; t < T; t += 64) states[(size_t)b * T + t] = path && t < len ? row[t] : -1;
        if (spans) {
            int32_t* sp = spans + (size_t)b * S_max * 2;
            for (int i = (path ? 2 * S : 0) + lane; i < 2 * S_max; i += 64) sp[i] = -1;      // no path, and the labels past label_len
            // a label state's frames are one run of the row: its first frame has another state before it, its last another one after it
            for (int t = lane; path && t < len; t += 64) {
                const int s = row[t];
                if (!(s & 1)) continue;
                if (t == 0 || row[t - 1] != s) sp[s - 1] = t;              // spans[k][0], k = s >> 1
                if (t == len - 1 || row[t + 1] != s) sp[s] = t;            // spans[k][1]
            }
        }
    }
    if (!loss && !post) return;
    ctc_wave_sync();
    float nll = 0.f;
    if (len > 0) nll = ctc_alpha(lp, alpha, len, c, lane);
    if (loss && lane == 0) loss[b] = nll;
    if (!post) return;
    ctc_wave_sync();
    float* po = post + (size_t)b * T * S_max;
    const bool feasible = len > 0 && nll < INFINITY;
    if (feasible)
        ctc_beta_post(lp, alpha, len, c, lane, nll, [&](int t, float occ) { if (c.live && (lane & 1)) po[(size_t)t * S_max + (lane >> 1)] = occ; });
    // everything the beta pass did not write: no path, the frames past seq_len, the labels past label_len
    for (int i = lane; i < T * S_max; i += 64) {
        const int t = i / S_max, k = i - t * S_max;
        if (!(feasible && t < len && k < S)) po[i] = 0.f;
    }
}

hipError_t launch_ctc_align(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C,
                            int S_max, int32_t* states, int32_t* spans, float* score, float* loss, float* post, hipStream_t st) {
    return launch_lds<ctc_align_kernel>(dim3(B), dim3(64), ctc_align_lds_bytes(T, S_max, loss || post), st, logits, seq_len, labels, label_len, T,
                                        C, S_max, states, spans, score, loss, post);
}

}  // namespace kws
