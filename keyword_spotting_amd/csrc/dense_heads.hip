// The class heads of a multi-head step (kws_step_heads): one launch behind the GRU stack that reads the top layer's seam once
// and produces, for up to two dense layers, logits -> relu / clip -> softmax -> the ctc_decode2 frame rule, and optionally the
// top layer's rows themselves (model/nn_outputs:0, [B,T,H] row-major).
//
// One workgroup = one 16-stream group x kHeadFrames frames.  Wave w projects the frames of slots w, w + 4, ...: a lane's xl
// float4 of tile n (kws_internal.h) is the B operand of the k-chunks 4n..4n+3, the A operands are the fragments of Wfc^T
// (padded to 16 rows) the fused epilogue of the GRU kernels uses, and the 16x16 result holds class 4g + r of stream s in lane
// (g, s).  The logits wait in LDS; behind a barrier one thread per (stream, frame) does the row's softmax and word, consecutive
// lanes on consecutive frames of one stream, so that a stream's rows leave as one contiguous run.
//
// Rows past seq_len.  A GRU layer that is not the last one stores its carried state for frames t >= seq_len[b]
// (gru_resident.hip, the frame's store of hreg), where dynamic_rnn emits the zero row.  This kernel therefore takes seq_len
// itself and replaces the loaded row by zeros: nn_outputs = 0, logits = bfc (the accumulator's initial value, every product
// an exact zero), and the frame has no word.  It never depends on what the seam holds there.
//
// prev_word is in/out, and the frame blocks of one stream are different workgroups: the block with t = 0 reads it, the block
// with t = T - 1 writes it.  Settled by construction: the host copies each head's prev_word into a side buffer on the call's
// stream ahead of the launch (DenseHead::prev_in, as the int8 path's oct_prev), and only that copy is read here.  A block with
// t0 > 0 gets the word of frame t0 - 1 by projecting that frame itself in slot 0 -- the same loop body, so the same
// instruction sequence and the same bits as the block that owns the frame.
//
// The phases -- operand load, seam row with the zero row and the nn_outputs store, projection, the row's softmax and word, tokens and the
// carried word -- are the functions of dense_heads_device.h, the ones bank_heads_kernel (bank_heads.hip) calls: one text per phase.
#include "dense_heads_device.h"
#include "launch.h"

namespace kws {

template <int NT>
__global__ void __launch_bounds__(256) dense_heads_kernel(const DenseHeadsParams p) {
    __shared__ float lgs[2][16][kHeadSlots][8];      // logits of [head][stream][slot]: a lane of the row phase reads its 8 as two float4
    __shared__ int words[2][16][kHeadSlots];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int G = blockIdx.x, t0 = blockIdx.y * kHeadFrames, T = p.T;
    const int b = G * kStreamsPerGroup + s;
    const bool bvalid = b < p.B;

    // A operands of each head; an absent head (C == 0) keeps zeros and is skipped below
    float wa[2][4 * NT];
    f32x4 bias4[2];
#pragma unroll
    for (int hd = 0; hd < 2; ++hd) head_operands<NT>(p.head[hd], p.head[hd].C > 0, lane, g, wa[hd], bias4[hd]);
    int len_s = T;
    if (p.seq_len && bvalid) len_s = p.seq_len[b];

    const float4* src = p.h_top + (size_t)G * T * NT * 64 + lane;
    const int f_end = min(kHeadSlots, T - t0 + 1);
    for (int f = (w == 0 && t0 == 0) ? 4 : w; f < f_end; f += 4) {      // the first block has no halo
        const int t = t0 - 1 + f;
        f32x4 v[NT];
        seam_row_step<NT>(src, t, len_s, p.nn_outputs, f > 0 && bvalid, b, T, g, v);
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            if (p.head[hd].C == 0) continue;
            KWS_HEAD_PROJECT(acc, NT, wa[hd], bias4[hd], v);      // dense_heads_device.h: the fused epilogue's summation order
            if (g < 2) *reinterpret_cast<f32x4*>(&lgs[hd][s][f][4 * g]) = acc;
        }
    }
    __syncthreads();

    // one thread per (stream, slot): the row's relu / clip, softmax and word
    for (int item = tid; item < 16 * kHeadSlots; item += 256) {
        const int si = item / kHeadSlots, f = item - si * kHeadSlots;
        const int t = t0 - 1 + f, bi = G * kStreamsPerGroup + si;
        const bool in_call = t >= 0 && t < T;
        const int len = (p.seq_len && bi < p.B) ? p.seq_len[bi] : T;
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
            const DenseHead& hp = p.head[hd];
            if (hp.C == 0) continue;
            if (!in_call) { words[hd][si][f] = -1; continue; }
            float lg[kMaxClasses], pr[kMaxClasses];
            load_row8(&lgs[hd][si][f][0], lg);
            const int word = head_row(lg, pr, hp.C, p.use_relu, p.value_clip, hp.decode_thres);
            words[hd][si][f] = t < len ? word : -1;
            if (f > 0 && bi < p.B) {
                const size_t row = (size_t)bi * T + t;
                if (hp.logits) store_row(hp.logits + row * hp.C, lg, hp.C);
                if (hp.softmax) store_row(hp.softmax + row * hp.C, pr, hp.C);
            }
        }
    }
    __syncthreads();

    heads_tokens(p, &words[0][0][0], G, t0, tid);
}

hipError_t launch_dense_heads(const DenseHeadsParams& p, int hidden, hipStream_t st) {
    const dim3 grid(groups_of(p.B), (p.T + kHeadFrames - 1) / kHeadFrames);
    return with_int<4, 8, 16>(hidden % 16 == 0 ? hidden / 16 : -1, [&](auto nt) {
        return launch_lds<dense_heads_kernel<nt()>>(grid, dim3(256), 0, st, p);
    });
}

}  // namespace kws
