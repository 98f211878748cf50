// Both class heads and both decode windows of a two-head stream manager (kws_stream_create_heads, kws_step_heads_window): ONE
// launch behind the GRU stack, whose layers all write seams as a kws_step_heads call plans them.  The reference README
// ("Customize keyword") keeps both dense layers on the frozen stack and says "do softmax and decode respectively";
// server_demo.py:122-129 ORs the two decisions; detector.py:202-208 clears the window and the state on a detection.
//
// One workgroup = one 16-stream group and the WHOLE chunk, in blocks of kHeadFrames frames: wave w projects the frames w, w + 4,
// ... of the block for both heads (KWS_HEAD_PROJECT, dense_heads_device.h -- the code dense_heads_kernel compiles, so the same bits),
// the logits wait in LDS, and behind a barrier one thread per (stream, frame) does relu / clip, softmax and the frame word
// (head_row).  Each head's words go to that head's LDS row cw[head][stream][t]: the words of the whole chunk stay in LDS, so no
// halo frame is needed -- the window decides a chunk's first frame against its predecessor itself (window_device.h).
//
// Behind the frame loop, when the weight fragments are dead, the two windows are evaluated one after the other with the pieces
// the fused GRU tails and window_inc_kernel use (window_tail_request / window_tail), each on its own label matcher and its own
// ring staging.  Then the coupling: fired = hit_1 | hit_2, and if fired the q == 0 lane of the stream writes head = count = 0
// for BOTH windows and restart = 1 -- "the other head fired" is the same state change as "this head fired"
// (tests/test_heads_stream_host.py).  hit[b] = hit_1 | hit_2 << 1.
//
// RAGGED (kws_stream_feed_ragged): stream b has frames[b] <= T frames -- rows at or past it get no word and are not written --
// and skip[b] behaves as in window_inc_kernel<true>: no slot in either window, restart untouched, hit 0.
//
// T == 0 (a chunk that completes no frame): no stack ran, h_top is not read; an empty entry goes into both windows.
//
// The LDS carve, the seam row, the logit row and the coupling are the functions of dense_heads_device.h, the ones bank_heads_window_kernel
// (bank_heads.hip) calls: one text per phase.  The operand load is written out here: through head_operands this kernel was 0.5 us per
// chunk slower at 4096 streams than the parent's (profiles/heads_family_refactor_ab.txt), with it inline it is not.
#include "dense_heads_device.h"
#include "launch.h"
#include "window_device.h"

namespace kws {

template <int NT, bool RAGGED>
__global__ void __launch_bounds__(256) heads_window_kernel(const HeadsWindowParams p) {
    extern __shared__ __attribute__((aligned(16))) char hlds[];
    const int T = p.T, B = p.B;
    const HeadsWindowLds L = heads_window_carve(hlds, T, p.win[0].nq, p.win[1].nq);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int G = blockIdx.x, b0 = G * kStreamsPerGroup;
    window_tail_prepare(p.win[0], L.dl, tid);
    window_tail_prepare(p.win[1], L.dl + 256, tid);

    if (T > 0) {
        float wa[2][4 * NT];
        f32x4 bias4[2];
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {      // head_operands' two statements, inline: as the function this kernel measured 0.5 us slower per chunk
#pragma unroll
            for (int kc = 0; kc < 4 * NT; ++kc) wa[hd][kc] = p.head[hd].wfc[kc * 64 + lane];
            bias4[hd] = ld4(p.head[hd].bfc + 4 * g);
        }
        const float4* src = p.h_top + (size_t)G * T * NT * 64 + lane;
        for (int t0 = 0; t0 < T; t0 += kHeadFrames) {
            const int f_end = min(kHeadFrames, T - t0);
            for (int f = w; f < f_end; f += 4) {
                const int t = t0 + f;
                f32x4 v[NT];
                seam_row<NT>(src, t, v);
#pragma unroll
                for (int hd = 0; hd < 2; ++hd) {
                    KWS_HEAD_PROJECT(acc, NT, wa[hd], bias4[hd], v);
                    if (g < 2) *reinterpret_cast<f32x4*>(&L.lgs[(((hd * 16 + s) * kHeadFrames) + f) * 8 + 4 * g]) = acc;
                }
            }
            __syncthreads();
            // one thread per (stream, frame): consecutive lanes on consecutive frames of one stream
            for (int item = tid; item < 16 * kHeadFrames; item += 256) {
                const int si = item / kHeadFrames, f = item - si * kHeadFrames;
                const int t = t0 + f, bi = b0 + si;
                const int Tb = RAGGED ? min(p.frames[min(bi, B - 1)], T) : T;
                if (t >= Tb) continue;
#pragma unroll
                for (int hd = 0; hd < 2; ++hd) {
                    const HeadsWindowHead& hp = p.head[hd];
                    float lg[kMaxClasses], pr[kMaxClasses];
                    load_row8(&L.lgs[(((hd * 16 + si) * kHeadFrames) + f) * 8], lg);
                    const int word = head_row(lg, pr, hp.C, p.use_relu, p.value_clip, hp.decode_thres);
                    L.cw[(hd * 16 + si) * L.stride + t] = (int8_t)word;
                    if (hp.softmax && bi < B) store_row(hp.softmax + ((size_t)bi * T + t) * hp.C, pr, hp.C);
                }
            }
            __syncthreads();      // the block's logits are consumed, and (last block) the chunk's words are complete
        }
    } else {
        __syncthreads();          // the label matchers
    }

    // ---- the two windows, then the coupling
    WindowTailRegs<4> req1, req2;
    window_tail_request<4>(p.win[0], B, b0, tid, req1);
    window_tail_request<4>(p.win[1], B, b0, tid, req2);
    const int bt = min(b0 + (tid >> 4), B - 1);                  // window_tail's stream of this lane
    const int Tt = RAGGED ? min(p.frames[bt], T) : T;
    const bool live = RAGGED ? p.skip[bt] == 0 : true;
    const bool hit1 = window_tail<4>(p.win[0], B, b0, Tt, L.cw, L.stride, L.dl, L.scratch, tid, req1, live);
    const bool hit2 = window_tail<4>(p.win[1], B, b0, Tt, L.cw + 16 * L.stride, L.stride, L.dl + 256, L.scratch + window_tail_scratch_bytes(p.win[0].nq),
                                     tid, req2, live);
    heads_window_couple(p, b0, tid, bt, live, hit1, hit2, [](int) { return true; });
}

// kws_stream_recycle on a two-head manager: head 2's window of the recycled streams (head 1's goes with stream_recycle_kernel)
__global__ void window_reset_masked_kernel(const uint8_t* slots, int B, int* head, int* count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && slots[b] != 0) { head[b] = 0; count[b] = 0; }
}

hipError_t launch_window_reset_masked(const uint8_t* slots, int B, int* head, int* count, hipStream_t st) {
    return launch_lds<window_reset_masked_kernel>(dim3((B + 63) / 64), dim3(64), 0, st, slots, B, head, count);
}

hipError_t launch_heads_window(const HeadsWindowParams& p, int hidden, hipStream_t st) {
    const size_t lds = heads_window_lds_bytes(p.T, p.win[0].nq, p.win[1].nq);
    return with_int<4, 8, 16>(hidden % 16 == 0 ? hidden / 16 : -1, [&](auto nt) {
        return with_bool(p.frames != nullptr, [&](auto ragged) {
            return launch_lds<heads_window_kernel<nt(), ragged()>>(dim3(groups_of(p.B)), dim3(256), lds, st, p);
        });
    });
}

}  // namespace kws
