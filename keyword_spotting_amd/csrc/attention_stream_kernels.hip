// The sliding-window manager of the self-attention model (kws_attention_stream_*, api_attention_stream.hip): what detector.py:158-209
// does with its queue of softmax chunks, one stage earlier -- the model carries no state, so the queue holds MEL frames and the model
// runs over the whole window after every chunk.  Three kernels around the model's launches:
//   attn_stream_window_kernel   behind the front-end's gate launch: clear on silence, SimpleQueue.add of the chunk's frames
//   attn_stream_decide_kernel   behind the model: ctc_decode2 + ctc_predict over the window's softmax rows, clear on a hit
//   attn_stream_recycle_kernel  kws_attention_stream_recycle
#include "attention_internal.h"
#include "launch.h"

namespace kws {

// One 256-thread workgroup per stream.  The window is linear and oldest-first IN PLACE: an eviction moves the live frames behind the
// dropped slot to the front, 1024 floats per pass -- every thread reads its four, the workgroup meets, every thread writes.  A
// pass writes [base, base + 1024) and reads [base + off, base + off + 1024), off > 0: what it overwrites was read in this pass or an
// earlier one, always in front of a barrier; nothing is read after it has been overwritten.  The chunk's frames are appended behind
// the last pass's barrier (their place overlaps what the shift reads).
__global__ void __launch_bounds__(256) attn_stream_window_kernel(const AttnStreamWindowParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (p.skip[b]) {                          // an empty chunk: carry, window and slots stay as they are; the model sees length 0
        if (tid == 0) p.run_len[b] = 0;
        return;
    }
    int32_t* slots = p.slot_frames + (size_t)b * p.nq;
    int count = p.count[b], len = p.len[b];
    if (p.silent[b]) { count = 0; len = 0; }                         // detector.py:171-177
    const int nd = count == p.nq ? 1 : 0;                            // add(): drop the oldest when full (utils/queue.py:26-32)
    const int drop = nd ? slots[0] : 0;
    const int keep = len - drop;
    int f = p.frames[b];
    f = f < 0 ? 0 : (f > p.T ? p.T : f);
    f = f > p.W - keep ? p.W - keep : f;                             // (never: W = nq x the longest chunk's frames)
    const int moved = count - nd;
    const int sv = tid < moved ? slots[tid + nd] : 0;
    float* w = p.win + (size_t)b * p.W * p.F;
    const int nshift = drop > 0 ? keep * p.F : 0, off = drop * p.F;
    __syncthreads();                                                 // slots[] has been read
    for (int base = 0; base < nshift; base += 1024) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + tid + 256 * j;
            v[j] = i < nshift ? w[off + i] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + tid + 256 * j;
            if (i < nshift) w[i] = v[j];
        }
    }
    const float* src = p.mel + (size_t)b * p.T * p.F;
    float* dst = w + (size_t)keep * p.F;
    for (int i = tid; i < f * p.F; i += 256) dst[i] = src[i];
    if (tid < moved) slots[tid] = sv;
    if (tid == moved) slots[tid] = f;
    if (tid == 0) {
        p.count[b] = moved + 1;
        p.len[b] = keep + f;
        p.run_len[b] = keep + f;
    }
}

// One wave per stream, 64 rows per pass: the frame word of every row (ctc_decode2's rule, utils/prediction.py:67,74-75: the first
// maximum over classes 1..C-2, strictly above the threshold, else none), a row emits its word when it differs from the row before it
// (:76-80; the last row of the pass before is carried), and the label's matcher walks the pass's emissions in order -- the wave steps
// through the ballot's set bits together, so T' of several hundred rows costs a few passes and one table read per emitted word.
__global__ void __launch_bounds__(64) attn_stream_decide_kernel(const AttnStreamDecideParams p) {
    __shared__ uint8_t dl[256];
    const int b = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) dl[i] = p.delta[i];
    __syncthreads();
    const int n = p.run_len[b];
    int rows = n > 0 ? (p.c > 1 ? n / p.c + 1 : n) : 0;
    rows = rows > p.T1max ? p.T1max : rows;
    const int C = p.C;
    int state = 0, carry = -1;
    bool found = false;
    for (int base = 0; base < rows && !found; base += 64) {
        const int t = base + lane;
        int wd = -1;
        if (t < rows) {
            const float* row = p.softmax + ((size_t)b * p.T1max + t) * C;
            float best = row[1];
            int arg = 0;
            for (int cl = 2; cl < C - 1; ++cl)
                if (row[cl] > best) { best = row[cl]; arg = cl - 1; }
            wd = best > p.thres ? arg : -1;
        }
        const int up = __shfl_up(wd, 1);
        const int pv = lane == 0 ? carry : up;
        unsigned long long m = __builtin_amdgcn_ballot_w64(wd >= 0 && wd != pv);
        while (m && !found) {                                        // wave-uniform
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            const int word = __shfl(wd, l) + 1;
            state = __builtin_amdgcn_readfirstlane((int)dl[state * 16 + word]);
            found = state == p.n_label;
        }
        carry = __shfl(wd, 63);
    }
    if (lane == 0) {
        p.hit[b] = found ? 1 : 0;
        if (found) { p.count[b] = 0; p.len[b] = 0; }                 // detector.py:202-208
    }
}

__global__ void __launch_bounds__(64) attn_stream_recycle_kernel(const AttnStreamRecycleParams p) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B || !p.slots[b]) return;
    p.carry_len[b] = 0;
    p.count[b] = 0;
    p.len[b] = 0;
}

hipError_t launch_attn_stream_window(const AttnStreamWindowParams& p, hipStream_t st) {
    return launch_lds<attn_stream_window_kernel>(dim3(p.B), dim3(256), 0, st, p);
}
hipError_t launch_attn_stream_decide(const AttnStreamDecideParams& p, hipStream_t st) {
    return launch_lds<attn_stream_decide_kernel>(dim3(p.B), dim3(64), 0, st, p);
}
hipError_t launch_attn_stream_recycle(const AttnStreamRecycleParams& p, hipStream_t st) {
    return launch_lds<attn_stream_recycle_kernel>(dim3((p.B + 63) / 64), dim3(64), 0, st, p);
}

}  // namespace kws
