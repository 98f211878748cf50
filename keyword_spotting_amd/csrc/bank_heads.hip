// The class heads behind the GRU stack when head 2 comes from a bank of enrolled columns (kws_bank): every stream of a launch has the
// trained head 1 and, spliced in front of its blank, the n_new columns of ITS OWN bank slot user[b].
//
//   bank_heads_kernel<H/16, KEYWORDS>                 kws_step_bank: the grid and phases of dense_heads_kernel (dense_heads.hip) -- one
//                                                     workgroup = one 16-stream group x kHeadFrames frames plus the halo slot, rows past
//                                                     seq_len as there
//   bank_heads_window_kernel<H/16, RAGGED, KEYWORDS>  the bank stream manager (kws_stream_create_bank, kws_step_bank_window): the structure
//                                                     of heads_window_kernel (heads_window.hip) -- the whole chunk, both windows, the coupling
//
// The phases these kernels share with the dense ones are the functions of dense_heads_device.h, head 1 is KWS_HEAD_PROJECT / head_row /
// store_row from there: the bits kws_step_heads produces.  Head 2 runs no second MFMA projection: its frozen logits are head 1's
// accumulator, and the new classes are per-stream [H] x [H, n_new] products on the seam values the lane already holds (bank_device.h:
// the group's columns staged in LDS once per workgroup, 4 H/16 n_new FMAs per lane and frame, the four g lanes folded in a fixed
// order).  They wait in LDS where dense_heads_kernel keeps head 2's logits; the row phase splices them (bank_row) and runs head_row at
// head 2's threshold.
//
// KEYWORDS (kws_last_launch: bank_keyword_heads_kernel / bank_keyword_window_kernel) serves a bank whose slots carry keywords of their own
// (kws_bank_set_keyword, BankSlotKeyword): the kernel takes the slot table behind the plain arguments, head 2 of a stream is the
// C + n_used class head of ITS slot -- bank_row / head_row over the slot's first n_used columns, rows zero-padded to C + n_new -- and
// window 2 walks the slot's label matcher (sixteen of them staged in LDS, window_tail<R, true>).  A bank without keywords launches
// the plain forms.
//
// A stream whose user is outside [0, capacity) has no second head: its logits2 / softmax2 rows are zeros, its frames carry no head-2
// word (tokens 0, prev_word -1; in a manager wordless entries into window 2, hit_2 never set).
#include <type_traits>

#include "bank_device.h"
#include "launch.h"
#include "window_device.h"

namespace kws {

namespace {

// the plain arguments inside either form's
__device__ __forceinline__ const BankHeadsParams& bank_of(const BankHeadsParams& k) { return k; }
__device__ __forceinline__ const BankHeadsParams& bank_of(const BankKeywordHeadsParams& k) { return k.b; }
__device__ __forceinline__ const BankWindowParams& bank_of(const BankWindowParams& k) { return k; }
__device__ __forceinline__ const BankWindowParams& bank_of(const BankKeywordWindowParams& k) { return k.b; }

}  // namespace

template <int NT, bool KEYWORDS>
__global__ void __launch_bounds__(256) bank_heads_kernel(const std::conditional_t<KEYWORDS, BankKeywordHeadsParams, BankHeadsParams> k) {
    constexpr int H = 16 * NT;
    const BankHeadsParams& q = bank_of(k);
    const DenseHeadsParams& p = q.d;
    extern __shared__ __attribute__((aligned(16))) char blds[];
    float* lgs = reinterpret_cast<float*>(blds);                                                   // [head 1 | new classes][stream][slot][8]
    int* words = reinterpret_cast<int*>(blds + kBankHeadsLogitsBytes);                             // [head][stream][slot]
    float* cols = reinterpret_cast<float*>(blds + kBankHeadsLogitsBytes + kBankHeadsWordsBytes);   // bank_stage
    float* bias = cols + (size_t)16 * H * q.bank.n_new;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int G = blockIdx.x, t0 = blockIdx.y * kHeadFrames, T = p.T;
    const int b = G * kStreamsPerGroup + s;
    const bool bvalid = b < p.B;
    const bool two = p.head[1].C > 0;                 // head 2 is wanted
    const int C1 = p.head[0].C, n_new = q.bank.n_new;

    if (two) bank_stage<NT>(q.bank, G * kStreamsPerGroup, p.B, cols, bias, tid);
    float wa[4 * NT];
    f32x4 bias4;
    head_operands<NT>(p.head[0], true, lane, g, wa, bias4);
    int len_s = T;
    if (p.seq_len && bvalid) len_s = p.seq_len[b];
    __syncthreads();      // the staged columns

    const float4* src = p.h_top + (size_t)G * T * NT * 64 + lane;
    const int f_end = min(kHeadSlots, T - t0 + 1);
    for (int f = (w == 0 && t0 == 0) ? 4 : w; f < f_end; f += 4) {      // the first block has no halo
        const int t = t0 - 1 + f;
        f32x4 v[NT];
        seam_row_step<NT>(src, t, len_s, p.nn_outputs, f > 0 && bvalid, b, T, g, v);
        KWS_HEAD_PROJECT(acc, NT, wa, bias4, v);      // dense_heads_device.h: the fused epilogue's summation order
        if (g < 2) *reinterpret_cast<f32x4*>(&lgs[((0 * 16 + s) * kHeadSlots + f) * 8 + 4 * g]) = acc;
        if (two) {
            float nw[8];
            bank_project<NT>(v, cols, bias, n_new, lane, nw);
            if (g == 0) store_row8(&lgs[((1 * 16 + s) * kHeadSlots + f) * 8], nw);
        }
    }
    __syncthreads();

    // one thread per (stream, slot): the rows' relu / clip, softmax and word
    for (int item = tid; item < 16 * kHeadSlots; item += 256) {
        const int si = item / kHeadSlots, f = item - si * kHeadSlots;
        const int t = t0 - 1 + f, bi = G * kStreamsPerGroup + si;
        const bool in_call = t >= 0 && t < T;
        const int len = (p.seq_len && bi < p.B) ? p.seq_len[bi] : T;
        if (!in_call) { words[(0 * 16 + si) * kHeadSlots + f] = -1; words[(1 * 16 + si) * kHeadSlots + f] = -1; continue; }
        const size_t row = (size_t)bi * T + t;
        const bool out = f > 0 && bi < p.B;
        float lg[kMaxClasses], pr[kMaxClasses], raw[kMaxClasses];
        load_row8(&lgs[((0 * 16 + si) * kHeadSlots + f) * 8], raw);
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c) lg[c] = raw[c];
        {
            const DenseHead& hp = p.head[0];
            const int word = head_row(lg, pr, C1, p.use_relu, p.value_clip, hp.decode_thres);
            words[(0 * 16 + si) * kHeadSlots + f] = t < len ? word : -1;
            if (out) {
                if (hp.logits) store_row(hp.logits + row * C1, lg, C1);
                if (hp.softmax) store_row(hp.softmax + row * C1, pr, C1);
            }
        }
        if (two) {
            const DenseHead& hp = p.head[1];
            int word = -1;
            const int u = bank_user(q.bank, bi, p.B);
            if (u >= 0) {
                float nw[kMaxClasses];
                load_row8(&lgs[((1 * 16 + si) * kHeadSlots + f) * 8], nw);
                int n_used = n_new, C2 = hp.C;
                // the slot's own width: the C + n_used class head the user enrolled; the row's tail is zeros (bank_row, head_row)
                if constexpr (KEYWORDS) { n_used = k.slots[u].n_used; C2 = C1 + n_used; }
                bank_row(raw, nw, C1, n_used, lg);
                word = head_row(lg, pr, C2, p.use_relu, p.value_clip, hp.decode_thres);
            } else {
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) { lg[c] = 0.f; pr[c] = 0.f; }
            }
            words[(1 * 16 + si) * kHeadSlots + f] = t < len ? word : -1;
            if (out) {
                if (hp.logits) store_row(hp.logits + row * hp.C, lg, hp.C);
                if (hp.softmax) store_row(hp.softmax + row * hp.C, pr, hp.C);
            }
        }
    }
    __syncthreads();

    heads_tokens(p, words, G, t0, tid);
}

template <int NT, bool RAGGED, bool KEYWORDS>
__global__ void __launch_bounds__(256) bank_heads_window_kernel(const std::conditional_t<KEYWORDS, BankKeywordWindowParams, BankWindowParams> k) {
    constexpr int H = 16 * NT;
    const BankWindowParams& q = bank_of(k);
    const HeadsWindowParams& p = q.w;
    extern __shared__ __attribute__((aligned(16))) char hlds[];
    const int T = p.T, B = p.B;
    const HeadsWindowLds L = heads_window_carve(hlds, T, p.win[0].nq, p.win[1].nq);      // lgs: [head 1 | new classes][stream][frame][8]
    float* cols = reinterpret_cast<float*>(L.rest);                                      // bank_stage
    float* bias = cols + (size_t)16 * H * q.bank.n_new;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int G = blockIdx.x, b0 = G * kStreamsPerGroup;
    const int C1 = p.head[0].C, n_new = q.bank.n_new;
    window_tail_prepare(p.win[0], L.dl, tid);
    window_tail_prepare(p.win[1], L.dl + 256, tid);
    uint8_t* kwdl = reinterpret_cast<uint8_t*>(bias + 128);      // KEYWORDS: [16 streams][256] the slots' matchers
    int* kwn = reinterpret_cast<int*>(kwdl + 16 * 256);          //           [16][n_label, n_used | own << 8]
    if constexpr (KEYWORDS) bank_keywords_stage(q.bank, k.slots, b0, B, p.win[1].n_label, kwdl, kwn, tid);

    if (T > 0) {
        bank_stage<NT>(q.bank, b0, B, cols, bias, tid);
        float wa[4 * NT];
        f32x4 bias4;
        head_operands<NT>(p.head[0], true, lane, g, wa, bias4);
        const float4* src = p.h_top + (size_t)G * T * NT * 64 + lane;
        __syncthreads();      // the staged columns (and the label matchers)
        for (int t0 = 0; t0 < T; t0 += kHeadFrames) {
            const int f_end = min(kHeadFrames, T - t0);
            for (int f = w; f < f_end; f += 4) {
                const int t = t0 + f;
                f32x4 v[NT];
                seam_row<NT>(src, t, v);
                KWS_HEAD_PROJECT(acc, NT, wa, bias4, v);
                if (g < 2) *reinterpret_cast<f32x4*>(&L.lgs[(((0 * 16 + s) * kHeadFrames) + f) * 8 + 4 * g]) = acc;
                float nw[8];
                bank_project<NT>(v, cols, bias, n_new, lane, nw);
                if (g == 0) store_row8(&L.lgs[(((1 * 16 + s) * kHeadFrames) + f) * 8], nw);
            }
            __syncthreads();
            // one thread per (stream, frame): consecutive lanes on consecutive frames of one stream
            for (int item = tid; item < 16 * kHeadFrames; item += 256) {
                const int si = item / kHeadFrames, f = item - si * kHeadFrames;
                const int t = t0 + f, bi = b0 + si;
                const int Tb = RAGGED ? min(p.frames[min(bi, B - 1)], T) : T;
                if (t >= Tb) continue;
                float lg[kMaxClasses], pr[kMaxClasses], raw[kMaxClasses];
                load_row8(&L.lgs[(((0 * 16 + si) * kHeadFrames) + f) * 8], raw);
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) lg[c] = raw[c];
                {
                    const HeadsWindowHead& hp = p.head[0];
                    const int word = head_row(lg, pr, C1, p.use_relu, p.value_clip, hp.decode_thres);
                    L.cw[(0 * 16 + si) * L.stride + t] = (int8_t)word;
                    if (hp.softmax && bi < B) store_row(hp.softmax + ((size_t)bi * T + t) * C1, pr, C1);
                }
                {
                    const HeadsWindowHead& hp = p.head[1];
                    int word = -1;
                    if (bank_user(q.bank, bi, B) >= 0) {
                        float nw[kMaxClasses];
                        load_row8(&L.lgs[(((1 * 16 + si) * kHeadFrames) + f) * 8], nw);
                        int n_used = n_new, C2 = hp.C;
                        if constexpr (KEYWORDS) { n_used = bank_keyword_width(kwn, si); C2 = C1 + n_used; }      // the slot's own width; the row's tail is zeros
                        bank_row(raw, nw, C1, n_used, lg);
                        word = head_row(lg, pr, C2, p.use_relu, p.value_clip, hp.decode_thres);
                    } else {
#pragma unroll
                        for (int c = 0; c < kMaxClasses; ++c) pr[c] = 0.f;
                    }
                    L.cw[(1 * 16 + si) * L.stride + t] = (int8_t)word;
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
    // KEYWORDS: window 2 walks the matcher of the lane's stream's slot; window 2's own where the slot has none
    const int ts = tid >> 4;
    const uint8_t* dl2 = L.dl + 256;
    int nl2 = 0;
    if constexpr (KEYWORDS) {
        if (kwn[2 * ts + 1] & 256) dl2 = kwdl + ts * 256;
        nl2 = kwn[2 * ts];
    }
    const bool hit2w = window_tail<4, KEYWORDS>(p.win[1], B, b0, Tt, L.cw + 16 * L.stride, L.stride, dl2, L.scratch + window_tail_scratch_bytes(p.win[0].nq),
                                                tid, req2, live, nl2);
    // a stream without a slot never reports head 2 (its window holds wordless entries only; this covers the empty label too)
    heads_window_couple(p, b0, tid, bt, live, hit1, hit2w, [&](int b) { return bank_user(q.bank, b, B) >= 0; });
}

// kws_bank_set_keyword: one slot's entry, by value through the kernel arguments -- stream-ordered, and no host memory outlives the call
__global__ void __launch_bounds__(64) bank_set_keyword_kernel(BankSlotKeyword* dst, const BankSlotKeyword v) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&v);
    for (int i = threadIdx.x; i < (int)(sizeof(BankSlotKeyword) / 4); i += 64) reinterpret_cast<uint32_t*>(dst)[i] = src[i];
}
hipError_t launch_bank_set_keyword(BankSlotKeyword* dst, const BankSlotKeyword& v, hipStream_t st) {
    return launch_lds<bank_set_keyword_kernel>(dim3(1), dim3(64), 0, st, dst, v);
}

hipError_t launch_bank_heads(const BankHeadsParams& p, const BankSlotKeyword* slots, int hidden, hipStream_t st) {
    const dim3 grid(groups_of(p.d.B), (p.d.T + kHeadFrames - 1) / kHeadFrames);
    const size_t lds = bank_heads_lds_bytes(hidden, p.bank.n_new);
    return with_int<4, 8, 16>(hidden % 16 == 0 ? hidden / 16 : -1, [&](auto nt) {
        if (slots) return launch_lds<bank_heads_kernel<nt(), true>>(grid, dim3(256), lds, st, BankKeywordHeadsParams{p, slots});
        return launch_lds<bank_heads_kernel<nt(), false>>(grid, dim3(256), lds, st, p);
    });
}

hipError_t launch_bank_heads_window(const BankWindowParams& p, const BankSlotKeyword* slots, int hidden, hipStream_t st) {
    const size_t lds = bank_window_lds_bytes(p.w.T, p.w.win[0].nq, p.w.win[1].nq, hidden, p.bank.n_new);
    return with_int<4, 8, 16>(hidden % 16 == 0 ? hidden / 16 : -1, [&](auto nt) {
        return with_bool(p.w.frames != nullptr, [&](auto ragged) {
            if (slots)
                return launch_lds<bank_heads_window_kernel<nt(), ragged(), true>>(dim3(groups_of(p.w.B)), dim3(256), lds + kBankKeywordStageBytes, st,
                                                                                  BankKeywordWindowParams{p, slots});
            return launch_lds<bank_heads_window_kernel<nt(), ragged(), false>>(dim3(groups_of(p.w.B)), dim3(256), lds, st, p);
        });
    });
}

}  // namespace kws
