// The class heads behind the GRU stack when head 2 comes from a bank of enrolled columns (kws_bank): every stream of a launch has the
// trained head 1 and, spliced in front of its blank, the n_new columns of ITS OWN bank slot user[b].
//
//   bank_heads_kernel<H/16>                 kws_step_bank: the grid and phases of dense_heads_kernel (dense_heads.hip) -- one workgroup =
//                                           one 16-stream group x kHeadFrames frames plus the halo slot, rows past seq_len as there
//   bank_heads_window_kernel<H/16, RAGGED>  the bank stream manager (kws_stream_create_bank, kws_step_bank_window): the structure of
//                                           heads_window_kernel (heads_window.hip) -- the whole chunk, both windows, the coupling
//
// Head 1 is KWS_HEAD_PROJECT / head_row / store_row of dense_heads_device.h: the bits kws_step_heads produces.  Head 2 runs no second
// MFMA projection: its frozen logits are head 1's accumulator, and the new classes are per-stream [H] x [H, n_new] products on the
// seam values the lane already holds (bank_device.h: the group's columns staged in LDS once per workgroup, 4 H/16 n_new FMAs per lane
// and frame, the four g lanes folded in a fixed order).  They wait in LDS where dense_heads_kernel keeps head 2's logits; the row phase
// splices them (bank_row) and runs head_row at head 2's threshold.
//
// The keyword forms bank_keyword_heads_kernel / bank_keyword_window_kernel (the same text, bank_heads_kernels.inc) serve a bank whose slots
// carry keywords of their own (kws_bank_set_keyword, BankSlotKeyword): head 2 of a stream is the C + n_used class head of ITS slot --
// bank_row / head_row over the slot's first n_used columns, rows zero-padded to C + n_new -- and window 2 walks the slot's label
// matcher (sixteen of them staged in LDS, window_tail<R, true>).  A bank without keywords launches the plain kernels.
//
// A stream whose user is outside [0, capacity) has no second head: its logits2 / softmax2 rows are zeros, its frames carry no head-2
// word (tokens 0, prev_word -1; in a manager wordless entries into window 2, hit_2 never set).
#include "bank_device.h"
#include "launch.h"
#include "window_device.h"

namespace kws {

namespace {

constexpr int kBankSlots = kHeadFrames + 1;        // slot f <-> frame t0 - 1 + f; slot 0 is the halo (dense_heads.hip)

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

}  // namespace

#define KWS_BANK_KEYWORDS 0
#include "bank_heads_kernels.inc"
#undef KWS_BANK_KEYWORDS
#define KWS_BANK_KEYWORDS 1
#include "bank_heads_kernels.inc"
#undef KWS_BANK_KEYWORDS

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
        if (slots) return launch_lds<bank_keyword_heads_kernel<nt()>>(grid, dim3(256), lds, st, BankKeywordHeadsParams{p, slots});
        return launch_lds<bank_heads_kernel<nt()>>(grid, dim3(256), lds, st, p);
    });
}

hipError_t launch_bank_heads_window(const BankWindowParams& p, const BankSlotKeyword* slots, int hidden, hipStream_t st) {
    const size_t lds = bank_window_lds_bytes(p.w.T, p.w.win[0].nq, p.w.win[1].nq, hidden, p.bank.n_new);
    return with_int<4, 8, 16>(hidden % 16 == 0 ? hidden / 16 : -1, [&](auto nt) {
        return with_bool(p.w.frames != nullptr, [&](auto ragged) {
            if (slots)
                return launch_lds<bank_keyword_window_kernel<nt(), ragged()>>(dim3(groups_of(p.w.B)), dim3(256), lds + kBankKeywordStageBytes, st,
                                                                             BankKeywordWindowParams{p, slots});
            return launch_lds<bank_heads_window_kernel<nt(), ragged()>>(dim3(groups_of(p.w.B)), dim3(256), lds, st, p);
        });
    });
}

}  // namespace kws
