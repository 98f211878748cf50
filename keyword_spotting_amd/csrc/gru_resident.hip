// Resident streaming GRU layer kernel (hidden 128, fp32) for gfx950 (MI355X) and its launcher.
//
// Semantics, MFMA orientation and the xl exchange layout are those of gru_kernels.hip (see its header and DESIGN.md
// "Kernels"); this kernel keeps the layer's recurrent + candidate weights in registers (AGPR side of the unified file,
// 192 + 2*KCX fragments per wave) and the gate x-part in LDS, so nothing but the mel / previous layer's h stream is
// read per step.  (Builtin build: the gate x-part sits in the AGPRs that the recurrent weights leave free -- all of it in the
// first layer, 16 of 32 k-chunks above it -- and only the rest streams from LDS, see resident_kreg.)  The x-part MFMAs of frame t+1 are issued behind frame t's two barriers (software pipeline), so the
// LDS exchange latency overlaps independent matrix work.
//
// A translation unit of its own because of its code generation: with KWS_RESIDENT_VGPR_FORM (set by the Makefile when
// hipcc accepts -amdgpu-mfma-vgpr-form) every MFMA of the frame loop is the builtin, the accumulators live in VGPRs and
// the "+a"-pinned weight fragments are read from AGPRs as source A directly -- no accumulator copies and no hand-placed
// wait states: the compiler sees every hazard.  Without the option the h-part MFMAs are the inline-asm form of
// gru_device.h between resident_prefence() / resident_fence().
#include <cstddef>

#include "gru_device.h"
#include "launch.h"
#include "window_device.h"

namespace kws {

// The h-part chains of the frame loop: asm MFMAs need their wait states placed by hand (gru_device.h); builtin ones do not.
#if KWS_RESIDENT_VGPR_FORM
template <class... A> __device__ __forceinline__ void resident_prefence(A&...) {}
// (the activations behind an h-part chain stay one VALU cluster: nothing is scheduled across the end of the chain)
template <class... A> __device__ __forceinline__ void resident_fence(A&...) { __builtin_amdgcn_sched_barrier(0); }
#else
template <class... A> __device__ __forceinline__ void resident_prefence(A&... a) { mfma_prefence(a...); }
template <class... A> __device__ __forceinline__ void resident_fence(A&... a) { mfma_fence(a...); }
#endif


// Gate x-part k-chunks (4 A fragments each: {r0,u0,r1,u1}) that stay in AGPRs for the whole launch.  The recurrent and
// candidate h-part fragments take 192 of the 256 accumulator registers; with builtin MFMAs (source A straight from an AGPR)
// the other 64 hold gate x-part chunks instead of idling: the whole x-part of a first layer (KCX <= 16), 16 of the 32 chunks
// above it, 10 in the window-tail kernel (its tail needs the registers).  The weights are call-invariant, so every chunk
// kept here is one ds_read_b128 per wave and frame that is not issued.  The inline-asm build takes the A operand of its
// builtin x-part MFMAs from VGPRs and keeps the earlier placement (two chunks above the first layer).
#if KWS_RESIDENT_VGPR_FORM
constexpr int resident_kreg(int kcx, bool first, bool last, bool window) { return first ? kcx : (last && window) ? 10 : 16; }
#else
constexpr int resident_kreg(int, bool first, bool, bool) { return first ? 0 : 2; }
#endif
// LDS of one workgroup: hbuf | rhbuf | the gate x-part chunks that are not in registers | upper layers: the x block |
// last layer: the partial-logit ring | first layer: the mel frame.  (The window tail adds kWinTailWordsBytes behind that.)
constexpr size_t resident_lds_bytes(int kcx, bool first, bool last, bool window) {
    size_t n = 2 * 8 * 64 * 16 + (size_t)4 * (kcx - resident_kreg(kcx, first, last, window)) * 64 * 16;
    if (!first) n += 8 * 64 * 16;
    if (last) n += kPartialRingLdsBytes;
    if (first) n += (size_t)64 * xs_stride(kcx) * 4;
    return n;
}

// ------------------------------------------------------------------------------------------------
// Resident kernel, H = 128.  KCX = x-part k-chunks (ceil(I/4) for the first layer, 32 above it).
// ------------------------------------------------------------------------------------------------
// WINDOW (instantiated for the upper last layer only): the decode-window step of the stream manager rides at the end of
// every group (window_device.h); every other instantiation compiles exactly as without the parameter.
// MASKED: the call carries seq_len (dynamic_rnn copy-through past a stream's length).  Without it the kernel never reads
// p.seq_len and the state update has no select.  The body is shared by the two kernel templates below it.
template <int KCX, bool FIRST, bool LAST, bool MASKED, bool WINDOW>
__device__ __forceinline__ void gru_layer_resident_body(const GruLayerParams& p) {
    static_assert(!WINDOW || (LAST && !FIRST), "the window tail belongs to the last layer of a stack");
    static_assert(!WINDOW || !MASKED, "the window tail refuses seq_len");
    constexpr int H = 128, NT = 8, KCH = 32;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, g = lane >> 4, s = lane & 15;
    // Persistent over stream groups: the weights are staged ONCE per workgroup and launch; with more groups than the grid
    // (B > 16 x CUs) a workgroup takes groups blockIdx.x, blockIdx.x + gridDim.x, ... one after the other.  Everything
    // that depends on the group is (re)set at the top of the group loop below; the lambdas see it by reference.
    const int n_groups = (p.B + kStreamsPerGroup - 1) / kStreamsPerGroup;
    int group = blockIdx.x;
    int b_raw = group * kStreamsPerGroup + s;
    bool bvalid = b_raw < p.B;
    int b = bvalid ? b_raw : p.B - 1;
    const int T = p.T;
    const int n0 = 2 * w, n1 = 2 * w + 1;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* hbuf = reinterpret_cast<f32x4*>(smem);       // [NT][64]  h_{t-1}, xl layout
    f32x4* rhbuf = hbuf + NT * 64;                       // [NT][64]  r (.) h_{t-1}
    // Gate x-part k-chunks 0..KREG-1 stay in registers (resident_kreg); the rest, KL chunks, streams from LDS every frame
    constexpr int KREG = resident_kreg(KCX, FIRST, LAST, WINDOW), KL = KCX - KREG;
    static_assert(KREG >= 0 && KREG <= KCX && 192 + 4 * KREG <= 256, "the register chunks share the 256 AGPRs with the recurrent weights");
    f32x4* wlds = rhbuf + NT * 64;                       // [4 waves][KL][64] gate x-part, k-chunks KREG..KCX-1: {r0,u0,r1,u1}
    f32x4* xsb = wlds + 4 * KL * 64;                     // [NT][64]  upper layers: x(t+1) of the group, xl layout (see "x stream")
    char* const lds_tail = reinterpret_cast<char*>(xsb + (FIRST ? 0 : NT * 64));
    static_assert(resident_lds_bytes(KCX, FIRST, LAST, WINDOW) + (WINDOW ? kWinTailWordsBytes : 0) <= 160 * 1024, "LDS per CU");
    float* const pring = reinterpret_cast<float*>(lds_tail);     // LAST only: the partial logits of 16 frames (gru_device.h)
    int8_t* const cwords = WINDOW ? reinterpret_cast<int8_t*>(lds_tail + kPartialRingLdsBytes) : nullptr;
    const uint8_t* win_dl = reinterpret_cast<const uint8_t*>(cwords) + 16 * kWinTailWordsStride;     // WINDOW only: the label matcher
    constexpr size_t kWinOffset = offsetof(GruLayerParams, win);
    if constexpr (WINDOW) window_tail_prepare(window_tail_params_from_kernarg(kWinOffset), const_cast<uint8_t*>(win_dl), tid);   // (visible after the group loop's first barrier)
    // FIRST only: one frame of mel for the group, [16 streams x 4 lane groups][kXsStride] floats, row
    // (4s+g) holds x[s][4*kc+g] for kc = 0..KCX-1 -- each lane's B operands are contiguous
    constexpr int kXsStride = xs_stride(KCX);       // 4 * odd: rows 16 apart in one ds_read_b128 group spread over the banks
    float* xs = reinterpret_cast<float*>(lds_tail + (LAST ? kPartialRingLdsBytes : 0));

    // ---- stage weights: registers (recurrent + candidate) and LDS (gate x-part) ------------------
    // p.wh is the group-of-4 layout [NT][3][KCH/4][64][4]: one dwordx4 per four fragments.  p.wx is the
    // same layout above the first layer and fragment-major [NT][3][KCX][64] (interleaved k map) in it.
    float wgh[2][2][KCH];   // [tile][r|u][k-chunk]  A fragments of Wg rows I..I+H
    float wch[2][KCH];      // candidate, h-part
    float wcx[2][KCX];      // candidate, x-part
    float wgx[KREG ? KREG : 1][4];   // gate x-part k-chunks 0..KREG-1, {r0,u0,r1,u1} as in wlds
    const f32x4* wh4 = reinterpret_cast<const f32x4*>(p.wh);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = 2 * w + j;
#pragma unroll
        for (int k4 = 0; k4 < KCH / 4; ++k4) {
            const f32x4 vr = wh4[((n * 3 + 0) * (KCH / 4) + k4) * 64 + lane];
            const f32x4 vu = wh4[((n * 3 + 1) * (KCH / 4) + k4) * 64 + lane];
            const f32x4 vc = wh4[((n * 3 + 2) * (KCH / 4) + k4) * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                wgh[j][0][4 * k4 + e] = vr[e];
                wgh[j][1][4 * k4 + e] = vu[e];
                wch[j][4 * k4 + e] = vc[e];
            }
        }
    }
    if constexpr (FIRST) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kc = 0; kc < KCX; ++kc) wcx[j][kc] = p.wx[(((2 * w + j) * 3 + 2) * KCX + kc) * 64 + lane];
#pragma unroll
        for (int kc = 0; kc < KCX; ++kc) {
            f32x4 v;
            v.x = p.wx[((n0 * 3 + 0) * KCX + kc) * 64 + lane];
            v.y = p.wx[((n0 * 3 + 1) * KCX + kc) * 64 + lane];
            v.z = p.wx[((n1 * 3 + 0) * KCX + kc) * 64 + lane];
            v.w = p.wx[((n1 * 3 + 1) * KCX + kc) * 64 + lane];
            if (kc < KREG) { const int kr = kc < KREG ? kc : 0; wgx[kr][0] = v[0]; wgx[kr][1] = v[1]; wgx[kr][2] = v[2]; wgx[kr][3] = v[3]; }
            else wlds[(w * KL + kc - KREG) * 64 + lane] = v;
        }
    } else {
        const f32x4* wx4 = reinterpret_cast<const f32x4*>(p.wx);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k4 = 0; k4 < KCX / 4; ++k4) {
                const f32x4 vc = wx4[(((2 * w + j) * 3 + 2) * (KCX / 4) + k4) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) wcx[j][4 * k4 + e] = vc[e];
            }
#pragma unroll
        for (int k4 = 0; k4 < KCX / 4; ++k4) {
            const f32x4 r0 = wx4[((n0 * 3 + 0) * (KCX / 4) + k4) * 64 + lane];
            const f32x4 u0 = wx4[((n0 * 3 + 1) * (KCX / 4) + k4) * 64 + lane];
            const f32x4 r1 = wx4[((n1 * 3 + 0) * (KCX / 4) + k4) * 64 + lane];
            const f32x4 u1 = wx4[((n1 * 3 + 1) * (KCX / 4) + k4) * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4 v = {r0[e], u0[e], r1[e], u1[e]};
                const int kc = 4 * k4 + e, kr = kc < KREG ? kc : 0;
                if (kc < KREG) { wgx[kr][0] = v[0]; wgx[kr][1] = v[1]; wgx[kr][2] = v[2]; wgx[kr][3] = v[3]; }
                else wlds[(w * KL + kc - KREG) * 64 + lane] = v;
            }
        }
    }
    // park the recurrent fragments in AGPRs for the whole launch (192 of the 256; the register chunks of the gate x-part behind them)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
            asm volatile("" : "+a"(wgh[j][0][kc]));
            asm volatile("" : "+a"(wgh[j][1][kc]));
            asm volatile("" : "+a"(wch[j][kc]));
        }
    }
#if KWS_RESIDENT_VGPR_FORM      // (builtin MFMAs of the asm-form build take their A operand from VGPRs: no AGPR round trip for these)
    if constexpr (KREG > 0) {
#pragma unroll
        for (int kc = 0; kc < KREG; ++kc)
#pragma unroll
            for (int e = 0; e < 4; ++e) asm volatile("" : "+a"(wgx[kc][e]));
    }
#endif
    asm volatile("s_nop 7" ::: "memory");   // v_accvgpr_write -> MFMA SrcA distance
    f32x4 bias_r[2], bias_u[2], bias_c[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = 2 * w + j;
        bias_r[j] = ld4(p.bias + 0 * H + n * 16 + 4 * g);
        bias_u[j] = ld4(p.bias + 1 * H + n * 16 + 4 * g);
        bias_c[j] = ld4(p.bias + 2 * H + n * 16 + 4 * g);
    }
    float wfc[2][4];
    f32x4 bfc4 = splat4(0.f);
    if (LAST) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) wfc[j][e] = p.wfc[((2 * w + j) * 4 + e) * 64 + lane];
        if (w == 0) bfc4 = ld4(p.bfc + 4 * g);
    }

    // ---- per-group state: set by enter_group() -----------------------------------------------------
    int len_s = T;                       // MASKED only
    int carry = -1;                      // LAST only: the word before the flush's next block, of this lane's stream there (4w + lane / 16)
    f32x4 hreg[2];
    const float4* xl_src = nullptr;
    const float4* xprev = nullptr;
    const float4* xg_next = nullptr;     // upper layers: where this wave's next group_issue() reads (slice n0 of block min(t_req, T - 1))
    // the x-stream descriptors below (xl_row, xl_q, xl_active) do not depend on the group
    constexpr int XQ = KCX;                          // float4 pieces per mel row (I == 4*KCX)
    const int xl_row = lane / XQ, xl_q = lane % XQ;  // this lane's (stream-in-quarter, piece)
    const bool xl_active = FIRST && lane < 4 * XQ;
    auto enter_group = [&]() {
        b_raw = group * kStreamsPerGroup + s;
        bvalid = b_raw < p.B;
        b = bvalid ? b_raw : p.B - 1;
        const bool do_reset = p.reset != nullptr && p.reset[b] != 0;
        if constexpr (MASKED) len_s = p.seq_len ? p.seq_len[b] - p.t_base : T;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = 2 * w + j;
            hreg[j] = do_reset ? splat4(0.f) : ld4(p.state_in + (size_t)b * H + n * 16 + 4 * g);
            hbuf[n * 64 + lane] = hreg[j];
        }
        if (LAST) {
            carry = carried_word(p.prev_word, p.reset, group * kStreamsPerGroup + 4 * w + (lane >> 4), p.B);
        }
        if constexpr (FIRST) {
            const int xl_b = min(group * kStreamsPerGroup + 4 * w + (xl_active ? xl_row : 0), p.B - 1);
            xl_src = reinterpret_cast<const float4*>(p.x_mel + (size_t)xl_b * (p.t_stride ? p.t_stride : T) * p.I) + xl_q;
        } else {
            xprev = p.x_prev + (size_t)group * T * NT * 64 + lane;
            xg_next = xprev + ((size_t)(1 < T ? 1 : 0) * NT + n0) * 64;
        }
    };

    // ---- x stream --------------------------------------------------------------------------------
    // First layer: the four waves fetch the group's mel frame COOPERATIVELY -- wave w loads streams
    // 4w..4w+3 (one global_load_dwordx4, 4*I/4 active lanes) two frames ahead, scatters it into `xs`
    // late in the frame, and every wave reads its B operands back with three LDS reads.  A global load
    // costs ~30 cycles of MFMA time and an LDS read ~2.4 (tools/ubench/mfma_operands.hip); ten divergent
    // dword loads per wave per frame were 4.5 % of this kernel.
    // With a seam above this layer (kIssueAtEnd) the load of the NEXT staging step is issued right behind a frame's commit and
    // AHEAD of its two seam stores: the wait that guards the next commit sits ahead of that frame's stores in program order.
    // Issued at the top of the following frame instead, its address arithmetic reuses xl_inflight's registers and the compiler
    // drains vmcnt(0) -- the seam stores, a few hundred cycles old -- in front of the frame's first MFMA.  A layer that is
    // first AND last stores nothing per frame and keeps the request at the frame top.
    constexpr bool kIssueAtEnd = FIRST && !LAST;
    // Upper layers: the previous layer's xl-layout block (8 slices of 64 float4) is fetched ONCE per group -- wave w requests
    // slices 2w and 2w+1 of x(t+2) at the top of frame t, writes them to `xsb` behind barrier #1 (every wave has read x(t+1) out
    // of it by then; barrier #2 publishes them), and every wave reads the eight slices of x(t+2) during gates_h of frame t+1,
    // one ds_read_b128 per MFMA group.  A global load costs ~30 cycles of MFMA time and an LDS read ~2.4; each wave fetching
    // the whole block was 8 loads per wave and frame, four times the bytes.
    float4 xl_inflight = make_float4(0.f, 0.f, 0.f, 0.f);
    auto coop_issue = [&](int t_req) {               // global -> register (in flight)
        const int t = t_req < T ? t_req : T - 1;
        if (xl_active) xl_inflight = xl_src[(size_t)t * XQ];
    };
    auto coop_commit = [&]() {                       // register -> xs
        if (xl_active) {
            float* dst = xs + (4 * (4 * w + xl_row)) * kXsStride + xl_q;
            dst[0 * kXsStride] = xl_inflight.x;
            dst[1 * kXsStride] = xl_inflight.y;
            dst[2 * kXsStride] = xl_inflight.z;
            dst[3 * kXsStride] = xl_inflight.w;
        }
    };
    float xbuf0[KCX];
    auto read_xs = [&](float (&dst)[KCX]) {          // xs -> this lane's B operands
        const float* row = xs + (4 * s + g) * kXsStride;
#pragma unroll
        for (int k4 = 0; k4 < KCX / 4; ++k4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * k4);
            dst[4 * k4 + 0] = v[0]; dst[4 * k4 + 1] = v[1]; dst[4 * k4 + 2] = v[2]; dst[4 * k4 + 3] = v[3];
        }
        if constexpr (KCX % 4 >= 2) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(row + (KCX / 4) * 4);
            dst[(KCX / 4) * 4 + 0] = v[0]; dst[(KCX / 4) * 4 + 1] = v[1];
        }
        if constexpr (KCX % 2 == 1) dst[KCX - 1] = row[KCX - 1];
    };
    auto load_x_slice = [&](float (&dst)[KCX], int t_req, const int sl) {   // upper layers, prologue; sl: unrolled constant
        if constexpr (!FIRST) {
            const int t = t_req < T ? t_req : T - 1;
            const float4 v = xprev[((size_t)t * NT + sl) * 64];
            dst[4 * sl + 0] = v.x; dst[4 * sl + 1] = v.y; dst[4 * sl + 2] = v.z; dst[4 * sl + 3] = v.w;
        }
    };
    float4 xg_inflight[2];                                      // upper layers: this wave's two slices of the group's next block
    auto group_issue = [&](int t_req) {                         // global -> register (in flight); t_req = 1, 2, 3, ... within a group
        if constexpr (!FIRST) {
            xg_inflight[0] = xg_next[0];
            xg_inflight[1] = xg_next[64];
            if (t_req + 1 < T) xg_next += NT * 64;
        }
    };
    auto group_commit = [&]() {                                 // register -> xsb
        if constexpr (!FIRST) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                xsb[(2 * w + j) * 64 + lane] = (f32x4){xg_inflight[j].x, xg_inflight[j].y, xg_inflight[j].z, xg_inflight[j].w};
        }
    };
    auto read_x_slice = [&](float (&dst)[KCX], const int sl) {  // xsb -> this lane's B operands of k-chunks 4sl..4sl+3
        if constexpr (!FIRST) {
            const f32x4 v = xsb[sl * 64 + lane];
            dst[4 * sl + 0] = v[0]; dst[4 * sl + 1] = v[1]; dst[4 * sl + 2] = v[2]; dst[4 * sl + 3] = v[3];
        }
    };

    f32x4 acc_r[2], acc_u[2], acc_c[2];
    // gate x-part for k-chunks [K0, K1): A fragments stream from LDS through a 3-deep register ring
    // (two ds_read_b128 in flight behind the MFMAs that consume the third); chunks below KREG come from wgx
    auto gates_x_part = [&](const float (&xB)[KCX], auto k0_, auto k1_, auto pin_) {
        constexpr int K0 = decltype(k0_)::value, K1 = decltype(k1_)::value;
        constexpr bool PIN = decltype(pin_)::value;
        constexpr int R0 = K0 < KREG ? KREG : K0;          // first chunk that streams from LDS
        f32x4 ring[3];
        if (R0 < K1) ring[R0 % 3] = wlds[(w * KL + R0 - KREG) * 64 + lane];
        if (R0 + 1 < K1) ring[(R0 + 1) % 3] = wlds[(w * KL + R0 + 1 - KREG) * 64 + lane];
#pragma unroll
        for (int kc = K0; kc < K1; ++kc) {
            if (kc + 2 < K1 && kc + 2 >= R0 + 2) ring[(kc + 2) % 3] = wlds[(w * KL + kc + 2 - KREG) * 64 + lane];
            if (PIN) __builtin_amdgcn_sched_barrier(0);   // keep the read two groups ahead of its MFMAs
            const int kr = kc < KREG ? kc : 0;
            const f32x4 a4 = kc < KREG ? (f32x4){wgx[kr][0], wgx[kr][1], wgx[kr][2], wgx[kr][3]} : ring[kc % 3];
            acc_r[0] = mfma4(a4.x, xB[kc], acc_r[0]);
            acc_u[0] = mfma4(a4.y, xB[kc], acc_u[0]);
            acc_r[1] = mfma4(a4.z, xB[kc], acc_r[1]);
            acc_u[1] = mfma4(a4.w, xB[kc], acc_u[1]);
            if (PIN) __builtin_amdgcn_sched_barrier(0);
        }
    };
    using pinned = std::true_type;
    constexpr int KSPLIT = KCX / 2;
    using k_lo = std::integral_constant<int, 0>;
    using k_mid = std::integral_constant<int, KSPLIT>;
    using k_hi = std::integral_constant<int, KCX>;
    auto cand_x = [&](const float (&xB)[KCX]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) acc_c[j] = bias_c[j];
#pragma unroll
        for (int kc = 0; kc < KCX; ++kc) {
            acc_c[0] = mfma4(wcx[0][kc], xB[kc], acc_c[0]);
            acc_c[1] = mfma4(wcx[1][kc], xB[kc], acc_c[1]);
        }
    };

    f32x4 hb_a, hb_b;            // exchange-read pipeline registers (two float4 in flight)

    // One frame (xcur == xnxt == the single B-operand buffer: x(t+1) lands in it during this frame).
    auto frame = [&](int t, float (&xcur)[KCX], float (&xnxt)[KCX]) {
        // gates, h-part:  acc_{r,u} += Wg[I:,:]^T h_{t-1}   (hb_a/hb_b were fetched behind cand_x);
        // upper layers: this wave's share of x(t+2) is requested at the top, one slice of x(t+1) is read from xsb per group
        // (first layer: the mel row for the next commit was requested at the end of the previous frame)
        resident_prefence(acc_r[0], acc_u[0], acc_r[1], acc_u[1]);
#pragma unroll
        for (int nn = 0; nn < NT; ++nn) {
            const f32x4 hb = (nn & 1) ? hb_b : hb_a;
            if (nn + 2 < NT) {
                if (nn & 1) hb_b = hbuf[(nn + 2) * 64 + lane]; else hb_a = hbuf[(nn + 2) * 64 + lane];
            }
            if constexpr (FIRST) { if (!kIssueAtEnd && nn == 0) coop_issue(t + 2); }
            else { if (nn == 0) group_issue(t + 2); read_x_slice(xnxt, nn); }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kc = 4 * nn + e;
                const float hv = hb[e];
                KWS_MFMA_A(acc_r[0], wgh[0][0][kc], hv);
                KWS_MFMA_A(acc_u[0], wgh[0][1][kc], hv);
                KWS_MFMA_A(acc_r[1], wgh[1][0][kc], hv);
                KWS_MFMA_A(acc_u[1], wgh[1][1][kc], hv);
            }
        }
        resident_fence(acc_r[0], acc_u[0], acc_r[1], acc_u[1]);
        if constexpr (FIRST) read_xs(xcur);          // x(t+1), committed to LDS during frame t-1
        // ---- region A: the 16 sigmoids as one VALU cluster (r first so r(.)h reaches LDS early), then the
        // first half of frame t+1's gate x-part as cover for the exchange
        f32x4 u[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x2 r_lo = sigmoid2((f32x2){acc_r[j][0], acc_r[j][1]});
            const f32x2 r_hi = sigmoid2((f32x2){acc_r[j][2], acc_r[j][3]});
            const f32x2 rh_lo = r_lo * (f32x2){hreg[j][0], hreg[j][1]};
            const f32x2 rh_hi = r_hi * (f32x2){hreg[j][2], hreg[j][3]};
            rhbuf[(2 * w + j) * 64 + lane] = (f32x4){rh_lo.x, rh_lo.y, rh_hi.x, rh_hi.y};
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x2 u_lo = sigmoid2((f32x2){acc_u[j][0], acc_u[j][1]});
            const f32x2 u_hi = sigmoid2((f32x2){acc_u[j][2], acc_u[j][3]});
            u[j] = (f32x4){u_lo.x, u_lo.y, u_hi.x, u_hi.y};
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) { acc_r[j] = bias_r[j]; acc_u[j] = bias_u[j]; }
        __builtin_amdgcn_sched_barrier(0);
        gates_x_part(xcur, k_lo{}, k_mid{}, pinned{});
        lds_barrier();           // #1: r(.)h visible; every wave is done reading hbuf (and x(t+1) out of xsb)
        hb_a = rhbuf[0 * 64 + lane];
        hb_b = rhbuf[1 * 64 + lane];
        group_commit();          // x(t+2): visible after barrier #2, read in frame t+1
        gates_x_part(xcur, k_mid{}, k_hi{}, pinned{});     // second half hides the rhbuf read latency

        // candidate, h-part:  acc_c += Wc[I:,:]^T (r (.) h_{t-1})
        resident_prefence(acc_c[0], acc_c[1]);
#pragma unroll
        for (int nn = 0; nn < NT; ++nn) {
            const f32x4 rb = (nn & 1) ? hb_b : hb_a;
            if (nn + 2 < NT) {
                if (nn & 1) hb_b = rhbuf[(nn + 2) * 64 + lane]; else hb_a = rhbuf[(nn + 2) * 64 + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kc = 4 * nn + e;
                const float rv = rb[e];
                KWS_MFMA_A(acc_c[0], wch[0][kc], rv);
                KWS_MFMA_A(acc_c[1], wch[1][kc], rv);
            }
        }
        resident_fence(acc_c[0], acc_c[1]);
        // ---- region B: tanh + state update as one VALU cluster
        const unsigned live = !MASKED || t < len_s ? 0xffffffffu : 0u;   // MASKED: dynamic_rnn copy-through past seq_len
        f32x4 hout[2];                                                    // MASKED && LAST: zero output rows past seq_len
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const f32x2 c = tanh2((f32x2){acc_c[j][2 * h2], acc_c[j][2 * h2 + 1]});
                const f32x2 uu = {u[j][2 * h2], u[j][2 * h2 + 1]};
                const f32x2 hh = {hreg[j][2 * h2], hreg[j][2 * h2 + 1]};
                // u*h + (1-u)*c with (1-u)*c rounded on its own and u*h fused into the sum: written out, because left to
                // contraction the compiler picks which product to fuse per instantiation, and the last bit follows its pick
                const f32x2 hn = __builtin_elementwise_fma(uu, hh, (1.0f - uu) * c);
                if constexpr (!MASKED) {
                    hreg[j][2 * h2] = hn.x;
                    hreg[j][2 * h2 + 1] = hn.y;
                    continue;
                }
                hreg[j][2 * h2] = bitsel(live, hn.x, hh.x);
                hreg[j][2 * h2 + 1] = bitsel(live, hn.y, hh.y);
                if (LAST) {
                    hout[j][2 * h2] = bitsel(live, hn.x, 0.f);
                    hout[j][2 * h2 + 1] = bitsel(live, hn.y, 0.f);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) acc_c[j] = bias_c[j];
        constexpr int NCX = 2 * KCX;                         // candidate x-part MFMAs of frame t+1
        constexpr int NPOST = NCX >= 32 ? 16 : 8;            // kept for after barrier #2 (covers the hbuf read)
        constexpr int NPRE = NCX - NPOST;
        auto cand_x_mfma = [&](auto mc) {
            constexpr int m = decltype(mc)::value, kc = m / 2;
            if constexpr (m % 2 == 0) acc_c[0] = mfma4(wcx[0][kc], xcur[kc], acc_c[0]);
            else acc_c[1] = mfma4(wcx[1][kc], xcur[kc], acc_c[1]);
        };
        if constexpr (FIRST) {
            coop_commit();                           // x(t+2): visible after barrier #2, read in frame t+1
            if constexpr (kIssueAtEnd) coop_issue(t + 3);     // ahead of the seam stores below
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            hbuf[(2 * w + j) * 64 + lane] = hreg[j];
            if (!LAST) {
                const f32x4 o = hreg[j];
                p.h_out[((size_t)group * T + t) * NT * 64 + (2 * w + j) * 64 + lane] =
                    make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        if constexpr (LAST) {
            // partial logits over this wave's 32 units, Wfc^T[:, units] h'[units], into the frame's slot of the ring (gru_device.h).
            // The fence keeps region B one VALU run: without it single logit MFMAs move up between the ops of the state update
            // and split its packed multiplies and adds
            __builtin_amdgcn_sched_barrier(0);
            f32x4 accf = bfc4;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) accf = mfma4(wfc[j][e], MASKED ? hout[j][e] : hreg[j][e], accf);
            if (g < 2) *reinterpret_cast<f32x4*>(partial_slot(pring, t) + (w * 16 + s) * 8 + 4 * g) = accf;
        }
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, NPRE>(cand_x_mfma);     // most of frame t+1's candidate x-part covers the LDS write
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();           // #2: h_t and the frame's partial logits visible; every wave is done reading rhbuf
        hb_a = hbuf[0 * 64 + lane];
        hb_b = hbuf[1 * 64 + lane];
        __builtin_amdgcn_sched_barrier(0);
        static_for<NPRE, NCX>(cand_x_mfma);   // the rest of frame t+1's candidate x-part hides the hbuf read
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (LAST) {
            // every 16 frames and at the end of the call: no barrier, see epilogue_flush_partials
            if (((t + 1) & (kRingFrames - 1)) == 0 || t == T - 1) {
                const int t0 = t & ~(kRingFrames - 1);
                epilogue_flush_partials(p, pring, cwords, group, t0, t - t0 + 1, w, lane, t == T - 1, carry);
            }
        }
    };

    for (; group < n_groups; group += gridDim.x) {
    enter_group();
    if constexpr (!FIRST) {
        if (T > 0) {             // x(1) into xsb (the previous group's closing barrier has freed it); x(0) straight into registers
            group_issue(1);
#pragma unroll
            for (int sl = 0; sl < NT; ++sl) load_x_slice(xbuf0, 0, sl);
            group_commit();
        }
    }
    __syncthreads();             // staged weights (first group) / this group's state and x(1) are in LDS
    if (T > 0) {
        if constexpr (FIRST) {
            coop_issue(0);
            coop_commit();
            __syncthreads();
            read_xs(xbuf0);                          // x(0)
            coop_issue(1);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) { acc_r[j] = bias_r[j]; acc_u[j] = bias_u[j]; }
        gates_x_part(xbuf0, k_lo{}, k_hi{}, pinned{});
        hb_a = hbuf[0 * 64 + lane];
        hb_b = hbuf[1 * 64 + lane];
        cand_x(xbuf0);
        if constexpr (FIRST) {
            __syncthreads();                         // every wave has read x(0) out of xs
            coop_commit();                           // x(1)
            if constexpr (kIssueAtEnd) coop_issue(2);
            __syncthreads();
        }
    }
    for (int t = 0; t < T; ++t) frame(t, xbuf0, xbuf0);

    if (bvalid) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            *reinterpret_cast<f32x4*>(p.state_out + (size_t)b * H + (2 * w + j) * 16 + 4 * g) = hreg[j];
    }
    __syncthreads();             // every wave is done with this group's LDS state before the next group overwrites it
    if constexpr (WINDOW) {
        // detector.py:195-209 for this group's 16 streams: the call's frame words wait in cwords, the scratch is hbuf | rhbuf
        const WindowTail win = window_tail_params_from_kernarg(kWinOffset);
        WindowTailRegs<2> wreq;
        window_tail_request<2>(win, p.B, group * kStreamsPerGroup, tid, wreq);
        window_tail<2>(win, p.B, group * kStreamsPerGroup, T, cwords, kWinTailWordsStride, win_dl, reinterpret_cast<char*>(hbuf), tid, wreq);
        __syncthreads();
    }
    }
}

// The kernels: a call without seq_len runs gru_layer_resident, one with it gru_layer_resident_masked (never the window tail).
template <int KCX, bool FIRST, bool LAST, bool WINDOW = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
gru_layer_resident(const GruLayerParams p) { gru_layer_resident_body<KCX, FIRST, LAST, false, WINDOW>(p); }
template <int KCX, bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
gru_layer_resident_masked(const GruLayerParams p) { gru_layer_resident_body<KCX, FIRST, LAST, true, false>(p); }
template <int KCX, bool FIRST, bool LAST, bool MASKED>
inline constexpr auto resident_kernel = MASKED ? &gru_layer_resident_masked<KCX, FIRST, LAST> : &gru_layer_resident<KCX, FIRST, LAST, false>;

// ------------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------------
int gru_resident_kcx(int in_dim, bool first) { return first ? (in_dim + 3) / 4 : 32; }

bool gru_resident_supported(int hidden, int in_dim, bool first) {
    if (hidden != 128) return false;
    if (!first) return in_dim == 128;
    // instantiated KCX = 8, 10, 12, 15, 16 (rows must be whole float4s, and the cooperative mel staging needs
    // 4 streams x KCX float4 pieces <= 64 lanes): the reference's 40 (README.md:17) and 60 (config/rnn_config.py:63),
    // plus the other common front-end widths up to 64
    return in_dim == 32 || in_dim == 40 || in_dim == 48 || in_dim == 60 || in_dim == 64;
}

bool gru_resident_takes_window(bool first, bool last) { return last && !first; }

// the resident kernels loop over stream groups themselves: one workgroup per CU at most (each fills a CU's register file),
// the weights staged once per workgroup however many groups it takes
hipError_t launch_gru_layer_resident(const GruLayerParams& p, bool first, bool last, hipStream_t st) {
    const bool window = p.win.tab != nullptr;
    const size_t lds = resident_lds_bytes(p.KCX, first, last, window);
    const dim3 grid(persistent_grid(p.B));
    if (window) {                             // with the window tail: the last layer of a stack only
        if (!gru_resident_takes_window(first, last) || p.seq_len) return hipErrorInvalidValue;
        return launch_lds<gru_layer_resident<32, false, true, true>>(grid, dim3(256), lds + kWinTailWordsBytes, st, p);
    }
    return with_bool(p.seq_len != nullptr, [&](auto ma) {
        return with_bool(last, [&](auto la) {
            if (!first) return launch_lds<resident_kernel<32, false, la(), ma()>>(grid, dim3(256), lds, st, p);
            return with_int<8, 10, 12, 15, 16>(p.KCX, [&](auto kcx) {
                return launch_lds<resident_kernel<kcx(), true, la(), ma()>>(grid, dim3(256), lds, st, p);
            });
        });
    });
}

}  // namespace kws
