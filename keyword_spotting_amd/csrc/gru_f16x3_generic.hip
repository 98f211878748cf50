// "f16x3" for the shapes the register-resident kernels (gru_f16x3.hip: hidden = 128) do not cover -- BASELINE configs[4]: 4 x GRU
// h = 256, n_mel = 60 (config/rnn_config.py:76,84) -- with the weights STREAMED FROM L2 every frame, as gru_layer_generic /
// gru_stack_generic_pipelined (gru_kernels.hip) stream their fp32 weights.  Same semantics (models/rnn_ctc.py:155-165,202-284;
// TF-1.x GRUCell), same boundary, same tolerance as every f16x3 kernel: logits within 1e-4 of the fp64 oracle.
//
// Why: an h = 256 layer's weights are 1.5 MiB whether they are fp32 or (hi, lo) fp16 pairs, so either way a workgroup re-reads
// 1.5 MiB per frame out of its XCD's L2.  The fp32 kernel then spends 28.8 us per frame in v_mfma_f32_16x16x4_f32 (0.63 of the
// fp32 MFMA peak); three v_mfma_f32_16x16x32_f16 per operand pair need a quarter of that matrix time, and what remains is the
// L2 -> CU stream itself: tools/ubench/l2_stream_f16x3.hip measured 12.7-13.8 us per frame for 256 workgroups streaming at
// once (31 TB/s out of the eight L2s), 2.1-2.3x the fp32 kernel -- above the 1.5x the round-5 review set as the bar for building this.
//
// Operand split, exponent-scale folding, mel pre-scale and the K permutation are gru_f16x3.hip's (v = hi + 2^-11 lo; three MFMAs
// per product: main += Wh Xh, lo += Wl Xh + Wh Xl; a wave's pair of C tiles, split and packed, IS one 32-wide chunk of the next
// B operand).  One workgroup = 4 waves = 16 streams; wave w owns tiles [TPW w, TPW w + TPW) of r, u, c and h' (TPW = H / 64) and
// streams their operands: per input / hidden chunk one ROW = all of the wave's tiles x gates x (hi, lo) -- 24 KiB per wave at
// h = 256 -- through two register sets, the next row's buffer loads issued ahead of the current row's MFMAs.  Table layout
// p.w: [H/16 tiles][3 gates][KX + H/32 chunks][hi|lo][64 lanes] x 16 B, x chunks first (kws_create).
// The layers meet through the split seam [G][T][H/32 chunks][hi|lo][64 lanes] x 16 B, as in gru_f16x3.hip; in the layer-pipelined
// launch (all L x G workgroups in one grid, gru_stack_f16x3_pipelined) it lives in fine-grained memory behind per-group frame
// counters, exactly the protocol of gru_stack_generic_pipelined.
#include <cstddef>

#include "f16x3_device.h"
#include "gru_device.h"
#include "launch.h"
#include "pipeline_device.h"

namespace kws {

namespace {
typedef int i32x4 __attribute__((ext_vector_type(4)));
}  // namespace

size_t gru_f16x3_generic_lds_bytes(int hidden, bool last) {
    const size_t hc = hidden / 32;
    size_t n = 3 * hc * 2 * 64 * 16;              // hb, rhb, xsb (the first layer's input needs <= 2 chunks of xsb)
    n += (size_t)3 * hidden * 4 + 16 * 4 + 16;    // biases + class bias + the pipelined launch's "next frame is there" flag
    if (last) n += kEpilogueLdsBytes;
    return n;
}

// TPW: tiles per wave, H = 64 TPW (2: h = 128, 4: h = 256).  PIPE: the layer-pipelined launch.
template <int TPW, bool FIRST, bool LAST, bool PIPE>
__device__ __forceinline__ void gru_f16x3_generic_body(const GruF16Params& p, const int group) {
    constexpr int H = 64 * TPW, HC = H / 32, CPW = TPW / 2;      // CPW: chunks of the hidden vector a wave produces
    static_assert(TPW == 2 || TPW == 4, "h = 128 or 256");
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int b_raw = group * kStreamsPerGroup + s;
    const bool bvalid = b_raw < p.B;
    const int b = bvalid ? b_raw : p.B - 1;
    const int T = p.T;
    const int KX = FIRST ? 2 * ((p.I + 63) / 64) : HC, KC = KX + HC;      // the first layer's x chunks padded to an even count (zero operands)

    extern __shared__ __attribute__((aligned(16))) char smem[];
    u32x4* hb = reinterpret_cast<u32x4*>(smem);              // [HC][hi|lo][64]  h_{t-1}
    u32x4* rhb = hb + HC * 2 * 64;                             // [HC][2][64]      r (.) h_{t-1}
    u32x4* xsb = rhb + HC * 2 * 64;                            // [HC][2][64]      this frame's input (the first layer uses KX <= 2 chunks)
    float* biasl = reinterpret_cast<float*>(xsb + HC * 2 * 64); // [3][H] + [16]
    const EpilogueLds epi = epilogue_carve(reinterpret_cast<char*>(biasl + 3 * H + 16 + 4));  // LAST only ([3H + 16 .. +4): the pipelined launch's flag)

    // the weight stream: buffer loads, lane offset in one VGPR, the operand index in the scalar offset (1 KiB per operand)
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(p.w), (short)0, 0x7fffffff, 0x00020000);
    const int lane16 = lane * 16;
    auto wload = [&](int tile, int q, int c, int hl) -> u32x4 {
        return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, lane16, ((((tile * 3 + q) * KC + c) * 2 + hl)) * 1024, 0));
    };

    // kws_create folded the exponent scales into the weights (gates: -log2 e, candidate: 2 log2 e): the biases get them here
    for (int i = tid; i < 3 * H; i += 256) biasl[i] = p.bias[i] * (i < 2 * H ? -kLog2e : 2.0f * kLog2e);
    if (LAST && tid < 16) biasl[3 * H + tid] = p.bfc[tid];
    for (int i = tid; i < HC * 2 * 64; i += 256) xsb[i] = (u32x4){0u, 0u, 0u, 0u};
    const f32x4* bl = reinterpret_cast<const f32x4*>(biasl);

    const bool do_reset = p.reset != nullptr && p.reset[b] != 0;
    const int len_s = p.seq_len ? p.seq_len[b] : T;
    f32x4 hreg[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) hreg[j] = do_reset ? splat4(0.f) : ld4(p.state_in + (size_t)b * H + (TPW * w + j) * 16 + 4 * g);
#pragma unroll
    for (int jj = 0; jj < CPW; ++jj) {
        u32x4 hi, lo;
        split8_scaled(hreg[2 * jj], hreg[2 * jj + 1], hi, lo);
        hb[((CPW * w + jj) * 2 + 0) * 64 + lane] = hi;
        hb[((CPW * w + jj) * 2 + 1) * 64 + lane] = lo;
    }
    if (LAST) epilogue_carry_init(epi, p.epi.prev_word, p.reset, group, p.B, tid);
    // the projection's operands: this wave's chunks of Wfc^T (hi, lo), resident
    u32x4 wfc[CPW][2];
    if (LAST) {
#pragma unroll
        for (int jj = 0; jj < CPW; ++jj)
#pragma unroll
            for (int hl = 0; hl < 2; ++hl) wfc[jj][hl] = __builtin_bit_cast(u32x4, p.wfc[((CPW * w + jj) * 2 + hl) * 64 + lane]);
    }

    // ---- input: FIRST: wave w brings streams 4w..4w+3 of the mel frame (one dwordx4 per lane), scales, clamps, splits and scatters
    // them into the B-operand image (gru_f16x3.hip's staging); above: the seam row of the frame, already split, in operand order ----
    const int XQ = FIRST ? p.I / 4 : 1;
    const int xl_row = lane / XQ, xl_q = lane % XQ;
    const bool xl_active = FIRST && lane < 4 * XQ;
    const float* mel_row = nullptr;
    if (FIRST) mel_row = p.x_mel + (size_t)min(group * kStreamsPerGroup + 4 * w + (xl_active ? xl_row : 0), p.B - 1) * T * p.I + xl_q * 4;
    const int xs_lane = ((((xl_q * 4) / 32) * 2 + 0) * 64 + (((xl_q * 4) % 32) / 8) * 16 + (4 * w + xl_row)) * 4 + ((xl_q * 4) % 8) / 2;   // dwords
    unsigned* const xsb_dw = reinterpret_cast<unsigned*>(xsb);
    f32x4 melv = splat4(0.f);
    auto mel_fetch = [&](int t_req) {
        if (xl_active) melv = ld4(mel_row + (size_t)(t_req < T ? t_req : T - 1) * p.I);
    };
    auto mel_commit = [&]() {
        if (xl_active) {
            uint2 hi, lo;
            mel_split4(melv, hi, lo);
            *reinterpret_cast<uint2*>(xsb_dw + xs_lane) = hi;
            *reinterpret_cast<uint2*>(xsb_dw + 64 * 4 + xs_lane) = lo;
        }
    };
    // this group's [T][HC][2][64] x 16 B blocks of the seams
    const __amdgpu_buffer_rsrc_t xp_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        FIRST ? const_cast<uint4*>(p.w) : const_cast<uint4*>(p.x_prev + (size_t)group * T * HC * 2 * 64), (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t ho_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        LAST ? const_cast<uint4*>(p.w) : const_cast<uint4*>(p.h_out + (size_t)group * T * HC * 2 * 64), (short)0, 0x7fffffff, 0x00020000);
    constexpr int XF = HC * 2 / 4;                // seam operands (1 KiB) of a frame per wave
    u32x4 xin[XF];
    auto seam_fetch = [&](int t_req) {          // the pipelined launch reads rows another CU has just written: system scope
        const int t = t_req < T ? t_req : T - 1;
#pragma unroll
        for (int i = 0; i < XF; ++i)
            xin[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xp_rsrc, lane16, (t * (HC * 2) + (w + 4 * i)) * 1024, PIPE ? kSysScope : 0));
    };
    auto seam_commit = [&]() {
#pragma unroll
        for (int i = 0; i < XF; ++i) xsb[(w + 4 * i) * 64 + lane] = xin[i];
    };

    if (FIRST) { mel_fetch(0); mel_commit(); mel_fetch(1); }
    else if (!PIPE) { seam_fetch(0); seam_commit(); seam_fetch(1); }
    __syncthreads();

    // ---- rows: all of the wave's tiles for one chunk, in ONE register image (24 operands at h = 256).  X rows carry the three
    // gates, H rows r and u, C rows two chunks of the candidate's recurrent part (so that every row keeps >= 16 KiB per wave in
    // flight).  Two images A / B ping-pong through the whole frame: every phase has an even number of rows (kws_create pads the
    // first layer's x-part to an even chunk count), starts in A, and the load that would run past a phase's end fetches the
    // NEXT phase's first row instead -- the weights do not depend on the data, so the stream never drains at a phase
    // boundary, a barrier or a frame boundary (the candidate's first row lands during the r / u activations, the next frame's
    // first x row during tanh / update).
    struct Row { u32x4 a[TPW * 6]; };
    auto load_x = [&](Row& r, int c) {
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
                for (int hl = 0; hl < 2; ++hl) r.a[(j * 3 + q) * 2 + hl] = wload(TPW * w + j, q, c, hl);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto load_h = [&](Row& r, int m) {
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int hl = 0; hl < 2; ++hl) r.a[(j * 2 + q) * 2 + hl] = wload(TPW * w + j, q, KX + m, hl);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto load_c = [&](Row& r, int m2) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < TPW; ++j)
#pragma unroll
                for (int hl = 0; hl < 2; ++hl) r.a[(k * TPW + j) * 2 + hl] = wload(TPW * w + j, 2, KX + 2 * m2 + k, hl);
        __builtin_amdgcn_sched_barrier(0);
    };
    // Both images are always loaded or loading: a phase enters with its first TWO rows requested by the phase before it, every
    // image is re-requested the moment its MFMAs have been issued -- with the next row of the phase, or of the next phase.
    Row ra, rb;
    load_x(ra, 0);
    load_x(rb, 1);
    // layer-pipelined launch, layers above the first: has the layer below already published the NEXT frame?  Asked by one lane a
    // phase ahead (the answer travels through LDS, so the whole workgroup takes the same branch); if yes the frame's input is
    // fetched behind barrier #1 and the poll / fetch / barrier at the top of the next frame disappears
    int* const next_flag = reinterpret_cast<int*>(biasl + 3 * H + 16);
    bool have_x = false;

    for (int t = 0; t < T; ++t) {
        f32x4 am[TPW][3], al[TPW][3];
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                am[j][q] = bl[(q * H + (TPW * w + j) * 16) / 4 + g];
                al[j][q] = splat4(0.f);
            }
        if (PIPE && !FIRST && !have_x) {
            pipeline_wait(p.epi.ready_in, p.epi.pipe_error, group, t, lane);     // frame t of the layer below has landed
            seam_fetch(t);
            seam_commit();
            __syncthreads();
        }
        int ahead = 0;
        if (PIPE && !FIRST && tid == 0 && t + 1 < T)
            ahead = __hip_atomic_load(p.epi.ready_in + group, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // (lands under the MFMAs below)
        // One row against one 32-wide chunk of a B operand in LDS (op: its hi block, the lo block 64 x 16 B behind it): gates
        // 0..NQ-1 of every tile, three MFMAs per product, pinned behind the row's load.  X rows carry NQ = 3 gates, H rows 2.
        auto mma_gates = [&](auto nq_, const Row& r, const u32x4* op) {
            constexpr int NQ = decltype(nq_)::value;
            const u32x4 xh = op[lane], xl = op[64 + lane];
#pragma unroll
            for (int j = 0; j < TPW; ++j)
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    am[j][q] = mfma_f16(r.a[(j * NQ + q) * 2 + 0], xh, am[j][q]);
                    al[j][q] = mfma_f16(r.a[(j * NQ + q) * 2 + 1], xh, al[j][q]);
                    al[j][q] = mfma_f16(r.a[(j * NQ + q) * 2 + 0], xl, al[j][q]);
                }
            __builtin_amdgcn_sched_barrier(0);
        };
        // ... a candidate row: two chunks of r (.) h, gate 2 of every tile
        auto mma_cand = [&](const Row& r, int m2) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const u32x4 xh = rhb[((2 * m2 + k) * 2 + 0) * 64 + lane], xl = rhb[((2 * m2 + k) * 2 + 1) * 64 + lane];
#pragma unroll
                for (int j = 0; j < TPW; ++j) {
                    am[j][2] = mfma_f16(r.a[(k * TPW + j) * 2 + 0], xh, am[j][2]);
                    al[j][2] = mfma_f16(r.a[(k * TPW + j) * 2 + 1], xh, al[j][2]);
                    al[j][2] = mfma_f16(r.a[(k * TPW + j) * 2 + 0], xl, al[j][2]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        constexpr std::integral_constant<int, 3> kGatesX{};
        constexpr std::integral_constant<int, 2> kGatesH{};
        // ---- x-part of r, u, c ----
#pragma nounroll
        for (int c = 0; c < KX; c += 2) {                       // KX is even
            mma_gates(kGatesX, ra, xsb + c * 2 * 64);
            if (c + 2 < KX) load_x(ra, c + 2); else load_h(ra, 0);
            mma_gates(kGatesX, rb, xsb + (c + 1) * 2 * 64);
            if (c + 3 < KX) load_x(rb, c + 3); else load_h(rb, 1);
        }
        // ---- recurrent part of r and u ----
#pragma nounroll
        for (int m = 0; m < HC; m += 2) {                       // HC is even
            mma_gates(kGatesH, ra, hb + m * 2 * 64);
            if (m + 2 < HC) load_h(ra, m + 2);
            else {
                // ... the candidate's rows do not depend on the exchange below.  Pipelined producer: the seam rows of the frame
                // before must be written through before the counter moves behind barrier #1; draining HERE costs nothing -- all
                // that is still in flight is the row the next MFMAs wait for anyway -- whereas in front of the barrier it would
                // also wait for the two candidate rows requested now
                if (PIPE && !LAST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                load_c(ra, 0);
            }
            mma_gates(kGatesH, rb, hb + (m + 1) * 2 * 64);
            if (m + 3 < HC) load_h(rb, m + 3); else load_c(rb, 1);
        }
        // ---- r; r (.) h split -> LDS (the u sigmoid waits for the candidate phase: only the update needs it) ----
#pragma unroll
        for (int jj = 0; jj < CPW; ++jj) {
            f32x4 rh[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int j = 2 * jj + k;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pr = __builtin_fmaf(al[j][0][e], kLoInv, am[j][0][e]);
                    rh[k][e] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(pr)) * hreg[j][e];
                }
            }
            u32x4 hi, lo;
            split8_scaled(rh[0], rh[1], hi, lo);
            rhb[((CPW * w + jj) * 2 + 0) * 64 + lane] = hi;
            rhb[((CPW * w + jj) * 2 + 1) * 64 + lane] = lo;
        }
        if (PIPE && !FIRST && tid == 0) *next_flag = ahead > t + 1 ? 1 : 0;
        __syncthreads();              // #1: r (.) h visible; hb and xsb fully consumed
        if (PIPE && !LAST && t > 0 && tid == 0) pipeline_publish(p.epi.ready_out, group, t);      // frames 0..t-1 are out (every wave drained its stores above)
        // the next frame's input: xsb is free now
        if (FIRST) { mel_commit(); mel_fetch(t + 2); }
        else if (!PIPE) { seam_commit(); seam_fetch(t + 2); }
        else {
            have_x = *next_flag != 0;
            if (have_x) seam_fetch(t + 1);           // committed behind the candidate MFMAs
        }
        // ---- recurrent part of the candidate; the u sigmoid rides in the stream's shadow ----
        f32x4 u[TPW];
        // HC / 2 rows, an even count (HC = 4 or 8); the first pair peeled
        mma_cand(ra, 0);
        if (2 < HC / 2) load_c(ra, 2); else load_x(ra, 0);                    // ... the next frame's first x rows
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                u[j][e] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(__builtin_fmaf(al[j][1][e], kLoInv, am[j][1][e])));
        mma_cand(rb, 1);
        if (3 < HC / 2) load_c(rb, 3); else load_x(rb, 1);
#pragma nounroll
        for (int m2 = 2; m2 < HC / 2; m2 += 2) {
            mma_cand(ra, m2);
            if (m2 + 2 < HC / 2) load_c(ra, m2 + 2); else load_x(ra, 0);
            mma_cand(rb, m2 + 1);
            if (m2 + 3 < HC / 2) load_c(rb, m2 + 3); else load_x(rb, 1);
        }
        if (PIPE && !FIRST && have_x) seam_commit();
        // ---- tanh, update, split -> LDS, seam / projection ----
        const unsigned live = t < len_s ? 0xffffffffu : 0u;
        f32x4 fm = splat4(0.f), fl = splat4(0.f);
        if (LAST && w == 0) fm = bl[(3 * H) / 4 + g];
#pragma unroll
        for (int jj = 0; jj < CPW; ++jj) {
            f32x4 hout[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int j = 2 * jj + k;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pc = __builtin_fmaf(al[j][2][e], kLoInv, am[j][2][e]);
                    const float c = __builtin_fmaf(__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(pc)), -2.0f, 1.0f);      // tanh
                    const float hn = __builtin_fmaf(u[j][e], hreg[j][e] - c, c);                                                 // c + u (h - c)
                    hreg[j][e] = bitsel(live, hn, hreg[j][e]);
                    hout[k][e] = bitsel(live, hn, 0.f);
                }
            }
            u32x4 hi, lo;
            split8_scaled(hreg[2 * jj], hreg[2 * jj + 1], hi, lo);
            hb[((CPW * w + jj) * 2 + 0) * 64 + lane] = hi;
            hb[((CPW * w + jj) * 2 + 1) * 64 + lane] = lo;
            // the layer's OUTPUT row is zero past seq_len (dynamic_rnn), its state is copied through
            u32x4 ohi = hi, olo = lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) { ohi[e] &= live; olo[e] &= live; }
            if (!LAST) {
                const int frag = (t * HC + CPW * w + jj) * 2;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, ohi), ho_rsrc, lane16, (frag + 0) * 1024, PIPE ? kSysScope : 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, olo), ho_rsrc, lane16, (frag + 1) * 1024, PIPE ? kSysScope : 0);
            } else {
                fm = mfma_f16(wfc[jj][0], ohi, fm);
                fl = mfma_f16(wfc[jj][1], ohi, fl);
                fl = mfma_f16(wfc[jj][0], olo, fl);
            }
        }
        if (LAST) {
            const f32x4 accf = fm + fl * kLoInv;
            if (g < 2) *reinterpret_cast<f32x4*>(epi.pstage + (w * 16 + s) * 8 + 4 * g) = accf;
        }
        __syncthreads();              // #2: h(t), x(t+1), the partial logits visible
        if (LAST) {
            if (w == (t & 3)) epilogue_fold(epi, t, lane);
            if (((t + 1) & (kRingFrames - 1)) == 0 || t == T - 1) {
                const int t0 = t & ~(kRingFrames - 1);
                __syncthreads();
                epilogue_flush(p.epi, epi, group, t0, t - t0 + 1, w, lane, t == T - 1);
            }
        }
    }
    if (PIPE && !LAST) pipeline_close(p.epi.ready_out, group, T, tid);
    if (bvalid) {
#pragma unroll
        for (int j = 0; j < TPW; ++j)
            *reinterpret_cast<f32x4*>(p.state_out + (size_t)b * H + (TPW * w + j) * 16 + 4 * g) = hreg[j];
    }
}

template <int TPW, bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) gru_layer_f16x3_generic(const GruF16Params p) {
    gru_f16x3_generic_body<TPW, FIRST, LAST, false>(p, blockIdx.x);
}

// Layer-pipelined launch: ONE grid of L x G workgroups, XCD-affine as gru_stack_generic_pipelined (block i -> XCD i % 8 serves
// layer (i % 8) % L: the workgroups behind one L2 all stream the same layer's 1.5 MiB).
template <int TPW>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) gru_stack_f16x3_pipelined(const GruF16StackParams sp) {
    int layer, group;
    if (!pipelined_block(sp.L, sp.G, sp.xcd_affine, layer, group)) return;
    if (layer == 0) gru_f16x3_generic_body<TPW, true, false, true>(sp.layer[0], group);
    else if (layer == sp.L - 1) gru_f16x3_generic_body<TPW, false, true, true>(sp.layer[layer], group);
    else gru_f16x3_generic_body<TPW, false, false, true>(sp.layer[layer], group);
}

bool gru_f16x3_generic_supported(int hidden, int n_mel) { return (hidden == 128 || hidden == 256) && n_mel % 4 == 0 && n_mel >= 4 && n_mel <= 64; }

hipError_t launch_gru_layer_f16x3_generic(const GruF16Params& p, int hidden, bool first, bool last, hipStream_t st) {
    if (p.T <= 0 || p.B <= 0) return hipSuccess;
    // one workgroup per CU (each wants the whole register file)
    const size_t lds = one_workgroup_per_cu(gru_f16x3_generic_lds_bytes(hidden, last));
    return with_layer_shape<2, 4>(hidden, first, last, [&](auto tpw, auto fi, auto la) {
        return launch_lds<gru_layer_f16x3_generic<tpw(), fi(), la()>>(dim3(groups_of(p.B)), dim3(256), lds, st, p);
    });
}

hipError_t launch_gru_stack_f16x3_pipelined(const GruF16StackParams& sp, int hidden, hipStream_t st) {
    const size_t lds = one_workgroup_per_cu(gru_f16x3_generic_lds_bytes(hidden, true));
    const dim3 grid(pipelined_grid(sp.L, sp.G, sp.xcd_affine));
    return with_tpw<2, 4>(hidden, [&](auto tpw) {
        return launch_lds<gru_stack_f16x3_pipelined<tpw()>>(grid, dim3(256), lds, st, sp);
    });
}

}  // namespace kws
