// Streaming GRU layer kernels for gfx950 (MI355X).
//
// Replaces, per launch, one layer of the TF while_loop the reference builds at
// models/rnn_ctc.py:228-243 (GRUCell x L under MultiRNNCell + dynamic_rnn) and, in the last layer's
// epilogue, models/rnn_ctc.py:247-284 (inference2: dense), :165 (softmax) and
// utils/prediction.py:65-86 (ctc_decode2's per-frame rule).
//
// Mapping (see DESIGN.md "Kernels"):
//   * one workgroup = 4 waves = 16 streams; the MFMA is v_mfma_f32_16x16x4_f32 with
//     M = 16 output units, N = 16 streams, K = 4 input rows.  Orientation D[unit][stream]:
//     A = weights (lane (g,i): W[k(g)][unit i]), B = activations (lane (g,s): act[s][k(g)]).
//   * wave w owns units [32w, 32w+32) (two 16-unit tiles) of r, u, c and h'.
//   * the K index is permuted so that the C/D register image of a tile IS the B operand of four
//     k-chunks (kws_internal.h "xl" layout): h' feeds the next step with no transpose, only an
//     8 KiB LDS exchange so that every wave sees all 128 units.
//   * the resident kernel (hidden 128: weights in registers and LDS) is a translation unit of its own,
//     gru_resident.hip; this file holds the generic and the layer-pipelined kernels.
#include <cstddef>

#include "gru_device.h"
#include "launch.h"
#include "pipeline_device.h"
#include "window_device.h"

namespace kws {

// ------------------------------------------------------------------------------------------------
// Generic kernel: H = 64*TPW, weights streamed from L2 every frame (group-of-4 fragment layout).
// Same orientation, exchange layout and epilogue; no software pipeline.
//
// WRAP (the wrapped instantiations only; every other one compiles exactly as without it): the cell wrappers of GruWrapLayer.
//   * layer norm: at the top of each frame the layer's input block is staged in LDS, its mean and then the variance around it
//     are reduced per stream (lane (g, s) holds features 16 k4 + 4g + e of stream s: the four lanes s, s+16, s+32, s+48 span
//     the vector), and each wave writes its share of the normalised operand (x - mu) * rsqrt(var + 1e-5) * ibeta + igamma
//     next to it; the existing x-part MFMAs read that.  Padding features (k >= I) stay out of the statistics and feed 0.
//   * residual: the seam keeps the xl layout, so output tile n of this layer is the register image of the input k-group n of
//     the same frame: 0.7071 (h' + x) is lane-local.  It goes to the seam / the dense layer; hreg, hbuf and state_out keep h'.
// ------------------------------------------------------------------------------------------------
constexpr float kResidualScale = 0.7071067811865475f;     // utils/custom_wrapper.py:116
constexpr float kLayerNormEps = 1e-5f;                    // utils/custom_wrapper.py:126

namespace {
// One "row" of the weight stream = the fragments of all TPW tiles of a wave for one k-group (half rows, two tiles at TPW = 4, were
// measured 10-15 % slower)
template <int TPW> struct RowX { f32x4 a[TPW][3]; f32x4 xb; };      // x-part of r, u, c and the frame's input block
template <int TPW> struct RowH { f32x4 a[TPW][2]; };                // h-part of r, u
template <int TPW> struct RowC { f32x4 a[TPW]; };                   // h-part of c
}  // namespace

template <int TPW, bool FIRST, bool LAST, bool PIPE, bool WRAP = false>
__device__ __forceinline__ void gru_layer_generic_body(const GruLayerParams& p, const int group,
                                                       const GruWrapLayer& wl = GruWrapLayer{nullptr, 0.f, 0}) {
    constexpr int NT = 4 * TPW, H = 64 * TPW;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int b_raw = group * kStreamsPerGroup + s;
    const bool bvalid = b_raw < p.B;
    const int b = bvalid ? b_raw : p.B - 1;
    const int T = p.T, I = p.I;
    const int KCX4 = p.KCX / 4;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* hbuf = reinterpret_cast<f32x4*>(smem);
    f32x4* rhbuf = hbuf + NT * 64;
    f32x4* xstage = rhbuf + NT * 64;                                                     // pipelined launch only
    f32x4* biasl = xstage + NT * 64;                                                      // [3][NT][4 g] bias fragments
    const EpilogueLds epi = epilogue_carve(reinterpret_cast<char*>(biasl + 3 * NT * 4));  // LAST only
    // WRAP: [KCX/4][64] float4, the normalised frame (first layer: staged and normalised in place); the raw input of an upper
    // layer is staged in xstage.  Behind the epilogue area whether or not this layer is the last (gru_wrapped_extra_lds).
    f32x4* const xln = WRAP ? reinterpret_cast<f32x4*>(reinterpret_cast<char*>(biasl + 3 * NT * 4) + kEpilogueLdsBytes) : nullptr;
    const bool w_ln = WRAP && wl.igamma != nullptr;
    const bool w_res = WRAP && !FIRST && wl.residual != 0;
    const bool w_staged = w_ln || w_res;                  // the x operand comes from LDS

    // The weight stream (and the seam of a layer-by-layer launch) goes through BUFFER loads: lane offset in one VGPR that
    // never changes, everything else in the scalar offset.  With flat global loads every fragment fetched per frame cost
    // two or three VALU instructions of 64-bit address arithmetic -- about one per MFMA, beside an f32 MFMA stream that
    // shares the FP32 pipe with them (profiles/r2_configC_pmc.json: 2.0 VALU instructions per MFMA).
    const __amdgpu_buffer_rsrc_t wx_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wx), (short)0, 0x7fffffff, 0x00020000);   // [NT][3][KCX4][64] float4
    const __amdgpu_buffer_rsrc_t wh_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.wh), (short)0, 0x7fffffff, 0x00020000);   // [NT][3][NT][64] float4
    const int lane16 = lane * 16;
    auto bload = [&](const __amdgpu_buffer_rsrc_t& r, int frag) -> f32x4 {      // frag: wave-uniform fragment index (1 KiB each)
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, lane16, frag * 1024, 0));
    };

    // biases live in LDS (the accumulators are re-initialised from there every frame): at TPW = 4 the 48 registers
    // they would pin are the difference between fitting the 512-register file and spilling
    f32x4 hreg[TPW];
    const bool do_reset = p.reset != nullptr && p.reset[b] != 0;
    const int len_s = p.seq_len ? p.seq_len[b] - p.t_base : T;
    for (int i = tid; i < 3 * NT * 4; i += 256) biasl[i] = ld4(p.bias + 4 * i);   // [gate][tile][g] = bias[gate*H + 16*tile + 4g ..]
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int n = TPW * w + j;
        hreg[j] = do_reset ? splat4(0.f) : ld4(p.state_in + (size_t)b * H + n * 16 + 4 * g);
        hbuf[n * 64 + lane] = hreg[j];
    }
    f32x4 bfc4 = splat4(0.f);
    if (LAST) {
        if (w == 0) bfc4 = ld4(p.bfc + 4 * g);
        epilogue_carry_init(epi, p.prev_word, p.reset, group, p.B, tid);
    }
    const float* xrow = FIRST ? p.x_mel + (size_t)b * (p.t_stride ? p.t_stride : T) * I : nullptr;
    const __amdgpu_buffer_rsrc_t xp_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        FIRST ? const_cast<float*>(p.wh) : const_cast<float*>(reinterpret_cast<const float*>(p.x_prev + (size_t)group * T * NT * 64)),
        (short)0, 0x7fffffff, 0x00020000);       // this group's [T][NT][64] float4 block of the seam
    const __amdgpu_buffer_rsrc_t ho_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        LAST ? const_cast<float*>(p.wh) : reinterpret_cast<float*>(p.h_out + (size_t)group * T * NT * 64), (short)0, 0x7fffffff, 0x00020000);
    const bool vec_ok = (I & 3) == 0;
    __syncthreads();

    auto mel_operand = [&](int t, int k4) -> f32x4 {     // the first layer's x operand (zero past I)
        f32x4 xb;
        const int k = 16 * k4 + 4 * g;
        const float* src = xrow + (size_t)t * I + k;
        if (vec_ok && k + 3 < I) {
            xb = ld4(src);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) xb[e] = (k + e < I) ? src[e] : 0.f;
        }
        return xb;
    };
    auto x_operand = [&](int t, int k4) -> f32x4 {
        if (WRAP && w_staged) return (w_ln ? xln : xstage)[k4 * 64 + lane];     // WRAP: staged at the top of the frame (wrap_frame)
        if (FIRST) return mel_operand(t, k4);
        if (PIPE) return xstage[k4 * 64 + lane];       // staged at the top of the frame (below)
        return bload(xp_rsrc, t * NT + k4);
    };
    // Weight fragments stream from L2 every frame, row by row (RowX / RowH / RowC above); rows ping-pong between two register
    // sets, the next row's loads pinned ahead of the current row's MFMAs (12 TPW MFMAs = 1.5k cycles at TPW = 4, more than an
    // L2 round trip).  Left to hipcc, every tile's three loads were waited for right before their MFMAs and the kernel ran
    // latency-bound at half the MFMA rate.
    // The streaming loops must stay rolled (#pragma nounroll): unrolled, hipcc materialises a 64-bit address pair per load and
    // the TPW = 4 kernels spill.  A load past a phase's last row fetches that last row again.
    auto load_x = [&](RowX<TPW>& r, int t, int q) {
        const int kk = q < KCX4 ? q : KCX4 - 1;
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) r.a[j][c] = bload(wx_rsrc, ((TPW * w + j) * 3 + c) * KCX4 + kk);
        r.xb = x_operand(t, kk);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto load_h = [&](RowH<TPW>& r, int q) {
        const int kk = q < NT ? q : NT - 1;
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int c = 0; c < 2; ++c) r.a[j][c] = bload(wh_rsrc, ((TPW * w + j) * 3 + c) * NT + kk);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto load_c = [&](RowC<TPW>& r, int q) {
        const int kk = q < NT ? q : NT - 1;
#pragma unroll
        for (int j = 0; j < TPW; ++j) r.a[j] = bload(wh_rsrc, ((TPW * w + j) * 3 + 2) * NT + kk);
        __builtin_amdgcn_sched_barrier(0);
    };
    // WRAP: frame t's input block to LDS and, under layer norm, the normalised operand beside it (see the header above)
    auto wrap_frame = [&](int t) {
        f32x4* const raw = FIRST ? xln : xstage;
        if (FIRST) {
            // wave w stages k-groups w, w + 4, ...: up to four loads in flight ahead of their LDS stores
            for (int k0 = w; k0 < KCX4; k0 += 16) {
                f32x4 v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) if (k0 + 4 * i < KCX4) v[i] = mel_operand(t, k0 + 4 * i);
#pragma unroll
                for (int i = 0; i < 4; ++i) if (k0 + 4 * i < KCX4) raw[(k0 + 4 * i) * 64 + lane] = v[i];
            }
            __syncthreads();
        } else if (!PIPE) {                              // the layer-pipelined launch staged it above
            f32x4 v[NT / 4];
#pragma unroll
            for (int i = 0; i < NT / 4; ++i) v[i] = bload(xp_rsrc, t * NT + w + 4 * i);
#pragma unroll
            for (int i = 0; i < NT / 4; ++i) raw[(w + 4 * i) * 64 + lane] = v[i];
            __syncthreads();
        }
        if (!w_ln) return;
        // tf.nn.moments: the mean, then the population variance around it (not E[x^2] - mu^2: mel magnitudes carry a large DC
        // part) -- per lane over its features, then over the stream's four lanes.  Every wave reduces the whole block in the
        // same order, and the xor exchanges add the same two values on both lanes: every lane of a stream has the same bits.
        float sum = 0.f;
        for (int k4 = 0; k4 < KCX4; ++k4) {
            const f32x4 v = raw[k4 * 64 + lane];
            sum += (v[0] + v[1]) + (v[2] + v[3]);
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float mu = sum / (float)I;
        float sq = 0.f;
        for (int k4 = 0; k4 < KCX4; ++k4) {
            const f32x4 v = raw[k4 * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float d = v[e] - mu;
                if (FIRST) d = (16 * k4 + 4 * g + e < I) ? d : 0.f;       // padding features
                sq = fmaf(d, d, sq);
            }
        }
        sq += __shfl_xor(sq, 16);
        sq += __shfl_xor(sq, 32);
        const float scale = wl.ibeta * rsqrtf(sq / (float)I + kLayerNormEps);
        if (FIRST) __syncthreads();                      // normalised in place: every wave is done reading the raw block
        for (int k0 = w; k0 < KCX4; k0 += 16) {
            f32x4 gm[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) if (k0 + 4 * i < KCX4) gm[i] = ld4(wl.igamma + 16 * (k0 + 4 * i) + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k4 = k0 + 4 * i;
                if (k4 < KCX4) {
                    const f32x4 v = raw[k4 * 64 + lane];
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        o[e] = fmaf(v[e] - mu, scale, gm[i][e]);
                        if (FIRST) o[e] = (16 * k4 + 4 * g + e < I) ? o[e] : 0.f;   // padding feeds exactly 0
                    }
                    xln[k4 * 64 + lane] = o;
                }
            }
        }
        __syncthreads();
    };
    for (int t = 0; t < T; ++t) {
        f32x4 acc_r[TPW], acc_u[TPW], acc_c[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int n = TPW * w + j;
            acc_r[j] = biasl[(0 * NT + n) * 4 + g]; acc_u[j] = biasl[(1 * NT + n) * 4 + g]; acc_c[j] = biasl[(2 * NT + n) * 4 + g];
        }
        // a row's MFMAs.  Lambdas in the frame loop, the scheduling barrier behind each call: as function templates over the
        // accumulator arrays the hidden-256 kernels were allocated 44 more VGPRs and 32 more AGPRs (profiles/gru_shared_phases_isa.txt)
        auto mma_x = [&](const RowX<TPW>& r) {
#pragma unroll
            for (int j = 0; j < TPW; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc_r[j] = mfma4(r.a[j][0][e], r.xb[e], acc_r[j]);
                    acc_u[j] = mfma4(r.a[j][1][e], r.xb[e], acc_u[j]);
                    acc_c[j] = mfma4(r.a[j][2][e], r.xb[e], acc_c[j]);
                }
        };
        auto mma_h = [&](const RowH<TPW>& r, const f32x4 hb) {
#pragma unroll
            for (int j = 0; j < TPW; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc_r[j] = mfma4(r.a[j][0][e], hb[e], acc_r[j]);
                    acc_u[j] = mfma4(r.a[j][1][e], hb[e], acc_u[j]);
                }
        };
        auto mma_c = [&](const RowC<TPW>& r, const f32x4 rb) {
#pragma unroll
            for (int j = 0; j < TPW; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc_c[j] = mfma4(r.a[j][e], rb[e], acc_c[j]);
        };
        if (PIPE && !FIRST) {
            pipeline_wait(p.ready_in, p.pipe_error, group, t, lane);       // frame t of the layer below has landed
            // The frame's input block was written by a workgroup on another CU / XCD while this kernel runs:
            // system-scope (sc0 sc1) loads go past the non-coherent cache levels, dword by dword, at memory
            // latency -- so the whole block is fetched at once (all loads in flight) and parked in LDS.
            // (16-byte sc0 sc1 buffer loads: dword-granular system-scope accesses cost ~6x the fabric time per byte;
            // tearing is no concern, the rows are ordered by the frame counter)
            f32x4 xv[NT / 4];
#pragma unroll
            for (int i = 0; i < NT / 4; ++i)
                xv[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xp_rsrc, lane16, (t * NT + (w + 4 * i)) * 1024, kSysScope));
#pragma unroll
            for (int i = 0; i < NT / 4; ++i) xstage[(w + 4 * i) * 64 + lane] = xv[i];
            __syncthreads();
        }
        if constexpr (WRAP) {
            if (w_staged) wrap_frame(t);
        }
        // x-part (gates and candidate): one row per k-group, ping-pong, unrolled by two
        {
            RowX<TPW> ra, rb;
            load_x(ra, t, 0);
#pragma nounroll
            for (int q = 0; q < KCX4; q += 2) {
                load_x(rb, t, q + 1);
                mma_x(ra); __builtin_amdgcn_sched_barrier(0);
                if (q + 1 < KCX4) {
                    load_x(ra, t, q + 2);
                    mma_x(rb); __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // gates, h-part (NT rows: an even count)
        {
            RowH<TPW> ra, rb;
            load_h(ra, 0);
#pragma nounroll
            for (int q = 0; q < NT; q += 2) {
                load_h(rb, q + 1);
                mma_h(ra, hbuf[q * 64 + lane]); __builtin_amdgcn_sched_barrier(0);
                load_h(ra, q + 2);
                mma_h(rb, hbuf[(q + 1) * 64 + lane]); __builtin_amdgcn_sched_barrier(0);
            }
        }
        f32x4 u[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            f32x4 rh;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                rh[e] = sigmoid_f(acc_r[j][e]) * hreg[j][e];
                u[j][e] = sigmoid_f(acc_u[j][e]);
            }
            rhbuf[(TPW * w + j) * 64 + lane] = rh;
        }
        RowC<TPW> ca, cb;
        if (PIPE && !LAST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // last frame's rows (half a frame old): written through
        load_c(ca, 0);                 // does not depend on the exchange: issued ahead of the barrier
        __syncthreads();
        if (PIPE && !LAST && t > 0 && tid == 0) pipeline_publish(p.ready_out, group, t);      // frames 0..t-1: drained above
#pragma nounroll
        for (int q = 0; q < NT; q += 2) {
            load_c(cb, q + 1);
            mma_c(ca, rhbuf[q * 64 + lane]); __builtin_amdgcn_sched_barrier(0);
            load_c(ca, q + 2);
            mma_c(cb, rhbuf[(q + 1) * 64 + lane]); __builtin_amdgcn_sched_barrier(0);
        }
        const unsigned live = t < len_s ? 0xffffffffu : 0u;
        f32x4 accf = bfc4;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int n = TPW * w + j;
            f32x4 hout;
            f32x4 xr = splat4(0.f), seam = splat4(0.f);     // WRAP: this tile's input (raw, frame t) and the layer's output
            if (WRAP && w_res) xr = xstage[n * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float c = tanh_f(acc_c[j][e]);
                // explicit fma: which of the two products -ffp-contract fuses must not depend on the instantiation
                // (sequential and pipelined launches have to agree bit for bit)
                const float hn = fmaf(u[j][e], hreg[j][e], (1.0f - u[j][e]) * c);
                hreg[j][e] = bitsel(live, hn, hreg[j][e]);
                hout[e] = bitsel(live, hn, 0.f);
                if (WRAP) {
                    const float o = w_res ? kResidualScale * (hn + xr[e]) : hn;     // utils/custom_wrapper.py:116
                    hout[e] = bitsel(live, o, 0.f);
                    seam[e] = bitsel(live, o, hreg[j][e]);
                }
            }
            hbuf[n * 64 + lane] = hreg[j];
            if (!LAST) {
                const f32x4 o = WRAP ? seam : hreg[j];
                float4* dst = p.h_out + ((size_t)group * T + t) * NT * 64 + n * 64 + lane;
                if (PIPE) {
                    typedef int i32x4 __attribute__((ext_vector_type(4)));
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, o), ho_rsrc, lane16, (t * NT + n) * 1024, kSysScope);
                } else {
                    *dst = make_float4(o[0], o[1], o[2], o[3]);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) accf = mfma4(p.wfc[(n * 4 + e) * 64 + lane], hout[e], accf);
            }
        }
        if (LAST && g < 2) *reinterpret_cast<f32x4*>(epi.pstage + (w * 16 + s) * 8 + 4 * g) = accf;
        __syncthreads();
        // Pipelined producer: the counter of frame t moves at the NEXT frame's mid barrier (below), after every wave has
        // drained its stores there -- __syncthreads() itself does not wait for global stores (workgroup scope), and a
        // consumer on another CU must not see the counter before the rows (found by tools/stress_determinism.py: only
        // the first call after create showed it, later calls re-read the identical rows of the previous call).
        if (LAST) {
            if (w == (t & 3)) epilogue_fold(epi, t, lane);
            if (((t + 1) & (kRingFrames - 1)) == 0 || t == T - 1) {
                const int t0 = t & ~(kRingFrames - 1);
                __syncthreads();
                epilogue_flush(p, epi, group, t0, t - t0 + 1, w, lane, t == T - 1);
            }
        }
    }
    if (PIPE && !LAST) pipeline_close(p.ready_out, group, T, tid);
    if (bvalid) {
#pragma unroll
        for (int j = 0; j < TPW; ++j)
            *reinterpret_cast<f32x4*>(p.state_out + (size_t)b * H + (TPW * w + j) * 16 + 4 * g) = hreg[j];
    }
}

template <int TPW, bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) gru_layer_generic(const GruLayerParams p) {
    gru_layer_generic_body<TPW, FIRST, LAST, false>(p, blockIdx.x);
}

// Layer-pipelined launch: ONE grid of L x G workgroups, layer-major, so that every layer of every 16-stream group
// runs concurrently on its own CU and layer l consumes frame t of layer l-1 as soon as it is published (a per-group
// frame counter in global memory: release after the h_out stores, acquire before the x loads).  Wall time becomes
// (T + L - 1) frame times instead of L x T.  It pays when L x G workgroups fit the chip at once -- BASELINE
// configs[4] (L = 4, B = 1024: 256 workgroups on 256 CUs) -- and cannot deadlock in any case: a workgroup only
// waits for one with a smaller index, and workgroups are dispatched in index order.
//
// XCD affinity: workgroups are dealt round-robin to the 8 XCDs (block i -> XCD i % 8), each with its own 4 MB L2.
// Layer-major order would put every layer's weight stream (1.5 MB per layer at H = 256, 6 MB in all) through every
// L2; with L dividing 8 the mapping below gives XCD x the layer x % L only (measured at configs[4]: 9.32 vs 9.53 ms),
// and a workgroup still waits only for block i - 1.
template <int TPW>
__global__ void __launch_bounds__(256) gru_stack_generic_pipelined(const GruStackParams sp) {
    int layer, group;
    if (!pipelined_block(sp.L, sp.G, sp.xcd_affine, layer, group)) return;
    if (layer == 0) gru_layer_generic_body<TPW, true, false, true>(sp.layer[0], group);
    else if (layer == sp.L - 1) gru_layer_generic_body<TPW, false, true, true>(sp.layer[layer], group);
    else gru_layer_generic_body<TPW, false, false, true>(sp.layer[layer], group);
}

// The wrapped instantiations (GruWrapLayer): the same launches with the cell wrappers of a second kernel argument.
template <int TPW, bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) gru_layer_generic_wrapped(const GruLayerParams p, const GruWrapLayer wl) {
    gru_layer_generic_body<TPW, FIRST, LAST, false, true>(p, blockIdx.x, wl);
}
template <int TPW>
__global__ void __launch_bounds__(256) gru_stack_generic_pipelined_wrapped(const GruStackParams sp, const GruWrapParams wp) {
    int layer, group;
    if (!pipelined_block(sp.L, sp.G, sp.xcd_affine, layer, group)) return;
    if (layer == 0) gru_layer_generic_body<TPW, true, false, true, true>(sp.layer[0], group, wp.layer[0]);
    else if (layer == sp.L - 1) gru_layer_generic_body<TPW, false, true, true, true>(sp.layer[layer], group, wp.layer[layer]);
    else gru_layer_generic_body<TPW, false, false, true, true>(sp.layer[layer], group, wp.layer[layer]);
}
static_assert(sizeof(GruStackParams) + sizeof(GruWrapParams) <= 4096, "kernel arguments");

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static size_t generic_lds_bytes(int hidden, bool last) {
    size_t n = (size_t)3 * (hidden / 16) * 64 * 16 + (size_t)3 * hidden * 4;
    if (last) n += kEpilogueLdsBytes;
    return n;
}

hipError_t launch_gru_stack_generic_pipelined(const GruStackParams& sp, int hidden, hipStream_t st) {
    const size_t lds = one_workgroup_per_cu(generic_lds_bytes(hidden, true));
    const dim3 grid(pipelined_grid(sp.L, sp.G, sp.xcd_affine));
    return with_tpw<1, 2, 4>(hidden, [&](auto tpw) {
        return launch_lds<gru_stack_generic_pipelined<tpw()>>(grid, dim3(256), lds, st, sp);
    });
}

hipError_t launch_gru_layer_generic(const GruLayerParams& p, int hidden, bool first, bool last,
                                    hipStream_t st) {
    size_t lds = generic_lds_bytes(hidden, last);
    // a time block of an overlapped call (t_stride set): another layer's kernel runs beside this one on another stream;
    // keep one workgroup per CU or the dispatcher stacks both kernels onto the same CUs (measured: 2.2x slower each;
    // within ONE launch it spreads workgroups by itself, and padding then only costs occupancy when groups > CUs)
    if (p.t_stride != 0) lds = one_workgroup_per_cu(lds);
    return with_layer_shape<1, 2, 4>(hidden, first, last, [&](auto tpw, auto fi, auto la) {
        return launch_lds<gru_layer_generic<tpw(), fi(), la()>>(dim3(groups_of(p.B)), dim3(256), lds, st, p);
    });
}

hipError_t launch_gru_layer_generic_wrapped(const GruLayerParams& p, const GruWrapLayer& wl, int hidden, bool first, bool last,
                                            hipStream_t st) {
    // the epilogue area is carved whether or not the layer is the last: the normalised frame lies behind it
    size_t lds = generic_lds_bytes(hidden, true) + gru_wrapped_extra_lds(p.KCX / 4);
    if (p.t_stride != 0) lds = one_workgroup_per_cu(lds);     // as launch_gru_layer_generic
    return with_layer_shape<1, 2, 4>(hidden, first, last, [&](auto tpw, auto fi, auto la) {
        return launch_lds<gru_layer_generic_wrapped<tpw(), fi(), la()>>(dim3(groups_of(p.B)), dim3(256), lds, st, p, wl);
    });
}

hipError_t launch_gru_stack_generic_pipelined_wrapped(const GruStackParams& sp, const GruWrapParams& wp, int hidden, hipStream_t st) {
    int kx4 = 0;
    for (int l = 0; l < sp.L; ++l) kx4 = sp.layer[l].KCX / 4 > kx4 ? sp.layer[l].KCX / 4 : kx4;
    const size_t lds = one_workgroup_per_cu(generic_lds_bytes(hidden, true) + gru_wrapped_extra_lds(kx4));     // as the plain launch
    const dim3 grid(pipelined_grid(sp.L, sp.G, sp.xcd_affine));
    return with_tpw<1, 2, 4>(hidden, [&](auto tpw) {
        return launch_lds<gru_stack_generic_pipelined_wrapped<tpw()>>(grid, dim3(256), lds, st, sp, wp);
    });
}

}  // namespace kws
