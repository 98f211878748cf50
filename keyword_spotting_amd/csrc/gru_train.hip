// Training of the GRU stack (models/rnn_ctc.py:34-101,179-284): the two frame loops, one launch per layer each.
//
//   gru_train_forward<TPW, STATE>   the taped forward of one layer: TF 1.x GRUCell under dynamic_rnn(sequence_length) and
//                             DropoutWrapper(output_keep_prob) -- a mask per frame, or variational_recurrent's one mask per stream
//                             (the mask's strides are launch arguments) --, from the zero state (STATE: from state_in)
//                               [r,u] = sigma(xg_ru + h.Wg_h)    c = tanh(xg_c + (r o h).Wc_h)    h' = u o h + (1 - u) o c
//                               y = h' o mask / keep_prob   (what goes up; the carried state is the undropped h')
//                             at t >= seq_len[b] the state is copied and y = 0.  It keeps r, u, c, h (the state the frame started
//                             from) and r o h of every frame t < seq_len -- the gates and the candidate as their pre-activations.
//   gru_train_backward<TPW, STATE>  back-propagation through time of one layer, frames in reverse.  With dh' = dy o mask / keep_prob + the
//                             carried dh:
//                               du = dh' o (h - c)    dc = dh' o (1 - u)    dh = dh' o u
//                               dc^ = dc o (1 - c^2)  du^ = du o u (1 - u)
//                               d(rh) = dc^ . Wc_h^T  dh += d(rh) o r       dr^ = d(rh) o h o r (1 - r)
//                               dh += [dr^ | du^] . Wg_h^T
//                             It writes dr^ | du^ | dc^ [B*T, 3H]; frames t >= seq_len[b] pass dh through and write zeros.
//   STATE = true              the same two loops from a carried state (kws_train_grad_state): h starts from state_in and ends in
//                             state_out, dh starts from dstate_out and ends in dstate_in; the loads and stores sit outside the frame
//                             loops, and the STATE = false instantiations are the machine code they were without the parameter.
//
// What is NOT in the frame loops: every product with the layer's input.  x . (Wg_x | Wc_x) + bias of all frames is one GEMM in front of
// the forward loop (xg), the dx of all frames one GEMM behind the backward loop, and the weight gradients one reduction over the B*T
// rows (train_kernels.hip): none of them is on a frame's dependent chain, and as whole-batch GEMMs they fill the chip where a
// frame loop has one workgroup per 16 streams.
//
// Mapping, as the serving kernels (gru_kernels.hip): one workgroup = 4 waves = 16 streams, v_mfma_f32_16x16x4_f32 with D[unit][stream],
// wave w owns units [16 TPW w, 16 TPW (w + 1)), activation blocks cross the waves through LDS in the "xl" layout (kws_internal.h): the
// register image of an output tile is the B operand of four k-chunks, lane (g, s) component e <-> unit 16 n + 4 g + e.  The weights
// are plain row-major copies (wh [H, 3H], wht [3H, H]) that stream from L2 every frame, 16 consecutive floats per lane group.
// The activations are expf / tanhf and true divisions, not the serving kernels' v_exp / v_rcp forms: a gradient is compared with a
// float32 reference at a few ulps, and the 3e-7 of the fast forms is several times that.  The tape keeps the PRE-activations: the
// backward loop recomputes r, u, c from them (the forward's bits) together with 1 - u, u (1 - u), r (1 - r) and 1 - c^2 in forms
// that do not cancel (sigmoid_parts, tanh_slope).
#include "gru_device.h"
#include <type_traits>
#include "launch.h"

namespace kws {

namespace {

// sigma(a) with its complement and its derivative, none of them through a cancellation: with e = exp(-|a|) and s = 1 / (1 + e) the
// larger of sigma and 1 - sigma is s, the smaller e s, and sigma (1 - sigma) = e s^2.  (1 - sigma formed from the rounded sigma has
// a relative error of 2^-24 / (1 - sigma): the gate bias starts at 1 and u sits near 1 for much of a sequence.)
struct SigmoidParts { float v, comp, dv; };
__device__ __forceinline__ SigmoidParts sigmoid_parts(float a) {
    const float e = expf(-fabsf(a)), s = 1.0f / (1.0f + e), es = e * s;
    SigmoidParts o;
    o.v = a >= 0.f ? s : es;
    o.comp = a >= 0.f ? es : s;
    o.dv = es * s;
    return o;
}
// 1 - tanh(a)^2 = 4 e / (1 + e)^2 with e = exp(-2 |a|), likewise
__device__ __forceinline__ float tanh_slope(float a) {
    const float e = expf(-2.0f * fabsf(a)), s = 1.0f / (1.0f + e);
    return 4.0f * e * s * s;
}
__device__ __forceinline__ int clamp_len(int v, int T) { return v < 0 ? 0 : (v > T ? T : v); }
// the longest sequence of the group's streams: frames past it are dead for the whole workgroup
__device__ __forceinline__ int group_frames(const int32_t* seq_len, int group, int B, int T) {
    int tmax = 0;
    for (int i = 0; i < kStreamsPerGroup; ++i) {
        const int bb = group * kStreamsPerGroup + i;
        if (bb < B) { const int v = clamp_len(seq_len[bb], T); tmax = v > tmax ? v : tmax; }
    }
    return tmax;
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// where the dropout mask of (stream b, frame t) begins: one mask per frame, or one per stream held for all frames (kws_internal.h)
template <int H, typename Params>
__device__ __forceinline__ size_t mask_row(const Params& p, int b, int t) { return ((size_t)b * p.drop_bs + (size_t)t * p.drop_ts) * H; }
// v o mask / keep_prob on four consecutive units (the offset is a multiple of 4): a true division, as TensorFlow's x / keep_prob * mask --
// a rounded reciprocal would scale every output of the layer by the same relative error, which does not average out
__device__ __forceinline__ f32x4 dropped(f32x4 v, const uint8_t* drop, size_t at, float keep_prob) {
    const uint32_t m = *reinterpret_cast<const uint32_t*>(drop + at);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ((m >> (8 * e)) & 0xffu) ? v[e] / keep_prob : 0.f;
    return v;
}

}  // namespace

// STATE: the layer starts from state_in[b] and leaves the state after frame seq_len[b] - 1 in
// state_out[b] (TrainStateIo, kws_internal.h; each pointer may be null).  Lane (g, s) of wave w holds, for tile j, units
// 16 (TPW w + j) + 4 g .. + 3 of stream s: one 16-byte piece of the row state[b], read before the frame loop and written behind it by
// the same lane -- so state_out may be state_in, and a workgroup or a stream that runs no frame copies the bits.
template <int TPW, bool STATE>
__global__ void __launch_bounds__(256) gru_train_forward(const std::conditional_t<STATE, TrainForwardStateParams, TrainForwardParams> p) {
    constexpr int NT = 4 * TPW, H = 64 * TPW, H3 = 3 * H;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int group = blockIdx.x, T = p.T;
    const int b_raw = group * kStreamsPerGroup + s;
    const bool bvalid = b_raw < p.B;
    const int b = bvalid ? b_raw : p.B - 1;
    const int len = bvalid ? clamp_len(p.seq_len[b], T) : 0;
    const int tmax = group_frames(p.seq_len, group, p.B, T);

    __shared__ f32x4 hbuf[NT * 64], rhbuf[NT * 64];
    f32x4 hreg[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        hreg[j] = splat4(0.f);
        if constexpr (STATE) {
            if (bvalid && p.io.in) hreg[j] = ld4(p.io.in + (size_t)b * H + (TPW * w + j) * 16 + 4 * g);
        }
        hbuf[(TPW * w + j) * 64 + lane] = hreg[j];
    }
    __syncthreads();

    for (int t = 0; t < tmax; ++t) {
        const size_t row = (size_t)b * T + t;
        f32x4 acc_r[TPW], acc_u[TPW], acc_c[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const float* xr = p.xg + row * H3 + (TPW * w + j) * 16 + 4 * g;
            acc_r[j] = ld4(xr); acc_u[j] = ld4(xr + H); acc_c[j] = ld4(xr + 2 * H);
        }
        // gates, h-part: k-block kb = units 16 kb .. 16 kb + 15 of h, chunk e of it has k = 16 kb + 4 g + e on lane group g
        // (odd k-blocks into a second accumulator: half the chain length for the rounding error, independent MFMAs for the pipe)
        f32x4 odd_r[TPW], odd_u[TPW], odd_c[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) { odd_r[j] = splat4(0.f); odd_u[j] = splat4(0.f); odd_c[j] = splat4(0.f); }
#pragma nounroll
        for (int kb = 0; kb < NT; kb += 2) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x4 hb = hbuf[(kb + q) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* wrow = p.wh + (size_t)(16 * (kb + q) + 4 * g + e) * H3 + 16 * TPW * w + s;
#pragma unroll
                    for (int j = 0; j < TPW; ++j) {
                        f32x4& ar = q ? odd_r[j] : acc_r[j];
                        f32x4& au = q ? odd_u[j] : acc_u[j];
                        ar = mfma4(wrow[16 * j], hb[e], ar);
                        au = mfma4(wrow[H + 16 * j], hb[e], au);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) { acc_r[j] += odd_r[j]; acc_u[j] += odd_u[j]; }
        f32x4 uu[TPW], un[TPW], rh[TPW];          // u, 1 - u, r o h
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const SigmoidParts u = sigmoid_parts(acc_u[j][e]);
                uu[j][e] = u.v;
                un[j][e] = u.comp;
                rh[j][e] = sigmoid_parts(acc_r[j][e]).v * hreg[j][e];
            }
            rhbuf[(TPW * w + j) * 64 + lane] = rh[j];
        }
        __syncthreads();
#pragma nounroll
        for (int kb = 0; kb < NT; kb += 2) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x4 rb = rhbuf[(kb + q) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* wrow = p.wh + (size_t)(16 * (kb + q) + 4 * g + e) * H3 + 2 * H + 16 * TPW * w + s;
#pragma unroll
                    for (int j = 0; j < TPW; ++j) {
                        f32x4& ac = q ? odd_c[j] : acc_c[j];
                        ac = mfma4(wrow[16 * j], rb[e], ac);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) acc_c[j] += odd_c[j];
        const bool live = t < len;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int n = TPW * w + j;
            const size_t at = row * H + n * 16 + 4 * g;
            f32x4 hn, y = splat4(0.f);
#pragma unroll
            for (int e = 0; e < 4; ++e) hn[e] = fmaf(uu[j][e], hreg[j][e], un[j][e] * tanhf(acc_c[j][e]));
            if (live) {
                st4(p.ar + at, acc_r[j]); st4(p.au + at, acc_u[j]); st4(p.ac + at, acc_c[j]); st4(p.hp + at, hreg[j]); st4(p.rh + at, rh[j]);
                y = p.drop ? dropped(hn, p.drop, mask_row<H>(p, b, t) + n * 16 + 4 * g, p.keep_prob) : hn;
                hreg[j] = hn;          // a dead frame copies the state
            }
            if (bvalid) st4(p.y + at, y);
            hbuf[n * 64 + lane] = hreg[j];
        }
        __syncthreads();
    }
    if (bvalid) {        // frames no stream of the group has
        for (int t = tmax; t < T; ++t) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) st4(p.y + ((size_t)b * T + t) * H + (TPW * w + j) * 16 + 4 * g, splat4(0.f));
        }
    }
    if constexpr (STATE) {
        if (bvalid && p.io.out) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) st4(p.io.out + (size_t)b * H + (TPW * w + j) * 16 + 4 * g, hreg[j]);
        }
    }
}

// STATE: dh starts from dstate_out[b] (io.in) and what is left after frame 0 goes to dstate_in[b] (io.out), by the same lanes as above
template <int TPW, bool STATE>
__global__ void __launch_bounds__(256) gru_train_backward(const std::conditional_t<STATE, TrainBackwardStateParams, TrainBackwardParams> p) {
    constexpr int NT = 4 * TPW, H = 64 * TPW, H3 = 3 * H;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, g = lane >> 4, s = lane & 15;
    const int group = blockIdx.x, T = p.T;
    const int b_raw = group * kStreamsPerGroup + s;
    const bool bvalid = b_raw < p.B;
    const int b = bvalid ? b_raw : p.B - 1;
    const int len = bvalid ? clamp_len(p.seq_len[b], T) : 0;
    const int tmax = group_frames(p.seq_len, group, p.B, T);

    __shared__ f32x4 dcbuf[NT * 64], dubuf[NT * 64], drbuf[NT * 64];
    f32x4 dh[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        dh[j] = splat4(0.f);
        if constexpr (STATE) {
            if (bvalid && p.io.in) dh[j] = ld4(p.io.in + (size_t)b * H + (TPW * w + j) * 16 + 4 * g);
        }
    }
    if (bvalid) {
        for (int t = tmax; t < T; ++t) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                float* o = p.dhat + ((size_t)b * T + t) * H3 + (TPW * w + j) * 16 + 4 * g;
                st4(o, splat4(0.f)); st4(o + H, splat4(0.f)); st4(o + 2 * H, splat4(0.f));
            }
        }
    }

    for (int t = tmax - 1; t >= 0; --t) {
        const size_t row = (size_t)b * T + t;
        const bool live = t < len;
        f32x4 ar[TPW], hp[TPW], dhn[TPW], dch[TPW], duh[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int n = TPW * w + j;
            const size_t at = row * H + n * 16 + 4 * g;
            f32x4 au = splat4(0.f), ac = splat4(0.f), dy = splat4(0.f);
            ar[j] = splat4(0.f); hp[j] = splat4(0.f);
            if (live) {          // the tape has rows t < seq_len only
                ar[j] = ld4(p.ar + at); au = ld4(p.au + at); ac = ld4(p.ac + at); hp[j] = ld4(p.hp + at); dy = ld4(p.dy + at);
                if (p.drop) dy = dropped(dy, p.drop, mask_row<H>(p, b, t) + n * 16 + 4 * g, p.keep_prob);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const SigmoidParts u = sigmoid_parts(au[e]);          // the forward's own values: the same functions of the same floats
                const float c = tanhf(ac[e]);
                const float dhp = dy[e] + dh[j][e];
                const float du = dhp * (hp[j][e] - c), dc = dhp * u.comp;
                dhn[j][e] = dhp * u.v;
                dch[j][e] = live ? dc * tanh_slope(ac[e]) : 0.f;
                duh[j][e] = live ? du * u.dv : 0.f;
            }
            dcbuf[n * 64 + lane] = dch[j];
            dubuf[n * 64 + lane] = duh[j];
        }
        __syncthreads();
        // d(rh) = dc^ . Wc_h^T and, beside it, the u half of [dr^ | du^] . Wg_h^T: neither waits for the other
        // (the r half of Wg_h^T, which has to wait for dr^, goes into an accumulator of its own: acc_hr)
        f32x4 acc_rh[TPW], odd_rh[TPW], acc_h[TPW], acc_hr[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) { acc_rh[j] = splat4(0.f); odd_rh[j] = splat4(0.f); acc_h[j] = splat4(0.f); acc_hr[j] = splat4(0.f); }
#pragma nounroll
        for (int kb = 0; kb < NT; kb += 2) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x4 cb = dcbuf[(kb + q) * 64 + lane], ub = dubuf[(kb + q) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 16 * (kb + q) + 4 * g + e;
                    const float* wc = p.wht + (size_t)(2 * H + k) * H + 16 * TPW * w + s;
                    const float* wu = p.wht + (size_t)(H + k) * H + 16 * TPW * w + s;
#pragma unroll
                    for (int j = 0; j < TPW; ++j) {
                        f32x4& arh = q ? odd_rh[j] : acc_rh[j];
                        arh = mfma4(wc[16 * j], cb[e], arh);
                        acc_h[j] = mfma4(wu[16 * j], ub[e], acc_h[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) acc_rh[j] += odd_rh[j];
        f32x4 drh[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = acc_rh[j][e];
                const SigmoidParts r = sigmoid_parts(ar[j][e]);
                dhn[j][e] = fmaf(d, r.v, dhn[j][e]);          // dh += d(rh) o r
                drh[j][e] = live ? d * hp[j][e] * r.dv : 0.f;
            }
            drbuf[(TPW * w + j) * 64 + lane] = drh[j];
        }
        __syncthreads();
#pragma unroll 2
        for (int kb = 0; kb < NT; ++kb) {
            const f32x4 rb = drbuf[kb * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* wr = p.wht + (size_t)(16 * kb + 4 * g + e) * H + 16 * TPW * w + s;
#pragma unroll
                for (int j = 0; j < TPW; ++j) acc_hr[j] = mfma4(wr[16 * j], rb[e], acc_hr[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) dh[j][e] = live ? dhn[j][e] + (acc_h[j][e] + acc_hr[j][e]) : dh[j][e];
            if (bvalid) {
                float* o = p.dhat + row * H3 + (TPW * w + j) * 16 + 4 * g;
                st4(o, drh[j]); st4(o + H, duh[j]); st4(o + 2 * H, dch[j]);
            }
        }
        // the next frame's stores to dcbuf / dubuf come behind this frame's second barrier, which every wave passes only after its
        // first-phase reads; drbuf is next written behind the next frame's first barrier, after every wave's second-phase reads
    }
    if constexpr (STATE) {
        if (bvalid && p.io.out) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) st4(p.io.out + (size_t)b * H + (TPW * w + j) * 16 + 4 * g, dh[j]);
        }
    }
}


hipError_t launch_gru_train_forward(const TrainForwardParams& p, int hidden, hipStream_t st) {
    return with_tpw<1, 2, 4>(hidden, [&](auto tpw) {
        return launch_lds<gru_train_forward<tpw(), false>>(dim3(groups_of(p.B)), dim3(256), 0, st, p);
    });
}

hipError_t launch_gru_train_backward(const TrainBackwardParams& p, int hidden, hipStream_t st) {
    return with_tpw<1, 2, 4>(hidden, [&](auto tpw) {
        return launch_lds<gru_train_backward<tpw(), false>>(dim3(groups_of(p.B)), dim3(256), 0, st, p);
    });
}

hipError_t launch_gru_train_forward_state(const TrainForwardStateParams& p, int hidden, hipStream_t st) {
    return with_tpw<1, 2, 4>(hidden, [&](auto tpw) {
        return launch_lds<gru_train_forward<tpw(), true>>(dim3(groups_of(p.B)), dim3(256), 0, st, p);
    });
}

hipError_t launch_gru_train_backward_state(const TrainBackwardStateParams& p, int hidden, hipStream_t st) {
    return with_tpw<1, 2, 4>(hidden, [&](auto tpw) {
        return launch_lds<gru_train_backward<tpw(), true>>(dim3(groups_of(p.B)), dim3(256), 0, st, p);
    });
}

}  // namespace kws
