// CTC prefix beam search (the decoder the reference leaves commented out: tf.nn.ctc_beam_search_decoder(log(softmax), seqLengths,
// beam_width=config.beam_size, top_paths=1), models/rnn_ctc.py:105-110, :166-176), in its exact-candidate form: the top K
// labellings of each utterance with their log-probabilities.  The blank is the LAST class; tests/beam_model.py restates the rules.
//
//   ctc_beam_kernel   one wave per utterance, as ctc_loss_kernel.  Beam entry i lives in lane i: lp_b, lp_nb, last label, length, a
//                     hash of the prefix and of its parent.  The prefix strings live in LDS that belongs to the wave alone, one row
//                     of kBeamRow bytes per entry, double-buffered.  A frame:
//     1. lane q of a resident prefix computes its stay and looks for its parent among the residents -- hash and length as the
//        filter, the string comparison as the decision -- and merges the parent's extension by last(q) into its own lp_nb'; that
//        extension is struck from the candidates (a stamp per candidate in LDS).
//     2. candidate k = 8 e + c (c < C - 1: entry e extended by label c; c = 7: entry e stays) sits in lane k & 63, at most four per
//        lane; its score goes to LDS as a 64-bit key (ordered score bits, then the smaller index wins a tie).
//     3. every candidate counts the keys above its own: that rank is its slot in the next beam (rank < W survives), so the beam is
//        always in descending order and one input always gives the same bits.
//     4. survivors leave (lp_b', lp_nb', source entry, label) in LDS; lane r picks slot r up, the wave copies the strings.
// Hand-offs are wavefront-scope fences plus wave_barrier (ctc_wave_sync): no workgroup barrier, no atomics, no cross-wave traffic.
#include "ctc_device.h"
#include "launch.h"

namespace kws {

namespace {

constexpr int kBeamRowWords = kBeamRow / 4;
constexpr uint32_t kBeamHashSeed = 0x811c9dc5u;

__device__ __forceinline__ uint32_t beam_hash_push(uint32_t h, int c) { return (h ^ (uint32_t)(c + 1)) * 0x01000193u; }

// float bits whose unsigned order is the float order; every score above -inf maps above 0
__device__ __forceinline__ uint32_t beam_ordered_bits(float s) {
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the first n bytes of rows a and b (kBeamRow bytes each, 4-byte aligned) are equal; the bytes behind a prefix are not defined
__device__ __forceinline__ bool beam_prefix_equal(const uint32_t* a, const uint32_t* b, int n) {
    bool same = true;
    for (int w = 0; 4 * w < n && w < kBeamRowWords; ++w) {
        uint32_t x = a[w] ^ b[w];
        const int rem = n - 4 * w;
        if (rem < 4) x &= (1u << (8 * rem)) - 1u;
        same = same && x == 0;
    }
    return same;
}

// what the extension of a prefix (lp_b, lp_b (+) lp_nb, last label) by label c starts from: a repeat of the last label needs a blank between
__device__ __forceinline__ float beam_extend_from(int c, int last, float b, float tot) { return c == last ? b : tot; }

__device__ __forceinline__ int beam_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

}  // namespace

__global__ void __launch_bounds__(64) ctc_beam_kernel(const float* __restrict__ logits, const int32_t* __restrict__ seq_len, int T, int C, int W,
                                                      int K, int L_max, int merge_repeated, int32_t* __restrict__ paths,
                                                      int32_t* __restrict__ lengths, float* __restrict__ log_prob) {
    extern __shared__ float beam_lds[];
    const int u = blockIdx.x, lane = threadIdx.x;
    const int blank = C - 1;
    int len_u = seq_len ? seq_len[u] : T;
    len_u = beam_uniform(len_u < 0 ? 0 : (len_u > T ? T : len_u));
    const float* lg = logits + (size_t)u * T * C;

    float* lp = beam_lds;                                                             // [T][8]
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(lp + (size_t)T * kCtcRow);   // [256]; T * 32 bytes: 8-byte aligned
    uint32_t* stamp = reinterpret_cast<uint32_t*>(keys + kBeamCandidates);            // [256] frame + 1 in which a candidate was merged away
    float* sel_b = reinterpret_cast<float*>(stamp + kBeamCandidates);                 // [32] the next beam, by slot
    float* sel_nb = sel_b + kBeamMax;
    int32_t* sel_src = reinterpret_cast<int32_t*>(sel_nb + kBeamMax);                 // source entry | label << 8 (7: a stay)
    uint32_t* str0 = reinterpret_cast<uint32_t*>(sel_src + kBeamMax);                 // [2][32][kBeamRow bytes]
    uint32_t* cur = str0;
    uint32_t* nxt = str0 + kBeamMax * kBeamRowWords;

    // log-softmax of the live frames, 8 per pass: lane >> 3 is the frame, lane & 7 the class
    for (int t0 = 0; t0 < len_u; t0 += 8) {
        const int t = t0 + (lane >> 3), k = lane & 7;
        const bool on = t < len_u && k < C;
        const float v = ctc_row_log_softmax(on ? lg[(size_t)t * C + k] : -INFINITY);
        if (on) lp[t * kCtcRow + k] = v;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) stamp[lane + 64 * j] = 0u;
    ctc_wave_sync();

    // entry `lane` of the beam; the empty prefix (last = -1) at (0, -inf) in lane 0
    int n = 1;
    float b = lane == 0 ? 0.f : -INFINITY, nb = -INFINITY;
    int last = -1, len = 0;
    uint32_t hash = kBeamHashSeed, phash = 0u;

    for (int t = 0; t < len_u; ++t) {
        const float* row = lp + t * kCtcRow;
        const bool res = lane < n;
        // 1. the stay of resident `lane`, and the extension of its parent that lands on it
        const float tot = ctc_logaddexp(b, nb);
        float sb = res ? tot + row[blank] : -INFINITY;
        float snb = res && len > 0 ? nb + row[last] : -INFINITY;
        int par = -1;
        for (int i = 0; i < n; ++i) {
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)hash, i);
            const int li = __builtin_amdgcn_readlane(len, i);
            if (res && len > 0 && par < 0 && phash == hi && len == li + 1 &&
                beam_prefix_equal(cur + i * kBeamRowWords, cur + lane * kBeamRowWords, li))
                par = i;
        }
        const int pi = par < 0 ? 0 : par;
        const float pb = __shfl(b, pi, 64), ptot = __shfl(tot, pi, 64);
        const int plast = __shfl(last, pi, 64);
        if (par >= 0) {
            const float src = beam_extend_from(last, plast, pb, ptot);
            if (src > -INFINITY) snb = ctc_logaddexp(snb, row[last] + src);
            stamp[par * 8 + last] = (uint32_t)(t + 1);
        }
        ctc_wave_sync();

        // 2. the candidates of this lane: k = lane + 64 j, entry k >> 3, label k & 7
        const int c = lane & 7;
        const int groups = (n + 7) >> 3;
        float cb[4], cnb[4];
        unsigned long long key[4];
        int nvalid = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cb[j] = -INFINITY; cnb[j] = -INFINITY; key[j] = 0ull;
            if (j < groups) {          // uniform
                const int e = (lane >> 3) + 8 * j, k = lane + 64 * j;
                const float eb = __shfl(b, e, 64), etot = __shfl(tot, e, 64), esb = __shfl(sb, e, 64), esnb = __shfl(snb, e, 64);
                const int elast = __shfl(last, e, 64), elen = __shfl(len, e, 64);
                bool valid = e < n;
                float s = -INFINITY;
                if (c == 7) {
                    cb[j] = esb; cnb[j] = esnb;
                    s = ctc_logaddexp(esb, esnb);
                } else if (c < blank) {
                    const float src = beam_extend_from(c, elast, eb, etot);
                    valid = valid && elen < L_max && stamp[k] != (uint32_t)(t + 1);
                    s = row[c] + src;
                    cnb[j] = s;
                } else {
                    valid = false;
                }
                valid = valid && s > -INFINITY;          // (a NaN is no candidate either)
                if (valid) key[j] = ((unsigned long long)beam_ordered_bits(s) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)k);
                keys[k] = key[j];
                nvalid += __popcll(__ballot(valid));
            }
        }
        ctc_wave_sync();

        // 3. rank = the number of keys above this one; 4. the survivors' new entries by slot
        int rank[4] = {0, 0, 0, 0};
        const int m = n * 8;
        for (int k2 = 0; k2 < m; k2 += 2) {
            const unsigned long long x0 = keys[k2], x1 = keys[k2 + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < groups) rank[j] += (x0 > key[j] ? 1 : 0) + (x1 > key[j] ? 1 : 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (key[j] != 0ull && rank[j] < W) {
                sel_b[rank[j]] = cb[j];
                sel_nb[rank[j]] = cnb[j];
                sel_src[rank[j]] = ((lane >> 3) + 8 * j) | (c << 8);
            }
        }
        const int n2 = beam_uniform(nvalid < W ? nvalid : W);
        ctc_wave_sync();

        const bool res2 = lane < n2;
        const int src = res2 ? sel_src[lane] : 0;
        const int se = src & 31, sc = (src >> 8) & 7;
        const uint32_t oh = (uint32_t)__shfl((int)hash, se, 64), oph = (uint32_t)__shfl((int)phash, se, 64);
        const int olast = __shfl(last, se, 64), olen = __shfl(len, se, 64);
        for (int r0 = 0; r0 < n2; r0 += 4) {          // four rows of sixteen words per pass
            const int r = r0 + (lane >> 4), w = lane & 15;
            if (r < n2 && 4 * w < L_max) nxt[r * kBeamRowWords + w] = cur[(sel_src[r] & 31) * kBeamRowWords + w];
        }
        if (res2) {
            b = sel_b[lane]; nb = sel_nb[lane];
            if (sc == 7) { hash = oh; phash = oph; last = olast; len = olen; }
            else {
                hash = beam_hash_push(oh, sc); phash = oh; last = sc; len = olen + 1;
                if (len > kBeamRow) len = kBeamRow;          // L_max <= kBeamRow keeps it there; never index past a row
                reinterpret_cast<uint8_t*>(nxt)[lane * kBeamRow + len - 1] = (uint8_t)sc;
            }
        } else {
            b = -INFINITY; nb = -INFINITY; last = -1; len = 0; hash = 0u; phash = 0u;
        }
        n = n2;
        uint32_t* swap = cur; cur = nxt; nxt = swap;
        ctc_wave_sync();
    }

    // the K best, already in descending order of lp_b (+) lp_nb: lane k writes rank k
    if (lane < K) {
        int32_t* out = paths + ((size_t)u * K + lane) * L_max;
        const uint8_t* s = reinterpret_cast<const uint8_t*>(cur) + lane * kBeamRow;
        int o = 0;
        if (lane < n) {
            int prev = -1;
            for (int i = 0; i < len; ++i) {
                const int ci = s[i];
                if (!(merge_repeated && ci == prev) && o < L_max) out[o++] = ci;
                prev = ci;
            }
        }
        lengths[(size_t)u * K + lane] = o;
        log_prob[(size_t)u * K + lane] = lane < n ? ctc_logaddexp(b, nb) : -INFINITY;
        for (int i = o; i < L_max; ++i) out[i] = -1;
    }
}

hipError_t launch_ctc_beam(const float* logits, const int32_t* seq_len, int B, int T, int C, int W, int K, int L_max, int merge_repeated,
                           int32_t* paths, int32_t* lengths, float* log_prob, hipStream_t st) {
    return launch_lds<ctc_beam_kernel>(dim3(B), dim3(64), ctc_beam_lds_bytes(T), st, logits, seq_len, T, C, W, K, L_max, merge_repeated, paths,
                                       lengths, log_prob);
}

}  // namespace kws
