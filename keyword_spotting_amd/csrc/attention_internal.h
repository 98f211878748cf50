// Kernel/host surface of the self-attention CTC model (attention_kernels.hip, api_attention.hip).  Not part of the ABI.
#pragma once
#include "kws_internal.h"

namespace kws {

// Row tile of every attention kernel: one workgroup covers 32 rows (stacked frames) of ONE utterance.  Each utterance's
// activations start at row b * Tp of the scratch, Tp = T'_max rounded up to this tile, so a tile never spans two utterances
// and the tiling of utterance b depends on T'_b alone (batch independence).
constexpr int kAttnRows = 32;

// A [K, N] fp32 matrix packed as v_mfma_f32_16x16x4_f32 B operands: [K/16][N/16][64 lanes] float4, lane l, component j =
// W[16 kc + 4 (l / 16) + j][16 nt + l % 16] (rows past K zero).  The A operand of the same product reads the matching
// float4 X[m][16 kc + 4 (l / 16) ...] out of LDS, so both sides agree on the k order inside a chunk.
// f16x3 handles (attention_f16x3.hip) carry the same matrices as v_mfma_f32_16x16x32_f16 B operands behind the same pointers:
// [K/32][N/16][hi | lo][64 lanes] x 8 halves (16 bytes, the unit the float4 pointers count), lane l, element j =
// W[32 kc + 8 (l / 16) + j][16 nt + l % 16], hi = fp16(w), lo = fp16((w - hi) 2^11); W_in is stored times 2^8.
struct AttnLayerW {
    const float4* wqkv;   // [H/16][3H/16][64]
    const float* bqkv;    // [3H]
    const float* ga;      // LN_a gamma [H]
    const float* ba;      // LN_a beta  [H]
    const float4* w1;     // [H/16][Fi/16][64]
    const float* b1;      // [Fi]
    const float4* w2;     // [Fi/16][H/16][64]
    const float* b2;      // [H]
    const float* gb;      // LN_b gamma [H]
    const float* bb;      // LN_b beta  [H]
};

struct AttnParams {
    const float* mel;       // [B, T_max, F]
    const int32_t* lengths; // [B] or null (= T_max); clamped to [0, T_max]
    int B, T_max, F, c;     // c = combine_frame
    int KE;                 // c * F rounded up to 16 (the embedding GEMM's k extent; f16x3: to 32)
    int T1max;              // T'_max: rows of the outputs per utterance
    int Tp, ntile;          // scratch rows per utterance (multiple of kAttnRows) and its tiles
    int Fi, C, use_relu;
    const float4* w_in;     // [KE/16][H/16][64]
    const float* b_in;      // [H]
    const float* pe;        // [>= T1max][H]
    const float* w_out;     // [H][C] row-major
    const float* b_out;     // [C]
    float* S;               // [B][Tp][H]   layer input before its LN_b (layer 0: the embedding)
    float* QKV;             // [B][Tp][3H]
    float* U;               // [B][Tp][H]   att + x, before LN_a
    float4* st_a;           // [B][ntile]   (count, mean, M2) of U per row tile
    float4* st_b;           // [B][ntile]   ... of S (the FFN's z + y)
    float* logits;          // [B][T1max][C] or null
    float* softmax;         // [B][T1max][C] or null
};

// prev == null: the layer's input is the embedding (no LN_b in front of it)
hipError_t launch_attn_embed(const AttnParams& p, int H, hipStream_t st);
hipError_t launch_attn_qkv(const AttnParams& p, const AttnLayerW& w, const AttnLayerW* prev, int H, hipStream_t st);
hipError_t launch_attn_core(const AttnParams& p, const AttnLayerW* prev, int H, int D, hipStream_t st);
hipError_t launch_attn_ffn(const AttnParams& p, const AttnLayerW& w, int H, hipStream_t st);
hipError_t launch_attn_out(const AttnParams& p, const AttnLayerW& last, int H, hipStream_t st);
// the f16x3 forms of the three GEMM kernels (attention_f16x3.hip); the core and the output kernel are shared
hipError_t launch_attn_embed_f16x3(const AttnParams& p, int H, hipStream_t st);
hipError_t launch_attn_qkv_f16x3(const AttnParams& p, const AttnLayerW& w, const AttnLayerW* prev, int H, hipStream_t st);
hipError_t launch_attn_ffn_f16x3(const AttnParams& p, const AttnLayerW& w, int H, hipStream_t st);

// ---- the sliding-window manager (attention_stream_kernels.hip, api_attention_stream.hip).  Per stream the manager owns a LINEAR
// window win[b] = [W][F] mel frames, oldest first, of which the first len[b] are live, and the frame counts of its count[b] <= nq
// slots (chunks), oldest first: slot_frames[b][0 .. count[b]).  W = nq x the frames of the longest chunk, so a slot always fits.

// Behind the front-end's ragged gate launch (frames / skip / silent are its outputs; mel [B][T][F] the chunk's frames).  Per stream:
// skip -> nothing but run_len[b] = 0; else clear on silent, drop the oldest slot with its frames when nq slots are held
// (SimpleQueue.add), append the chunk's frames as the newest slot; run_len[b] = len[b], the length the model runs over.
struct AttnStreamWindowParams {
    const float* mel;
    const int32_t* frames;
    const uint8_t *skip, *silent;
    float* win;
    int32_t *slot_frames, *count, *len, *run_len;
    int B, T, W, F, nq;
};
// Behind the model: ctc_decode2's frame rule over the T'_b = frames_out(run_len[b]) softmax rows (none where run_len[b] == 0), repeats
// collapsed, the label's matcher (window_label_delta) over the emitted words; hit[b]; a hit empties the window (count, len = 0).
struct AttnStreamDecideParams {
    const float* softmax;   // [B][T1max][C]
    const int32_t* run_len;
    int32_t *count, *len, *hit;
    int B, T1max, C, c, n_label;
    float thres;
    uint8_t delta[256];
};
// kws_attention_stream_recycle: slots[b] != 0 -> carry length 0, empty window
struct AttnStreamRecycleParams {
    const uint8_t* slots;
    int32_t *carry_len, *count, *len;
    int B;
};
hipError_t launch_attn_stream_window(const AttnStreamWindowParams& p, hipStream_t st);
hipError_t launch_attn_stream_decide(const AttnStreamDecideParams& p, hipStream_t st);
hipError_t launch_attn_stream_recycle(const AttnStreamRecycleParams& p, hipStream_t st);

}  // namespace kws
