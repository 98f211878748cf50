// Internal declarations shared by the HIP translation units of libkws_amd.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kws_amd.h"

// Experiment / test switches compiled into the kernel sources (timing counters, ablations, the self-test's negative control).
// A product build defines none of them; tools/build_variant.sh -- the only place that defines KWS_VARIANT_BUILD -- passes them
// to every translation unit, so kws_version() of such a library names them (KWS_VARIANT_TAG) and a stray -D in a product
// build does not compile.
#if defined(KWS_FAULT_INJECT) || defined(KWS_ABL_NOFLUSH) || defined(KWS_ABL_NOMEL) || defined(KWS_F16_TIMING) || defined(KWS_FE_TIMING) || \
    defined(KWS_FE_OCC) || defined(KWS_FE_FT) || defined(KWS_FE_SF) || defined(KWS_FE_NOSTAGE) || defined(KWS_FE_NODFT) || defined(KWS_FE_NOMEL) || \
    defined(KWS_OABL_NODIV) || defined(KWS_OABL_NODOT) || defined(KWS_OVERLAP_MIN_T) || defined(KWS_EXP_F16_WLO_ZERO)
#ifndef KWS_VARIANT_BUILD
#error "an experiment switch (KWS_FAULT_INJECT / KWS_ABL_* / KWS_*_TIMING / KWS_FE_* / KWS_OABL_* / KWS_OVERLAP_MIN_T) is defined in a product build: use tools/build_variant.sh"
#endif
#endif
#ifdef KWS_VARIANT_BUILD
#define KWS_VARIANT_TAG_1(name) "; " #name
#ifdef KWS_FAULT_INJECT
#define KWS_TAG_FAULT KWS_VARIANT_TAG_1(FAULT_INJECT)
#else
#define KWS_TAG_FAULT ""
#endif
#ifdef KWS_ABL_NOFLUSH
#define KWS_TAG_NOFLUSH KWS_VARIANT_TAG_1(ABL_NOFLUSH)
#else
#define KWS_TAG_NOFLUSH ""
#endif
#ifdef KWS_ABL_NOMEL
#define KWS_TAG_NOMEL KWS_VARIANT_TAG_1(ABL_NOMEL)
#else
#define KWS_TAG_NOMEL ""
#endif
#if defined(KWS_F16_TIMING) || defined(KWS_FE_TIMING)
#define KWS_TAG_TIMING KWS_VARIANT_TAG_1(TIMING)
#else
#define KWS_TAG_TIMING ""
#endif
#ifdef KWS_EXP_F16_WLO_ZERO
#define KWS_TAG_WLO KWS_VARIANT_TAG_1(EXP_F16_WLO_ZERO)
#else
#define KWS_TAG_WLO ""
#endif
#define KWS_VARIANT_TAG "; VARIANT BUILD" KWS_TAG_FAULT KWS_TAG_NOFLUSH KWS_TAG_NOMEL KWS_TAG_TIMING KWS_TAG_WLO
#else
#define KWS_VARIANT_TAG ""
#endif

namespace kws {

constexpr int kStreamsPerGroup = 16;  // MFMA N dimension: one workgroup advances 16 streams
constexpr int kMaxClasses = 8;

// One launch = one GRU layer over all T frames of the call, for every 16-stream group.
//
// Exchange layout ("xl"): a [H x 16 streams] activation block is stored as [H/16][64 lanes] float4,
// lane = 16*g + s, component r  <->  unit 16*n + 4*g + r of stream s.  This is at once the MFMA
// 16x16x4 C/D register image of tile n and, read back as float4, the B operand of the four
// k-chunks 4n..4n+3 -- so hidden state never needs a cross-lane transpose.
// The incremental decode window of a stream manager (window_device.h), run as the tail of the last layer's launch or by
// window_inc_kernel.  tab == nullptr: none.
struct WindowTail {
    uint8_t* tab;               // [B][nq][32]  per queued chunk: tab[16] matcher state after its frames 1..n-1 when entered in state q; ftab[16] the same
                                //              with its first frame decided against its predecessor's last word (window_device.h)
    uint32_t* meta;             // [B][nq]      bit 16: the chunk has frames; bits 0-7: first frame's word + 1; bits 8-15: last frame's word + 1
    int* head;                  // [B]
    int* count;                 // [B]
    const uint8_t* delta;       // [16 states][16 words] label matcher (KMP automaton), device memory
    const uint8_t* clear_before;// [B] or null
    int32_t* hit;               // [B]
    uint8_t* restart;           // [B] or null
    int nq, n_label;
};
constexpr int kWinTailMaxFrames = 64;   // chunk lengths the fused tail takes (its per-frame words wait in LDS): longer -> window_inc_kernel
constexpr int kWinTailMaxChunks = 24;   // window lengths the fused tail takes (the rings of 16 streams are staged in 16 KiB of LDS)
constexpr int kWinTailWordsStride = kWinTailMaxFrames + 4;                    // bytes per stream row of the words (68: rows on different banks)
constexpr size_t kWinTailWordsBytes = (size_t)16 * kWinTailWordsStride + 256;   // the call's words [16 streams][stride] + the label matcher [16][16]
__host__ __device__ inline size_t window_tail_scratch_bytes(int nq) { return (size_t)16 * (nq * 32 + 32); }

struct GruLayerParams {
    // weights (device, packed by pack.cpp)
    const float* wx;        // x-part fragments  [NT][3][KCX/4][64][4]; resident first layer: [NT][3][KCX][64]
    const float* wh;        // h-part fragments  [NT][3][H/16][64][4]
    const float* bias;      // [3][H]  (r, u, c)
    const float* wfc;       // LAST: [H/4][64] fragments of Wfc^T padded to 16 rows
    const float* bfc;       // LAST: [16] padded
    // activations
    const float* x_mel;     // FIRST: mel [B,T,I]
    const float4* x_prev;   // !FIRST: previous layer's output, xl layout [G][T][NT][64]
    float4* h_out;          // !LAST: this layer's output, xl layout
    const float* state_in;  // [B,H] of this layer
    float* state_out;       // [B,H]
    const int32_t* seq_len; // [B] or null
    const uint8_t* reset;   // [B] or null
    // LAST-layer epilogue
    float* logits;          // [B,T,C] or null
    float* softmax;         // [B,T,C] or null
    int8_t* tokens;         // [B,T] or null
    int32_t* prev_word;     // [B] or null
    float decode_thres;
    float value_clip;
    int use_relu;
    int B, T, I, C;
    int t_stride;           // frames per stream row of x_mel / logits / softmax / tokens (0: T) -- a call on a time block
    int t_base;             // of a longer sequence passes pre-offset pointers, the full row stride, and its first frame
    int KCX;                // x-part k-chunks (generic: multiple of 4)
    // layer-pipelined launch (generic kernel): frames published by the layer below / by this layer, per group
    const int* ready_in;
    int* ready_out;
    int* pipe_error;
    // LAST, kernels instantiated with the window tail only (kws_stream_feed): the decode-window step of detector.py:195-209
    // for the group's 16 streams, after their last frame (kept at the end: every other field keeps its offset)
    WindowTail win;
};
struct GruStackParams {
    GruLayerParams layer[8];
    int L, G;
    int xcd_affine;   // L divides 8: block i -> (layer = (i % 8) % L, group = (i / 8) * (8 / L) + (i % 8) / L)
};
hipError_t launch_gru_stack_generic_pipelined(const GruStackParams& sp, int hidden, hipStream_t st);

// Cell wrappers of the reference's get_cell (models/rnn_ctc.py:186-197): ResidualWrapper(LayerNormalizer(GRUCell)), the residual on
// layers >= 1 only (utils/custom_wrapper.py:95-158).  A kernel argument of the wrapped generic instantiations only, so that
// GruLayerParams / GruStackParams and every plain instantiation stay as they are.
struct GruWrapLayer {
    const float* igamma;    // layer norm: the per-feature SHIFT, [16 * KCX/4] floats (zero past I); null: no layer norm on this layer
    float ibeta;            // layer norm: the scalar SCALE.  The reference binds _ln(inputs, ibeta, igamma) to _ln(input, s, b)
                            // (custom_wrapper.py:130 against :145): its names are swapped, and kept here as they are in checkpoints
    int residual;           // 0.7071 (h' + x) is the layer's output (seam / dense layer); the recurrent state stays h'
};
struct GruWrapParams { GruWrapLayer layer[8]; };
// extra dynamic LDS of a wrapped launch whose layers take at most kx4 input k-groups (16 features each): the normalised frame
constexpr size_t gru_wrapped_extra_lds(int kx4) { return (size_t)kx4 * 64 * 16; }
hipError_t launch_gru_layer_generic_wrapped(const GruLayerParams& p, const GruWrapLayer& wl, int hidden, bool first, bool last,
                                            hipStream_t st);
hipError_t launch_gru_stack_generic_pipelined_wrapped(const GruStackParams& sp, const GruWrapParams& wp, int hidden, hipStream_t st);

// bf16 fused stack (gru_bf16.hip): every layer in one launch, no inter-layer scratch
struct GruBf16Params {
    const uint4* w[2];      // per layer: [8 tiles][3 gates][KC_l chunks][64 lanes] bf16x8 A operands (x chunks first)
    const float* bias[2];   // per layer [3][128] fp32
    const uint4* wfc;       // [4 chunks][64]  Wfc^T padded to 16 rows
    const float* bfc;       // [16]
    const float* x_mel;     // [B,T,I]
    const float* state_in;  // [L,B,128]
    float* state_out;
    const int32_t* seq_len;
    const uint8_t* reset;
    GruLayerParams epi;     // logits / softmax / tokens / prev_word / thresholds for the epilogue
    int B, T, I, L;
};
bool gru_bf16_supported(int hidden, int n_mel, int layers);
hipError_t launch_gru_stack_bf16(const GruBf16Params& p, int kx0, int nl, hipStream_t st);    // p.epi.win.tab != null: with the window tail
bool gru_stack_bf16_takes_window(int kx0, int nl);          // the launch above has a window-tail instantiation for this shape
const char* gru_stack_bf16_kernel_name(int kx0, int nl);   // the kernel launch_gru_stack_bf16 picks (KWS_BF16_WAVES aware)
bool gru_bf16_vgpr_form();                                  // built with -mllvm -amdgpu-mfma-vgpr-form=1 (csrc/Makefile)

// "f16x3": fp32-accuracy stack on the fp16 matrix pipe, operands split hi + 2^-11 lo (gru_f16x3.hip); one layer per launch
struct GruF16Params {
    const uint4* w;         // [8 tiles][3 gates][KX + 4 chunks][hi|lo][64 lanes] f16x8 A operands (x chunks first)
    const float* bias;      // [3][128] fp32
    const uint4* wfc;       // LAST: [4 chunks][hi|lo][64]  Wfc^T padded to 16 rows
    const float* bfc;       // [16]
    const float* x_mel;     // FIRST: [B,T,I]
    const uint4* x_prev;    // !FIRST: the layer below's output, split, B-operand order: [G][T][4 chunks][hi|lo][64 lanes]
    uint4* h_out;           // !LAST: this layer's output, same layout
    const float* state_in;  // [B,128] of this layer
    float* state_out;
    const int32_t* seq_len;
    const uint8_t* reset;
    GruLayerParams epi;     // LAST: logits / softmax / tokens / prev_word / thresholds for the epilogue
    int B, T, I;
};
// ... for the shapes the resident kernels do not cover (hidden = 256: BASELINE configs[4]), weights streamed from L2 every frame
// (gru_f16x3_generic.hip): one layer per launch, or all L x G workgroups in one layer-pipelined grid.  Tables as above with
// H/16 tiles, H/32 hidden chunks and the first layer's x chunks padded to an even count; the pipelined launch takes ready_in /
// ready_out / pipe_error from p.epi.
struct GruF16StackParams {
    GruF16Params layer[8];
    int L, G;
    int xcd_affine;
};
static_assert(sizeof(GruF16StackParams) <= 4096, "kernel arguments");
bool gru_f16x3_generic_supported(int hidden, int n_mel);
hipError_t launch_gru_layer_f16x3_generic(const GruF16Params& p, int hidden, bool first, bool last, hipStream_t st);
hipError_t launch_gru_stack_f16x3_pipelined(const GruF16StackParams& sp, int hidden, hipStream_t st);
bool gru_f16x3_supported(int hidden, int n_mel);
hipError_t launch_gru_layer_f16x3(const GruF16Params& p, bool first, bool last, hipStream_t st);    // last && p.epi.win.tab: with the window tail
bool gru_f16x3_vgpr_form();                                 // gru_f16x3.hip built with -mllvm -amdgpu-mfma-vgpr-form=1 (csrc/Makefile)

// int8 ("octbit") GRU layers and class projection (gru_octbit.hip)
struct GruOctbitParams {
    const uint32_t* wg;     // gates  [4 K-quarters][2 unit groups][2 units per lane][32 = 16 couples x (even,odd)][64 lanes]  int16 pairs
    const uint32_t* wc;     // cand.  [8 K-eighths][2 units per lane][16][64 lanes]
    const float* bias;      // [3][128] (r, u, c)
    const float* b127;      // [384]  127 * column sums of Wq: gates 256, candidate 128 (octbit_graph.py:202-204)
    float scale_g, scale_c; // octize_weight_int8_signed scales
    const float4* x_prev;   // previous layer's output, xl layout
    float4* h_out;          // this layer's output, xl layout
    const float* state_in;  // [B,128]
    float* state_out;
    const int32_t* seq_len;
    const uint8_t* reset;
    uint32_t* aq;           // activation exchange [G][2][16 streams][128 dwords]
    float2* range;          // top layer only: (min, max) of each stream's emitted rows, for the projection; else null
    int B, T;
};
struct OctbitFcParams {
    const uint32_t* wfc;    // [8 tiles][4 g][kMaxClasses][even,odd] int16 pairs
    const float* b127;      // [kMaxClasses]
    const float* bfc;       // [16] padded
    float scale_w;
    const float4* h_top;    // top layer output, xl layout
    const int32_t* seq_len; // rows t >= seq_len[b] are zero rows, whatever the seam holds (or null)
    float2* range;          // [G*16] (min, max) of each stream's [T,H] block
    int range_ready;        // the top int8 layer already produced it
    const int32_t* prev_in; // copy of prev_word taken before the launch (or null)
    float* logits; float* softmax; int8_t* tokens; int32_t* prev_word;
    float decode_thres, value_clip;
    int use_relu, B, T, C;
};
hipError_t launch_gru_layer_octbit(const GruOctbitParams& p, hipStream_t st);
hipError_t launch_octbit_fc(const OctbitFcParams& p, hipStream_t st);

// the class heads of a multi-head step (dense_heads.hip): behind a stack whose top layer wrote a seam like every other layer
struct DenseHead {
    const float* wfc;       // [H/4][64] fragments of Wfc^T padded to 16 rows (GruLayerParams::wfc)
    const float* bfc;       // [16] padded
    float* logits;          // [B,T,C] or null
    float* softmax;         // [B,T,C] or null
    int8_t* tokens;         // [B,T] or null
    int32_t* prev_word;     // [B] or null: written by the block that holds frame T - 1
    const int32_t* prev_in; // copy of prev_word taken before the launch (null iff prev_word is)
    float decode_thres;
    int C;                  // 0: this head is not wanted
};
struct DenseHeadsParams {
    const float4* h_top;    // top layer output, xl layout [G][T][H/16][64]
    const int32_t* seq_len; // [B] or null: frames t >= seq_len[b] are the zero row, whatever the seam holds there
    const uint8_t* reset;   // [B] or null: non-zero -> the stream's previous word is -1
    float* nn_outputs;      // [B,T,H] row-major or null, 16-byte aligned
    DenseHead head[2];
    float value_clip;
    int use_relu, B, T;
};
constexpr int kHeadFrames = 32;          // frames per workgroup
constexpr int kHeadsMaxFrames = 65535 * kHeadFrames;      // grid.y
hipError_t launch_dense_heads(const DenseHeadsParams& p, int hidden, hipStream_t st);

// Both class heads AND both decode windows of a two-head stream manager (heads_window.hip): one launch behind a stack planned as
// a heads step, one workgroup per 16-stream group over the whole chunk -- each head's rows -> frame words -> that head's
// incremental window, then the coupling: a hit of either head clears both windows and requests the restart.
struct HeadsWindowHead {
    const float* wfc;       // as DenseHead
    const float* bfc;
    float* softmax;         // [B,T,C] or null: bitwise dense_heads_kernel's rows
    float decode_thres;     // the window's threshold
    int C;
};
struct HeadsWindowParams {
    const float4* h_top;    // top layer output, xl layout [G][T][H/16][64]; unused when T == 0
    HeadsWindowHead head[2];
    WindowTail win[2];      // clear_before is the same array in both; hit / restart of the tails are overwritten by the coupling
    int32_t* hit;           // [B] hit_1 | hit_2 << 1
    uint8_t* restart;       // [B] or null
    // ragged chunks (kws_stream_feed_ragged): stream b's chunk is its first frames[b] <= T rows; skip[b] != 0: no slot in either
    // window, no clear, hit 0, restart untouched.  frames == null: every stream has T frames.
    const int32_t* frames;
    const uint8_t* skip;
    float value_clip;
    int use_relu, B, T;
};
constexpr size_t kHeadsWindowLogitsBytes = (size_t)2 * 16 * kHeadFrames * 8 * sizeof(float);      // [head][stream][frame][8]
// LDS of the launch: logits of a frame block, both heads' frame words [2][16][round_up(T, 16)], two label matchers, two rings
__host__ __device__ inline int heads_window_stride(int T) { return T > 0 ? (T + 15) & ~15 : 16; }
__host__ __device__ inline size_t heads_window_lds_bytes(int T, int nq1, int nq2) {
    return kHeadsWindowLogitsBytes + (size_t)2 * 16 * heads_window_stride(T) + 512 + window_tail_scratch_bytes(nq1) + window_tail_scratch_bytes(nq2);
}
hipError_t launch_heads_window(const HeadsWindowParams& p, int hidden, hipStream_t st);

// A bank of enrolled heads (bank_heads.hip, bank_device.h): head 2 of stream b is head 1's logits with the n_new columns of bank slot
// user[b] spliced in front of the blank.  The two kernels keep the grid and phases of dense_heads_kernel / heads_window_kernel; of
// head[1] they read C (= head 1's C + n_new), the threshold and the outputs -- never wfc / bfc.
struct BankRef {
    const float* Wn;        // [capacity][H][n_new]  (the layout kws_enroll_get writes)
    const float* bn;        // [capacity][n_new]
    const int32_t* user;    // [B] slot of each stream; outside [0, capacity): the stream has no second head
    int capacity, n_new;
};
struct BankHeadsParams { DenseHeadsParams d; BankRef bank; };       // d.head[0] is always bound (its outputs may all be null)
struct BankWindowParams { HeadsWindowParams w; BankRef bank; };
// A slot's keyword of its own (kws_bank_set_keyword): the matcher of its label (api_window.hip's KMP table, what window_tail walks),
// the label's length, and the width of its head -- head 2 of a stream on the slot has C + n_used classes (the slot's first n_used
// columns), rows zero-padded to C + n_new.  own == 0: no keyword of its own -- the manager's label2 over all n_new columns.
struct BankSlotKeyword {
    uint8_t delta[256];
    int32_t n_label, n_used, own, pad;
};
static_assert(sizeof(BankSlotKeyword) == 272, "16-byte loads of the matcher");
// The keyword forms of the two kernels (a bank on which kws_bank_set_keyword was ever called): the slot table [capacity] behind the
// arguments of the plain forms, which keep their layout
struct BankKeywordHeadsParams { BankHeadsParams b; const BankSlotKeyword* slots; };
struct BankKeywordWindowParams { BankWindowParams b; const BankSlotKeyword* slots; };
constexpr size_t kBankHeadsLogitsBytes = (size_t)2 * 16 * (kHeadFrames + 1) * 8 * sizeof(float);      // [head 1 | new classes][stream][slot][8]
constexpr size_t kBankHeadsWordsBytes = (size_t)2 * 16 * (kHeadFrames + 1) * sizeof(int);
// LDS of a group's staged columns [n_new][H/16][64 lanes][4] and biases [16][8]
__host__ __device__ inline size_t bank_stage_bytes(int H, int n_new) { return ((size_t)16 * H * n_new + 128) * sizeof(float); }
__host__ __device__ inline size_t bank_heads_lds_bytes(int H, int n_new) { return kBankHeadsLogitsBytes + kBankHeadsWordsBytes + bank_stage_bytes(H, n_new); }
__host__ __device__ inline size_t bank_window_lds_bytes(int T, int nq1, int nq2, int H, int n_new) {
    return heads_window_lds_bytes(T, nq1, nq2) + bank_stage_bytes(H, n_new);
}
// ... the keyword form stages the group's sixteen matchers and per stream (n_label, n_used) behind the columns
constexpr size_t kBankKeywordStageBytes = (size_t)16 * 256 + 16 * 2 * sizeof(int);
__host__ __device__ inline size_t bank_keyword_window_lds_bytes(int T, int nq1, int nq2, int H, int n_new) {
    return bank_window_lds_bytes(T, nq1, nq2, H, n_new) + kBankKeywordStageBytes;
}
hipError_t launch_bank_set_keyword(BankSlotKeyword* dst, const BankSlotKeyword& v, hipStream_t st);      // *dst = v, stream-ordered
// slots == null: the plain kernels; else their keyword forms
hipError_t launch_bank_heads(const BankHeadsParams& p, const BankSlotKeyword* slots, int hidden, hipStream_t st);
hipError_t launch_bank_heads_window(const BankWindowParams& p, const BankSlotKeyword* slots, int hidden, hipStream_t st);

// decode window of the stream manager (stream_kernels.hip)
struct WindowParams {
    int8_t* words;            // [B][nq][tmax] per-frame ctc_decode2 word (-1 none); tmax % 16 == 0
    int* lens;                // [B][nq]
    int* head;                // [B]
    int* count;               // [B]
    const float* softmax;     // [B][T][C] this chunk
    const uint8_t* clear_before;  // [B] or null
    int32_t* hit;             // [B]
    uint8_t* restart;         // [B] or null
    int32_t label[16];
    int label_len;
    float thres;
    int B, T, C, nq, tmax;
};
hipError_t launch_window_step(const WindowParams& p, hipStream_t st);
// the incremental form (summaries per queued chunk, window_device.h): softmax [B][T][C] -> per-frame words -> window tail
struct WindowIncParams {
    WindowTail win;
    uint8_t delta[256];       // by value: the standalone step takes the label per call
    const float* softmax;
    float thres;
    int B, T, C;
    // ragged chunks (kws_stream_feed_ragged): stream b's chunk has frames[b] <= T frames (softmax rows keep the stride T);
    // skip[b] != 0: no slot, no clear, hit 0, restart untouched.  frames == null: every stream has T frames.
    const int32_t* frames;
    const uint8_t* skip;
};
hipError_t launch_window_inc(const WindowIncParams& p, hipStream_t st);
hipError_t launch_window_reset(int B, int* head, int* count, hipStream_t st);
// ... of the streams with slots[b] != 0 only (kws_stream_recycle on a two-head manager: head 2's window)
hipError_t launch_window_reset_masked(const uint8_t* slots, int B, int* head, int* count, hipStream_t st);
// kws_stream_recycle: the streams with slots[b] != 0 become fresh streams -- state rows [L][b][H] zero, restart 0, window empty
// (head = count = 0), carry length 0.  carry_out != null: the handle leaves the lock-step carry layout ([B][n_carry] in carry_in)
// in the same pass -- the other streams' carried samples are copied to rows of fft - 1 floats and len_out = n_carry.
// carry_out == null: len_out is the per-stream length array in place (recycled streams only).
struct StreamRecycleParams {
    const uint8_t* slots;
    float* state;
    uint8_t* restart;
    int *head, *count;
    const float* carry_in;
    float* carry_out;
    int32_t* len_out;
    int n_carry, carry_out_stride, L, B, H;
};
hipError_t launch_stream_recycle(const StreamRecycleParams& p, hipStream_t st);

// PCM -> mel front-end (frontend_kernels.hip)
struct FrontendParams {
    const float* pcm;    // [B, n_samples - n_carry]  the new samples (float input)
    const int16_t* pcm_i16;   // fft_frontend.hip only: int16 PCM instead (scaled by 2^-15 as RingBuffer.get does), pcm unused
    // fft_frontend.hip only, the head of a stream-manager iteration fused into the same launch (gate != 0): vad over the new
    // samples -> silent / reset masks, and the next sample carry (the last n_next samples of [carry | chunk])
    int gate;
    int fft_blocks;      // set by launch_mel_fft400: transform blocks in the grid (multiple of 8)
    float vad_thres;
    const uint8_t* restart;
    uint8_t* silent;
    uint8_t* reset;
    float* next;
    int n_next;
    const float* carry;  // [B, n_carry] samples carried over from the previous chunk (n_carry may be 0)
    float* mel;          // [B, T, n_mel]
    const float* dft;    // [nf_tiles x (cos|sin) x parity][kc4][64][4]  A fragments: bins 0..fft/4 over the folded samples of one parity
    const float* melw;   // [mel_tiles][nf_tiles][direct|mirror][4][64]  A fragments of the mel basis, xl k map over k = 0..fft/4
    int n_samples, T, fft, hop, n_mel, nf_tiles, mel_tiles, kc4, B, n_carry;   // n_samples = n_carry + new samples
#ifdef KWS_FE_TIMING
    long long* timing;
#endif
    int mel_lo[4], mel_cnt[4], mel_off[4];   // fft_frontend.hip: per mel tile, first 4-bin group, number of groups (multiple of 4), offset of its fragments in melw (in groups)
    // fft_frontend.hip, the ragged stream-manager feed (frames != null; kws_stream_feed_ragged): every stream has its own
    // chunk length and carry length.  T = frames of n_max new samples after a full carry; frames t >= frames[b] are dead.
    const int32_t* lens;      // [B] new samples of stream b, clamped to [0, n_max]; null: n_max for every stream
    const int32_t* carry_len; // [B] carried samples of stream b (rows of carry_stride floats); null: n_carry for every stream
    int32_t* next_len;        // [B] out: samples carried into the next chunk (rows of next: fft - 1 floats)
    int32_t* frames;          // [B] out: frames of stream b in this chunk
    uint8_t* skip;            // [B] out: 1 = empty chunk, the iteration is skipped for this stream
    int n_max, carry_stride;  // row stride of the new samples / of carry (floats)
    // fft_frontend.hip, whole utterances of their own lengths (launch_features_fft400; kws_frontend_run_lengths): rows of n_max samples,
    // lens as above, T = frames of n_max samples.  n_mfcc > 0: mel is [B, T, 3 n_mfcc] (utils/mfcc.py:72-99)
    const float* dct;         // [mel_tiles][dct_tiles][64 lanes][4]  A fragments of D^T: lane (g, i), component e = D[filter 16 tile + 4g + e][16 ct + i]
    int n_mfcc, dct_tiles;    // coefficients (0: mel output), ceil(n_mfcc / 16)
    int power;                // mel output: 1 = |X|, 2 = |X|^2
    // fft_frontend.hip, the dataset's framing of whole utterances (centred != 0; kws_frontend_create_dataset): frame t is centred on
    // sample t * hop of an utterance reflected at both ends, under a Hann window; T_b = 1 + n_b / hop frames (0 for n_b <= fft / 2)
    int centred;
    float pre_emphasis;       // c: y[0] = x[0], y[i] = x[i] - c x[i-1] in front of the frames (0: none)
    const float* win;         // [fft] the window
};
hipError_t launch_mel_frontend(const FrontendParams& p, int B, hipStream_t st);
// fft 400 only (fft_frontend.hip): p.dft = twiddles [12][16] (cos, sin), p.melw = basis fragments [tile][group of its run][64]
hipError_t launch_mel_fft400(const FrontendParams& p, int B, hipStream_t st);      // honours p.pcm_i16 and p.gate
// ... B whole utterances with per-utterance lengths -> mel (p.power) or MFCC + deltas (p.n_mfcc > 0: two launches); float PCM, no gate;
// p.centred: the dataset's frames (DatasetFrames)
hipError_t launch_features_fft400(const FrontendParams& p, int B, hipStream_t st);
// ... the linear spectrum of the same utterances (kws_frontend_run_linear; the kEpiLinear epilogue): p.mel = spec [B, T, 201], and behind
// it one workgroup per utterance that writes frames_out [B] = T_b and energy_out [B] = sum_{t < T_b} sum_f spec^2
hipError_t launch_linear_fft400(const FrontendParams& p, int B, int32_t* frames_out, float* energy_out, hipStream_t st);
// ... and the reader's noise mix in front of the three feature epilogues (kws_frontend_augment; the Mixed tag): R rows of T frames, row r
// = features(spec[src[r]] + factor_r * noise_spec[noise[r]][start[r] ..]) into p.mel = out [R, T, feature].  augment_plan_kernel turns
// the row arrays into one PlanRow per row; how the spectra and the plan reach the feature launch through FrontendParams (no field of
// its own: the struct is the kernarg of every front-end kernel) is the business of bind_mix_rows / mix_rows in fft_frontend.hip alone.
constexpr int kPlanInts = 8;
struct PlanRow {     // clean row b and noise row k (-1: a zero row / nothing mixed in), first noise frame and how many from there on, the float factor, T_r
    int32_t src, noise, start, noise_avail, factor_bits, frames, pad[2];
};
static_assert(sizeof(PlanRow) == kPlanInts * sizeof(int32_t), "a plan row is kPlanInts ints");
struct AugmentRows {
    const int32_t *frames, *noise_frames;      // [B], [K]
    const float *energy, *noise_energy;        // [B], [K]
    const int32_t *src, *noise, *start;        // [R]
    const float* gain_db;                      // [R]
    int B, K, R, T, Tn;
    int32_t* plan;                             // PlanRow [R] followed by lens [R]
};
hipError_t launch_augment_fft400(const FrontendParams& p, const float* spec, const float* noise_spec, const AugmentRows& rows, hipStream_t st);
hipError_t launch_carry_tail(const float* carry, int n_carry, const float* chunk, int n_chunk, float* next, int n_next, int B,
                             hipStream_t st);

// launchers (gru_resident.hip, gru_kernels.hip)
bool gru_resident_supported(int hidden, int in_dim, bool first);
int gru_resident_kcx(int in_dim, bool first);
hipError_t launch_gru_layer_resident(const GruLayerParams& p, bool first, bool last, hipStream_t st);    // p.win.tab != null: with the window tail
bool gru_resident_takes_window(bool first, bool last);
hipError_t launch_gru_layer_generic(const GruLayerParams& p, int hidden, bool first, bool last,
                                    hipStream_t st);

// decode_kernels.hip
hipError_t launch_ctc_decode(int kind, const float* softmax, const int32_t* lengths, int B, int T, int C,
                             int lockout, float thres, float loose_thres, int32_t* words,
                             int32_t* counts, int max_words, hipStream_t st);
hipError_t launch_ctc_predict(const int32_t* words, const int32_t* counts, int B, int max_words,
                              const int32_t* label_digits, int label_len, int32_t* hit, hipStream_t st);
hipError_t launch_vad(const float* pcm, int B, int N, float thres, uint8_t* speech, float* abs_sum,
                      hipStream_t st);

// state_out = reset[b] ? 0 : state_in for [L,B,H] (a kws_step over zero frames; in-place allowed)
hipError_t launch_state_passthrough(const float* state_in, float* state_out, const uint8_t* reset, int32_t* prev_word, int L, int B, int H,
                                    hipStream_t st);
// ... and, fused into the same pass, the next sample carry: next [B,n_next] = the last n_next samples of [carry | chunk]
// (n_next = 0: none)
hipError_t launch_vad_gate(const void* pcm, int pcm_int16, int B, int N, float thres, float* pcm_f32, const uint8_t* restart,
                           uint8_t* silent, uint8_t* reset, const float* carry, int n_carry, float* next, int n_next, hipStream_t st);

// enroll_kernels.hip (ctc_device.h): the LDS one wave's utterance takes -- lp [T][8] and alpha [T][2 S_max + 1], in floats
__host__ __device__ inline size_t ctc_wave_lds_floats(int T, int S_max) { return (size_t)T * (8 + 2 * S_max + 1); }
inline size_t ctc_loss_lds_bytes(int T, int S_max) { return sizeof(float) * ctc_wave_lds_floats(T, S_max); }
// ... and an enrolment's workgroup: parameters, both Adam moments and the K slots' partial gradients ((H + 1) n floats each), K waves
inline size_t enroll_fit_lds_bytes(int H, int n, int K, int T, int S_max) {
    return sizeof(float) * ((size_t)(3 + K) * (H + 1) * n + (size_t)K * ctc_wave_lds_floats(T, S_max));
}
// logits [B,T,C]; seq_len / label_len [B], labels [B,S_max]: device copies the host side has range-checked; grad [B,T,C] or null
hipError_t launch_ctc_loss(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C,
                           int S_max, float* loss, float* grad, hipStream_t st);
// frame_loss_kernels.hip: the frame-wise softmax cross-entropy of utterance b over its labelled frames (targets >= 0, t < seq_len[b]),
// ce_b = sum_t w[y_t] (logsumexp(z_t) - z_t[y_t]) / W_b with W_b = sum_t w[y_t] (0 / 0 when W_b == 0; NaN when a live target lies
// outside [-1, C)), one workgroup per utterance.  Everything is device memory; seq_len is clamped to [0, T], nothing at t >= seq_len is read.
struct FrameLossParams {
    const float* logits;          // [B,T,C]
    const int32_t* seq_len;       // [B]
    const int32_t* targets;       // [B,T]: -1 no target, 0..C-1 (the blank, C-1, is a target like the others)
    const float* weight;          // [C] or null (all 1)
    float* ce;                    // [B] or null: ce_b alone
    float* loss;                  // [B] or null: loss[b] = (mix_prev != 0 ? mix_prev * loss[b] : 0) + mix_ce * ce_b
    float* grad;                  // [B,T,C] or null: scale * (w[y_t] / W_b) (softmax(z_t) - onehot(y_t)) ...
    float scale, mix_prev, mix_ce;
    int accumulate;               // ... 0: written to every row of the utterance (zeros where no target counts); 1: added to the rows with one
    int T, C;
};
hipError_t launch_frame_loss(const FrameLossParams& p, int B, hipStream_t st);
// align_kernels.hip: CTC forced alignment, one wave per utterance.  LDS: lp [T][8] floats | the Viterbi back-pointers, two 64-bit masks
// per frame | the path's state per frame, [T] int32 | and, only when the loss or the posteriors are asked for, alpha [T][2 S_max + 1]
// floats: 4 T (13 + (2 S_max + 1 if with_alpha)) bytes
inline size_t ctc_align_lds_bytes(int T, int S_max, bool with_alpha) {
    return (size_t)T * (sizeof(float) * 8 + 2 * sizeof(unsigned long long) + sizeof(int32_t) + (with_alpha ? sizeof(float) * (2 * S_max + 1) : 0));
}
// logits [B,T,C]; seq_len / label_len [B], labels [B,S_max]: device copies the host side has range-checked; states [B,T], spans
// [B,S_max,2], loss [B], post [B,T,S_max]: each or null; score [B]
hipError_t launch_ctc_align(const float* logits, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int C,
                            int S_max, int32_t* states, int32_t* spans, float* score, float* loss, float* post, hipStream_t st);
// beam_kernels.hip: CTC prefix beam search, one wave per utterance.  A beam of at most kBeamMax prefixes of at most kBeamRow labels
// (a row of bytes each, double-buffered); a frame has at most kBeamMax stays + kBeamMax x 7 extensions = kBeamCandidates candidates.
// LDS: lp [T][8] | the candidates' 64-bit keys | their merged-away stamps | the next beam's (lp_b, lp_nb, source) | the two string buffers
constexpr int kBeamMax = 32, kBeamRow = 64, kBeamCandidates = 8 * kBeamMax;
inline size_t ctc_beam_lds_bytes(int T) {
    return sizeof(float) * 8 * (size_t)T + kBeamCandidates * (8 + 4) + kBeamMax * 3 * 4 + 2 * kBeamMax * kBeamRow;
}
// logits [B,T,C]; seq_len [B] on the device or null (T); paths [B,K,L_max], lengths [B,K], log_prob [B,K]
hipError_t launch_ctc_beam(const float* logits, const int32_t* seq_len, int B, int T, int C, int W, int K, int L_max, int merge_repeated,
                           int32_t* paths, int32_t* lengths, float* log_prob, hipStream_t st);
struct EnrollFitParams {
    const float *nn, *logits1;                      // [E*K,T,H], [E*K,T,C]
    const int32_t *seq_len, *labels, *label_len;    // [E*K], [E*K,S_max], [E*K]
    float *W, *b, *mW, *mb, *vW, *vb;               // [E,H,n] / [E,n]: the new columns, their bias, Adam's moments
    float* loss_trace;                              // [iterations, E*K] or null
    float lr;
    int K, n, C, T, S_max, iterations, step0;       // step0: optimiser steps taken before this launch
};
hipError_t launch_enroll_fit(const EnrollFitParams& p, int hidden, int E, hipStream_t st);
// The fit on frame-wise targets (kws_enroll_fit_frames, frame_weight > 0): per step and slot loss = ctc_weight ctc_b + frame_weight ce_b
// with ce_b FrameLossParams' cross-entropy of the spliced rows over the C + n classes, and the gradient of that with respect to the new
// columns.  ctc_weight == 0: fit.labels / label_len are not read, fit.S_max is 0 and nothing in LDS grows with T.
struct EnrollFitFramesParams {
    EnrollFitParams fit;
    const int32_t* targets;       // [E*K,T]: -1 no target, 0..C+n-1 in the extended head's numbering
    const float* weight;          // [kMaxClasses]: the class weights (ones: none)
    float* frame_loss;            // [iterations, E*K] or null: ce_b alone
    float ctc_weight, frame_weight;
};
inline size_t enroll_fit_frames_lds_bytes(int H, int n, int K, int T, int S_max, bool ctc) {
    return ctc ? enroll_fit_lds_bytes(H, n, K, T, S_max) : enroll_fit_lds_bytes(H, n, K, 0, 0);
}
hipError_t launch_enroll_fit_frames(const EnrollFitFramesParams& q, int hidden, int E, hipStream_t st);

// Training of the stack (gru_train.hip: the two frame loops; train_kernels.hip: everything around them).  Every activation block is
// plain row-major [B*T, width] fp32, row = b * T + t; `live` [B*T] is 1 for t < seq_len[b].
//   packed weights of a layer, rebuilt on the device after every update (train_pack_kernel):
//     wx [I, 3H] the x rows of (Wg | Wc), columns r | u | c      wh [H, 3H] the h rows      wht [3H, H] = wh transposed      b3 [3H]
struct TrainForwardParams {
    const float* xg;        // [B*T, 3H] x-part products + bias (rows past seq_len: the bias)
    const float* wh;
    const int32_t* seq_len; // [B], device
    const uint8_t* drop;    // this layer's output-dropout mask, or null: the mask row of (b, t) is b * drop_bs + t * drop_ts, H bytes each --
    int drop_bs, drop_ts;   // one mask per frame [B*T, H]: (T, 1); one per stream held for all frames [B, H] (variational): (1, 0)
    float *ar, *au, *ac, *hp, *rh;  // the tape [B*T, H]: pre-activations of r, u, c, the state the frame started from, r o hp; rows t < seq_len only
    float* y;               // [B*T, H] what goes up: h' o mask / keep_prob, zero rows at t >= seq_len
    float keep_prob;
    int B, T;
};
struct TrainBackwardParams {
    const float* dy;        // [B*T, H] gradient with respect to y
    const float* wht;
    const int32_t* seq_len;
    const uint8_t* drop;
    int drop_bs, drop_ts;   // as the forward's
    const float *ar, *au, *ac, *hp;
    float* dhat;            // [B*T, 3H] pre-activation gradients dr^ | du^ | dc^, zero rows at t >= seq_len
    float keep_prob;
    int B, T;
};
hipError_t launch_gru_train_forward(const TrainForwardParams& p, int hidden, hipStream_t st);
hipError_t launch_gru_train_backward(const TrainBackwardParams& p, int hidden, hipStream_t st);
// The same launches from a carried state (kws_train_grad_state): one layer's rows [B, H] fp32, 16-byte aligned, either may be null
// and out may be in.  Forward: in = state_in[l] (null: zeros), out = state_out[l], the state after frame seq_len[b] - 1.  Backward:
// in = dstate_out[l] (null: zeros), out = dstate_in[l].  A stream with seq_len[b] == 0 copies in to out bitwise; rows b >= B are not written.
struct TrainStateIo { const float* in; float* out; };
struct TrainForwardStateParams : TrainForwardParams { TrainStateIo io; };
struct TrainBackwardStateParams : TrainBackwardParams { TrainStateIo io; };
hipError_t launch_gru_train_forward_state(const TrainForwardStateParams& p, int hidden, hipStream_t st);
hipError_t launch_gru_train_backward_state(const TrainBackwardStateParams& p, int hidden, hipStream_t st);
// out [M, N] = bias + a [M, K] . W, W(k, n) = w[k * swk + n * swn]; a row with live[row] == 0 reads as zeros (so out = bias there)
struct TrainRowsGemm {
    const float* a; int lda;
    const uint8_t* live;    // [M] or null
    const float* w; int swk, swn;
    const float* bias;      // [N] or null
    float* out; int ldo;
    int M, K, N;
};
hipError_t launch_train_rows_gemm(const TrainRowsGemm& p, hipStream_t st);
// One product of the weight-gradient launch: out [K, N] (at float offset `out` of a blob-layout image, row stride ldo) =
// sum over the live rows of a[row, 0..K)^T d[row, 0..N).  src: kWgradRows = a; kWgradOnes = a row of ones with K = 1 (a bias: the
// column sums); kWgradInput = the launch's x (the caller's features: the one operand that is not the handle's own memory).
// A wave owns 16 k x 64 n outputs ("unit"); the job's units are [unit0, unit0 + ceil(K / 16) * ceil(N / 64)).
enum { kWgradRows = 0, kWgradOnes = 1, kWgradInput = 2 };
struct TrainWgradJob {
    const float* a; const float* d;
    size_t out;
    int src, lda, K, ldd, N, ldo, unit0, pad;
};
// partial [chunks][P]: chunk c sums rows [c * chunk_rows, (c + 1) * chunk_rows); the jobs cover every float of the blob image
hipError_t launch_train_wgrad(const TrainWgradJob* jobs, int njobs, int units, const float* x, const uint8_t* live, int M, int chunk_rows,
                              int chunks, float* partial, size_t P, hipStream_t st);
constexpr int kTrainReduceSpan = 1024;      // floats of the blob one workgroup of the reduction sums
inline int train_reduce_blocks(size_t P) { return (int)((P + kTrainReduceSpan - 1) / kTrainReduceSpan); }
// grad[i] = sum_c partial[c][i] in chunk order; sumsq[block] = the block's sum of grad^2 (double, fixed tree)
hipError_t launch_train_reduce(const float* partial, int chunks, size_t P, float* grad, double* sumsq, hipStream_t st);
// the optimiser over the flat blob: norm = sqrt(sum of sumsq in block order); max_grad_norm > 0: g *= clip / max(norm, clip);
// adam != 0: TensorFlow's Adam with step size lr_t (bias corrections folded in by the host); else momentum 0.9 with use_nesterov
hipError_t launch_train_update(float* theta, float* m, float* v, const float* grad, const double* sumsq, int nblocks, size_t P, int adam,
                               float lr_t, float max_grad_norm, float* grad_norm_or_null, hipStream_t st);
struct TrainPackLayer { const float *wg, *bg, *wc, *bc; float *wx, *wh, *wht, *b3; int in; };
struct TrainPackParams { TrainPackLayer layer[8]; int L, H; };
hipError_t launch_train_pack(const TrainPackParams& p, hipStream_t st);
hipError_t launch_train_rowmask(const int32_t* seq_len, int B, int T, uint8_t* live, hipStream_t st);
// g [rows, C], ctc_loss_kernel's grad_logits of `logits`: each frame's occupancies renormalised to sum 1, then g *= s
hipError_t launch_train_scale(float* g, const float* logits, size_t rows, int C, float s, hipStream_t st);
// The cell wrappers in training (train_wrap_kernels.hip), rows [M, I]; live [M] as above: dead rows are written as zeros and not read.
//   forward: x^ = xn ibeta + igamma with xn = (in - mean) rstd, rstd = 1 / sqrt(var + 1e-5); ibeta (one float) and igamma [I] on the device
struct TrainLnForward {
    const float* in; const uint8_t* live; const float *ibeta, *igamma;
    float *xhat, *xn, *rstd;          // [M, I], [M, I], [M]
    int M, I;
};
hipError_t launch_train_ln_forward(const TrainLnForward& p, hipStream_t st);
//   backward: g [M, I] = dx^; din [M, I] = rstd (dn - mean(dn) - xn mean(dn o xn)) with dn = g ibeta, plus resid [M, I] where given;
//   din null: not wanted (layer 0).  gs [M]: sum_i g_i xn_i, the row's term of d ibeta
struct TrainLnBackward {
    const float *g, *xn, *rstd; const uint8_t* live; const float* ibeta; const float* resid;
    float *din, *gs;
    int M, I;
};
hipError_t launch_train_ln_backward(const TrainLnBackward& p, hipStream_t st);
// out = s (a + b) over n floats (n % 4 == 0, 16-byte aligned blocks); b null: out = s a; out may be a
hipError_t launch_train_residual(const float* a, const float* b_or_null, float s, float* out, size_t n, hipStream_t st);

// Training of the self-attention CTC model (attention_train_kernels.hip; host: api_attention_train.hip).  Activation blocks are
// row-major [B*T1, width] fp32, row = b * T1 + t with T1 = T'_max; t1 [B] (device) holds every utterance's T'_b, and a row is live
// iff t < t1[b].  Every weight product and weight gradient goes through the GEMM / wgrad / reduce / update kernels above.
//
// The keep decision of a dropout site (include/kws_amd.h, kws_attention_drop_keep): a counter hash, stateless in
// (seed, site, layer, b, head, row, col).  thr = floor(keep_prob * 2^32) computed in double by attn_drop_threshold.
enum { kAttnDropProb = 0, kAttnDropAtt = 1, kAttnDropFfn = 2 };
__host__ __device__ inline uint64_t attn_drop_threshold(float keep_prob) { return (uint64_t)((double)keep_prob * 4294967296.0); }
__host__ __device__ inline bool attn_drop_keep(uint64_t seed, int site, int layer, int b, int head, int row, int col, uint64_t thr) {
    const uint64_t ctr = ((uint64_t)site << 62) | ((uint64_t)layer << 58) | ((uint64_t)head << 52) | ((uint64_t)b << 28) |
                         ((uint64_t)row << 14) | (uint64_t)col;
    uint64_t x = seed + ctr * 0x9E3779B97F4A7C15ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (x >> 32) < thr;
}
struct AttnTrainDrop { uint64_t seed, thr; float keep_prob; int layer; };      // keep_prob == 1: no hash is evaluated
// xs [B*T1, c F]: the stacked rows of mel [B, T, F] (tlen [B]: frames T_b; pad frames, frames past T_b and dead rows read as 0)
hipError_t launch_attn_train_stack(const float* mel, const int32_t* tlen, const int32_t* t1, int B, int T, int T1, int F, int c, float* xs,
                                   hipStream_t st);
// x [B*T1, H] += pe[t] on live rows, 0 on dead rows
hipError_t launch_attn_train_addpe(float* x, const float* pe, const int32_t* t1, int B, int T1, int H, hipStream_t st);
// v [B*T1, N]: live rows relu(v) (relu != 0) or v, dead rows 0
hipError_t launch_attn_train_relu(float* v, const int32_t* t1, int B, int T1, int N, int relu, hipStream_t st);
// g [B*T1, N] = post > 0 on a live row ? g : 0 (tf ReluGrad on the taped output of the relu)
hipError_t launch_attn_train_relumask(float* g, const float* post, const int32_t* t1, int B, int T1, int N, hipStream_t st);
struct AttnTrainCore {
    const float* qkv;       // [B*T1, 3H]
    const int32_t* t1;
    float* att;             // [B*T1, H]   forward out / backward in: O = (P o keep / keep_prob) V
    float* lse;             // [B*T1, NH]  log-sum-exp of the scaled scores
    const float* datt;      // [B*T1, H]   backward: dO
    float* dsum;            // [B*T1, NH]  backward: rowsum(dO o O), written by the dq launch, read by the dk/dv launch
    float* dqkv;            // [B*T1, 3H]  backward out
    AttnTrainDrop drop;
    int B, T1, H, NH;
};
hipError_t launch_attn_train_core_forward(const AttnTrainCore& p, hipStream_t st);
hipError_t launch_attn_train_core_dq(const AttnTrainCore& p, hipStream_t st);
hipError_t launch_attn_train_core_dkv(const AttnTrainCore& p, hipStream_t st);
// u = (a o keep / keep_prob) + r on live rows (site's mask; 0 on dead rows) and the (count, mean, M2) of each 32-row tile of u
struct AttnTrainResid {
    const float *a, *r; const int32_t* t1; float* u; float4* part;      // part [B][ntile]
    AttnTrainDrop drop; int site, B, T1, H;
};
hipError_t launch_attn_train_resid(const AttnTrainResid& p, hipStream_t st);
// block layer norm over each utterance's [T'_b, H]: the tiles' partials merged in tile order; xn = (u - mean) rstd, y = xn g + bt; rstd [B]
struct AttnTrainLn {
    const float* u; const float4* part; const int32_t* t1; const float *g, *bt;
    float *xn, *y, *rstd; int B, T1, H;
};
hipError_t launch_attn_train_ln_forward(const AttnTrainLn& p, hipStream_t st);
// backward: dy = g1 + g2 (g2 null: g1), prod = dy o xn (the rows' terms of d beta and d gamma), the tiles' (sum dxn, sum dxn o xn)
// with dxn = dy gamma; then dx = rstd (dxn - mean(dxn) - xn mean(dxn o xn)) and ddrop = dx o keep / keep_prob of `site` (null: not wanted)
struct AttnTrainLnBwd {
    const float *g1, *g2, *xn, *rstd, *gamma; const int32_t* t1;
    float *dy, *prod; float2* sums;      // sums [B][ntile]
    float *dx, *ddrop;
    AttnTrainDrop drop; int site, B, T1, H;
};
hipError_t launch_attn_train_ln_bwd_sums(const AttnTrainLnBwd& p, hipStream_t st);
hipError_t launch_attn_train_ln_bwd_apply(const AttnTrainLnBwd& p, hipStream_t st);

// octbit_kernels.hip
hipError_t launch_octbit_matmul(const float* x, const int8_t* Wq, float scale_w, const float* bias,
                                float* out, int A, int K, int N, int per_row, float* range_ws,
                                hipStream_t st);

}  // namespace kws
