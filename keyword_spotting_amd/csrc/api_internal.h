// Host-side state and helpers shared by the C ABI translation units of libkws_amd.so: one api_*.hip per surface (model, step, ops,
// attention, attention_stream, window, frontend, stream -- which drives the two before it through kws_host --, enroll, bank, beam, train,
// attention_train), weight_pack.hip, selftest.hip.  What only the train handles share -- and the call ordering the enrolment handle takes
// from them -- is train_core.h / api_train_core.hip.  Never included by a kernel file: the kernel/host surface is kws_internal.h.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "kws_internal.h"
#include "attention_internal.h"

// Helpers shared across the host files; hidden, so the library's dynamic symbol table holds the C ABI and the kernels only.
#pragma GCC visibility push(hidden)
namespace kws_host {

extern thread_local std::string g_last_error;   // kws_last_error(); set by fail()
// kws_selftest is running on this thread: the temporary handles it creates do not recurse through KWS_SELFTEST=1.  A function,
// not a shared thread_local: a constant-initialised one read from another file would go through a TLS init hook that a hidden
// reference cannot resolve to null.
bool in_selftest();

// Live handles (model / front-end / window): a stream handle borrows all three, and its owner may destroy one of them
// first.  kws_stream_feed checks its borrowed pointers here -- pointer AND the serial it saw at kws_stream_create, so a new
// handle that reuses a freed address does not pass -- and fails with KWS_ERR_INVALID_ARGUMENT instead of touching freed
// memory.
unsigned long long live_register(const void* h);
void live_unregister(const void* h);
unsigned long long live_serial(const void* h);      // 0: not a live handle

int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

// scope guard of kws_model::in_call
struct BusyGuard {
    std::atomic<int>* flag;
    bool owned;
    explicit BusyGuard(std::atomic<int>& f) : flag(&f), owned(f.exchange(1, std::memory_order_acquire) == 0) {}
    ~BusyGuard() { if (owned) flag->store(0, std::memory_order_release); }
    BusyGuard(const BusyGuard&) = delete;
    BusyGuard& operator=(const BusyGuard&) = delete;
};
#define KWS_HIP(call)                                         \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) return kws_host::hip_fail(e_, #call); \
    } while (0)
// ... the same for a call that returns a KWS code, and a launcher's hipError_t as one (KWS_OK, or hip_fail(e, what))
#define KWS_TRY(call) do { const int rc_ = (call); if (rc_ != KWS_OK) return rc_; } while (0)
inline int hip_done(hipError_t e, const char* what) { return e == hipSuccess ? KWS_OK : hip_fail(e, what); }

// fp32 -> fp16 bits, round to nearest even (what v_cvt_f16_f32 does); the host compiler is clang: _Float16 is native
inline uint16_t f16_rne(float x) {
    const _Float16 h = static_cast<_Float16>(x);
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
inline float f16_value(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return static_cast<float>(h);
}
// v = hi + 2^-11 lo (gru_f16x3.hip, attention_f16x3.hip): the two fp16 pieces of a weight
inline void f16_split(float v, uint16_t* hi, uint16_t* lo) {
    *hi = f16_rne(v);
    *lo = f16_rne((v - f16_value(*hi)) * 2048.0f);
#ifdef KWS_EXP_F16_WLO_ZERO      // experiment builds only (tools/build_variant.sh wlo0 -DKWS_EXP_F16_WLO_ZERO): single-piece fp16 WEIGHTS in the
    *lo = 0;                     // f16x3 kernels -- the hardware check of the rounding model behind the "f16x1" decision
#endif
}

// The canonical weight blob (kws_weights_nbytes): per layer Wg [(in+H), 2H], bg [2H], Wc [(in+H), H], bc [H]; then
// Wfc [H, C] and bfc [C].  Offsets in floats, from the config alone.
struct BlobLayout {
    struct Layer { int in; size_t wg, bg, wc, bc; };
    Layer layer[8];
    size_t wfc, bfc, total;
};
BlobLayout blob_layout(const kws_config& c);
// ... and behind it, with the layer norm (kws_weights_nbytes_wrapped): per layer ibeta (1 float), igamma (I_l floats)
struct WrapLayout { size_t ibeta[8], igamma[8], total; };
WrapLayout wrap_layout(const kws_config& c, const kws_cell_wrappers& w);

struct LayerDev {
    int in_dim;
    // offsets (floats) into the single device allocation
    size_t wx_res, wx_gen, wh_gen, bias;   // wx_res: first-layer x-part, interleaved k map (resident kernel)
    int kcx_res, kcx_gen;
    bool resident_ok;
};

// Where the packer put each precision's tables in the handle's one device allocation (offsets in floats)
struct PackedWeights {
    std::vector<LayerDev> layers;
    size_t wfc_off = 0, bfc_off = 0;
    // bf16 stack: offsets (floats) of the packed bf16 A operands
    size_t bf_w[2] = {0, 0}, bf_wfc = 0;
    int bf_kx0 = 0;
    // f16x3 split stack: per layer the packed (hi, lo) fp16 A operands, and the projection's
    std::vector<size_t> f16_w;
    size_t f16_wfc = 0;
    int f16_kx0 = 0;
    bool f16_generic = false;        // hidden != 128: the L2-streaming kernels (gru_f16x3_generic.hip)
    // int8 ("octbit") variant: per quantised layer the packed int16 couples + 127*colsum, and the projection
    struct OctLayer { bool quantised = false; size_t wg = 0, wc = 0, b127 = 0; float scale_g = 0.f, scale_c = 0.f; };
    std::vector<OctLayer> oct;
    size_t oct_wfc = 0, oct_b127fc = 0;
    float oct_scale_fc = 0.f;
    // cell wrappers (kws_create_wrapped, fp32 generic kernels): per layer the layer norm's igamma padded to the k-groups of the
    // x-part (16 * kcx_gen / 4 floats, zero past I_l) and its ibeta
    std::vector<size_t> ln_igamma;
    std::vector<float> ln_ibeta;
    // second class head (kws_create_heads): its fragments and padded bias, behind every other table
    size_t wfc2_off = 0, bfc2_off = 0;
};
// (config, canonical blob [+ the wrapper tables of wrap_layout]) -> the device image of every table the config's precision
// launches with, and where each one is.  KWS_OK, or the error code with kws_last_error() set.  Host code only.
// num_classes2 > 0: Wfc2 [H, C2] and bfc2 [C2] follow in the blob (kws_weights_nbytes_heads) and are packed as the first head is.
int pack_weights(const kws_config& cfg, const kws_cell_wrappers& wrap, const float* blob, PackedWeights* pk, std::vector<float>* image,
                 int num_classes2 = 0);

// What kws_step_heads adds to a step: the top layer's rows and the outputs of each head (on[i]: head i is wanted)
struct HeadsArgs {
    float* nn_outputs = nullptr;
    kws_head_io head[2] = {};
    bool on[2] = {false, false};
    // a two-head stream manager's iteration (kws_step_heads_window, kws_stream_feed on a kws_stream_create_heads handle; filled by
    // heads_window_args): heads_window_kernel follows the top layer in dense_heads_kernel's place, on these two windows' tails; head[i]
    // gives window i's threshold and an optional softmax; frames (StepArgs::seq_len too) / skip: the ragged feed's per-stream frame
    // counts and skip flags, or null.  With T == 0 it is the step's only launch besides the state pass
    bool window = false;
    kws::WindowTail win[2] = {};
    const int32_t* frames = nullptr; const uint8_t* skip = nullptr;
    int32_t* hit = nullptr; uint8_t* restart = nullptr;
    // a bank of enrolled heads (kws_step_bank, kws_step_bank_window, a kws_stream_create_bank manager): head 2 of stream b comes from bank
    // slot user[b] instead of the handle's own second head -- bank_heads_kernel / bank_heads_window_kernel in the two kernels' places
    const kws::BankRef* bank = nullptr;
    // ... and the bank's slot table once kws_bank_set_keyword was called on it (bank_slots): the keyword forms of the two kernels
    const kws::BankSlotKeyword* bank_slots = nullptr;
};
// The arguments of one kws_step (include/kws_amd.h), and what the stream manager adds to them
struct StepArgs {
    const float *mel = nullptr, *state_in = nullptr;
    float *logits = nullptr, *softmax = nullptr, *state_out = nullptr;
    const int32_t* seq_len = nullptr;
    const uint8_t* reset_mask = nullptr;
    int8_t* tokens = nullptr;
    int32_t* prev_word = nullptr;
    float decode2_thres = 0.f;
    int B = 0, T = 0;
    hipStream_t stream = nullptr;
    const kws::WindowTail* wt = nullptr;   // the stream manager's decode window, to ride at the end of the last layer's launch
    const HeadsArgs* heads = nullptr;      // kws_step_heads: no layer is `last`, the heads follow the top layer (kws_model::Tail)
    bool locked = false;                   // the caller (kws_stream_feed) already holds the handle and has ordered the stream
};

// api_step.hip: one step (kws_step and the stream manager), whether the launch plan of `a` (plan_step; a.wt offered) lets the last
// launch take the window tail, and the ordering of a call against the handle's previous one
int step_impl(kws_handle h, const StepArgs& a);
bool step_takes_window(kws_handle h, const StepArgs& a);
int call_enter(kws_handle h, hipStream_t st);
int call_leave(kws_handle h, hipStream_t st);
// ... device blocks that only grow, `have` their common size in the owner's unit: when want > *have the device is synchronised (the
// old blocks may still be in use), every block is freed and allocated anew (fine: fine-grained memory), *have = want and
// scratch_allocs counts ONE growth.  KWS_OK, the error of `what`, or -- fine only -- api_step.hip's internal kNoFineGrainedMemory
int grow_device(kws_model* h, size_t* have, size_t want, bool fine, std::initializer_list<std::pair<void**, size_t>> blocks, const char* what);

// api_window.hip: the one label rule (digits 1..9, else the error); the n digits go to `digits` as numbers when it is given
int label_digits(const char* label, int n, int32_t* digits);
// ... the LDS one incremental window step over chunks of T frames needs, and what a workgroup may hold
size_t window_inc_lds_bytes(int T, int nq);
constexpr size_t kWindowIncLdsMax = 160 * 1024;
// ... binds `label` to the window's incremental state (the queued summaries are label-specific)
int window_bind_label(kws_window* w, const char* label);
// ... the matcher itself: the KMP automaton of `label` (n digits 1..9, n <= 15) over emitted words, delta[q * 16 + w]
void window_label_delta(const char* label, int n, uint8_t* delta);
// ... the incremental window as kernel arguments: of window_inc_kernel, or of the tail of a GRU launch (StepArgs::wt)
kws::WindowTail window_tail_params(kws_window* w, const uint8_t* clear_before, int32_t* hit, uint8_t* restart);

// api_step.hip: the HeadsArgs of a two-head manager's iteration on windows w1 and w2 (labels bound by the caller), for a StepArgs
// with heads = the result: the stack planned as a heads step, then heads_window_kernel.  The caller adds softmax / frames / skip.
HeadsArgs heads_window_args(kws_window* w1, kws_window* w2, const uint8_t* clear_before, int32_t* hit, uint8_t* restart);
// ... the refusals a pair of windows shares between kws_stream_create_heads and kws_step_heads_window (class counts, batch, LDS)
// bank != null: head 2 has the bank's C + n_new classes and the launch stages the group's columns too
int heads_window_check(const kws_model* h, const kws_window* w1, const kws_window* w2, int B, int T, const kws_bank* bank = nullptr);

// api_stream.hip: kws_stream_create (window2 == null), kws_stream_create_heads and kws_stream_create_bank (bank and user given; checked
// by the caller with bank_serves); `who` names the entry point in the refusals
int stream_create_impl(const char* who, kws_handle model, kws_frontend_handle frontend, kws_window_handle window, kws_window_handle window2,
                       int B, int max_chunk_samples, float vad_thres, const char* label, const char* label2, float* state, uint8_t* restart,
                       kws_stream_handle* out, kws_bank* bank = nullptr, const int32_t* user = nullptr);
// api_bank.hip: the refusal of a bank that is not alive or was created for another hidden size / class count than the model's
int bank_serves(const kws_bank* bank, const kws_model* h, const char* who);
// ... the bank and a launch's per-stream slots as kernel arguments
kws::BankRef bank_ref(const kws_bank* bank, const int32_t* user);
// ... its slot table for the keyword forms of the bank kernels, or null while no slot was ever given a keyword (the plain kernels)
const kws::BankSlotKeyword* bank_slots(const kws_bank* bank);

// api_enroll.hip: what every CTC entry point does with its host arrays (kws_ctc_loss, kws_enroll_fit, kws_train_grad / _step).
// seq_len / label_len / labels against the shape; classes = the class count the labels index (blank = classes - 1)
int check_labels(const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int S_max, int classes);
bool misaligned(const void* p);      // not 4-byte aligned
// ... [seq_len | label_len | labels] as the one block that travels to the device
void pack_ints(const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int S_max, std::vector<int32_t>* out);

// api_frame_loss.hip: frame-wise targets (kws_frame_loss, kws_[attention_]train_*_frames).  The refusals of a kws_frame_targets for C
// classes, of host class weights (null: none) and of seq_len against T alone
int check_frame_targets(const kws_frame_targets* ft, int C);
int check_class_weight(const float* w, int C);
int check_seq_len(const int32_t* seq_len, int B, int T);
// ... the class weights (null: ones) as kMaxClasses floats behind the ints of an upload block
void append_class_weights(const float* w, int C, std::vector<int32_t>* ints);
// ... and what a train handle's frame_loss launch takes from ft (frame_weight > 0) for a batch of B: the targets, ce_b's destination, the
// gradient's scale frame_weight / B, and -- behind a CTC term -- accumulate mode with loss[b] = ctc_weight loss[b] + frame_weight ce_b.
// The caller adds logits, seq_len, weight, loss, grad, T and C
kws::FrameLossParams train_frame_term(const kws_frame_targets& ft, int B);

// api_attention.hip: the canonical blob of the attention model (offsets in floats) and the refusals of its config, shared with the
// train handle (api_attention_train.hip)
enum { kQkvW, kQkvB, kLnaBeta, kLnaGamma, kW1, kB1, kW2, kB2, kLnbBeta, kLnbGamma, kLayerParts };
struct AttnLayout {
    size_t w_in, b_in, layer[8][kLayerParts], w_out, b_out, total;
};
AttnLayout attn_layout(const kws_attention_config& c);
bool attn_config_ok(const kws_attention_config* c, int* code);      // false: *code is the failure, kws_last_error names the field
// ... kws_attention_run for a caller that already holds the handle (kws_attention::in_call; api_attention_stream.hip): the scratch of
// a call shape and the staging block of the stream managers (both only grow; growing synchronises), the ordering of a call against
// the handle's previous one (attn_call_enter waits for last_done on a stream switch, attn_call_leave records it), and the model's
// 2 + 3L launches themselves -- arguments validated by the caller, the scratch reserved
int attn_reserve_locked(kws_attention* h, int B, int T_max);
int attn_stage_reserve_locked(kws_attention* h, size_t bytes);
int attn_call_enter(kws_attention* h, hipStream_t st);
int attn_call_leave(kws_attention* h, hipStream_t st);
int attn_run_locked(kws_attention* h, const float* mel, const int32_t* lengths, int B, int T_max, float* logits, float* softmax,
                    hipStream_t st);

// api_frontend.hip: the 400-point FFT kernel takes a launch of B x T frames (else the dense-DFT kernel, which has magnitude mel only)
bool frontend_takes_fft400(const kws_frontend* h, int B, int T);
// ... the refusal of `what` ("per-stream chunk lengths") on a handle whose launches go to the dense-DFT kernel
int frontend_needs_fft400(const kws_frontend* h, const char* what);
// ... the refusal of a KWS_FRAMES_DATASET handle by the streaming entry point `who`
int frontend_needs_deploy_frames(const char* who);
// ... `seed` (or zeros) with everything that comes from the handle and the call shape; the samples, lengths and outputs are the caller's
kws::FrontendParams frontend_params(const kws_frontend* h, bool fft400, int B, int T, const kws::FrontendParams* seed = nullptr);
// ... mel of [carry | chunk]; `gate` (FFT kernel only): its gate fields ride along -- pcm_i16 (read in place of chunk), vad, masks, next carry
int frontend_run_impl(kws_frontend_handle h, const float* carry, int n_carry, const float* chunk, int n_chunk, int B, float* mel,
                      void* stream, const kws::FrontendParams* gate = nullptr);

}  // namespace kws_host
#pragma GCC visibility pop

// A bank of enrolled heads (api_bank.hip): `capacity` slots of n_new columns [H, n_new] + bias for a model of hidden size H whose
// trained head has C classes.  One device allocation, fixed for the handle's life; kws_bank_set is a stream-ordered copy into it.
struct kws_bank {
    int H = 0, C = 0, n_new = 0, capacity = 0;
    float* store = nullptr;          // Wn [capacity,H,n_new] | bn [capacity,n_new]
    float *Wn = nullptr, *bn = nullptr;
    // Per-slot keywords (kws_bank_set_keyword): the device table [capacity] behind bn in `store`, the host's copy of what each slot was
    // last given (n_used, own, the label for kws_bank_get_keyword), and whether any slot ever got one -- from then on every launch on
    // the bank takes the keyword form of its kernel.
    kws::BankSlotKeyword* slots = nullptr;
    struct Keyword { int n_used = 0; bool own = false; char label[16] = {0}; };
    std::vector<Keyword> keyword;
    bool keywords_ever = false;
    std::atomic<int> in_call{0};
};

struct kws_model {
    kws_config cfg;
    kws_cell_wrappers wrap = {0, 0};
    bool wrapped = false;            // a wrapper is on: the fp32 generic kernels' wrapped instantiations, never the resident ones
    int device = 0;
    int kernel_kind = KWS_KERNEL_AUTO;
    kws_host::PackedWeights pk;
    float* d_weights = nullptr;
    uint32_t* oct_aq = nullptr;      // int8 activation exchange [groups][2][16][128]
    float2* oct_range = nullptr;     // [groups*16]
    int32_t* oct_prev = nullptr;     // [B] copy of prev_word
    size_t oct_groups = 0;
    int num_classes2 = 0;            // > 0: a heads handle (kws_create_heads); kws_step_heads serves both heads
    int32_t* heads_prev = nullptr;   // [2][heads_groups * 16] copies of the two heads' prev_word (dense_heads.hip)
    size_t heads_groups = 0;
    // Inter-layer seams.  ONE device allocation per memory kind that only ever grows (kws_reserve or the first call that
    // needs more); each kws_step carves the buffers of its launch layout out of it -- sequential (1-2 buffers of T
    // frames), layers overlapped on HIP streams (2(L-1) buffers of a time block), layer-pipelined (L-1 fine-grained
    // buffers) -- so alternating layouts never reallocates, and a step within the reserved size never synchronises.
    struct Arena { char* base = nullptr; size_t bytes = 0; };
    Arena arena, arena_fine;
    int scratch_allocs = 0;          // (re)allocations so far; each one synchronised the device (kws_scratch_stats)
    float4* scratch[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // this call's seams: l -> scratch[l % nscratch]
    int nscratch = 0;
    bool pipe_disabled = false;      // fine-grained memory unavailable, or a pipelined launch timed out: never the pipelined launch again
    // time-blocked overlap of the layers on separate HIP streams (step_overlapped)
    hipStream_t lane_stream[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> ovl_events;
    hipEvent_t ovl_tail[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // end of the last overlapped call, per lane
    bool ovl_tail_valid = false;     // the last call was overlapped: the next one waits for ovl_tail before it touches the seams
    // layer-pipelined launch of the generic kernel
    int num_cus = 0;
    int* pipe_ready = nullptr;       // [L][groups] frames published
    size_t pipe_groups = 0;
    int* pipe_error_host = nullptr;  // mapped pinned flag the kernel raises if a wait times out
    int* pipe_error_dev = nullptr;
    // One host thread at a time per handle (kws_amd.h): a second thread that enters kws_step / kws_reserve / kws_kernel_times
    // while another is inside gets KWS_ERR_BUSY instead of racing on the scratch arena and the profiling slots.
    std::atomic<int> in_call{0};
    // The seams (and the stream managers' staging below) are shared by all calls of the handle.  Every call records
    // `last_done` on its stream when its last launch is queued; a call that arrives on ANOTHER HIP stream than the one before
    // makes its stream wait for that event (device-side ordering: no host stall, nothing that touches other handles' work,
    // legal under stream capture).  The common path -- same stream as before -- pays one hipEventRecord.
    hipStream_t last_stream = nullptr;
    bool last_stream_valid = false;
    hipEvent_t last_done = nullptr;
    // Staging of the stream managers that borrow this handle (kws_stream_feed): widened PCM, mel, softmax and the two masks
    // of ONE chunk.  They live only inside a feed, feeds of one handle are ordered (one host thread at a time, stream
    // switches ordered by last_done), so every manager on the handle carves the same block: M managers cost M x their
    // per-stream state, not M x a chunk's intermediates.  Grows at kws_stream_create only.
    Arena stage;
    // profiling
    bool profiling = false;
    struct Pending { int slot; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
    std::vector<float> ms_sum;
    std::vector<int32_t> launches;
    // kernel the last kws_step launched per profiling slot, as a small tag: the name is only formatted when somebody asks
    // (kws_last_launch, kws_selftest) -- not on the launch path, where a 22-frame call is ~100 us of device time
    enum LaunchFamily : uint8_t { kNone = 0, kBf16Stack, kF16x3, kPipelined, kOctbit, kResident, kGeneric, kF16x3Generic, kF16x3Pipelined,
                                  kGenericWrapped, kPipelinedWrapped };
    // What follows the top layer inside its profiling slot: nothing (also every layer below; a kws_step_heads call that wants no head and
    // no nn_outputs), the class epilogue in the layer's own kernel -- alone, or with the stream manager's window step behind it --, or
    // one more launch: the int8 projection, the two class heads, the two heads with their windows
    enum Tail : uint8_t { kTailNone = 0, kTailEpilogue, kTailWindow, kTailOctbitFc, kTailDenseHeads, kTailHeadsWindow, kTailBankHeads, kTailBankWindow,
                          kTailBankKeywordHeads, kTailBankKeywordWindow };
    struct LaunchTag {
        uint8_t family = kNone, kx = 0, first = 0, tail = kTailNone;
        bool last() const { return tail == kTailEpilogue || tail == kTailWindow; }      // the kernels' template argument
    };
    LaunchTag launch_tag[8];
    std::string launch_name(int slot) const {
        const LaunchTag& t = launch_tag[slot];
        const uint8_t f = t.family;
        const char* layer = f == kF16x3 ? "gru_layer_f16x3" : f == kF16x3Generic ? "gru_layer_f16x3_generic" : f == kResident ? "gru_layer_resident" :
                            f == kGeneric || f == kGenericWrapped ? "gru_layer_generic" : nullptr;
        const char* stack = f == kPipelined || f == kPipelinedWrapped ? "gru_stack_generic_pipelined" : f == kF16x3Pipelined ? "gru_stack_f16x3_pipelined" : nullptr;
        const char* wrapped = f == kGenericWrapped || f == kPipelinedWrapped ? ", wrapped" : "";
        char nm[96] = "";
        if (layer) snprintf(nm, sizeof(nm), "%s<%d, %s, %s%s>", layer, t.kx, t.first ? "true" : "false", t.last() ? "true" : "false", wrapped);
        else if (stack) snprintf(nm, sizeof(nm), "%s<%d%s> (all %d layers, one launch)", stack, t.kx, wrapped, cfg.num_layers);
        else if (f == kOctbit) snprintf(nm, sizeof(nm), "gru_layer_octbit_kernel");
        std::string out = t.family == kBf16Stack ? std::string(kws::gru_stack_bf16_kernel_name(pk.bf_kx0, cfg.num_layers)) : std::string(nm);
        switch (t.tail) {      // what ran behind the layer is timed in its slot
            case kTailWindow: out += " + window tail"; break;
            case kTailOctbitFc: if (t.family == kOctbit) out += " + octbit_fc_kernel"; break;      // (a one-layer int8 model's fp32 layer is named alone)
            case kTailDenseHeads: out += " + dense_heads_kernel<" + std::to_string(cfg.hidden / 16) + ">"; break;
            case kTailHeadsWindow: out += " + heads_window_kernel<" + std::to_string(cfg.hidden / 16) + ">"; break;
            case kTailBankHeads: out += " + bank_heads_kernel<" + std::to_string(cfg.hidden / 16) + ">"; break;
            case kTailBankWindow: out += " + bank_heads_window_kernel<" + std::to_string(cfg.hidden / 16) + ">"; break;
            case kTailBankKeywordHeads: out += " + bank_keyword_heads_kernel<" + std::to_string(cfg.hidden / 16) + ">"; break;
            case kTailBankKeywordWindow: out += " + bank_keyword_window_kernel<" + std::to_string(cfg.hidden / 16) + ">"; break;
        }
        return out;
    }
};

struct kws_attention {
    kws_attention_config cfg;
    int precision = KWS_FP32;         // KWS_FP32 or KWS_F16X3: which GEMM image d_w holds and which GEMM kernels run
    std::vector<float> blob;          // the canonical blob (the self-test's host loop reads it)
    std::vector<float> pe;            // [pe_rows][H]
    int pe_rows = 0, KE = 0;
    float* d_w = nullptr;             // packed weights, biases, LN tables and the positional table: one allocation
    kws::AttnLayerW layer[8];
    const float4* w_in = nullptr;
    const float *b_in = nullptr, *w_out = nullptr, *b_out = nullptr, *d_pe = nullptr;
    char* scratch = nullptr;          // activations and LN partials; only grows
    size_t scratch_bytes = 0;
    // Staging of the stream managers that borrow this handle (kws_attention_stream_feed): one chunk's mel, the softmax, the gate's masks
    // and the lengths the model runs over.  They live only inside a feed and feeds of one handle are ordered, so every manager on the
    // handle carves the same block, as the GRU managers do with kws_model::stage.  Grows at kws_attention_stream_create only.
    char* stage = nullptr;
    size_t stage_bytes = 0;
    std::atomic<int> in_call{0};
    hipStream_t last_stream = nullptr;
    bool last_stream_valid = false;
    hipEvent_t last_done = nullptr;
};

struct kws_window {
    int B = 0, nq = 0, tmax = 0, tmax_pad = 0, C = 0;
    float thres = 0.f;
    int8_t* words = nullptr;
    int *lens = nullptr, *head = nullptr, *count = nullptr;
    // the incremental form (kws_window_step_incremental, kws_stream_feed): a summary per queued chunk instead of its frames
    // (window_device.h); a state of its own -- a window is driven through one of the two entry points, not both
    uint8_t* inc_tab = nullptr;      // [B][nq][32]  tab | ftab
    uint32_t* inc_meta = nullptr;    // [B][nq]
    int *inc_head = nullptr, *inc_count = nullptr;
    uint8_t* inc_delta_dev = nullptr;   // [256] label matcher of the bound label
    uint8_t inc_delta[256] = {0};
    char inc_label[17] = {0};
    bool inc_bound = false;
};

struct kws_stream {
    kws_model* model = nullptr;
    kws_frontend* fe = nullptr;
    kws_window* win = nullptr;
    kws_window* win2 = nullptr;      // kws_stream_create_heads: head 2's window (null: a plain manager, head 1 through the fused tail)
    unsigned long long model_serial = 0, fe_serial = 0, win_serial = 0, win2_serial = 0;   // live_serial() of the borrowed handles at create
    int B = 0, max_chunk = 0, tmax = 0, n_carry = 0, cur = 0;
    float vad_thres = 0.f;
    char label[17] = {0};
    char label2[17] = {0};           // win2's
    kws_bank* bank = nullptr;        // kws_stream_create_bank: head 2 of stream b from bank slot user[b] (null: the model's own second head)
    unsigned long long bank_serial = 0;
    const int32_t* user = nullptr;   // caller-owned [B], borrowed like state / restart
    float* state = nullptr;          // caller-owned [L,B,H]
    uint8_t* restart = nullptr;      // caller-owned [B]
    float* carry[2] = {nullptr, nullptr};   // [B, fft - 1] each: the carried samples ping-pong (the only device memory a manager owns)
    // Carry layout.  Lock-step (ragged == false): every stream carries n_carry samples, rows of n_carry floats.  Ragged (from the
    // first kws_stream_feed_ragged / kws_stream_recycle until kws_stream_reset): stream b carries carry_len[cur][b] samples, rows
    // of fft - 1 floats; the lengths ping-pong with the samples.
    bool ragged = false;
    int32_t* carry_len[2] = {nullptr, nullptr};   // [B] each
    // one chunk's intermediates, carved out of the MODEL handle's staging block (kws_model::stage) at every feed by stream_carve
    // (api_stream.hip), which also sizes them at kws_stream_create:
    size_t stage_bytes = 0;
    float* pcm_f32 = nullptr;        // [B, max_chunk]  int16 input widened here (front-ends other than the 400-point FFT, sub-frame chunks)
    float* mel = nullptr;            // [B, tmax, n_mel]
    float* softmax = nullptr;        // [B, tmax, C]; not carved for a two-head manager (its words never leave the kernel)
    uint8_t* silent = nullptr;       // [B]
    uint8_t* reset = nullptr;        // [B]
    int32_t* frames = nullptr;       // [B] int32  frames of each stream's chunk (ragged feed)
    uint8_t* skip = nullptr;         // [B]        empty chunk: iteration skipped (ragged feed)
};

struct kws_frontend {
    kws_frontend_config cfg;
    // kws_frontend_create_features: what the handle produces (kws_frontend_create: mel, power 1)
    int kind = KWS_FEAT_MEL, power = 1, n_mfcc = 0;
    // kws_frontend_create_dataset: how the utterance is framed (kws_frontend_create_features: KWS_FRAMES_DEPLOY, 0)
    int framing = KWS_FRAMES_DEPLOY;
    float pre_emphasis = 0.f;
    bool plain() const { return kind == KWS_FEAT_MEL && power == 1 && framing == KWS_FRAMES_DEPLOY; }     // what the streaming paths take
    // pack_frontend_tables (api_frontend.hip): the kernel tables in the one device allocation (offsets in floats), and the two bases
    float* d_tables = nullptr;
    size_t dft_off = 0, melw_off = 0;         // frontend_kernels.hip tables (every fft_size)
    size_t fft_tw_off = 0, fft_mel_off = 0;   // fft_frontend.hip tables (fft_size 400 only)
    int mel_lo[4] = {0, 0, 0, 0}, mel_cnt[4] = {0, 0, 0, 0}, mel_off[4] = {0, 0, 0, 0};
    bool use_fft = false;          // fft_size 400 without KWS_FRONTEND_DENSE=1
    int nf_tiles = 0, mel_tiles = 0, kc4 = 0, dct_tiles = 0;
    std::vector<float> basis;      // [n_mel][fft/2+1]
    size_t dct_off = 0;            // fft_frontend.hip: A fragments of D^T (MFCC only)
    std::vector<float> dct;        // [n_mel][n_mfcc]
    size_t win_off = 0;            // fft_frontend.hip: the Hann window (KWS_FRAMES_DATASET only)
    std::vector<float> window;     // [fft]
};
