// C ABI of libkws_amd.so (include/kws_amd.h): kws_step -- launch selection, the seam arenas, profiling slots, the launches.

#include "api_internal.h"
#include "launch.h"

using namespace kws_host;

namespace {
using M = kws_model;
// ---- the launch plan: what a kws_step of shape (B, T) launches, decided once ------------------------------------------
#ifndef KWS_OVERLAP_MIN_T
#define KWS_OVERLAP_MIN_T 64
#endif
struct SeamLayout { int nbuf; size_t bytes_each; bool fine; };
constexpr int kNoFineGrainedMemory = 1;      // grow_device, provision: internal, never returned through the ABI
using Tail = kws_model::Tail;

// What a step asks of the plan: its shape, kws_set_profiling's switch (a field, so that kws_reserve can ask for both answers), and
// what the caller wants behind the stack -- the class epilogue (kws_step), the window tail where it fits (StepArgs::wt), or, for a
// kws_step_heads call, dense_heads_kernel, heads_window_kernel or nothing.
struct PlanRequest {
    int B, T;
    bool profiling;
    Tail want;
    bool heads() const { return want != M::kTailEpilogue && want != M::kTailWindow; }
};
PlanRequest plan_request(const kws_model* h, const StepArgs& a) {
    Tail want = M::kTailEpilogue;
    if (a.heads) {
        const bool bank = a.heads->bank != nullptr;      // head 2 from a bank of enrolled columns: the bank kernels in the two kernels' places
        const bool keywords = bank && a.heads->bank_slots;      // ... and their keyword forms once a slot of the bank has a keyword of its own
        want = a.heads->window ? (keywords ? M::kTailBankKeywordWindow : bank ? M::kTailBankWindow : M::kTailHeadsWindow) :
               (a.heads->on[0] || a.heads->on[1] || a.heads->nn_outputs) ?
                   (keywords ? M::kTailBankKeywordHeads : bank ? M::kTailBankHeads : M::kTailDenseHeads) : M::kTailNone;
    }
    else if (a.wt && a.wt->nq <= kws::kWinTailMaxChunks) want = M::kTailWindow;
    return {a.B, a.T, h->profiling, want};
}

struct StepPlan {
    // kStack: the whole stack in one launch, no seam (bf16).  kSequential: one launch per layer.  kPipelined: all L x groups
    // workgroups in one grid, layer l consuming frame t of layer l-1 as soon as it is published.  kOverlapped: the per-layer
    // kernels on separate HIP streams over time blocks (step_overlapped).
    enum Layout : uint8_t { kZeroFrames, kStack, kSequential, kPipelined, kOverlapped } layout;
    kws_model::LaunchTag tag[8];   // per profiling slot, exactly what kws_last_launch is to report after this step; empty: no launch
    Tail tail;                     // what follows the top layer: the tail of the last tagged slot (every other slot has none)
    SeamLayout seams;
    int nb, Tb;                    // kOverlapped only: time blocks and their length
    bool streaming;                // some layer addresses its seam through 32-bit buffer offsets (the 2 GiB check)
};

// The one place that decides kernel family, launch layout, what follows the top layer and the seams.  Pure: reads the handle, touches
// nothing, and nobody writes to its result.  A heads step (PlanRequest::heads) is one launch per layer, none of them `last`, the top
// layer's seam among the buffers; the overlapped and layer-pipelined layouts stay with kws_step.
StepPlan plan_step(const kws_model* h, const PlanRequest& r) {
    const int B = r.B, T = r.T;
    const bool profiling = r.profiling, heads = r.heads();
    // KWS_NO_PIPELINE=1: never the layer-pipelined launch -- what a device without fine-grained memory gets (pipe_disabled), for A/B
    // runs and for the tests of the layouts that take its place (tests/test_gpu_wrapped.py)
    static const bool no_pipe = [] { const char* e = getenv("KWS_NO_PIPELINE"); return e && e[0] == '1'; }();
    static const bool no_tail = [] { const char* e = getenv("KWS_NO_WINDOW_TAIL"); return e && e[0] == '1'; }();     // A/B switch (tools/bench_e2e.py)
    const kws_config& c = h->cfg;
    const int L = c.num_layers, H = c.hidden;
    StepPlan p = {};
    if (B <= 0 || T <= 0) return p;
    const long long groups = kws::groups_of(B);
    const bool fits = h->num_cus > 0 && groups * L <= h->num_cus;      // all L x groups workgroups on the chip at once, one per CU
    // The tail rides only where the last layer's kernel has a tail instantiation (below, per family), for chunks and windows its LDS
    // staging holds, and with one group per workgroup: it is ~2 us of latency-bound work at the end of a group.  At the end of the
    // launch that replaces a ~4 us launch of its own; in a persistent workgroup it would sit between two groups, on the critical
    // path once per group (measured, bf16, 16384 streams: 0.349-0.359 ms per chunk with the tail against 0.338-0.340 with
    // window_inc_kernel behind the stack).  Everywhere else window_inc_kernel follows the stack.
    const bool window = r.want == M::kTailWindow && !no_tail && T <= kws::kWinTailMaxFrames && groups <= (h->num_cus > 0 ? h->num_cus : 256);

    if (c.precision == KWS_BF16) {
        p.layout = StepPlan::kStack;
        p.tail = window && kws::gru_stack_bf16_takes_window(h->pk.bf_kx0, L) ? M::kTailWindow : M::kTailEpilogue;
        p.tag[0] = {M::kBf16Stack, 0, 0, p.tail};
        return p;
    }
    const bool int8 = c.precision == KWS_INT8, f16 = c.precision == KWS_F16X3;
    // the cell wrappers exist in the generic kernels only (kws_set_kernel refuses RESIDENT on a wrapped handle)
    auto resident = [&](int l) {
        return !h->wrapped && (h->kernel_kind == KWS_KERNEL_RESIDENT || (h->kernel_kind == KWS_KERNEL_AUTO && h->pk.layers[l].resident_ok));
    };
    bool any_resident = false, all_resident = true;
    for (int l = 0; l < L; ++l) { any_resident |= resident(l); all_resident &= resident(l); }
    const bool f16_streams = f16 && h->pk.f16_generic;      // hidden = 256: weights streamed from L2 (gru_f16x3_generic.hip)
    p.streaming = f16_streams || (!f16 && !all_resident);
    // The layer-pipelined launch needs the streaming kernel on every layer; it pays when the layers would otherwise leave CUs idle.
    // AUTO keeps the resident kernels where they exist even when this launch would be faster (H=128, L=2: +10 % at B <= 2048;
    // L=4, B=1024: 2.2x; select it with KWS_KERNEL_GENERIC): the two kernel families round differently in the last bit, and a
    // stream's result must not depend on how many neighbours it is batched or sharded with.
    const bool pipelined = !heads && !h->pipe_disabled && !no_pipe && (c.precision == KWS_FP32 || f16_streams) && L >= 2 &&
                           h->kernel_kind != KWS_KERNEL_RESIDENT && !any_resident && fits;
    // Layers overlapped on HIP streams: the pipelined kernel has its own in-kernel pipeline; profiling times one launch after another
    const bool overlapped = !heads && !profiling && c.precision == KWS_FP32 && L >= 2 && L <= 5 && !pipelined && fits && T >= KWS_OVERLAP_MIN_T;
    p.layout = pipelined ? StepPlan::kPipelined : overlapped ? StepPlan::kOverlapped : StepPlan::kSequential;

    // int8: no GRU layer is `last` -- every layer hands its output rows on through the seam, and the class projection is its own
    // OctbitMatMul call over the whole [T,H] block behind the top layer, whichever kernel ran that layer
    p.tail = heads ? r.want : int8 ? M::kTailOctbitFc : M::kTailEpilogue;
    if (pipelined) {      // one launch, timed as the last layer's slot
        const uint8_t family = f16 ? M::kF16x3Pipelined : h->wrapped ? M::kPipelinedWrapped : M::kPipelined;
        p.tag[L - 1] = {family, (uint8_t)(H / 64), 0, p.tail};
    }
    for (int l = 0; l < L && !pipelined; ++l) {
        const bool first = l == 0, top = l == L - 1;
        const uint8_t family = f16_streams ? M::kF16x3Generic : f16 ? M::kF16x3 : (int8 && h->pk.oct[l].quantised) ? M::kOctbit :
                               resident(l) ? M::kResident : h->wrapped ? M::kGenericWrapped : M::kGeneric;
        const int kx = family == M::kF16x3 ? (first ? h->pk.f16_kx0 : 4) : family == M::kResident ? h->pk.layers[l].kcx_res : H / 64;
        // the window tail rides behind the epilogue where the top layer's kernel has a tail instantiation
        const bool has_tail = family == M::kF16x3 || (family == M::kResident && kws::gru_resident_takes_window(first, true));
        if (top && window && has_tail && p.tail == M::kTailEpilogue && !overlapped) p.tail = M::kTailWindow;
        p.tag[l] = {family, (uint8_t)kx, first, top ? p.tail : M::kTailNone};
    }

    if (heads) {               // every layer has a seam, the top one's is what the heads read
        p.seams = {L >= 2 ? 2 : 1, (size_t)groups * (size_t)H * 16 * sizeof(float) * T, false};
    } else if (L >= 2 || int8) {      // a single fp32 / f16x3 layer has no seam
        const size_t frame_bytes = (size_t)groups * (size_t)H * 16 * sizeof(float);
        if (pipelined) p.seams = {L - 1, frame_bytes * T, true};      // read by another XCD while the kernel runs: fine-grained memory
        else if (overlapped) {
            const int nb = std::max(2, std::min(8, T / 32));      // more blocks: less fill/drain, more launch prologues (8: +6 % over 4)
            p.Tb = ((T + nb - 1) / nb + 15) & ~15;                // multiple of the epilogue ring
            p.nb = (T + p.Tb - 1) / p.Tb;
            p.seams = {2 * (L - 1), frame_bytes * p.Tb, false};       // double-buffered per block parity
        } else p.seams = {(L > 2 || int8) ? 2 : 1, frame_bytes * T, false};      // sequential launches ping-pong two buffers
    }
    return p;
}

// ---- scratch: the arena a plan's seams are carved from, and the side buffers ----------------------------------------
// Grows the arena if this layout does not fit (the only place kws_step can synchronise: the old block may still be in
// use) and points h->scratch[] at the call's buffers.
int carve_seams(kws_handle h, const SeamLayout& want) {
    SeamLayout s = want;
    s.bytes_each = (s.bytes_each + 255) & ~size_t(255);
    kws_model::Arena& A = s.fine ? h->arena_fine : h->arena;
    const size_t need = (size_t)s.nbuf * s.bytes_each;
    KWS_TRY(grow_device(h, &A.bytes, need, s.fine, {{reinterpret_cast<void**>(&A.base), need}}, "hipMalloc(scratch)"));
    for (int i = 0; i < 8; ++i)
        h->scratch[i] = i < s.nbuf ? reinterpret_cast<float4*>(A.base + (size_t)i * s.bytes_each) : nullptr;
    h->nscratch = s.nbuf;
    return KWS_OK;
}

// Everything besides the seams that depends on the batch size: int8 exchange buffers, the pipelined launch's counters.
int ensure_side_buffers(kws_handle h, int B, bool pipelined, bool heads) {
    const size_t groups = (size_t)kws::groups_of(B);
    auto block = [](auto** p, size_t bytes) { return std::pair<void**, size_t>(reinterpret_cast<void**>(p), bytes); };
    if (heads)      // the two heads' prev_word as they were before the launch (dense_heads.hip)
        KWS_TRY(grow_device(h, &h->heads_groups, groups, false, {block(&h->heads_prev, 2 * groups * 16 * sizeof(int32_t))}, "hipMalloc(heads prev_word)"));
    if (h->cfg.precision == KWS_INT8)
        KWS_TRY(grow_device(h, &h->oct_groups, groups, false, {block(&h->oct_aq, groups * 2 * 16 * 128 * sizeof(uint32_t)),
                            block(&h->oct_range, groups * 16 * sizeof(float2)), block(&h->oct_prev, groups * 16 * sizeof(int32_t))}, "hipMalloc(int8 exchange)"));
    if (pipelined) {
        if (!h->pipe_error_host) {
            KWS_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->pipe_error_host), sizeof(int), hipHostMallocMapped));
            *h->pipe_error_host = 0;
            KWS_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->pipe_error_dev), h->pipe_error_host, 0));
        }
        KWS_TRY(grow_device(h, &h->pipe_groups, groups, true, {block(&h->pipe_ready, (size_t)h->cfg.num_layers * groups * sizeof(int))}, "hipMalloc(pipe_ready)"));
    }
    return KWS_OK;
}

// The buffers `plan` launches with.  A device without fine-grained memory gives the pipelined launch up for this handle, and the
// call is planned again, once -- the one write to a plan after plan_step: this call runs its layers one launch after another
// (planned as under profiling, whose one effect is that the layers are not overlapped); only later calls may overlap them.
int provision(kws_handle h, StepPlan& plan, PlanRequest r) {
    if (plan.layout == StepPlan::kStack) return KWS_OK;
    int rc = ensure_side_buffers(h, r.B, plan.layout == StepPlan::kPipelined, r.heads());
    if (rc == KWS_OK) rc = carve_seams(h, plan.seams);
    if (rc == kNoFineGrainedMemory) {
        h->pipe_disabled = true;
        r.profiling = true;
        plan = plan_step(h, r);
        rc = carve_seams(h, plan.seams);
    }
    return rc;
}

// A layer-pipelined launch whose wait for the layer below timed out raises a mapped host flag; its results are invalid.
// The flag is looked at (without synchronising) on every kws_step, by kws_poll_error, after the event syncs of
// kws_kernel_times and in kws_destroy -- a step's own flag can only be seen once its kernel has run, so a caller that
// needs certainty synchronises the stream and asks kws_poll_error.
int check_pipe_error(kws_handle h) {
    if (h->pipe_error_host && *reinterpret_cast<volatile int*>(h->pipe_error_host)) {
        *reinterpret_cast<volatile int*>(h->pipe_error_host) = 0;
        h->pipe_disabled = true;             // later steps launch layer by layer
        return fail(KWS_ERR_HIP, "a layer-pipelined launch timed out waiting for the layer below; the results of that step are invalid");
    }
    return KWS_OK;
}

// One profiling slot around `launch` (kws_set_profiling): two events from the pool (or new ones), recorded before and behind it
// and queued for kws_kernel_times.  Just `launch` while profiling is off.
template <typename Launch>
int profiled(kws_model* h, hipStream_t st, int slot, Launch&& launch) {
    if (!h->profiling) return launch();
    kws_model::Pending pd = {slot, nullptr, nullptr};
    for (hipEvent_t* ev : {&pd.a, &pd.b}) {
        if (!h->event_pool.empty()) { *ev = h->event_pool.back(); h->event_pool.pop_back(); }
        else KWS_HIP(hipEventCreate(ev));
    }
    KWS_HIP(hipEventRecord(pd.a, st));
    KWS_TRY(launch());
    KWS_HIP(hipEventRecord(pd.b, st));
    h->pending.push_back(pd);
    return KWS_OK;
}

// ---- one family's parameters from the step's arguments ---------------------------------------------------------------
// The last layer's epilogue fields (every layer's parameters carry them).  A launch over the time block [t0, t0 + frames) of the
// call (step_overlapped) passes t0 and its length: the rows keep the call's T as their stride.
void set_epilogue(kws::GruLayerParams& p, const StepArgs& a, const kws_config& c, bool last, int t0 = 0, int frames = 0) {
    const int C = c.num_classes;
    p.logits = a.logits ? a.logits + (size_t)t0 * C : nullptr;
    p.softmax = a.softmax ? a.softmax + (size_t)t0 * C : nullptr;
    p.tokens = a.tokens ? a.tokens + t0 : nullptr;
    p.prev_word = a.prev_word;
    p.decode_thres = a.decode2_thres;
    p.value_clip = c.value_clip;
    p.use_relu = c.use_relu;
    p.B = a.B; p.T = frames ? frames : a.T; p.C = C;
    if (frames) { p.t_stride = a.T; p.t_base = t0; }
    if (a.wt && last) p.win = *a.wt;
}
// Head of a layer-pipelined launch (GruStackParams / GruF16StackParams): the stack's shape and block map
template <typename Stack>
void begin_pipelined(const kws_model* h, Stack& sp, int B) {
    memset(&sp, 0, sizeof(sp));
    sp.L = h->cfg.num_layers; sp.G = kws::groups_of(B); sp.xcd_affine = kws::pipelined_xcd_affine(sp.L);
}
// ... and the frame counters of layer l in it
void set_pipeline(kws::GruLayerParams& p, const kws_model* h, int l, bool last) {
    p.ready_in = l == 0 ? nullptr : h->pipe_ready + (size_t)(l - 1) * h->pipe_groups;
    p.ready_out = last ? nullptr : h->pipe_ready + (size_t)l * h->pipe_groups;
    p.pipe_error = h->pipe_error_dev;
}

// Layer l of the fp32 kernels over the whole call (launch_slot narrows it to a time block)
void set_fp32_layer(kws::GruLayerParams& p, const kws_model* h, const StepArgs& a, int l, bool resident, bool last) {
    const LayerDev& Ld = h->pk.layers[l];
    const size_t state_off = (size_t)l * a.B * h->cfg.hidden;
    memset(&p, 0, sizeof(p));
    // resident kernels read the group-of-4 layouts too (dwordx4 prologue), except the first layer's
    // x-part, whose k map is the interleaved one
    p.wx = h->d_weights + ((resident && l == 0) ? Ld.wx_res : Ld.wx_gen);
    p.wh = h->d_weights + Ld.wh_gen;
    p.bias = h->d_weights + Ld.bias;
    p.wfc = h->d_weights + h->pk.wfc_off;
    p.bfc = h->d_weights + h->pk.bfc_off;
    p.x_mel = a.mel;
    p.x_prev = l == 0 ? nullptr : h->scratch[(l - 1) % h->nscratch];
    p.h_out = last ? nullptr : h->scratch[l % h->nscratch];
    p.state_in = a.state_in + state_off;
    p.state_out = a.state_out + state_off;
    p.seq_len = a.seq_len;
    p.reset = a.reset_mask;
    set_epilogue(p, a, h->cfg, last);
    p.I = Ld.in_dim;
    p.KCX = resident ? Ld.kcx_res : Ld.kcx_gen;
}
// ... and its cell wrappers (wrapped handles)
kws::GruWrapLayer wrap_layer(const kws_model* h, int l) {
    kws::GruWrapLayer w = {nullptr, 0.f, 0};
    if (h->wrap.use_layer_norm) { w.igamma = h->d_weights + h->pk.ln_igamma[l]; w.ibeta = h->pk.ln_ibeta[l]; }
    w.residual = h->wrap.use_residual && l > 0;
    return w;
}

// Layer l of the f16x3 kernels; the seams (same size as the fp32 ones) hold the layer outputs already split into fp16 pairs
void set_f16_layer(kws::GruF16Params& fp, const kws_model* h, const StepArgs& a, int l, bool last) {
    const size_t state_off = (size_t)l * a.B * h->cfg.hidden;
    memset(&fp, 0, sizeof(fp));
    fp.w = reinterpret_cast<const uint4*>(h->d_weights + h->pk.f16_w[l]);
    fp.bias = h->d_weights + h->pk.layers[l].bias;
    fp.wfc = reinterpret_cast<const uint4*>(h->d_weights + h->pk.f16_wfc);
    fp.bfc = h->d_weights + h->pk.bfc_off;
    fp.x_mel = a.mel;
    fp.x_prev = l == 0 ? nullptr : reinterpret_cast<const uint4*>(h->scratch[(l - 1) % h->nscratch]);
    fp.h_out = last ? nullptr : reinterpret_cast<uint4*>(h->scratch[l % h->nscratch]);
    fp.state_in = a.state_in + state_off;
    fp.state_out = a.state_out + state_off;
    fp.seq_len = a.seq_len; fp.reset = a.reset_mask;
    set_epilogue(fp.epi, a, h->cfg, last);
    fp.B = a.B; fp.T = a.T; fp.I = h->pk.layers[l].in_dim;
}

// Both layers of the bf16 stack
void set_bf16_stack(kws::GruBf16Params& bp, const kws_model* h, const StepArgs& a) {
    const int L = h->cfg.num_layers;
    memset(&bp, 0, sizeof(bp));
    for (int l = 0; l < L; ++l) {
        bp.w[l] = reinterpret_cast<const uint4*>(h->d_weights + h->pk.bf_w[l]);
        bp.bias[l] = h->d_weights + h->pk.layers[l].bias;
    }
    bp.wfc = reinterpret_cast<const uint4*>(h->d_weights + h->pk.bf_wfc);
    bp.bfc = h->d_weights + h->pk.bfc_off;
    bp.x_mel = a.mel; bp.state_in = a.state_in; bp.state_out = a.state_out;
    bp.seq_len = a.seq_len; bp.reset = a.reset_mask;
    set_epilogue(bp.epi, a, h->cfg, true);
    bp.B = a.B; bp.T = a.T; bp.I = h->cfg.n_mel; bp.L = L;
}

// Quantised layer l of the int8 graph, and the class projection behind its top layer
void set_octbit_layer(kws::GruOctbitParams& op, const kws_model* h, const StepArgs& a, int l) {
    const PackedWeights::OctLayer& O = h->pk.oct[l];
    const size_t state_off = (size_t)l * a.B * h->cfg.hidden;
    memset(&op, 0, sizeof(op));
    op.wg = reinterpret_cast<const uint32_t*>(h->d_weights + O.wg);
    op.wc = reinterpret_cast<const uint32_t*>(h->d_weights + O.wc);
    op.bias = h->d_weights + h->pk.layers[l].bias; op.b127 = h->d_weights + O.b127;
    op.scale_g = O.scale_g; op.scale_c = O.scale_c;
    op.x_prev = l == 0 ? nullptr : h->scratch[(l - 1) % h->nscratch];
    op.h_out = h->scratch[l % h->nscratch];
    op.state_in = a.state_in + state_off; op.state_out = a.state_out + state_off;
    op.seq_len = a.seq_len; op.reset = a.reset_mask;
    op.aq = h->oct_aq; op.B = a.B; op.T = a.T;
    op.range = (l == h->cfg.num_layers - 1) ? h->oct_range : nullptr;
}
void set_octbit_fc(kws::OctbitFcParams& fp, const kws_model* h, const StepArgs& a) {
    const kws_config& c = h->cfg;
    const int top = c.num_layers - 1;
    memset(&fp, 0, sizeof(fp));
    fp.wfc = reinterpret_cast<const uint32_t*>(h->d_weights + h->pk.oct_wfc);
    fp.b127 = h->d_weights + h->pk.oct_b127fc;
    fp.bfc = h->d_weights + h->pk.bfc_off;
    fp.scale_w = h->pk.oct_scale_fc;
    fp.h_top = h->scratch[top % h->nscratch];
    fp.seq_len = a.seq_len;
    fp.range = h->oct_range;
    fp.range_ready = h->pk.oct[top].quantised ? 1 : 0;
    fp.prev_in = a.prev_word ? h->oct_prev : nullptr;
    fp.logits = a.logits; fp.softmax = a.softmax; fp.tokens = a.tokens; fp.prev_word = a.prev_word;
    fp.decode_thres = a.decode2_thres; fp.value_clip = c.value_clip; fp.use_relu = c.use_relu;
    fp.B = a.B; fp.T = a.T; fp.C = c.num_classes;
}

// Head i's weights, bias and class count (DenseHead, HeadsWindowHead)
template <typename Head>
void bind_head(Head& d, const kws_model* h, int i) {
    d.wfc = h->d_weights + (i ? h->pk.wfc2_off : h->pk.wfc_off);
    d.bfc = h->d_weights + (i ? h->pk.bfc2_off : h->pk.bfc_off);
    d.C = i ? h->num_classes2 : h->cfg.num_classes;
}
// The heads behind the top layer of a kws_step_heads call
void set_dense_heads(kws::DenseHeadsParams& dp, const kws_model* h, const StepArgs& a) {
    const kws_config& c = h->cfg;
    const HeadsArgs& ha = *a.heads;
    memset(&dp, 0, sizeof(dp));
    dp.h_top = h->scratch[(c.num_layers - 1) % h->nscratch];
    dp.seq_len = a.seq_len; dp.reset = a.reset_mask;
    dp.nn_outputs = ha.nn_outputs;
    for (int i = 0; i < 2; ++i) {
        if (!ha.on[i]) continue;
        kws::DenseHead& d = dp.head[i];
        const kws_head_io& io = ha.head[i];
        bind_head(d, h, i);
        d.logits = io.logits; d.softmax = io.softmax; d.tokens = io.tokens; d.prev_word = io.prev_word;
        d.prev_in = io.prev_word ? h->heads_prev + (size_t)i * h->heads_groups * 16 : nullptr;
        d.decode_thres = io.decode2_thres;
    }
    dp.value_clip = c.value_clip; dp.use_relu = c.use_relu;
    dp.B = a.B; dp.T = a.T;
}
// heads_window_kernel behind the top layer of a two-head manager's iteration: the caller's windows and outputs, this handle's heads
void set_heads_window(kws::HeadsWindowParams& hp, const kws_model* h, const StepArgs& a) {
    const kws_config& c = h->cfg;
    const HeadsArgs& ha = *a.heads;
    memset(&hp, 0, sizeof(hp));
    hp.h_top = a.T > 0 ? h->scratch[(c.num_layers - 1) % h->nscratch] : nullptr;
    for (int i = 0; i < 2; ++i) {
        bind_head(hp.head[i], h, i);
        hp.head[i].softmax = ha.head[i].softmax; hp.head[i].decode_thres = ha.head[i].decode2_thres;
        hp.win[i] = ha.win[i];
    }
    hp.hit = ha.hit; hp.restart = ha.restart; hp.frames = ha.frames; hp.skip = ha.skip;
    hp.value_clip = c.value_clip; hp.use_relu = c.use_relu;
    hp.B = a.B; hp.T = a.T;
}

// ... and their bank forms: head 2 has the bank's C + n_new classes and no weights of its own; head 1 is always bound (projected for
// head 2's frozen logits even where none of its outputs is wanted)
void set_bank_heads(kws::BankHeadsParams& bp, const kws_model* h, const StepArgs& a) {
    set_dense_heads(bp.d, h, a);
    kws::DenseHead& h1 = bp.d.head[0];
    if (!a.heads->on[0]) { bind_head(h1, h, 0); h1.decode_thres = 0.f; }
    bp.bank = *a.heads->bank;
    if (a.heads->on[1]) bp.d.head[1].C = h->cfg.num_classes + bp.bank.n_new;
}
void set_bank_window(kws::BankWindowParams& bp, const kws_model* h, const StepArgs& a) {
    set_heads_window(bp.w, h, a);
    bp.bank = *a.heads->bank;
    bp.w.head[1].C = h->cfg.num_classes + bp.bank.n_new;
}
// heads_window_kernel, or its bank form, on the windows of a.heads (behind the top layer, or alone on a zero-frame chunk)
int launch_window_tail_kernel(const kws_model* h, const StepArgs& a, hipStream_t st) {
    if (a.heads->bank) {
        kws::BankWindowParams bp;
        set_bank_window(bp, h, a);
        // (a keyword set on the bank AFTER the manager was sized: the keyword form's LDS is checked where it is launched)
        const size_t lds = kws::bank_keyword_window_lds_bytes(a.T, bp.w.win[0].nq, bp.w.win[1].nq, h->cfg.hidden, bp.bank.n_new);
        if (a.heads->bank_slots && lds > kWindowIncLdsMax)
            return fail(KWS_ERR_UNSUPPORTED, "the bank window step with per-slot keywords needs %zu bytes of LDS for this chunk (%zu of them the "
                        "group's keyword matchers; limit %zu): use shorter chunks or windows", lds, kws::kBankKeywordStageBytes, kWindowIncLdsMax);
        return hip_done(kws::launch_bank_heads_window(bp, a.heads->bank_slots, h->cfg.hidden, st), "launch bank_heads_window");
    }
    kws::HeadsWindowParams hp;
    set_heads_window(hp, h, a);
    return hip_done(kws::launch_heads_window(hp, h->cfg.hidden, st), "launch heads_window");
}

// ---- the launches ----------------------------------------------------------------------------------------------------
// The launch of profiling slot l as the plan tagged it, on `st`.  step_overlapped passes the time block [t0, t0 + frames) of the
// call: seams double-buffered per block parity, and behind block 0 the state is the one the block before left in state_out.
int launch_slot(const kws_model* h, const StepArgs& a, const StepPlan& plan, int l, hipStream_t st, int t0 = 0, int frames = 0) {
    const kws_config& c = h->cfg;
    const int H = c.hidden, L = c.num_layers;
    const M::LaunchTag& t = plan.tag[l];
    hipError_t e = hipSuccess;
    const char* what = "";
    switch (t.family) {
        case M::kBf16Stack: {
            kws::GruBf16Params bp;
            set_bf16_stack(bp, h, a);
            e = kws::launch_gru_stack_bf16(bp, h->pk.bf_kx0, L, st); what = "launch gru_stack_bf16";
            break;
        }
        case M::kF16x3: case M::kF16x3Generic: {
            kws::GruF16Params fp;
            set_f16_layer(fp, h, a, l, t.last());
            if (t.family == M::kF16x3) { e = kws::launch_gru_layer_f16x3(fp, t.first, t.last(), st); what = "launch gru_layer_f16x3"; }
            else { e = kws::launch_gru_layer_f16x3_generic(fp, H, t.first, t.last(), st); what = "launch gru_layer_f16x3_generic"; }
            break;
        }
        case M::kF16x3Pipelined: {
            kws::GruF16StackParams sp;
            begin_pipelined(h, sp, a.B);
            for (int k = 0; k < L; ++k) {
                set_f16_layer(sp.layer[k], h, a, k, k == L - 1);
                set_pipeline(sp.layer[k].epi, h, k, k == L - 1);
            }
            e = kws::launch_gru_stack_f16x3_pipelined(sp, H, st); what = "launch gru_stack_f16x3_pipelined";
            break;
        }
        case M::kPipelined: case M::kPipelinedWrapped: {
            kws::GruStackParams sp;
            begin_pipelined(h, sp, a.B);
            for (int k = 0; k < L; ++k) {
                set_fp32_layer(sp.layer[k], h, a, k, false, k == L - 1);
                set_pipeline(sp.layer[k], h, k, k == L - 1);
            }
            if (t.family == M::kPipelinedWrapped) {
                kws::GruWrapParams wp;
                memset(&wp, 0, sizeof(wp));
                for (int k = 0; k < L; ++k) wp.layer[k] = wrap_layer(h, k);
                e = kws::launch_gru_stack_generic_pipelined_wrapped(sp, wp, H, st);
            } else {
                e = kws::launch_gru_stack_generic_pipelined(sp, H, st);
            }
            what = "launch gru_stack_generic_pipelined";
            break;
        }
        case M::kOctbit: {
            kws::GruOctbitParams op;
            set_octbit_layer(op, h, a, l);
            e = kws::launch_gru_layer_octbit(op, st); what = "launch gru_layer_octbit";
            break;
        }
        case M::kResident: case M::kGeneric: case M::kGenericWrapped: {
            const bool first = l == 0, last = t.last();
            kws::GruLayerParams p;
            set_fp32_layer(p, h, a, l, t.family == M::kResident, last);
            if (plan.layout == StepPlan::kOverlapped) {
                const int parity = (t0 / plan.Tb) & 1;
                p.x_mel = a.mel + (size_t)t0 * c.n_mel;
                p.x_prev = first ? nullptr : h->scratch[2 * (l - 1) + parity];
                p.h_out = last ? nullptr : h->scratch[2 * l + parity];
                if (t0 > 0) { p.state_in = p.state_out; p.reset = nullptr; }
                set_epilogue(p, a, c, last, t0, frames);
                what = "launch (overlapped layers)";
            } else {
                what = t.family == M::kResident ? "launch gru_layer_resident" : "launch gru_layer_generic";
            }
            if (t.family == M::kResident) e = kws::launch_gru_layer_resident(p, t.first, last, st);
            else if (t.family == M::kGenericWrapped) e = kws::launch_gru_layer_generic_wrapped(p, wrap_layer(h, l), H, t.first, last, st);
            else e = kws::launch_gru_layer_generic(p, H, t.first, last, st);
            break;
        }
        default: return KWS_OK;      // an empty slot: its layer runs inside another slot's launch
    }
    if (e != hipSuccess) return hip_fail(e, what);
    switch (t.tail) {      // one more launch inside the top layer's slot, on the rows it left in its seam
        case M::kTailHeadsWindow: case M::kTailBankWindow: case M::kTailBankKeywordWindow:      // both heads and both windows of a two-head manager
            return launch_window_tail_kernel(h, a, st);
        case M::kTailBankHeads: case M::kTailBankKeywordHeads: {        // the class heads, head 2 from each stream's bank slot
            kws::BankHeadsParams bp;
            set_bank_heads(bp, h, a);
            return hip_done(kws::launch_bank_heads(bp, a.heads->bank_slots, H, st), "launch bank_heads");
        }
        case M::kTailDenseHeads: {       // the class heads
            kws::DenseHeadsParams dp;
            set_dense_heads(dp, h, a);
            return hip_done(kws::launch_dense_heads(dp, H, st), "launch dense_heads");
        }
        case M::kTailOctbitFc: {         // the int8 class projection, whichever kernel ran the top layer
            kws::OctbitFcParams fp;
            set_octbit_fc(fp, h, a);
            return hip_done(kws::launch_octbit_fc(fp, st), "launch octbit_fc");
        }
        default: return KWS_OK;          // the layer's own kernel did it (epilogue, window tail), or nothing is wanted
    }
}

// Layers on separate HIP streams, time-blocked.  When L x groups workgroups fit the chip at once, the layers of a
// long call need not run one after another: the call is cut into time blocks, layer l works on block k while layer
// l-1 already works on block k+1 (its own stream, ordered by events; seam buffers double-buffered per block parity).
// The kernels are the ones a plain call uses -- a call on frames [t0, t1) with the state carried is bit-identical to
// the corresponding slice of one long call (tests/test_gpu_parity.py) -- so the result does not depend on whether
// this path was taken.  Wall time ~ (slowest layer) x (1 + 1/blocks) instead of the sum over layers.
int step_overlapped(kws_handle h, const StepArgs& a, const StepPlan& plan) {
    const int L = h->cfg.num_layers, T = a.T, nb = plan.nb, Tb = plan.Tb;
    const hipStream_t st = a.stream;
    for (int l = 1; l < L; ++l)
        if (!h->lane_stream[l]) KWS_HIP(hipStreamCreateWithFlags(&h->lane_stream[l], hipStreamNonBlocking));
    while ((int)h->ovl_events.size() < L * nb + 1) {
        hipEvent_t ev;
        KWS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        h->ovl_events.push_back(ev);
    }
    auto done = [&](int l, int k) { return h->ovl_events[1 + l * nb + k]; };
    KWS_HIP(hipEventRecord(h->ovl_events[0], st));                          // everything queued before this call
    for (int l = 1; l < L; ++l) KWS_HIP(hipStreamWaitEvent(h->lane_stream[l], h->ovl_events[0], 0));
    for (int k = 0; k < nb; ++k) {
        const int t0 = k * Tb, tk = (T - t0 < Tb) ? T - t0 : Tb;
        for (int l = 0; l < L; ++l) {
            const bool first = l == 0, last = l == L - 1;
            hipStream_t sx = first ? st : h->lane_stream[l];
            if (!first) KWS_HIP(hipStreamWaitEvent(sx, done(l - 1, k), 0));                    // its input block
            if (!last && k >= 2) KWS_HIP(hipStreamWaitEvent(sx, done(l + 1, k - 2), 0));       // its output buffer is free again
            KWS_TRY(launch_slot(h, a, plan, l, sx, t0, tk));
            KWS_HIP(hipEventRecord(done(l, k), sx));
        }
    }
    for (int l = 1; l < L; ++l) {
        KWS_HIP(hipStreamWaitEvent(st, done(l, nb - 1), 0));                                   // rejoin the caller's stream
        if (!h->ovl_tail[l]) KWS_HIP(hipEventCreateWithFlags(&h->ovl_tail[l], hipEventDisableTiming));
        KWS_HIP(hipEventRecord(h->ovl_tail[l], h->lane_stream[l]));
    }
    h->ovl_tail_valid = true;
    return KWS_OK;
}

// A step over zero frames.  dynamic_rnn hands the initial state back -- and clean_state() (detector.py:313-316) has already zeroed
// it for the streams the mask names, together with the previous word of every head the call names: one state pass per prev_word array
// (kws_step: one; kws_step_heads: two, the second pass copying state_out onto itself), or a plain copy without a mask.  A two-head
// manager then makes its empty entry into both windows.  No GRU kernel runs: h->launch_tag stays what the step before left.
int step_zero_frames(kws_handle h, const StepArgs& a) {
    const int H = h->cfg.hidden, L = h->cfg.num_layers, B = a.B;
    const hipStream_t st = a.stream;
    const bool window = a.heads && a.heads->window;
    int32_t* prev[2] = {a.prev_word, nullptr};      // kws_step's; a two-head manager keeps no words outside its windows
    int passes = 1;
    if (a.heads && !window) { prev[0] = a.heads->head[0].prev_word; prev[1] = a.heads->head[1].prev_word; passes = 2; }
    for (int i = 0; a.reset_mask && i < passes; ++i)
        KWS_TRY(hip_done(kws::launch_state_passthrough(i ? a.state_out : a.state_in, a.state_out, a.reset_mask, prev[i], L, B, H, st), "launch state_passthrough"));
    if (!a.reset_mask && a.state_out != a.state_in)
        KWS_HIP(hipMemcpyAsync(a.state_out, a.state_in, (size_t)L * B * H * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (!window) return KWS_OK;
    return launch_window_tail_kernel(h, a, st);
}

int step_body(kws_handle h, const StepArgs& a) {
    const kws_config& c = h->cfg;
    const int H = c.hidden, L = c.num_layers, B = a.B, T = a.T;
    const hipStream_t st = a.stream;
    KWS_TRY(check_pipe_error(h));      // raised by an earlier layer-pipelined step of this handle
    // the handle's weights and scratch live on the device that was current at kws_create
    int dev = -1;
    if (hipGetDevice(&dev) == hipSuccess && dev != h->device)
        return fail(KWS_ERR_INVALID_ARGUMENT, "handle was created on device %d, the current device is %d", h->device, dev);
    if (h->ovl_tail_valid) {
        // the previous call ran its upper layers on the handle's own streams: whatever stream this call comes in on,
        // it must not touch the seam buffers (or reallocate them) before those kernels are done
        for (int l = 1; l < L; ++l)
            if (h->ovl_tail[l]) KWS_HIP(hipStreamWaitEvent(st, h->ovl_tail[l], 0));
        h->ovl_tail_valid = false;
    }
    if (T == 0) return step_zero_frames(h, a);
    const PlanRequest req = plan_request(h, a);
    StepPlan plan = plan_step(h, req);
    if (!a.mel) return fail(KWS_ERR_INVALID_ARGUMENT, "mel is null");
    // the streaming kernels address a group's seam (T x H/16 KiB) through buffer instructions with 32-bit offsets
    if (plan.streaming && (long long)T * (H / 16) >= (1LL << 21))
        return fail(KWS_ERR_UNSUPPORTED, "T=%d frames of hidden=%d exceed the 2 GiB a stream group's seam may span: split the call "
                    "(state carried across calls gives identical results)", T, H);
    if ((reinterpret_cast<uintptr_t>(a.mel) & 15) != 0) return fail(KWS_ERR_INVALID_ARGUMENT, "mel must be 16-byte aligned");
    if (a.heads && T > kws::kHeadsMaxFrames)
        return fail(KWS_ERR_UNSUPPORTED, "T=%d frames exceed the %d a kws_step_heads call takes: split the call", T, kws::kHeadsMaxFrames);
    KWS_TRY(provision(h, plan, req));
    if (plan.layout == StepPlan::kOverlapped) {
        KWS_TRY(step_overlapped(h, a, plan));
    } else {      // kStack, kSequential, kPipelined: every tagged slot is one launch on the call's stream
        if (c.precision == KWS_INT8 && a.prev_word)
            KWS_HIP(hipMemcpyAsync(h->oct_prev, a.prev_word, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        for (int i = 0; a.heads && i < 2; ++i)        // what the heads' first frame block reads while their last one writes prev_word
            if (a.heads->on[i] && a.heads->head[i].prev_word)
                KWS_HIP(hipMemcpyAsync(h->heads_prev + (size_t)i * h->heads_groups * 16, a.heads->head[i].prev_word, (size_t)B * sizeof(int32_t),
                                       hipMemcpyDeviceToDevice, st));
        if (plan.layout == StepPlan::kPipelined)      // the frame counters, cleared on the call's stream first
            KWS_HIP(hipMemsetAsync(h->pipe_ready, 0, (size_t)L * h->pipe_groups * sizeof(int), st));
        for (int l = 0; l < L; ++l)
            if (plan.tag[l].family != kws_model::kNone) KWS_TRY(profiled(h, st, l, [&] { return launch_slot(h, a, plan, l, st); }));
    }
    for (int l = 0; l < 8; ++l) h->launch_tag[l] = plan.tag[l];
    return KWS_OK;
}

}  // namespace

// Does the plan of `a` -- a step that offers a window tail (a.wt) -- let the last launch take it along?  (kws_stream_feed asks before
// it hands one to step_impl, which asks again; where the plan says no, window_inc_kernel follows the stack instead.)
bool kws_host::step_takes_window(kws_handle h, const StepArgs& a) { return plan_step(h, plan_request(h, a)).tail == M::kTailWindow; }

int kws_host::grow_device(kws_model* h, size_t* have, size_t want, bool fine, std::initializer_list<std::pair<void**, size_t>> blocks, const char* what) {
    if (want <= *have) return KWS_OK;
    KWS_HIP(hipDeviceSynchronize());
    for (const auto& b : blocks) { if (*b.first) hipFree(*b.first); *b.first = nullptr; }
    *have = 0;
    for (const auto& b : blocks) {
        const hipError_t e = fine ? hipExtMallocWithFlags(b.first, b.second, hipDeviceMallocFinegrained) : hipMalloc(b.first, b.second);
        if (e == hipSuccess) continue;
        *b.first = nullptr;
        (void)hipGetLastError();
        return fine ? kNoFineGrainedMemory : hip_fail(e, what);
    }
    *have = want;
    ++h->scratch_allocs;
    return KWS_OK;
}

// Ordering of a call against the handle's previous one (kws_model::last_done): device-side, never a host wait.
int kws_host::call_enter(kws_handle h, hipStream_t st) {
    if (h->last_stream_valid && st != h->last_stream) KWS_HIP(hipStreamWaitEvent(st, h->last_done, 0));
    h->last_stream = st;
    h->last_stream_valid = true;
    return KWS_OK;
}
int kws_host::call_leave(kws_handle h, hipStream_t st) {
    KWS_HIP(hipEventRecord(h->last_done, st));
    return KWS_OK;
}

int kws_host::step_impl(kws_handle h, const StepArgs& a) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (a.wt && (a.seq_len || !step_takes_window(h, a))) return fail(KWS_ERR_UNSUPPORTED, "internal: this step cannot take a window tail");
    if (a.B < 0 || a.T < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative B=%d or T=%d", a.B, a.T);
    if (a.B == 0) return KWS_OK;   // nothing to advance (empty tensors have null data pointers)
    if (!a.state_in || !a.state_out) return fail(KWS_ERR_INVALID_ARGUMENT, "state_in/state_out must not be null");
    if (a.tokens && !a.prev_word) return fail(KWS_ERR_INVALID_ARGUMENT, "tokens requires prev_word");
    if (a.heads) {
        if (h->num_classes2 <= 0) return fail(KWS_ERR_INVALID_ARGUMENT, "kws_step_heads needs a handle with a second class head (kws_create_heads)");
        for (int i = 0; i < 2; ++i)
            if (a.heads->on[i] && a.heads->head[i].tokens && !a.heads->head[i].prev_word)
                return fail(KWS_ERR_INVALID_ARGUMENT, "head%d: tokens requires prev_word", i + 1);
        if ((reinterpret_cast<uintptr_t>(a.heads->nn_outputs) & 15) != 0) return fail(KWS_ERR_INVALID_ARGUMENT, "nn_outputs must be 16-byte aligned");
    }
    if (a.locked) return step_body(h, a);
    BusyGuard busy(h->in_call);
    if (!busy.owned)
        return fail(KWS_ERR_BUSY, "kws_step: another host thread is inside a call on this handle (one thread at a time per handle; "
                    "use one handle per thread)");
    int rc = call_enter(h, a.stream);       // the previous call's kernels may still own the seams: this stream waits for them on the device
    if (rc != KWS_OK) return rc;
    rc = step_body(h, a);
    const int rl = call_leave(h, a.stream);     // also after a failure: whatever was queued before it is what the next call must wait for
    return rc != KWS_OK ? rc : rl;
}

// what the LDS of a window step is made of, for the refusals below: the two-head step's terms, then a bank's columns and keyword matchers
static std::string heads_window_lds_terms(int T, int nq1, int nq2, size_t cols, size_t matchers) {
    std::string s = "logits " + std::to_string(kws::kHeadsWindowLogitsBytes) + ", frame words " + std::to_string((size_t)2 * 16 * kws::heads_window_stride(T)) +
                    ", label tables 512, rings " + std::to_string(kws::window_tail_scratch_bytes(nq1)) + " + " + std::to_string(kws::window_tail_scratch_bytes(nq2));
    if (cols) s += ", the group's columns " + std::to_string(cols);
    if (matchers) s += ", the group's keyword matchers " + std::to_string(matchers);
    return s;
}

int kws_host::heads_window_check(const kws_model* h, const kws_window* w1, const kws_window* w2, int B, int T, const kws_bank* bank) {
    if (h->num_classes2 <= 0)
        return fail(KWS_ERR_INVALID_ARGUMENT, "a two-head stream manager needs a model handle with a second class head (kws_create_heads)");
    if (w1 == w2) return fail(KWS_ERR_INVALID_ARGUMENT, "window1 and window2 are the same handle: each head queues its own chunks");
    const kws_window* w[2] = {w1, w2};
    const int C[2] = {h->cfg.num_classes, bank ? h->cfg.num_classes + bank->n_new : h->num_classes2};
    for (int i = 0; i < 2; ++i) {
        if (w[i]->C != C[i] || w[i]->B != B)
            return fail(KWS_ERR_INVALID_ARGUMENT, "window%d was created for B=%d C=%d, head %d needs B=%d C=%d", i + 1, w[i]->B, w[i]->C, i + 1, B, C[i]);
        if (T > w[i]->tmax)
            return fail(KWS_ERR_INVALID_ARGUMENT, "chunks of up to %d frames, window%d holds %d per chunk", T, i + 1, w[i]->tmax);
    }
    const size_t lds = kws::heads_window_lds_bytes(T, w1->nq, w2->nq);
    if (lds > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "chunks of up to %d frames with windows of %d and %d chunks need %zu bytes of LDS in the two-head window step "
                    "(%s; limit %zu): use shorter chunks", T, w1->nq, w2->nq, lds, heads_window_lds_terms(T, w1->nq, w2->nq, 0, 0).c_str(), kWindowIncLdsMax);
    if (!bank) return KWS_OK;
    // a bank with per-slot keywords launches the keyword form, which stages the group's sixteen matchers behind the columns
    const size_t cols = kws::bank_stage_bytes(bank->H, bank->n_new), matchers = bank->keywords_ever ? kws::kBankKeywordStageBytes : 0;
    if (lds + cols + matchers > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "chunks of up to %d frames with windows of %d and %d chunks and a bank of %d new classes at hidden=%d%s need %zu "
                    "bytes of LDS in the bank window step (%s; limit %zu): use shorter chunks or windows", T, w1->nq, w2->nq, bank->n_new, bank->H,
                    matchers ? " with per-slot keywords" : "", lds + cols + matchers, heads_window_lds_terms(T, w1->nq, w2->nq, cols, matchers).c_str(),
                    kWindowIncLdsMax);
    return KWS_OK;
}

HeadsArgs kws_host::heads_window_args(kws_window* w1, kws_window* w2, const uint8_t* clear_before, int32_t* hit, uint8_t* restart) {
    HeadsArgs ha;
    ha.window = true;
    // the tails write hit of their own window where the coupling overwrites it, and leave restart to the coupling
    ha.win[0] = window_tail_params(w1, clear_before, hit, nullptr);
    ha.win[1] = window_tail_params(w2, clear_before, hit, nullptr);
    ha.head[0].decode2_thres = w1->thres; ha.head[1].decode2_thres = w2->thres;
    ha.hit = hit; ha.restart = restart;
    return ha;
}

extern "C" {

int kws_step_heads_window(kws_handle h, const float* mel, const float* state_in, float* state_out, const uint8_t* reset_mask, int B, int T,
                          kws_window_handle window1, kws_window_handle window2, const char* label1, const char* label2,
                          const uint8_t* clear_before, float* softmax1, float* softmax2, int32_t* hit, uint8_t* restart, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!window1 || !window2 || !label1 || !label2 || !hit || !state_in || !state_out || (!mel && T > 0))
        return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (B < 1 || T < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d", B, T);
    if (!live_serial(h) || !live_serial(window1) || !live_serial(window2))
        return fail(KWS_ERR_INVALID_ARGUMENT, "model or window handle is not alive (destroyed, or not a handle)");
    KWS_TRY(heads_window_check(h, window1, window2, B, T));
    // rows of an even class count leave as float2 (store_row)
    if ((h->cfg.num_classes % 2 == 0 && (reinterpret_cast<uintptr_t>(softmax1) & 7) != 0) ||
        (h->num_classes2 % 2 == 0 && (reinterpret_cast<uintptr_t>(softmax2) & 7) != 0))
        return fail(KWS_ERR_INVALID_ARGUMENT, "softmax1 / softmax2 must be 8-byte aligned");
    KWS_TRY(window_bind_label(window1, label1));
    KWS_TRY(window_bind_label(window2, label2));
    HeadsArgs ha = heads_window_args(window1, window2, clear_before, hit, restart);
    ha.head[0].softmax = softmax1; ha.head[1].softmax = softmax2;
    StepArgs a;
    a.mel = mel; a.state_in = state_in; a.state_out = state_out; a.reset_mask = reset_mask;
    a.B = B; a.T = T; a.stream = static_cast<hipStream_t>(stream); a.heads = &ha;
    return step_impl(h, a);
}

int kws_step(kws_handle h, const float* mel, const float* state_in, float* logits, float* softmax,
             float* state_out, const int32_t* seq_len, const uint8_t* reset_mask, int8_t* tokens,
             int32_t* prev_word, float decode2_thres, int B, int T, void* stream) {
    const StepArgs a = {mel, state_in, logits, softmax, state_out, seq_len, reset_mask, tokens, prev_word, decode2_thres, B, T,
                        static_cast<hipStream_t>(stream)};
    return step_impl(h, a);
}

int kws_step_heads(kws_handle h, const float* mel, const float* state_in, float* state_out, const int32_t* seq_len,
                   const uint8_t* reset_mask, float* nn_outputs, const kws_head_io* head1, const kws_head_io* head2, int B, int T,
                   void* stream) {
    HeadsArgs ha;
    ha.nn_outputs = nn_outputs;
    if (head1) { ha.head[0] = *head1; ha.on[0] = true; }
    if (head2) { ha.head[1] = *head2; ha.on[1] = true; }
    StepArgs a;
    a.mel = mel; a.state_in = state_in; a.state_out = state_out; a.seq_len = seq_len; a.reset_mask = reset_mask;
    a.B = B; a.T = T; a.stream = static_cast<hipStream_t>(stream);
    a.heads = &ha;
    return step_impl(h, a);
}

int kws_reserve(kws_handle h, int B, int T) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    BusyGuard busy(h->in_call);
    if (!busy.owned) return fail(KWS_ERR_BUSY, "kws_reserve: another host thread is inside a call on this handle");
    if (B < 0 || T < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative B=%d or T=%d", B, T);
    // whichever launch layout kws_step picks for (B, T) -- it depends on kws_set_profiling too -- fits afterwards: the arenas only grow
    auto reserve = [&](const StepArgs& a, bool profiling) {
        PlanRequest r = plan_request(h, a);
        r.profiling = profiling;
        StepPlan plan = plan_step(h, r);
        return provision(h, plan, r);
    };
    StepArgs a;
    a.B = B; a.T = T;
    KWS_TRY(reserve(a, true));
    KWS_TRY(reserve(a, false));
    const HeadsArgs ha;      // a heads handle: kws_step_heads' layout too (one answer, whatever the profiling switch or the heads wanted)
    a.heads = &ha;
    return h->num_classes2 > 0 ? reserve(a, h->profiling) : KWS_OK;
}

int kws_scratch_stats(kws_handle h, size_t* bytes_reserved, int32_t* allocations) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (bytes_reserved) *bytes_reserved = h->arena.bytes + h->arena_fine.bytes;
    if (allocations) *allocations = h->scratch_allocs;
    return KWS_OK;
}

int kws_poll_error(kws_handle h) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    return check_pipe_error(h);
}

int kws_set_profiling(kws_handle h, int enable) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    h->profiling = enable != 0;
    return KWS_OK;
}

int kws_kernel_times(kws_handle h, float* ms_sum, int32_t* launches, int reset) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    BusyGuard busy(h->in_call);
    if (!busy.owned) return fail(KWS_ERR_BUSY, "kws_kernel_times: another host thread is inside a call on this handle");
    for (auto& pd : h->pending) {
        KWS_HIP(hipEventSynchronize(pd.b));
        float ms = 0.f;
        KWS_HIP(hipEventElapsedTime(&ms, pd.a, pd.b));
        h->ms_sum[pd.slot] += ms;
        h->launches[pd.slot] += 1;
        h->event_pool.push_back(pd.a);
        h->event_pool.push_back(pd.b);
    }
    h->pending.clear();
    for (int l = 0; l < h->cfg.num_layers; ++l) {
        if (ms_sum) ms_sum[l] = h->ms_sum[l];
        if (launches) launches[l] = h->launches[l];
    }
    if (reset) {
        std::fill(h->ms_sum.begin(), h->ms_sum.end(), 0.f);
        std::fill(h->launches.begin(), h->launches.end(), 0);
    }
    return check_pipe_error(h);
}

}  // extern "C"
