// C ABI of libkws_amd.so (include/kws_amd.h): the train handle -- taped forward, back-propagation through time, the CTC loss through
// ctc_loss_kernel, global-norm clipping and Adam / Nesterov on the canonical blob (gru_train.hip, train_kernels.hip), with the cell
// wrappers of kws_train_create_wrapped around the two frame loops (train_wrap_kernels.hip).
#include <new>

#include "api_internal.h"

using namespace kws_host;

struct kws_train {
    kws_train_config cfg;
    BlobLayout bl;
    WrapLayout wl;                   // the layer norm's ibeta / igamma behind the canonical blob (kws_train_create_wrapped)
    bool ln = false, res = false, var = false;      // wrappers.use_layer_norm, wrappers.use_residual, variational_recurrent
    size_t P = 0;                    // floats of the blob
    // one allocation fixed at create: theta | m | v | grad [4 P], the packed copies of every layer (wx, wh, wht, b3), then the
    // reduction's per-workgroup sums of squares (doubles)
    float* state = nullptr;
    float *theta = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr;
    kws::TrainPackParams pack = {};
    double* sumsq = nullptr;
    size_t state_bytes = 0;
    int nred = 0;
    // one allocation that only grows, carved for the shape of the call (carve): lengths and labels, the row mask, the job table of the
    // weight-gradient launch, the tape, the gradients of the activations, the row chunks' partial weight gradients.  With the layer norm
    // a layer also keeps xhat and xn [M, I_l] and rstd [M] from the forward, g = dxhat [M, I_l] and gs [M] (the rows' terms of d ibeta)
    // from the backward; with the residual a layer >= 1 keeps out [M, H] = 0.7071 (y + its input)
    char* arena = nullptr;
    size_t arena_bytes = 0;
    struct Carved {
        int B = 0, T = 0, S_max = -1;
        int32_t* ints = nullptr;
        uint8_t* live = nullptr;
        kws::TrainWgradJob* jobs = nullptr;
        float *xg = nullptr, *dy[2] = {nullptr, nullptr}, *logits = nullptr, *gl = nullptr, *partial = nullptr;
        struct Layer { float *ar, *au, *ac, *hp, *rh, *y, *dhat, *xhat, *xn, *rstd, *g, *gs, *out; } layer[8] = {};   // ar, au, ac: the pre-activations of r, u, c
        int njobs = 0, units = 0, chunk_rows = 0, chunks = 0;
    } cv;
    std::vector<kws::TrainWgradJob> jobs_host;
    bool jobs_dirty = false;         // carved anew since the table last went to the device
    std::vector<int32_t> ints_host;
    int steps = 0, allocs = 0, launches = 0;
    std::atomic<int> in_call{0};
    hipStream_t last_stream = nullptr;
    bool last_stream_valid = false;
    hipEvent_t last_done = nullptr;
};

namespace {

constexpr size_t kAlign = 256;
size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
constexpr float kResidualScale = 0.7071067811865475f;      // utils/custom_wrapper.py:116

bool residual_on(const kws_train* h, int l) { return h->res && l >= 1; }
// what layer l hands to the layer above and to the dense layer
const float* layer_output(const kws_train* h, const kws_train::Carved& cv, int l) { return residual_on(h, l) ? cv.layer[l].out : cv.layer[l].y; }

int train_enter(kws_train* h, hipStream_t st) {
    if (h->last_stream_valid && h->last_stream != st) KWS_HIP(hipStreamWaitEvent(st, h->last_done, 0));
    return KWS_OK;
}
int train_leave(kws_train* h, hipStream_t st) {
    KWS_HIP(hipEventRecord(h->last_done, st));
    h->last_stream = st;
    h->last_stream_valid = true;
    return KWS_OK;
}

// ... at the end of a call's queued work, failed or not: launches that went out before a failure are still on `st`, and a following
// call on another stream has to be ordered behind them.  rc: the call's result so far (its message stays the last error).
int train_finish(kws_train* h, hipStream_t st, int rc) {
    if (rc == KWS_OK) return train_leave(h, st);
    if (hipEventRecord(h->last_done, st) == hipSuccess) { h->last_stream = st; h->last_stream_valid = true; }
    return rc;
}

// Lays the arena out for (B, T, S_max).  base == null: only the size.  Returns the bytes.
size_t carve(const kws_train* h, int B, int T, int S_max, char* base, kws_train::Carved* cv) {
    const kws_config& c = h->cfg.model;
    const size_t M = (size_t)B * T, H = (size_t)c.hidden;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + at : nullptr; at += aligned(bytes); return p; };
    kws_train::Carved o;
    o.B = B; o.T = T; o.S_max = S_max;
    o.njobs = (h->ln ? 8 : 6) * c.num_layers + 2;
    o.chunk_rows = wgrad_chunk_rows(M);
    o.chunks = (int)((M + o.chunk_rows - 1) / o.chunk_rows);
    o.ints = reinterpret_cast<int32_t*>(take((size_t)B * (2 + S_max) * sizeof(int32_t)));
    o.live = reinterpret_cast<uint8_t*>(take(M));
    o.jobs = reinterpret_cast<kws::TrainWgradJob*>(take((size_t)o.njobs * sizeof(kws::TrainWgradJob)));
    auto floats = [&](size_t n) { return reinterpret_cast<float*>(take(n * sizeof(float))); };
    o.xg = floats(M * 3 * H);
    o.dy[0] = floats(M * H); o.dy[1] = floats(M * H);
    o.logits = floats(M * c.num_classes); o.gl = floats(M * c.num_classes);
    for (int l = 0; l < c.num_layers; ++l) {
        kws_train::Carved::Layer& y = o.layer[l];
        y.ar = floats(M * H); y.au = floats(M * H); y.ac = floats(M * H); y.hp = floats(M * H); y.rh = floats(M * H); y.y = floats(M * H);
        y.dhat = floats(M * 3 * H);
        const size_t in = (size_t)h->bl.layer[l].in;
        if (h->ln) { y.xhat = floats(M * in); y.xn = floats(M * in); y.rstd = floats(M); y.g = floats(M * in); y.gs = floats(M); }
        if (residual_on(h, l)) y.out = floats(M * H);
    }
    o.partial = floats((size_t)o.chunks * h->P);
    if (cv) *cv = o;
    return at;
}

// the products of the weight-gradient launch for the carved shape: per layer (Wg | Wc) x (input rows, state rows, bias), then the dense
// layer; with the layer norm the input rows are the taped xhat (on layer 0 too), and each layer adds the column sums of g (d igamma)
// and of gs (d ibeta) at wrap_layout's offsets
void build_jobs(kws_train* h) {
    const kws_config& c = h->cfg.model;
    const int H = c.hidden, C = c.num_classes;
    kws_train::Carved& cv = h->cv;
    h->jobs_host.clear();
    int unit = 0;
    auto add = [&](int src, const float* a, int lda, int K, const float* d, int ldd, int N, size_t out, int ldo) {
        kws::TrainWgradJob j = {};
        j.a = a; j.d = d; j.out = out; j.src = src; j.lda = lda; j.K = K; j.ldd = ldd; j.N = N; j.ldo = ldo; j.unit0 = unit;
        unit += ((K + 15) / 16) * ((N + 63) / 64);
        h->jobs_host.push_back(j);
    };
    for (int l = 0; l < c.num_layers; ++l) {
        const BlobLayout::Layer& b = h->bl.layer[l];
        const kws_train::Carved::Layer& y = cv.layer[l];
        const int in = b.in, src = l == 0 && !h->ln ? kws::kWgradInput : kws::kWgradRows;
        const float* below = h->ln ? y.xhat : l == 0 ? nullptr : layer_output(h, cv, l - 1);
        add(src, below, in, in, y.dhat, 3 * H, 2 * H, b.wg, 2 * H);
        add(kws::kWgradRows, y.hp, H, H, y.dhat, 3 * H, 2 * H, b.wg + (size_t)in * 2 * H, 2 * H);
        add(kws::kWgradOnes, nullptr, 0, 1, y.dhat, 3 * H, 2 * H, b.bg, 2 * H);
        add(src, below, in, in, y.dhat + 2 * H, 3 * H, H, b.wc, H);
        add(kws::kWgradRows, y.rh, H, H, y.dhat + 2 * H, 3 * H, H, b.wc + (size_t)in * H, H);
        add(kws::kWgradOnes, nullptr, 0, 1, y.dhat + 2 * H, 3 * H, H, b.bc, H);
    }
    add(kws::kWgradRows, layer_output(h, cv, c.num_layers - 1), H, H, cv.gl, C, C, h->bl.wfc, C);
    add(kws::kWgradOnes, nullptr, 0, 1, cv.gl, C, C, h->bl.bfc, C);
    for (int l = 0; h->ln && l < c.num_layers; ++l) {
        const int in = h->bl.layer[l].in;
        add(kws::kWgradOnes, nullptr, 0, 1, cv.layer[l].gs, 1, 1, h->wl.ibeta[l], 1);
        add(kws::kWgradOnes, nullptr, 0, 1, cv.layer[l].g, in, in, h->wl.igamma[l], in);
    }
    cv.units = unit;
}

// the arena for (B, T, S_max): grown if it has to be (waits for the device once), carved anew when the shape differs from the last call's
int prepare_shape(kws_train* h, int B, int T, int S_max) {
    if (h->cv.B == B && h->cv.T == T && h->cv.S_max == S_max && h->arena) return KWS_OK;
    const size_t need = carve(h, B, T, S_max, nullptr, nullptr);
    if (need > h->arena_bytes) {
        size_t free_b = 0, total_b = 0;
        KWS_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + h->arena_bytes)
            return fail(KWS_ERR_OUT_OF_MEMORY, "the tape of B=%d utterances x T=%d frames x %d layers takes %zu bytes: the device has %zu free "
                        "(%zu in all; fewer utterances per step or shorter ones)", B, T, h->cfg.model.num_layers, need, free_b + h->arena_bytes, total_b);
        KWS_HIP(hipDeviceSynchronize());
        if (h->arena) (void)hipFree(h->arena);
        h->arena = nullptr; h->arena_bytes = 0; h->cv = kws_train::Carved(); h->ints_host.clear();
        KWS_HIP(hipMalloc(reinterpret_cast<void**>(&h->arena), need));
        h->arena_bytes = need;
        ++h->allocs;
    }
    carve(h, B, T, S_max, h->arena, &h->cv);
    h->ints_host.clear();
    build_jobs(h);
    h->jobs_dirty = true;
    return KWS_OK;
}

int check_call(const kws_train_config& cfg, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
               int S_max, const float* loss) {
    if (B < 1 || T < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d: at least one utterance and one frame", B, T);
    if (S_max < 0 || S_max > 31)
        return fail(KWS_ERR_INVALID_ARGUMENT, "S_max=%d out of range [0,31]: one lane of a wave per state of the extended label", S_max);
    if (!x || !seq_len || !label_len || !loss || (!labels && S_max > 0)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(x) || misaligned(loss)) return fail(KWS_ERR_INVALID_ARGUMENT, "x and loss must be 4-byte aligned");
    if ((size_t)B * T > (size_t)0x7fffffff) return fail(KWS_ERR_UNSUPPORTED, "B=%d x T=%d: more than 2^31 - 1 frames in one call", B, T);
    KWS_TRY(check_labels(seq_len, labels, label_len, B, T, S_max, cfg.model.num_classes));
    const size_t lds = kws::ctc_loss_lds_bytes(T, S_max);
    if (lds > kWindowIncLdsMax)
        return fail(KWS_ERR_UNSUPPORTED, "the CTC loss keeps %d frames x (8 log-probabilities + %d states) in LDS: %zu bytes exceed the %zu a "
                    "workgroup may hold", T, 2 * S_max + 1, lds, kWindowIncLdsMax);
    return KWS_OK;
}

// the state pointers of a kws_train_*_state call: the kernels read and write a stream's state 16 bytes at a time
int check_state_io(const kws_train_state_io* io) {
    if (!io) return KWS_OK;
    const struct { const char* name; const void* p; } f[4] = {{"state_in", io->state_in}, {"state_out", io->state_out},
                                                            {"dstate_out", io->dstate_out}, {"dstate_in", io->dstate_in}};
    for (const auto& e : f)
        if (reinterpret_cast<uintptr_t>(e.p) % 16 != 0)
            return fail(KWS_ERR_INVALID_ARGUMENT, "io->%s must be 16-byte aligned (a lane moves four units of a stream's state at a time)", e.name);
    return KWS_OK;
}
// a call from or to a carried state: any of the four fields set (none: the plain call, its launches and its bits)
bool carries_state(const kws_train_state_io* io) { return io && (io->state_in || io->state_out || io->dstate_out || io->dstate_in); }

#define KWS_LAUNCH(h, call, what) do { KWS_TRY(hip_done((call), what)); ++(h)->launches; } while (0)

// forward, loss, backward: leaves loss [B], the logits and the gradient of sum(loss) / B + <dstate_out, state_out> (h->grad, with the sums
// of squares of its blocks); io: null or all null for the zero state and no state outputs
int grad_impl(kws_train* h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int S_max,
              const uint8_t* drop, float* loss, const kws_train_state_io* io, hipStream_t st) {
    const kws_config& c = h->cfg.model;
    const int H = c.hidden, C = c.num_classes, L = c.num_layers, M = B * T;
    const bool stateful = carries_state(io);
    const size_t state_layer = (size_t)B * H;          // floats of one layer of [L, B, H]
    KWS_TRY(prepare_shape(h, B, T, S_max));
    kws_train::Carved& cv = h->cv;
    if (h->jobs_dirty) {
        KWS_HIP(hipMemcpyAsync(cv.jobs, h->jobs_host.data(), h->jobs_host.size() * sizeof(kws::TrainWgradJob), hipMemcpyHostToDevice, st));
        h->jobs_dirty = false;
    }
    std::vector<int32_t> ints;
    pack_ints(seq_len, labels, label_len, B, S_max, &ints);
    if (ints != h->ints_host) {
        KWS_HIP(hipMemcpyAsync(cv.ints, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        h->ints_host.swap(ints);
    }
    const int32_t *d_seq = cv.ints, *d_len = cv.ints + B, *d_lab = cv.ints + 2 * (size_t)B;
    h->launches = 0;
    KWS_LAUNCH(h, kws::launch_train_rowmask(d_seq, B, T, cv.live, st), "launch train_rowmask");
    // the masks: one per frame [L, B, T, H], or one per stream held for all frames [L, B, H] (variational_recurrent)
    const size_t drop_layer = (h->var ? (size_t)B : (size_t)M) * H;
    const int drop_bs = h->var ? 1 : T, drop_ts = h->var ? 0 : 1;
    for (int l = 0; l < L; ++l) {
        const kws::TrainPackLayer& pk = h->pack.layer[l];
        const kws_train::Carved::Layer& y = cv.layer[l];
        const float* in = l == 0 ? x : layer_output(h, cv, l - 1);
        if (h->ln) {
            kws::TrainLnForward n = {};
            n.in = in; n.live = cv.live; n.ibeta = h->theta + h->wl.ibeta[l]; n.igamma = h->theta + h->wl.igamma[l];
            n.xhat = y.xhat; n.xn = y.xn; n.rstd = y.rstd; n.M = M; n.I = pk.in;
            KWS_LAUNCH(h, kws::launch_train_ln_forward(n, st), "launch train_ln_forward");
        }
        kws::TrainRowsGemm g = {};
        g.a = h->ln ? y.xhat : in; g.lda = pk.in; g.live = cv.live;
        g.w = pk.wx; g.swk = 3 * H; g.swn = 1; g.bias = pk.b3;
        g.out = cv.xg; g.ldo = 3 * H; g.M = M; g.K = pk.in; g.N = 3 * H;
        KWS_LAUNCH(h, kws::launch_train_rows_gemm(g, st), "launch train_rows_gemm (x-part)");
        kws::TrainForwardParams f = {};
        f.xg = cv.xg; f.wh = pk.wh; f.seq_len = d_seq; f.drop = drop ? drop + (size_t)l * drop_layer : nullptr;
        f.drop_bs = drop_bs; f.drop_ts = drop_ts;
        f.ar = y.ar; f.au = y.au; f.ac = y.ac; f.hp = y.hp; f.rh = y.rh; f.y = y.y; f.keep_prob = h->cfg.keep_prob; f.B = B; f.T = T;
        if (stateful) {
            kws::TrainForwardStateParams fs = {};
            static_cast<kws::TrainForwardParams&>(fs) = f;
            fs.io.in = io->state_in ? io->state_in + l * state_layer : nullptr;
            fs.io.out = io->state_out ? io->state_out + l * state_layer : nullptr;
            KWS_LAUNCH(h, kws::launch_gru_train_forward_state(fs, H, st), "launch gru_train_forward_state");
        } else {
            KWS_LAUNCH(h, kws::launch_gru_train_forward(f, H, st), "launch gru_train_forward");
        }
        if (residual_on(h, l))          // both operands are zero rows at t >= seq_len: so is out
            KWS_LAUNCH(h, kws::launch_train_residual(y.y, in, kResidualScale, y.out, (size_t)M * H, st), "launch train_residual (forward)");
    }
    const float* wfc = h->theta + h->bl.wfc;
    {
        kws::TrainRowsGemm g = {};
        g.a = layer_output(h, cv, L - 1); g.lda = H; g.w = wfc; g.swk = C; g.swn = 1; g.bias = h->theta + h->bl.bfc;
        g.out = cv.logits; g.ldo = C; g.M = M; g.K = H; g.N = C;
        KWS_LAUNCH(h, kws::launch_train_rows_gemm(g, st), "launch train_rows_gemm (logits)");
    }
    KWS_LAUNCH(h, kws::launch_ctc_loss(cv.logits, d_seq, d_lab, d_len, B, T, C, S_max, loss, cv.gl, st), "launch ctc_loss");
    KWS_LAUNCH(h, kws::launch_train_scale(cv.gl, cv.logits, (size_t)M, C, 1.0f / (float)B, st), "launch train_scale");      // loss = sum_b ctc_b / B
    {
        kws::TrainRowsGemm g = {};          // dy_top = grad_logits . Wfc^T
        g.a = cv.gl; g.lda = C; g.w = wfc; g.swk = 1; g.swn = C;
        g.out = cv.dy[0]; g.ldo = H; g.M = M; g.K = C; g.N = H;
        KWS_LAUNCH(h, kws::launch_train_rows_gemm(g, st), "launch train_rows_gemm (dy of the top layer)");
    }
    int cur = 0;
    for (int l = L - 1; l >= 0; --l) {
        const kws::TrainPackLayer& pk = h->pack.layer[l];
        const kws_train::Carved::Layer& y = cv.layer[l];
        // cv.dy[cur] holds dout of this layer.  With the residual it becomes 0.7071 dout in place: the dy of the frame loop, and the
        // share of d in that is added behind the x-part's
        if (residual_on(h, l))
            KWS_LAUNCH(h, kws::launch_train_residual(cv.dy[cur], nullptr, kResidualScale, cv.dy[cur], (size_t)M * H, st), "launch train_residual (dout)");
        kws::TrainBackwardParams b = {};
        b.dy = cv.dy[cur]; b.wht = pk.wht; b.seq_len = d_seq; b.drop = drop ? drop + (size_t)l * drop_layer : nullptr;
        b.drop_bs = drop_bs; b.drop_ts = drop_ts;
        b.ar = y.ar; b.au = y.au; b.ac = y.ac; b.hp = y.hp; b.dhat = y.dhat; b.keep_prob = h->cfg.keep_prob; b.B = B; b.T = T;
        if (stateful) {
            kws::TrainBackwardStateParams bs = {};
            static_cast<kws::TrainBackwardParams&>(bs) = b;
            bs.io.in = io->dstate_out ? io->dstate_out + l * state_layer : nullptr;
            bs.io.out = io->dstate_in ? io->dstate_in + l * state_layer : nullptr;
            KWS_LAUNCH(h, kws::launch_gru_train_backward_state(bs, H, st), "launch gru_train_backward_state");
        } else {
            KWS_LAUNCH(h, kws::launch_gru_train_backward(b, H, st), "launch gru_train_backward");
        }
        if (l > 0 || h->ln) {          // [dr^ | du^ | dc^] . (Wg_x | Wc_x)^T: the dy of the layer below, or dxhat under the layer norm
            kws::TrainRowsGemm g = {};
            g.a = y.dhat; g.lda = 3 * H; g.w = pk.wx; g.swk = 1; g.swn = 3 * H;
            g.out = h->ln ? y.g : cv.dy[cur ^ 1]; g.ldo = pk.in; g.M = M; g.K = 3 * H; g.N = pk.in;
            KWS_LAUNCH(h, kws::launch_train_rows_gemm(g, st), "launch train_rows_gemm (dx)");
        }
        if (h->ln) {
            kws::TrainLnBackward n = {};
            n.g = y.g; n.xn = y.xn; n.rstd = y.rstd; n.live = cv.live; n.ibeta = h->theta + h->wl.ibeta[l];
            n.resid = residual_on(h, l) ? cv.dy[cur] : nullptr; n.din = l > 0 ? cv.dy[cur ^ 1] : nullptr; n.gs = y.gs; n.M = M; n.I = pk.in;
            KWS_LAUNCH(h, kws::launch_train_ln_backward(n, st), "launch train_ln_backward");
        } else if (residual_on(h, l)) {
            KWS_LAUNCH(h, kws::launch_train_residual(cv.dy[cur ^ 1], cv.dy[cur], 1.0f, cv.dy[cur ^ 1], (size_t)M * H, st), "launch train_residual (d in)");
        }
        if (l > 0) cur ^= 1;
    }
    KWS_LAUNCH(h, kws::launch_train_wgrad(cv.jobs, cv.njobs, cv.units, x, cv.live, M, cv.chunk_rows, cv.chunks, cv.partial, h->P, st),
               "launch train_wgrad");
    KWS_LAUNCH(h, kws::launch_train_reduce(cv.partial, cv.chunks, h->P, h->grad, h->sumsq, st), "launch train_reduce");
    return KWS_OK;
}

// clip over h->grad (its blocks' sums of squares in h->sumsq), one optimiser step with the handle's moments and step count, re-pack
int update_impl(kws_train* h, float lr, float* grad_norm_or_null, hipStream_t st) {
    const bool adam = h->cfg.optimizer == KWS_OPT_ADAM;
    const double step = (double)(h->steps + 1);
    const float lr_t = adam ? (float)((double)lr * sqrt(1.0 - pow(0.999, step)) / (1.0 - pow(0.9, step))) : lr;
    KWS_LAUNCH(h, kws::launch_train_update(h->theta, h->m, h->v, h->grad, h->sumsq, h->nred, h->P, adam ? 1 : 0, lr_t, h->cfg.max_grad_norm,
                                           grad_norm_or_null, st), "launch train_update");
    KWS_LAUNCH(h, kws::launch_train_pack(h->pack, st), "launch train_pack");
    ++h->steps;
    return KWS_OK;
}

// every refusal of kws_train_create (wrapped: of kws_train_create_wrapped) that needs no device
int check_config(const kws_train_config& cfg, bool wrapped) {
    const kws_config& c = cfg.model;
    if (c.use_relu || c.value_clip > 0.f)
        return fail(KWS_ERR_UNSUPPORTED, "model.use_relu=%d / model.value_clip=%g: training through relu and clip is out of scope (the gradient of "
                    "TensorFlow's relu and clip at their ties is not pinned)", c.use_relu, (double)c.value_clip);
    if (wrapped) {
        const struct { const char* name; int v; } sw[3] = {{"wrappers.use_layer_norm", cfg.wrappers.use_layer_norm},
                                                           {"wrappers.use_residual", cfg.wrappers.use_residual},
                                                           {"variational_recurrent", cfg.variational_recurrent}};
        for (const auto& f : sw)
            if (f.v != 0 && f.v != 1) return fail(KWS_ERR_INVALID_ARGUMENT, "%s=%d: 0 or 1", f.name, f.v);
    } else {
        if (cfg.wrappers.use_layer_norm || cfg.wrappers.use_residual)
            return fail(KWS_ERR_UNSUPPORTED, "wrappers.use_layer_norm=%d / wrappers.use_residual=%d: kws_train_create trains the plain cell "
                        "(the wrapped stack: kws_train_create_wrapped)", cfg.wrappers.use_layer_norm, cfg.wrappers.use_residual);
        if (cfg.variational_recurrent)
            return fail(KWS_ERR_UNSUPPORTED, "variational_recurrent=%d: kws_train_create takes one mask per frame (DropoutWrapper's default; "
                        "one mask per stream: kws_train_create_wrapped)", cfg.variational_recurrent);
    }
    if (c.precision != KWS_FP32) return fail(KWS_ERR_UNSUPPORTED, "model.precision=%d: training is fp32 (KWS_FP32) only", c.precision);
    if (!(cfg.keep_prob > 0.f && cfg.keep_prob <= 1.f))
        return fail(KWS_ERR_UNSUPPORTED, "keep_prob=%g outside (0, 1]", (double)cfg.keep_prob);
    if (cfg.optimizer != KWS_OPT_ADAM && cfg.optimizer != KWS_OPT_NESTEROV)
        return fail(KWS_ERR_INVALID_ARGUMENT, "optimizer=%d: KWS_OPT_ADAM (0) or KWS_OPT_NESTEROV (1)", cfg.optimizer);
    if (!std::isfinite(cfg.max_grad_norm)) return fail(KWS_ERR_INVALID_ARGUMENT, "max_grad_norm=%g is not finite", (double)cfg.max_grad_norm);
    if (c.hidden != 64 && c.hidden != 128 && c.hidden != 256) return fail(KWS_ERR_INVALID_ARGUMENT, "model.hidden=%d unsupported (64, 128, 256)", c.hidden);
    if (c.num_layers < 1 || c.num_layers > 8) return fail(KWS_ERR_INVALID_ARGUMENT, "model.num_layers=%d out of range [1,8]", c.num_layers);
    if (c.n_mel < 1 || c.n_mel > 1024) return fail(KWS_ERR_INVALID_ARGUMENT, "model.n_mel=%d out of range [1,1024]", c.n_mel);
    if (c.num_classes < 3 || c.num_classes > kws::kMaxClasses)
        return fail(KWS_ERR_INVALID_ARGUMENT, "model.num_classes=%d out of range [3,8]", c.num_classes);
    return KWS_OK;
}

int probe_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    return KWS_OK;
}

int create_impl(const kws_train_config* cfg, bool wrapped, kws_train_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    KWS_TRY(check_config(*cfg, wrapped));
    const kws_config& c = cfg->model;
    KWS_TRY(probe_device());
    kws_train* h = new (std::nothrow) kws_train();
    if (!h) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    h->cfg = *cfg;
    h->bl = blob_layout(c);
    h->wl = wrap_layout(c, cfg->wrappers);
    h->ln = cfg->wrappers.use_layer_norm != 0; h->res = cfg->wrappers.use_residual != 0; h->var = cfg->variational_recurrent != 0;
    h->P = h->wl.total;          // the canonical blob's, without the layer norm
    h->nred = kws::train_reduce_blocks(h->P);
    const size_t H = (size_t)c.hidden;
    size_t floats = 4 * h->P;
    size_t pk_at[8];
    for (int l = 0; l < c.num_layers; ++l) {
        pk_at[l] = floats;
        floats += ((size_t)h->bl.layer[l].in + 2 * H) * 3 * H + 3 * H;
    }
    floats = (floats + 1) & ~(size_t)1;          // the doubles behind it
    h->state_bytes = floats * sizeof(float) + (size_t)h->nred * sizeof(double);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->state), h->state_bytes);
    if (e == hipSuccess) e = hipMemset(h->state, 0, h->state_bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->last_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { kws_train_destroy(h); return hip_fail(e, "kws_train_create"); }
    h->theta = h->state; h->m = h->theta + h->P; h->v = h->m + h->P; h->grad = h->v + h->P;
    h->sumsq = reinterpret_cast<double*>(h->state + floats);
    h->pack.L = c.num_layers; h->pack.H = c.hidden;
    for (int l = 0; l < c.num_layers; ++l) {
        const BlobLayout::Layer& b = h->bl.layer[l];
        kws::TrainPackLayer& p = h->pack.layer[l];
        p.in = b.in;
        p.wg = h->theta + b.wg; p.bg = h->theta + b.bg; p.wc = h->theta + b.wc; p.bc = h->theta + b.bc;
        p.wx = h->state + pk_at[l]; p.wh = p.wx + (size_t)b.in * 3 * H; p.wht = p.wh + H * 3 * H; p.b3 = p.wht + 3 * H * H;
    }
    *out = h;
    return KWS_OK;
}

}  // namespace

extern "C" {

size_t kws_sizeof_train_config(void) { return sizeof(kws_train_config); }

int kws_train_create(const kws_train_config* cfg, kws_train_handle* out) { return create_impl(cfg, false, out); }
int kws_train_create_wrapped(const kws_train_config* cfg, kws_train_handle* out) { return create_impl(cfg, true, out); }

int kws_train_check(const kws_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                    int T, int S_max, const float* loss) {
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    KWS_TRY(check_config(*cfg, false));
    return check_call(*cfg, x, seq_len, labels, label_len, B, T, S_max, loss);
}

int kws_train_check_wrapped(const kws_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                            int B, int T, int S_max, const float* loss) {
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    KWS_TRY(check_config(*cfg, true));
    return check_call(*cfg, x, seq_len, labels, label_len, B, T, S_max, loss);
}

size_t kws_sizeof_train_state_io(void) { return sizeof(kws_train_state_io); }

int kws_train_check_state(const kws_train_config* cfg, int wrapped, const float* x, const int32_t* seq_len, const int32_t* labels,
                          const int32_t* label_len, int B, int T, int S_max, const float* loss, const kws_train_state_io* io) {
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    KWS_TRY(check_config(*cfg, wrapped != 0));
    KWS_TRY(check_call(*cfg, x, seq_len, labels, label_len, B, T, S_max, loss));
    return check_state_io(io);
}

int kws_train_destroy(kws_train_handle h) {
    if (!h) return KWS_OK;
    hipDeviceSynchronize();
    if (h->state) hipFree(h->state);
    if (h->arena) hipFree(h->arena);
    if (h->last_done) hipEventDestroy(h->last_done);
    delete h;
    return KWS_OK;
}

int kws_train_set_weights(kws_train_handle h, const void* blob, size_t nbytes, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (nbytes != h->P * sizeof(float)) return fail(KWS_ERR_INVALID_ARGUMENT, "the weight blob has %zu bytes, the config needs %zu", nbytes, h->P * sizeof(float));
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(train_enter(h, st));
    KWS_TRY(train_finish(h, st, [&]() -> int {
        KWS_HIP(hipMemcpyAsync(h->theta, blob, nbytes, hipMemcpyHostToDevice, st));
        KWS_HIP(hipMemsetAsync(h->m, 0, 2 * h->P * sizeof(float), st));
        KWS_TRY(hip_done(kws::launch_train_pack(h->pack, st), "launch train_pack"));
        h->steps = 0;
        return KWS_OK;
    }()));
    KWS_HIP(hipStreamSynchronize(st));
    return KWS_OK;
}

int kws_train_get_weights(kws_train_handle h, void* blob, size_t nbytes, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (nbytes != h->P * sizeof(float)) return fail(KWS_ERR_INVALID_ARGUMENT, "the weight blob has %zu bytes, the config needs %zu", nbytes, h->P * sizeof(float));
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(train_enter(h, st));
    KWS_TRY(train_finish(h, st, hip_done(hipMemcpyAsync(blob, h->theta, nbytes, hipMemcpyDeviceToHost, st), "copy of the weights")));
    KWS_HIP(hipStreamSynchronize(st));
    return KWS_OK;
}

int kws_train_moments(kws_train_handle h, float* m, float* v, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!m || !v) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(train_enter(h, st));
    KWS_TRY(train_finish(h, st, [&]() -> int {
        KWS_HIP(hipMemcpyAsync(m, h->m, h->P * sizeof(float), hipMemcpyDeviceToHost, st));
        KWS_HIP(hipMemcpyAsync(v, h->v, h->P * sizeof(float), hipMemcpyDeviceToHost, st));
        return KWS_OK;
    }()));
    KWS_HIP(hipStreamSynchronize(st));
    return KWS_OK;
}

int kws_train_reserve(kws_train_handle h, int B, int T, int S_max) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (B < 1 || T < 1 || S_max < 0 || S_max > 31) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d S_max=%d", B, T, S_max);
    if ((size_t)B * T > (size_t)0x7fffffff) return fail(KWS_ERR_UNSUPPORTED, "B=%d x T=%d: more than 2^31 - 1 frames in one call", B, T);
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    return prepare_shape(h, B, T, S_max);      // the job table goes to the device with the next call, on its stream
}

int kws_train_grad(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                   int S_max, const uint8_t* drop_or_null, float* loss, float* grad_blob, float* logits_or_null, void* stream) {
    return kws_train_grad_state(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, loss, grad_blob, logits_or_null, nullptr, stream);
}

int kws_train_grad_state(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                         int T, int S_max, const uint8_t* drop_or_null, float* loss, float* grad_blob, float* logits_or_null,
                         const kws_train_state_io* io, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_call(h->cfg, x, seq_len, labels, label_len, B, T, S_max, loss));
    if (!grad_blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(grad_blob) || misaligned(logits_or_null) || misaligned(drop_or_null))
        return fail(KWS_ERR_INVALID_ARGUMENT, "grad_blob, logits and drop must be 4-byte aligned (the masks are read four units at a time)");
    KWS_TRY(check_state_io(io));
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(train_enter(h, st));
    return train_finish(h, st, [&]() -> int {
        KWS_TRY(grad_impl(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, loss, io, st));
        KWS_HIP(hipMemcpyAsync(grad_blob, h->grad, h->P * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (logits_or_null)
            KWS_HIP(hipMemcpyAsync(logits_or_null, h->cv.logits, (size_t)B * T * h->cfg.model.num_classes * sizeof(float), hipMemcpyDeviceToDevice, st));
        return KWS_OK;
    }());
}

int kws_train_step(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                   int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null, void* stream) {
    return kws_train_step_state(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, lr, loss, grad_norm_or_null, nullptr, stream);
}

int kws_train_step_state(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                         int T, int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null,
                         const kws_train_state_io* io, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_call(h->cfg, x, seq_len, labels, label_len, B, T, S_max, loss));
    if (!(lr > 0.f) || !std::isfinite(lr)) return fail(KWS_ERR_INVALID_ARGUMENT, "lr=%g has to be positive and finite", (double)lr);
    if (misaligned(grad_norm_or_null) || misaligned(drop_or_null))
        return fail(KWS_ERR_INVALID_ARGUMENT, "grad_norm and drop must be 4-byte aligned (the masks are read four units at a time)");
    KWS_TRY(check_state_io(io));
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(train_enter(h, st));
    return train_finish(h, st, [&]() -> int {
        KWS_TRY(grad_impl(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, loss, io, st));
        return update_impl(h, lr, grad_norm_or_null, st);
    }());
}

int kws_train_apply(kws_train_handle h, const float* grad_blob, float lr, float* grad_norm_or_null, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!grad_blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (!(lr > 0.f) || !std::isfinite(lr)) return fail(KWS_ERR_INVALID_ARGUMENT, "lr=%g has to be positive and finite", (double)lr);
    if (misaligned(grad_blob) || misaligned(grad_norm_or_null)) return fail(KWS_ERR_INVALID_ARGUMENT, "grad_blob and grad_norm must be 4-byte aligned");
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KWS_TRY(train_enter(h, st));
    return train_finish(h, st, [&]() -> int {
        h->launches = 0;
        // the caller's gradient as the one chunk of the reduction: h->grad = 0 + g, the blocks' sums of squares as behind a backward pass
        KWS_LAUNCH(h, kws::launch_train_reduce(grad_blob, 1, h->P, h->grad, h->sumsq, st), "launch train_reduce");
        return update_impl(h, lr, grad_norm_or_null, st);
    }());
}

int kws_train_stats(kws_train_handle h, size_t* device_bytes, int32_t* allocs, int32_t* steps, int32_t* launches, int32_t* chunk_rows) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (device_bytes) *device_bytes = h->state_bytes + h->arena_bytes;
    if (allocs) *allocs = h->allocs;
    if (steps) *steps = h->steps;
    if (launches) *launches = h->launches;
    if (chunk_rows) *chunk_rows = h->cv.chunk_rows;
    return KWS_OK;
}

}  // extern "C"
