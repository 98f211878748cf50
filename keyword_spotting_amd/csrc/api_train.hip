// C ABI of libkws_amd.so (include/kws_amd.h): the train handle -- taped forward, back-propagation through time, the CTC loss through
// ctc_loss_kernel, global-norm clipping and Adam / Nesterov on the canonical blob (gru_train.hip, train_kernels.hip), with the cell
// wrappers of kws_train_create_wrapped around the two frame loops (train_wrap_kernels.hip).  The _frames entry points put the frame-wise
// cross-entropy (frame_loss_kernels.hip) in the CTC loss's place or on top of it: grad_impl's ft.
#include <new>

#include "train_core.h"

using namespace kws_host;

struct kws_train : TrainCore {       // tail: the packed copies of every layer (wx, wh, wht, b3)
    kws_train_config cfg;
    BlobLayout bl;
    WrapLayout wl;                   // the layer norm's ibeta / igamma behind the canonical blob (kws_train_create_wrapped)
    bool ln = false, res = false, var = false;      // wrappers.use_layer_norm, wrappers.use_residual, variational_recurrent
    kws::TrainPackParams pack = {};
    // the arena, carved for the shape of the call (carve): lengths and labels, the row mask, the job table of the
    // weight-gradient launch, the tape, the gradients of the activations, the row chunks' partial weight gradients.  With the layer norm
    // a layer also keeps xhat and xn [M, I_l] and rstd [M] from the forward, g = dxhat [M, I_l] and gs [M] (the rows' terms of d ibeta)
    // from the backward; with the residual a layer >= 1 keeps out [M, H] = 0.7071 (y + its input)
    struct Carved {
        int B = 0, T = 0, S_max = -1;
        int32_t* ints = nullptr;
        uint8_t* live = nullptr;
        kws::TrainWgradJob* jobs = nullptr;
        float *xg = nullptr, *dy[2] = {nullptr, nullptr}, *logits = nullptr, *gl = nullptr, *partial = nullptr;
        struct Layer { float *ar, *au, *ac, *hp, *rh, *y, *dhat, *xhat, *xn, *rstd, *g, *gs, *out; } layer[8] = {};   // ar, au, ac: the pre-activations of r, u, c
        int njobs = 0, chunk_rows = 0, chunks = 0;
    } cv;
};

namespace {

constexpr float kResidualScale = 0.7071067811865475f;      // utils/custom_wrapper.py:116

bool residual_on(const kws_train* h, int l) { return h->res && l >= 1; }
// what layer l hands to the layer above and to the dense layer
const float* layer_output(const kws_train* h, const kws_train::Carved& cv, int l) { return residual_on(h, l) ? cv.layer[l].out : cv.layer[l].y; }

// Lays the arena out for (B, T, S_max).  base == null: only the size.  Returns the bytes.
size_t carve(const kws_train* h, int B, int T, int S_max, char* base, kws_train::Carved* cv) {
    const kws_config& c = h->cfg.model;
    const size_t M = (size_t)B * T, H = (size_t)c.hidden;
    Carver cut(base);
    kws_train::Carved o;
    o.B = B; o.T = T; o.S_max = S_max;
    o.njobs = (h->ln ? 8 : 6) * c.num_layers + 2;
    o.chunk_rows = wgrad_chunk_rows(M);
    o.chunks = (int)((M + o.chunk_rows - 1) / o.chunk_rows);
    o.ints = reinterpret_cast<int32_t*>(cut.take(((size_t)B * (2 + S_max) + kws::kMaxClasses) * sizeof(int32_t)));      // ... | class weights
    o.live = reinterpret_cast<uint8_t*>(cut.take(M));
    o.jobs = reinterpret_cast<kws::TrainWgradJob*>(cut.take((size_t)o.njobs * sizeof(kws::TrainWgradJob)));
    o.xg = cut.floats(M * 3 * H);
    o.dy[0] = cut.floats(M * H); o.dy[1] = cut.floats(M * H);
    o.logits = cut.floats(M * c.num_classes); o.gl = cut.floats(M * c.num_classes);
    for (int l = 0; l < c.num_layers; ++l) {
        kws_train::Carved::Layer& y = o.layer[l];
        y.ar = cut.floats(M * H); y.au = cut.floats(M * H); y.ac = cut.floats(M * H); y.hp = cut.floats(M * H); y.rh = cut.floats(M * H); y.y = cut.floats(M * H);
        y.dhat = cut.floats(M * 3 * H);
        const size_t in = (size_t)h->bl.layer[l].in;
        if (h->ln) { y.xhat = cut.floats(M * in); y.xn = cut.floats(M * in); y.rstd = cut.floats(M); y.g = cut.floats(M * in); y.gs = cut.floats(M); }
        if (residual_on(h, l)) y.out = cut.floats(M * H);
    }
    o.partial = cut.floats((size_t)o.chunks * h->P);
    if (cv) *cv = o;
    return cut.at;
}

// the products of the weight-gradient launch for the carved shape: per layer (Wg | Wc) x (input rows, state rows, bias), then the dense
// layer; with the layer norm the input rows are the taped xhat (on layer 0 too), and each layer adds the column sums of g (d igamma)
// and of gs (d ibeta) at wrap_layout's offsets
void build_jobs(kws_train* h) {
    const kws_config& c = h->cfg.model;
    const int H = c.hidden, C = c.num_classes;
    const kws_train::Carved& cv = h->cv;
    for (int l = 0; l < c.num_layers; ++l) {
        const BlobLayout::Layer& b = h->bl.layer[l];
        const kws_train::Carved::Layer& y = cv.layer[l];
        const int in = b.in, src = l == 0 && !h->ln ? kws::kWgradInput : kws::kWgradRows;
        const float* below = h->ln ? y.xhat : l == 0 ? nullptr : layer_output(h, cv, l - 1);
        h->add_job(src, below, in, in, y.dhat, 3 * H, 2 * H, b.wg, 2 * H);
        h->add_job(kws::kWgradRows, y.hp, H, H, y.dhat, 3 * H, 2 * H, b.wg + (size_t)in * 2 * H, 2 * H);
        h->add_job(kws::kWgradOnes, nullptr, 0, 1, y.dhat, 3 * H, 2 * H, b.bg, 2 * H);
        h->add_job(src, below, in, in, y.dhat + 2 * H, 3 * H, H, b.wc, H);
        h->add_job(kws::kWgradRows, y.rh, H, H, y.dhat + 2 * H, 3 * H, H, b.wc + (size_t)in * H, H);
        h->add_job(kws::kWgradOnes, nullptr, 0, 1, y.dhat + 2 * H, 3 * H, H, b.bc, H);
    }
    h->add_job(kws::kWgradRows, layer_output(h, cv, c.num_layers - 1), H, H, cv.gl, C, C, h->bl.wfc, C);
    h->add_job(kws::kWgradOnes, nullptr, 0, 1, cv.gl, C, C, h->bl.bfc, C);
    for (int l = 0; h->ln && l < c.num_layers; ++l) {
        const int in = h->bl.layer[l].in;
        h->add_job(kws::kWgradOnes, nullptr, 0, 1, cv.layer[l].gs, 1, 1, h->wl.ibeta[l], 1);
        h->add_job(kws::kWgradOnes, nullptr, 0, 1, cv.layer[l].g, in, in, h->wl.igamma[l], in);
    }
}

// the arena for (B, T, S_max): grown if it has to be (waits for the device once), carved anew when the shape differs from the last call's
int prepare_shape(kws_train* h, int B, int T, int S_max) {
    if (h->cv.B == B && h->cv.T == T && h->cv.S_max == S_max && h->arena) return KWS_OK;
    const int rc = train_arena_reserve(h, carve(h, B, T, S_max, nullptr, nullptr), B, T, h->cfg.model.num_layers);
    if (!h->arena) h->cv = kws_train::Carved();      // freed and not replaced: no layout
    KWS_TRY(rc);
    carve(h, B, T, S_max, h->arena, &h->cv);
    build_jobs(h);
    return KWS_OK;
}

// ctc false (a _frames call with ctc_weight 0): nothing about the labels, S_max or the LDS of ctc_loss_kernel
int check_call(const kws_train_config& cfg, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
               int S_max, const float* loss, bool ctc = true) {
    if (B < 1 || T < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d: at least one utterance and one frame", B, T);
    if (ctc) KWS_TRY(check_s_max(S_max));
    if (!x || !seq_len || !loss || (ctc && (!label_len || (!labels && S_max > 0)))) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(x) || misaligned(loss)) return fail(KWS_ERR_INVALID_ARGUMENT, "x and loss must be 4-byte aligned");
    if ((size_t)B * T > (size_t)0x7fffffff) return fail(KWS_ERR_UNSUPPORTED, "B=%d x T=%d: more than 2^31 - 1 frames in one call", B, T);
    if (!ctc) return check_seq_len(seq_len, B, T);
    KWS_TRY(check_labels(seq_len, labels, label_len, B, T, S_max, cfg.model.num_classes));
    return check_ctc_lds(T, S_max, "%d frames");
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

// forward, loss, backward: leaves loss [B], the logits and the gradient of sum(loss) / B + <dstate_out, state_out> (h->grad, with the sums
// of squares of its blocks); io: null or all null for the zero state and no state outputs.  ft: null for the CTC loss alone, else loss[b] =
// ctc_weight ctc_b + frame_weight ce_b on ft's targets (ctc_weight 0: labels, label_len and S_max are not looked at)
int grad_impl(kws_train* h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T, int S_max,
              const uint8_t* drop, float* loss, const kws_train_state_io* io, const kws_frame_targets* ft, hipStream_t st) {
    const kws_config& c = h->cfg.model;
    const int H = c.hidden, C = c.num_classes, L = c.num_layers, M = B * T;
    const bool stateful = carries_state(io);
    const bool ctc = !ft || ft->ctc_weight > 0.f, frames = ft && ft->frame_weight > 0.f;
    const size_t state_layer = (size_t)B * H;          // floats of one layer of [L, B, H]
    std::vector<int32_t> no_labels;
    if (!ctc) { no_labels.assign((size_t)B, 0); labels = nullptr; label_len = no_labels.data(); S_max = 0; }
    KWS_TRY(prepare_shape(h, B, T, S_max));
    kws_train::Carved& cv = h->cv;
    std::vector<int32_t> ints;
    pack_ints(seq_len, labels, label_len, B, S_max, &ints);
    if (frames) append_class_weights(ft->class_weight, C, &ints);
    KWS_TRY(train_upload(h, cv.jobs, cv.ints, &ints, st));
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
    if (ctc) {          // J = sum_b ctc_weight ctc_b / B (ctc_weight: 1 without frame targets)
        KWS_LAUNCH(h, kws::launch_ctc_loss(cv.logits, d_seq, d_lab, d_len, B, T, C, S_max, loss, cv.gl, st), "launch ctc_loss");
        KWS_LAUNCH(h, kws::launch_train_scale(cv.gl, cv.logits, (size_t)M, C, (ft ? ft->ctc_weight : 1.0f) / (float)B, st), "launch train_scale");
    }
    if (frames) {       // ... + sum_b frame_weight ce_b / B: alone it writes every row of the gradient, behind the CTC term it adds to it
        kws::FrameLossParams p = train_frame_term(*ft, B);
        p.logits = cv.logits; p.seq_len = d_seq; p.weight = reinterpret_cast<const float*>(cv.ints + (size_t)B * (2 + S_max));
        p.loss = loss; p.grad = cv.gl; p.T = T; p.C = C;
        KWS_LAUNCH(h, kws::launch_frame_loss(p, B, st), "launch frame_loss");
    }
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
    KWS_LAUNCH(h, kws::launch_train_wgrad(cv.jobs, cv.njobs, h->units, x, cv.live, M, cv.chunk_rows, cv.chunks, cv.partial, h->P, st),
               "launch train_wgrad");
    KWS_LAUNCH(h, kws::launch_train_reduce(cv.partial, cv.chunks, h->P, h->grad, h->sumsq, st), "launch train_reduce");
    return KWS_OK;
}

// the optimiser step over h->grad, then the packed copies of the new weights
int update_impl(kws_train* h, float lr, float* grad_norm_or_null, hipStream_t st) {
    KWS_TRY(train_update(h, lr, grad_norm_or_null, st));
    KWS_LAUNCH(h, kws::launch_train_pack(h->pack, st), "launch train_pack");
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
    KWS_TRY(check_optimizer(cfg.keep_prob, cfg.optimizer, cfg.max_grad_norm));
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
    h->optimizer = cfg->optimizer; h->max_grad_norm = cfg->max_grad_norm;
    const size_t H = (size_t)c.hidden;
    size_t pk_at[8], packed = 0;
    for (int l = 0; l < c.num_layers; ++l) {
        pk_at[l] = packed;
        packed += ((size_t)h->bl.layer[l].in + 2 * H) * 3 * H + 3 * H;
    }
    // wl.total: the canonical blob's, without the layer norm
    const int rc = train_core_create(h, h->wl.total, packed, nullptr, "kws_train_create");
    if (rc != KWS_OK) { delete h; return rc; }
    h->pack.L = c.num_layers; h->pack.H = c.hidden;
    for (int l = 0; l < c.num_layers; ++l) {
        const BlobLayout::Layer& b = h->bl.layer[l];
        kws::TrainPackLayer& p = h->pack.layer[l];
        p.in = b.in;
        p.wg = h->theta + b.wg; p.bg = h->theta + b.bg; p.wc = h->theta + b.wc; p.bc = h->theta + b.bc;
        p.wx = h->tail + pk_at[l]; p.wh = p.wx + (size_t)b.in * 3 * H; p.wht = p.wh + H * 3 * H; p.b3 = p.wht + 3 * H * H;
    }
    *out = h;
    return KWS_OK;
}

// kws_train_grad_state (ft null) and kws_train_grad_frames (ft checked)
int grad_call(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                     int S_max, const uint8_t* drop_or_null, float* loss, float* grad_blob, float* logits_or_null, const kws_train_state_io* io,
                     const kws_frame_targets* ft, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_call(h->cfg, x, seq_len, labels, label_len, B, T, S_max, loss, !ft || ft->ctc_weight > 0.f));
    if (!grad_blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(grad_blob) || misaligned(logits_or_null) || misaligned(drop_or_null))
        return fail(KWS_ERR_INVALID_ARGUMENT, "grad_blob, logits and drop must be 4-byte aligned (the masks are read four units at a time)");
    KWS_TRY(check_state_io(io));
    return train_call(h, stream, [&](hipStream_t st) -> int {
        KWS_TRY(grad_impl(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, loss, io, ft, st));
        KWS_HIP(hipMemcpyAsync(grad_blob, h->grad, h->P * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (logits_or_null)
            KWS_HIP(hipMemcpyAsync(logits_or_null, h->cv.logits, (size_t)B * T * h->cfg.model.num_classes * sizeof(float), hipMemcpyDeviceToDevice, st));
        return KWS_OK;
    });
}

// kws_train_step_state (ft null) and kws_train_step_frames (ft checked)
int step_call(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                     int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null, const kws_train_state_io* io,
                     const kws_frame_targets* ft, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_call(h->cfg, x, seq_len, labels, label_len, B, T, S_max, loss, !ft || ft->ctc_weight > 0.f));
    if (!(lr > 0.f) || !std::isfinite(lr)) return fail(KWS_ERR_INVALID_ARGUMENT, "lr=%g has to be positive and finite", (double)lr);
    if (misaligned(grad_norm_or_null) || misaligned(drop_or_null))
        return fail(KWS_ERR_INVALID_ARGUMENT, "grad_norm and drop must be 4-byte aligned (the masks are read four units at a time)");
    KWS_TRY(check_state_io(io));
    return train_call(h, stream, [&](hipStream_t st) -> int {
        KWS_TRY(grad_impl(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, loss, io, ft, st));
        return update_impl(h, lr, grad_norm_or_null, st);
    });
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

int kws_train_check_frames(const kws_train_config* cfg, int wrapped, const float* x, const int32_t* seq_len, const int32_t* labels,
                           const int32_t* label_len, int B, int T, int S_max, const float* loss, const kws_train_state_io* io,
                           const kws_frame_targets* ft) {
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    KWS_TRY(check_config(*cfg, wrapped != 0));
    KWS_TRY(check_frame_targets(ft, cfg->model.num_classes));
    KWS_TRY(check_call(*cfg, x, seq_len, labels, label_len, B, T, S_max, loss, ft->ctc_weight > 0.f));
    return check_state_io(io);
}

int kws_train_destroy(kws_train_handle h) {
    if (!h) return KWS_OK;
    train_core_destroy(h);
    delete h;
    return KWS_OK;
}

int kws_train_set_weights(kws_train_handle h, const void* blob, size_t nbytes, void* stream) {
    return train_set_weights(h, blob, nbytes, stream, [h](hipStream_t st) { return hip_done(kws::launch_train_pack(h->pack, st), "launch train_pack"); });
}
int kws_train_get_weights(kws_train_handle h, void* blob, size_t nbytes, void* stream) { return train_get_weights(h, blob, nbytes, stream); }
int kws_train_moments(kws_train_handle h, float* m, float* v, void* stream) { return train_moments(h, m, v, stream); }

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
    return grad_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, loss, grad_blob, logits_or_null, io, nullptr, stream);
}

int kws_train_grad_frames(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                          int T, int S_max, const uint8_t* drop_or_null, float* loss, float* grad_blob, float* logits_or_null,
                          const kws_train_state_io* io, const kws_frame_targets* ft, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_frame_targets(ft, h->cfg.model.num_classes));
    return grad_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, loss, grad_blob, logits_or_null, io, ft, stream);
}

int kws_train_step(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                   int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null, void* stream) {
    return kws_train_step_state(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, lr, loss, grad_norm_or_null, nullptr, stream);
}

int kws_train_step_state(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                         int T, int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null,
                         const kws_train_state_io* io, void* stream) {
    return step_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, lr, loss, grad_norm_or_null, io, nullptr, stream);
}

int kws_train_step_frames(kws_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
                          int T, int S_max, const uint8_t* drop_or_null, float lr, float* loss, float* grad_norm_or_null,
                          const kws_train_state_io* io, const kws_frame_targets* ft, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_frame_targets(ft, h->cfg.model.num_classes));
    return step_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_or_null, lr, loss, grad_norm_or_null, io, ft, stream);
}

int kws_train_apply(kws_train_handle h, const float* grad_blob, float lr, float* grad_norm_or_null, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    if (!grad_blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (!(lr > 0.f) || !std::isfinite(lr)) return fail(KWS_ERR_INVALID_ARGUMENT, "lr=%g has to be positive and finite", (double)lr);
    if (misaligned(grad_blob) || misaligned(grad_norm_or_null)) return fail(KWS_ERR_INVALID_ARGUMENT, "grad_blob and grad_norm must be 4-byte aligned");
    return train_call(h, stream, [&](hipStream_t st) -> int {
        h->launches = 0;
        // the caller's gradient as the one chunk of the reduction: h->grad = 0 + g, the blocks' sums of squares as behind a backward pass
        KWS_LAUNCH(h, kws::launch_train_reduce(grad_blob, 1, h->P, h->grad, h->sumsq, st), "launch train_reduce");
        return update_impl(h, lr, grad_norm_or_null, st);
    });
}

int kws_train_stats(kws_train_handle h, size_t* device_bytes, int32_t* allocs, int32_t* steps, int32_t* launches, int32_t* chunk_rows) {
    return train_stats(h, h ? h->cv.chunk_rows : 0, device_bytes, allocs, steps, launches, chunk_rows);
}

}  // extern "C"
