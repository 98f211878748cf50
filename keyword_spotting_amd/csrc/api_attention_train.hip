// C ABI of libkws_amd.so (include/kws_amd.h): the train handle of the self-attention CTC model -- taped forward, backward, the CTC loss
// through ctc_loss_kernel, global-norm clipping and Adam / Nesterov on the canonical blob.  The model-specific kernels are
// attention_train_kernels.hip; every product with a weight matrix, every weight gradient and the update are train_kernels.hip's.
//
// Launches of a kws_attention_train_grad call, L layers (kws_attention_train_stats counts them: 12 + 19 L + use_relu; _step: one more):
//   rowmask, stack, gemm (embedding), addpe
//   per layer: gemm (qkv), core forward, resid, ln forward, gemm (W1), relu, gemm (W2), resid, ln forward
//   gemm (logits), relu / dead rows, ctc_loss, scale, [relumask]      (_frames: frame_loss in place of ctc_loss + scale, or behind them)
//   gemm (d of the top layer's output)
//   per layer, top down: ln_b sums, ln_b apply, gemm (dh), relumask, gemm (dy), ln_a sums, ln_a apply, core dq, core dk/dv, gemm (dx)
//   residual (d of the embedding), wgrad, reduce
#include <new>

#include "train_core.h"
#include "attention_internal.h"

using namespace kws_host;

struct kws_attention_train : TrainCore {      // tail: the positional table
    kws_attention_train_config cfg;
    AttnLayout lay;
    int pe_rows = 0;
    // the arena, carved for the shape of the call
    struct Carved {
        int B = 0, T = 0, T1 = 0, S_max = -1;
        int32_t* ints = nullptr;          // T'_b [B] | label_len [B] | labels [B, S_max] | T_b [B] | class weights [8] (frame targets)
        uint8_t* live = nullptr;
        kws::TrainWgradJob* jobs = nullptr;
        float *xs = nullptr, *x[9] = {}, *sh[5] = {}, *de = nullptr, *logits = nullptr, *gl = nullptr, *dsum = nullptr, *partial = nullptr;
        float4* part = nullptr;
        float2* sums = nullptr;
        struct Layer { float *qkv, *att, *lse, *xn_a, *y, *hin, *xn_b, *rstd_a, *rstd_b, *dy_b, *prod_b, *dz, *dh, *dy_a, *prod_a, *dqkv; } layer[8] = {};
        int njobs = 0, chunk_rows = 0, chunks = 0;
    } cv;
};

namespace {

typedef kws_attention_train Handle;
constexpr size_t kMaxRows = (size_t)1 << 28;

int frames_out(const kws_attention_config& c, int T) { return c.combine_frame > 1 ? T / c.combine_frame + 1 : T; }

// Lays the arena out for (B, T, S_max).  base == null: only the size.
size_t carve(const Handle* h, int B, int T, int S_max, char* base, Handle::Carved* cv) {
    const kws_attention_config& c = h->cfg.model;
    const int T1 = frames_out(c, T), ntile = (T1 + kws::kAttnRows - 1) / kws::kAttnRows;
    const size_t M = (size_t)B * T1, H = (size_t)c.hidden, Fi = (size_t)c.ffn_inner, NH = (size_t)c.num_heads, C = (size_t)c.num_classes;
    Carver cut(base);
    Handle::Carved o;
    o.B = B; o.T = T; o.T1 = T1; o.S_max = S_max;
    o.njobs = 4 + 10 * c.num_layers;
    o.chunk_rows = wgrad_chunk_rows(M);
    o.chunks = (int)((M + o.chunk_rows - 1) / o.chunk_rows);
    o.ints = reinterpret_cast<int32_t*>(cut.take(((size_t)B * (3 + S_max) + kws::kMaxClasses) * sizeof(int32_t)));
    o.live = reinterpret_cast<uint8_t*>(cut.take(M));
    o.jobs = reinterpret_cast<kws::TrainWgradJob*>(cut.take((size_t)o.njobs * sizeof(kws::TrainWgradJob)));
    o.part = reinterpret_cast<float4*>(cut.take((size_t)B * ntile * sizeof(float4)));
    o.sums = reinterpret_cast<float2*>(cut.take((size_t)B * ntile * sizeof(float2)));
    o.xs = cut.floats(M * c.combine_frame * c.n_mel);
    for (int l = 0; l <= c.num_layers; ++l) o.x[l] = cut.floats(M * H);
    for (float*& s : o.sh) s = cut.floats(M * H);
    o.de = cut.floats(M * H);
    o.logits = cut.floats(M * C); o.gl = cut.floats(M * C);
    o.dsum = cut.floats(M * NH);
    for (int l = 0; l < c.num_layers; ++l) {
        Handle::Carved::Layer& y = o.layer[l];
        y.qkv = cut.floats(M * 3 * H); y.att = cut.floats(M * H); y.lse = cut.floats(M * NH); y.xn_a = cut.floats(M * H); y.y = cut.floats(M * H);
        y.hin = cut.floats(M * Fi); y.xn_b = cut.floats(M * H); y.rstd_a = cut.floats(B); y.rstd_b = cut.floats(B);
        y.dy_b = cut.floats(M * H); y.prod_b = cut.floats(M * H); y.dz = cut.floats(M * H); y.dh = cut.floats(M * Fi);
        y.dy_a = cut.floats(M * H); y.prod_a = cut.floats(M * H); y.dqkv = cut.floats(M * 3 * H);
    }
    o.partial = cut.floats((size_t)o.chunks * h->P);
    if (cv) *cv = o;
    return cut.at;
}

// the products of the weight-gradient launch for the carved shape, in blob order; the layer norms' d beta / d gamma are the column
// sums of dy and dy o xn
void build_jobs(Handle* h) {
    const kws_attention_config& c = h->cfg.model;
    const int H = c.hidden, Fi = c.ffn_inner, C = c.num_classes, cF = c.combine_frame * c.n_mel;
    const Handle::Carved& cv = h->cv;
    auto add = [&](const float* a, int lda, int K, const float* d, int ldd, int N, size_t out) {
        h->add_job(a ? kws::kWgradRows : kws::kWgradOnes, a, lda, K, d, ldd, N, out, N);
    };
    add(cv.xs, cF, cF, cv.de, H, H, h->lay.w_in);
    add(nullptr, 0, 1, cv.de, H, H, h->lay.b_in);
    for (int l = 0; l < c.num_layers; ++l) {
        const size_t* o = h->lay.layer[l];
        const Handle::Carved::Layer& y = cv.layer[l];
        add(cv.x[l], H, H, y.dqkv, 3 * H, 3 * H, o[kQkvW]);
        add(nullptr, 0, 1, y.dqkv, 3 * H, 3 * H, o[kQkvB]);
        add(nullptr, 0, 1, y.dy_a, H, H, o[kLnaBeta]);
        add(nullptr, 0, 1, y.prod_a, H, H, o[kLnaGamma]);
        add(y.y, H, H, y.dh, Fi, Fi, o[kW1]);
        add(nullptr, 0, 1, y.dh, Fi, Fi, o[kB1]);
        add(y.hin, Fi, Fi, y.dz, H, H, o[kW2]);
        add(nullptr, 0, 1, y.dz, H, H, o[kB2]);
        add(nullptr, 0, 1, y.dy_b, H, H, o[kLnbBeta]);
        add(nullptr, 0, 1, y.prod_b, H, H, o[kLnbGamma]);
    }
    add(cv.x[c.num_layers], H, H, cv.gl, C, C, h->lay.w_out);
    add(nullptr, 0, 1, cv.gl, C, C, h->lay.b_out);
}

// the arena for (B, T, S_max): grown if it has to be (waits for the device once), carved anew when the shape differs from the last call's
int prepare_shape(Handle* h, int B, int T, int S_max) {
    if (h->cv.B == B && h->cv.T == T && h->cv.S_max == S_max && h->arena) return KWS_OK;
    const int rc = train_arena_reserve(h, carve(h, B, T, S_max, nullptr, nullptr), B, T, h->cfg.model.num_layers);
    if (!h->arena) h->cv = Handle::Carved();      // freed and not replaced: no layout
    KWS_TRY(rc);
    carve(h, B, T, S_max, h->arena, &h->cv);
    build_jobs(h);
    return KWS_OK;
}

// every refusal of kws_attention_train_create that needs no device
int check_config(const kws_attention_train_config* cfg) {
    if (!cfg) return fail(KWS_ERR_INVALID_ARGUMENT, "config is null");
    int code = KWS_OK;
    if (!attn_config_ok(&cfg->model, &code)) return code;
    return check_optimizer(cfg->keep_prob, cfg->optimizer, cfg->max_grad_norm);
}

// ctc false (a _frames call with ctc_weight 0): nothing about S_max, the labels or the LDS of ctc_loss_kernel
int check_shape(const kws_attention_config& c, int B, int T, int S_max, bool ctc = true) {
    if (B < 1 || T < 1) return fail(KWS_ERR_INVALID_ARGUMENT, "bad shape B=%d T=%d: at least one utterance and one frame", B, T);
    if (ctc) KWS_TRY(check_s_max(S_max));
    if (T > c.max_frames) return fail(KWS_ERR_UNSUPPORTED, "T=%d exceeds model.max_frames=%d", T, c.max_frames);
    if (B > 65535) return fail(KWS_ERR_UNSUPPORTED, "B=%d unsupported (<= 65535)", B);
    const int T1 = frames_out(c, T);
    if ((size_t)B * T1 > kMaxRows) return fail(KWS_ERR_UNSUPPORTED, "B=%d x T'=%d: more than 2^28 rows in one call", B, T1);
    return ctc ? check_ctc_lds(T1, S_max, "T'=%d rows") : KWS_OK;
}

// the refusals of a grad / step call from host memory alone; t1 (if given): every utterance's T'_b
int check_call(const kws_attention_train_config& cfg, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B,
               int T, int S_max, const float* loss, std::vector<int32_t>* t1, bool ctc = true) {
    const kws_attention_config& c = cfg.model;
    KWS_TRY(check_shape(c, B, T, S_max, ctc));
    if (!x || !seq_len || !loss || (ctc && (!label_len || (!labels && S_max > 0)))) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(x) || misaligned(loss)) return fail(KWS_ERR_INVALID_ARGUMENT, "x and loss must be 4-byte aligned");
    std::vector<int32_t> rows((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (seq_len[b] < 0 || seq_len[b] > T) return fail(KWS_ERR_INVALID_ARGUMENT, "seq_len[%d]=%d out of range [0,%d]", b, seq_len[b], T);
        rows[b] = frames_out(c, seq_len[b]);
    }
    if (ctc) KWS_TRY(check_labels(rows.data(), labels, label_len, B, frames_out(c, T), S_max, c.num_classes));
    if (t1) t1->swap(rows);
    return KWS_OK;
}

// forward, loss, backward: leaves loss [B], the logits and the gradient of sum(loss) / B (h->grad, with the sums of squares of its blocks).
// ft: null for the CTC loss alone, else loss[b] = ctc_weight ctc_b + frame_weight ce_b on ft's targets [B, T'] (ctc_weight 0: labels,
// label_len and S_max are not looked at)
int grad_impl(Handle* h, const float* x, const int32_t* seq_len, const std::vector<int32_t>& t1, const int32_t* labels, const int32_t* label_len,
              int B, int T, int S_max, uint64_t seed, float* loss, const kws_frame_targets* ft, hipStream_t st) {
    const kws_attention_config& c = h->cfg.model;
    const int H = c.hidden, Fi = c.ffn_inner, C = c.num_classes, L = c.num_layers, NH = c.num_heads, cF = c.combine_frame * c.n_mel;
    const bool ctc = !ft || ft->ctc_weight > 0.f, frames = ft && ft->frame_weight > 0.f;
    std::vector<int32_t> no_labels;
    if (!ctc) { no_labels.assign((size_t)B, 0); labels = nullptr; label_len = no_labels.data(); S_max = 0; }
    KWS_TRY(prepare_shape(h, B, T, S_max));
    Handle::Carved& cv = h->cv;
    const int T1 = cv.T1, M = B * T1;
    std::vector<int32_t> ints;
    pack_ints(t1.data(), labels, label_len, B, S_max, &ints);
    ints.insert(ints.end(), seq_len, seq_len + B);
    if (frames) append_class_weights(ft->class_weight, C, &ints);
    KWS_TRY(train_upload(h, cv.jobs, cv.ints, &ints, st));
    const int32_t *d_t1 = cv.ints, *d_len = cv.ints + B, *d_lab = cv.ints + 2 * (size_t)B, *d_tlen = cv.ints + (size_t)B * (2 + S_max);
    const float kp = h->cfg.keep_prob;
    const bool drop = kp < 1.0f;
    auto drop_of = [&](int l) { kws::AttnTrainDrop d = {}; d.seed = seed; d.thr = kws::attn_drop_threshold(kp); d.keep_prob = kp; d.layer = l; return d; };
    auto gemm = [&](const float* a, int K, const float* w, int swk, int swn, const float* bias, float* out, int N, const char* what) -> int {
        kws::TrainRowsGemm g = {};
        g.a = a; g.lda = K; g.live = cv.live; g.w = w; g.swk = swk; g.swn = swn; g.bias = bias; g.out = out; g.ldo = N; g.M = M; g.K = K; g.N = N;
        KWS_LAUNCH(h, kws::launch_train_rows_gemm(g, st), what);
        return KWS_OK;
    };
    const float* th = h->theta;
    h->launches = 0;
    KWS_LAUNCH(h, kws::launch_train_rowmask(d_t1, B, T1, cv.live, st), "launch train_rowmask");
    KWS_LAUNCH(h, kws::launch_attn_train_stack(x, d_tlen, d_t1, B, T, T1, c.n_mel, c.combine_frame, cv.xs, st), "launch attn_train_stack");
    KWS_TRY(gemm(cv.xs, cF, th + h->lay.w_in, H, 1, th + h->lay.b_in, cv.x[0], H, "launch train_rows_gemm (embedding)"));
    KWS_LAUNCH(h, kws::launch_attn_train_addpe(cv.x[0], h->tail, d_t1, B, T1, H, st), "launch attn_train_addpe");
    float *s_z = cv.sh[0], *s_u = cv.sh[1];
    for (int l = 0; l < L; ++l) {
        const size_t* o = h->lay.layer[l];
        const Handle::Carved::Layer& y = cv.layer[l];
        KWS_TRY(gemm(cv.x[l], H, th + o[kQkvW], 3 * H, 1, th + o[kQkvB], y.qkv, 3 * H, "launch train_rows_gemm (qkv)"));
        kws::AttnTrainCore k = {};
        k.qkv = y.qkv; k.t1 = d_t1; k.att = y.att; k.lse = y.lse; k.drop = drop_of(l); k.B = B; k.T1 = T1; k.H = H; k.NH = NH;
        KWS_LAUNCH(h, kws::launch_attn_train_core_forward(k, st), "launch attn_train_core_forward");
        kws::AttnTrainResid r = {};
        r.a = y.att; r.r = cv.x[l]; r.t1 = d_t1; r.u = s_u; r.part = cv.part; r.drop = drop_of(l); r.site = kws::kAttnDropAtt; r.B = B; r.T1 = T1; r.H = H;
        KWS_LAUNCH(h, kws::launch_attn_train_resid(r, st), "launch attn_train_resid (attention)");
        kws::AttnTrainLn n = {};
        n.u = s_u; n.part = cv.part; n.t1 = d_t1; n.g = th + o[kLnaGamma]; n.bt = th + o[kLnaBeta]; n.xn = y.xn_a; n.y = y.y; n.rstd = y.rstd_a;
        n.B = B; n.T1 = T1; n.H = H;
        KWS_LAUNCH(h, kws::launch_attn_train_ln_forward(n, st), "launch attn_train_ln_forward (a)");
        KWS_TRY(gemm(y.y, H, th + o[kW1], Fi, 1, th + o[kB1], y.hin, Fi, "launch train_rows_gemm (W1)"));
        KWS_LAUNCH(h, kws::launch_attn_train_relu(y.hin, d_t1, B, T1, Fi, 1, st), "launch attn_train_relu");
        KWS_TRY(gemm(y.hin, Fi, th + o[kW2], H, 1, th + o[kB2], s_z, H, "launch train_rows_gemm (W2)"));
        r.a = s_z; r.r = y.y; r.site = kws::kAttnDropFfn;
        KWS_LAUNCH(h, kws::launch_attn_train_resid(r, st), "launch attn_train_resid (ffn)");
        n.g = th + o[kLnbGamma]; n.bt = th + o[kLnbBeta]; n.xn = y.xn_b; n.y = cv.x[l + 1]; n.rstd = y.rstd_b;
        KWS_LAUNCH(h, kws::launch_attn_train_ln_forward(n, st), "launch attn_train_ln_forward (b)");
    }
    KWS_TRY(gemm(cv.x[L], H, th + h->lay.w_out, C, 1, th + h->lay.b_out, cv.logits, C, "launch train_rows_gemm (logits)"));
    KWS_LAUNCH(h, kws::launch_attn_train_relu(cv.logits, d_t1, B, T1, C, c.use_relu, st), "launch attn_train_relu (logits)");
    if (ctc) {          // J = sum_b ctc_weight ctc_b / B (ctc_weight: 1 without frame targets)
        KWS_LAUNCH(h, kws::launch_ctc_loss(cv.logits, d_t1, d_lab, d_len, B, T1, C, S_max, loss, cv.gl, st), "launch ctc_loss");
        KWS_LAUNCH(h, kws::launch_train_scale(cv.gl, cv.logits, (size_t)M, C, (ft ? ft->ctc_weight : 1.0f) / (float)B, st), "launch train_scale");
    }
    if (frames) {       // ... + sum_b frame_weight ce_b / B: alone it writes every row of the gradient, behind the CTC term it adds to it
        kws::FrameLossParams p = train_frame_term(*ft, B);
        p.logits = cv.logits; p.seq_len = d_t1; p.weight = reinterpret_cast<const float*>(cv.ints + (size_t)B * (3 + S_max));
        p.loss = loss; p.grad = cv.gl; p.T = T1; p.C = C;
        KWS_LAUNCH(h, kws::launch_frame_loss(p, B, st), "launch frame_loss");
    }
    if (c.use_relu) KWS_LAUNCH(h, kws::launch_attn_train_relumask(cv.gl, cv.logits, d_t1, B, T1, C, st), "launch attn_train_relumask (logits)");
    // backward; sh: 0 = d through the qkv product (and of the top output), 1 = du, 2 = ds, 3 = d through W1, 4 = d of the attention output
    float *s_dxq = cv.sh[0], *s_du = cv.sh[1], *s_ds = cv.sh[2], *s_dyf = cv.sh[3], *s_datt = cv.sh[4];
    KWS_TRY(gemm(cv.gl, C, th + h->lay.w_out, 1, C, nullptr, s_dxq, H, "launch train_rows_gemm (d of the top layer)"));
    const float* g2 = nullptr;
    for (int l = L - 1; l >= 0; --l) {
        const size_t* o = h->lay.layer[l];
        const Handle::Carved::Layer& y = cv.layer[l];
        kws::AttnTrainLnBwd n = {};
        n.g1 = s_dxq; n.g2 = g2; n.xn = y.xn_b; n.rstd = y.rstd_b; n.gamma = th + o[kLnbGamma]; n.t1 = d_t1; n.dy = y.dy_b; n.prod = y.prod_b;
        n.sums = cv.sums; n.dx = drop ? s_ds : y.dz; n.ddrop = drop ? y.dz : nullptr; n.drop = drop_of(l); n.site = kws::kAttnDropFfn;
        n.B = B; n.T1 = T1; n.H = H;
        const float* ds = n.dx;
        KWS_LAUNCH(h, kws::launch_attn_train_ln_bwd_sums(n, st), "launch attn_train_ln_bwd_sums (b)");
        KWS_LAUNCH(h, kws::launch_attn_train_ln_bwd_apply(n, st), "launch attn_train_ln_bwd_apply (b)");
        KWS_TRY(gemm(y.dz, H, th + o[kW2], 1, H, nullptr, y.dh, Fi, "launch train_rows_gemm (dh)"));
        KWS_LAUNCH(h, kws::launch_attn_train_relumask(y.dh, y.hin, d_t1, B, T1, Fi, st), "launch attn_train_relumask");
        KWS_TRY(gemm(y.dh, Fi, th + o[kW1], 1, Fi, nullptr, s_dyf, H, "launch train_rows_gemm (dy)"));
        n.g1 = s_dyf; n.g2 = ds; n.xn = y.xn_a; n.rstd = y.rstd_a; n.gamma = th + o[kLnaGamma]; n.dy = y.dy_a; n.prod = y.prod_a;
        n.dx = s_du; n.ddrop = drop ? s_datt : nullptr; n.site = kws::kAttnDropAtt;
        KWS_LAUNCH(h, kws::launch_attn_train_ln_bwd_sums(n, st), "launch attn_train_ln_bwd_sums (a)");
        KWS_LAUNCH(h, kws::launch_attn_train_ln_bwd_apply(n, st), "launch attn_train_ln_bwd_apply (a)");
        kws::AttnTrainCore k = {};
        k.qkv = y.qkv; k.t1 = d_t1; k.att = y.att; k.lse = y.lse; k.datt = drop ? s_datt : s_du; k.dsum = cv.dsum; k.dqkv = y.dqkv;
        k.drop = drop_of(l); k.B = B; k.T1 = T1; k.H = H; k.NH = NH;
        KWS_LAUNCH(h, kws::launch_attn_train_core_dq(k, st), "launch attn_train_core_dq");
        KWS_LAUNCH(h, kws::launch_attn_train_core_dkv(k, st), "launch attn_train_core_dkv");
        KWS_TRY(gemm(y.dqkv, 3 * H, th + o[kQkvW], 1, 3 * H, nullptr, s_dxq, H, "launch train_rows_gemm (dx)"));
        g2 = s_du;
    }
    KWS_LAUNCH(h, kws::launch_train_residual(s_dxq, s_du, 1.0f, cv.de, (size_t)M * H, st), "launch train_residual (d of the embedding)");
    KWS_LAUNCH(h, kws::launch_train_wgrad(cv.jobs, cv.njobs, h->units, cv.xs, cv.live, M, cv.chunk_rows, cv.chunks, cv.partial, h->P, st),
               "launch train_wgrad");
    KWS_LAUNCH(h, kws::launch_train_reduce(cv.partial, cv.chunks, h->P, h->grad, h->sumsq, st), "launch train_reduce");
    return KWS_OK;
}

// kws_attention_train_grad (ft null) and kws_attention_train_grad_frames (ft checked)
int grad_call(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
              int B, int T, int S_max, uint64_t drop_seed, float* loss, float* grad_blob, float* logits_or_null, const kws_frame_targets* ft,
              void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    std::vector<int32_t> t1;
    KWS_TRY(check_call(h->cfg, x, seq_len, labels, label_len, B, T, S_max, loss, &t1, !ft || ft->ctc_weight > 0.f));
    if (!grad_blob) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    if (misaligned(grad_blob) || misaligned(logits_or_null)) return fail(KWS_ERR_INVALID_ARGUMENT, "grad_blob and logits must be 4-byte aligned");
    return train_call(h, stream, [&](hipStream_t st) -> int {
        KWS_TRY(grad_impl(h, x, seq_len, t1, labels, label_len, B, T, S_max, drop_seed, loss, ft, st));
        KWS_HIP(hipMemcpyAsync(grad_blob, h->grad, h->P * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (logits_or_null)
            KWS_HIP(hipMemcpyAsync(logits_or_null, h->cv.logits, (size_t)B * h->cv.T1 * h->cfg.model.num_classes * sizeof(float),
                                   hipMemcpyDeviceToDevice, st));
        return KWS_OK;
    });
}

// kws_attention_train_step (ft null) and kws_attention_train_step_frames (ft checked)
int step_call(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
              int B, int T, int S_max, uint64_t drop_seed, float lr, float* loss, float* grad_norm_or_null, const kws_frame_targets* ft,
              void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    std::vector<int32_t> t1;
    KWS_TRY(check_call(h->cfg, x, seq_len, labels, label_len, B, T, S_max, loss, &t1, !ft || ft->ctc_weight > 0.f));
    if (!(lr > 0.f) || !std::isfinite(lr)) return fail(KWS_ERR_INVALID_ARGUMENT, "lr=%g has to be positive and finite", (double)lr);
    if (misaligned(grad_norm_or_null)) return fail(KWS_ERR_INVALID_ARGUMENT, "grad_norm must be 4-byte aligned");
    return train_call(h, stream, [&](hipStream_t st) -> int {
        KWS_TRY(grad_impl(h, x, seq_len, t1, labels, label_len, B, T, S_max, drop_seed, loss, ft, st));
        return train_update(h, lr, grad_norm_or_null, st);
    });
}

}  // namespace

extern "C" {

size_t kws_sizeof_attention_train_config(void) { return sizeof(kws_attention_train_config); }

int kws_attention_drop_keep(uint64_t drop_seed, float keep_prob, int site, int layer, int b, int head, const int32_t* rows, const int32_t* cols,
                            int n, uint8_t* keep) {
    if (!(keep_prob > 0.f && keep_prob <= 1.f)) return fail(KWS_ERR_UNSUPPORTED, "keep_prob=%g outside (0, 1]", (double)keep_prob);
    if (site < 0 || site > 2) return fail(KWS_ERR_INVALID_ARGUMENT, "site=%d: 0 (probabilities), 1 (attention output), 2 (FFN output)", site);
    if (layer < 0 || layer > 7) return fail(KWS_ERR_INVALID_ARGUMENT, "layer=%d out of range [0,7]", layer);
    if (b < 0 || b > 65535) return fail(KWS_ERR_INVALID_ARGUMENT, "b=%d out of range [0,65535]", b);
    if (head < 0 || head > 15) return fail(KWS_ERR_INVALID_ARGUMENT, "head=%d out of range [0,15]", head);
    if (n < 0) return fail(KWS_ERR_INVALID_ARGUMENT, "negative n=%d", n);
    if (n > 0 && (!rows || !cols || !keep)) return fail(KWS_ERR_INVALID_ARGUMENT, "null pointer argument");
    for (int i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] > 16383 || cols[i] < 0 || cols[i] > 16383)
            return fail(KWS_ERR_INVALID_ARGUMENT, "coordinate %d: row=%d col=%d out of range [0,16383]", i, rows[i], cols[i]);
    const uint64_t thr = kws::attn_drop_threshold(keep_prob);
    for (int i = 0; i < n; ++i) keep[i] = keep_prob >= 1.0f || kws::attn_drop_keep(drop_seed, site, layer, b, head, rows[i], cols[i], thr) ? 1 : 0;
    return KWS_OK;
}

int kws_attention_train_check(const kws_attention_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels,
                              const int32_t* label_len, int B, int T, int S_max, const float* loss) {
    KWS_TRY(check_config(cfg));
    return check_call(*cfg, x, seq_len, labels, label_len, B, T, S_max, loss, nullptr);
}

int kws_attention_train_check_frames(const kws_attention_train_config* cfg, const float* x, const int32_t* seq_len, const int32_t* labels,
                                     const int32_t* label_len, int B, int T, int S_max, const float* loss, const kws_frame_targets* ft) {
    KWS_TRY(check_config(cfg));
    KWS_TRY(check_frame_targets(ft, cfg->model.num_classes));
    return check_call(*cfg, x, seq_len, labels, label_len, B, T, S_max, loss, nullptr, ft->ctc_weight > 0.f);
}

int kws_attention_train_create(const kws_attention_train_config* cfg, kws_attention_train_handle* out) {
    if (!out) return fail(KWS_ERR_INVALID_ARGUMENT, "out handle pointer is null");
    *out = nullptr;
    KWS_TRY(check_config(cfg));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(KWS_ERR_NO_DEVICE, "no HIP device visible");
    Handle* h = new (std::nothrow) Handle();
    if (!h) return fail(KWS_ERR_OUT_OF_MEMORY, "host allocation failed");
    const kws_attention_config& c = cfg->model;
    h->cfg = *cfg;
    h->lay = attn_layout(c);
    h->optimizer = cfg->optimizer; h->max_grad_norm = cfg->max_grad_norm;
    const int H = c.hidden;
    h->pe_rows = c.max_frames / c.combine_frame + 1;
    std::vector<float> pe((size_t)h->pe_rows * H);          // positional_encoding_op.cc:44-48: double, stored as float
    for (int p = 0; p < h->pe_rows; ++p)
        for (int i = 0; i < H / 2; ++i) {
            const double a = p / std::pow(10000.0, 2.0 * i / H);
            pe[(size_t)p * H + 2 * i] = (float)std::sin(a);
            pe[(size_t)p * H + 2 * i + 1] = (float)std::cos(a);
        }
    const int rc = train_core_create(h, h->lay.total, pe.size(), pe.data(), "kws_attention_train_create");
    if (rc != KWS_OK) { delete h; return rc; }
    *out = h;
    return KWS_OK;
}

int kws_attention_train_destroy(kws_attention_train_handle h) {
    if (!h) return KWS_OK;
    train_core_destroy(h);
    delete h;
    return KWS_OK;
}

int kws_attention_train_set_weights(kws_attention_train_handle h, const void* blob, size_t nbytes, void* stream) {
    return train_set_weights(h, blob, nbytes, stream, nullptr);
}
int kws_attention_train_get_weights(kws_attention_train_handle h, void* blob, size_t nbytes, void* stream) { return train_get_weights(h, blob, nbytes, stream); }
int kws_attention_train_moments(kws_attention_train_handle h, float* m, float* v, void* stream) { return train_moments(h, m, v, stream); }

int kws_attention_train_reserve(kws_attention_train_handle h, int B, int T, int S_max) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_shape(h->cfg.model, B, T, S_max));
    BusyGuard guard(h->in_call);
    if (!guard.owned) return fail(KWS_ERR_BUSY, "another host thread is inside a call on this train handle");
    return prepare_shape(h, B, T, S_max);      // the job table goes to the device with the next call, on its stream
}

int kws_attention_train_grad(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                             int B, int T, int S_max, uint64_t drop_seed, float* loss, float* grad_blob, float* logits_or_null, void* stream) {
    return grad_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_seed, loss, grad_blob, logits_or_null, nullptr, stream);
}

int kws_attention_train_grad_frames(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels,
                                    const int32_t* label_len, int B, int T, int S_max, uint64_t drop_seed, float* loss, float* grad_blob,
                                    float* logits_or_null, const kws_frame_targets* ft, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_frame_targets(ft, h->cfg.model.num_classes));
    return grad_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_seed, loss, grad_blob, logits_or_null, ft, stream);
}

int kws_attention_train_step(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                             int B, int T, int S_max, uint64_t drop_seed, float lr, float* loss, float* grad_norm_or_null, void* stream) {
    return step_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_seed, lr, loss, grad_norm_or_null, nullptr, stream);
}

int kws_attention_train_step_frames(kws_attention_train_handle h, const float* x, const int32_t* seq_len, const int32_t* labels,
                                    const int32_t* label_len, int B, int T, int S_max, uint64_t drop_seed, float lr, float* loss,
                                    float* grad_norm_or_null, const kws_frame_targets* ft, void* stream) {
    if (!h) return fail(KWS_ERR_INVALID_ARGUMENT, "handle is null");
    KWS_TRY(check_frame_targets(ft, h->cfg.model.num_classes));
    return step_call(h, x, seq_len, labels, label_len, B, T, S_max, drop_seed, lr, loss, grad_norm_or_null, ft, stream);
}

int kws_attention_train_stats(kws_attention_train_handle h, size_t* device_bytes, int32_t* allocs, int32_t* steps, int32_t* launches,
                              int32_t* chunk_rows) {
    return train_stats(h, h ? h->cv.chunk_rows : 0, device_bytes, allocs, steps, launches, chunk_rows);
}

}  // extern "C"
