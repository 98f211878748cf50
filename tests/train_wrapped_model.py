"""TEST INFRASTRUCTURE ONLY -- tests/train_model.py extended to the training graph get_cell builds with its wrappers
(models/rnn_ctc.py:179-199): per layer Residual(Dropout(LayerNormalizer(GRUCell))), the residual on layers >= 1 only, and the dropout's
variational_recurrent switch (one mask per stream and layer, held for all frames).  As there: a hand-written numpy fp64 forward /
backward by the formulas of include/kws_amd.h, and the same graph in torch ops for autograd in float64 and float32.

  layer norm   m = mean(in), v = mean((in - m)^2), rstd = 1 / sqrt(v + 1e-5), xn = (in - m) rstd, x^ = xn ibeta + igamma
               (wrapped_cell_model.layer_norm: ibeta the scalar scale, igamma the per-feature shift); the cell's x-part reads x^
  residual     out = 0.7071067811865475 (y + in) for l >= 1, y after dropout; the state stays the cell's
  backward     dy = k dout into the frame loop; g = dx^; dn = g ibeta, a = mean(dn), c = mean(dn o xn), d in = rstd (dn - a - xn c),
               d ibeta = sum g o xn, d igamma = sum_rows g; d in += k dout; rows t >= seq_len are zero rows and add exactly 0

With every switch off each function performs train_model's operations in train_model's order: the numbers are equal, not close.  The
dict form carries ibeta / igamma per layer under the layer norm (keyword_spotting_amd.weights); flat() puts them behind bfc, where
kws_weights_nbytes_wrapped puts them."""
import functools

import numpy as np

import enroll_model as E
import train_model as M
import wrapped_cell_model as W

K = W.RESIDUAL_SCALE
EPS = W.LN_EPSILON
LAYER_KEYS = ("Wg", "bg", "Wc", "bc")


def config_of(h, l, n_mel, c, ln=False, res=False, var=False):
    cfg = M.config_of(h, l, n_mel, c)
    cfg.use_layer_norm, cfg.use_residual, cfg.variational_recurrent = bool(ln), bool(res), bool(var)
    return cfg


def has_ln(w):
    return "ibeta" in w["layers"][0]


def flat(w):
    """dict form -> [(name, array)] in blob order: train_model.flat, then each layer's ibeta and igamma."""
    out = M.flat(w)
    if has_ln(w):
        for l, lay in enumerate(w["layers"]):
            out += [("l%d_ibeta" % l, lay["ibeta"]), ("l%d_igamma" % l, lay["igamma"])]
    return out


def unflat(w, arrays):
    """The inverse of flat for the arrays of a dict shaped like w."""
    n = len(w["layers"])
    out = dict(layers=[dict(zip(LAYER_KEYS, arrays[4 * l:4 * l + 4])) for l in range(n)], Wfc=arrays[4 * n], bfc=arrays[4 * n + 1])
    if has_ln(w):
        for l in range(n):
            out["layers"][l].update(ibeta=arrays[4 * n + 2 + 2 * l], igamma=arrays[4 * n + 3 + 2 * l])
    return out


def as_dtype(w, dtype):
    return unflat(w, [np.asarray(v, dtype) for _, v in flat(w)])


def blob_of(w):
    return np.concatenate([np.asarray(v, np.float64).ravel() for _, v in flat(w)])


def _mask(drop, l, t_len):
    """Layer l's mask as [B,T,H] booleans from uint8 [L,B,T,H], or [L,B,H] broadcast over the frames (variational)."""
    m = np.asarray(drop[l]) != 0
    return m if m.ndim == 3 else np.broadcast_to(m[:, None, :], (m.shape[0], t_len, m.shape[1]))


# ---- numpy fp64 ------------------------------------------------------------------------------------------------------------------

def forward(w, x, seq_len, ln=False, res=False, drop=None, keep_prob=1.0):
    """-> (logits [B,T,C], tape): tape["layers"][l] = train_model's entries (a: what the cell read, x^ under the layer norm), plus
    ain (the layer's input), xn [B,T,I] and rstd [B,T,1]."""
    w = as_dtype(w, np.float64)
    x = np.asarray(x, np.float64)
    b, t_len = x.shape[:2]
    live = np.arange(t_len)[None, :] < np.asarray(seq_len)[:, None]          # [B,T]
    a = np.where(live[:, :, None], x, 0.0)                                  # the padding may be anything, NaN included
    tape = []
    for l, lay in enumerate(w["layers"]):
        ain, xn, rstd = a, None, None
        if ln:
            m = ain.mean(axis=2, keepdims=True)
            v = ((ain - m) ** 2).mean(axis=2, keepdims=True)
            rstd = np.where(live[:, :, None], 1.0 / np.sqrt(v + EPS), 0.0)
            xn = (ain - m) * rstd
            a = np.where(live[:, :, None], xn * lay["ibeta"] + lay["igamma"], 0.0)
        hid = lay["bc"].shape[0]
        h = np.zeros((b, hid))
        r, u, c, hs, y = (np.zeros((b, t_len, hid)) for _ in range(5))
        for t in range(t_len):
            g = M.sigmoid(np.concatenate([a[:, t], h], axis=1) @ lay["Wg"] + lay["bg"])
            r[:, t], u[:, t] = g[:, :hid], g[:, hid:]
            c[:, t] = np.tanh(np.concatenate([a[:, t], r[:, t] * h], axis=1) @ lay["Wc"] + lay["bc"])
            hs[:, t] = h
            hn = u[:, t] * h + (1.0 - u[:, t]) * c[:, t]
            on = live[:, t, None]
            y[:, t] = np.where(on, hn, 0.0)
            h = np.where(on, hn, h)
        if drop is not None:
            y = y * _mask(drop, l, t_len) / keep_prob
        tape.append(dict(a=a, r=r, u=u, c=c, h=hs, live=live, ain=ain, xn=xn, rstd=rstd))
        a = K * (y + ain) if res and l >= 1 else y
    return a @ w["Wfc"] + w["bfc"], dict(layers=tape, top=a)


def loss_and_grad(w, x, seq_len, labels, ln=False, res=False, drop=None, keep_prob=1.0):
    """-> (loss [B] (+inf without a path), gradient of sum(loss) / B in the dict form, logits)."""
    w64 = as_dtype(w, np.float64)
    logits, tape = forward(w64, x, seq_len, ln, res, drop, keep_prob)
    b, t_len, _ = logits.shape
    loss, gl = np.zeros(b), np.zeros_like(logits)
    for i in range(b):
        loss[i], gl[i] = E.ctc_loss_grad(logits[i], seq_len[i], labels[i])
    gl /= b
    top = tape["top"]
    grads = dict(layers=[None] * len(w64["layers"]), Wfc=np.einsum("bth,btc->hc", top, gl), bfc=gl.sum(axis=(0, 1)))
    dy = gl @ w64["Wfc"].T
    for l in range(len(w64["layers"]) - 1, -1, -1):
        lay, tp = w64["layers"][l], tape["layers"][l]
        hid, n_in = lay["bc"].shape[0], tp["a"].shape[2]
        residual = res and l >= 1
        if residual:
            dy = K * dy          # the frame loop's dy, and the share of d in that is added below
        share = dy
        if drop is not None:
            dy = dy * _mask(drop, l, t_len) / keep_prob
        g = dict(Wg=np.zeros_like(lay["Wg"]), bg=np.zeros_like(lay["bg"]), Wc=np.zeros_like(lay["Wc"]), bc=np.zeros_like(lay["bc"]))
        dx = np.zeros_like(tp["a"])
        dh = np.zeros((b, hid))
        for t in range(t_len - 1, -1, -1):
            on = tp["live"][:, t, None]
            r, u, c, h, a = tp["r"][:, t], tp["u"][:, t], tp["c"][:, t], tp["h"][:, t], tp["a"][:, t]
            dhp = dy[:, t] + dh
            du, dc, dh_new = dhp * (h - c), dhp * (1.0 - u), dhp * u
            dc_hat = np.where(on, dc * (1.0 - c * c), 0.0)
            dxc_drh = dc_hat @ lay["Wc"].T
            drh = dxc_drh[:, n_in:]
            dh_new = dh_new + drh * r
            dr_hat = np.where(on, drh * h * r * (1.0 - r), 0.0)
            du_hat = np.where(on, du * u * (1.0 - u), 0.0)
            dg = np.concatenate([dr_hat, du_hat], axis=1)
            dxg_dhg = dg @ lay["Wg"].T
            dh_new = dh_new + dxg_dhg[:, n_in:]
            dx[:, t] = dxc_drh[:, :n_in] + dxg_dhg[:, :n_in]
            g["Wc"] += np.concatenate([a, r * h], axis=1).T @ dc_hat
            g["bc"] += dc_hat.sum(axis=0)
            g["Wg"] += np.concatenate([a, h], axis=1).T @ dg
            g["bg"] += dg.sum(axis=0)
            dh = np.where(on, dh_new, dh)
        if ln:          # dx is dx^: zero rows at t >= seq_len, as xn and rstd are
            dn = dx * lay["ibeta"]
            mean_dn = dn.mean(axis=2, keepdims=True)
            mean_dn_xn = (dn * tp["xn"]).mean(axis=2, keepdims=True)
            g["ibeta"] = (dx * tp["xn"]).sum()
            g["igamma"] = dx.sum(axis=(0, 1))
            dx = tp["rstd"] * (dn - mean_dn - tp["xn"] * mean_dn_xn)
        grads["layers"][l] = g
        dy = dx + share if residual else dx
    return loss, grads, logits


# ---- torch -----------------------------------------------------------------------------------------------------------------------

def torch_reference(w, x, seq_len, labels, dtype, ln=False, res=False, drop=None, keep_prob=1.0):
    """train_model.torch_reference with the three switches -> dict(loss, logits, grads (dict form, ibeta / igamma included))."""
    import torch
    import torch.nn.functional as F

    def leaf(v):
        return torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True)
    tw = unflat(w, [leaf(v) for _, v in flat(w)])
    seq_len = np.asarray(seq_len)
    b, t_len = x.shape[:2]
    live = torch.tensor(np.arange(t_len)[None, :] < seq_len[:, None])
    zero = torch.zeros((), dtype=dtype)
    a = torch.where(live[:, :, None], torch.tensor(np.asarray(x), dtype=dtype), zero)
    for l, lay in enumerate(tw["layers"]):
        ain = a
        if ln:
            m = ain.mean(dim=2, keepdim=True)
            v = ((ain - m) ** 2).mean(dim=2, keepdim=True)
            a = torch.where(live[:, :, None], (ain - m) / torch.sqrt(v + EPS) * lay["ibeta"] + lay["igamma"], zero)
        hid = lay["bc"].shape[0]
        h = torch.zeros(b, hid, dtype=dtype)
        ys = []
        for t in range(t_len):
            g = torch.sigmoid(torch.cat([a[:, t], h], dim=1) @ lay["Wg"] + lay["bg"])
            r, u = g[:, :hid], g[:, hid:]
            c = torch.tanh(torch.cat([a[:, t], r * h], dim=1) @ lay["Wc"] + lay["bc"])
            hn = u * h + (1.0 - u) * c
            on = live[:, t, None]
            ys.append(torch.where(on, hn, zero))
            h = torch.where(on, hn, h)
        a = torch.stack(ys, dim=1)
        if drop is not None:
            a = a * torch.tensor(_mask(drop, l, t_len).astype(np.float64), dtype=dtype) / keep_prob
        if res and l >= 1:
            a = K * (a + ain)
    logits = a @ tw["Wfc"] + tw["bfc"]
    idx = [i for i in range(b) if seq_len[i] > 0]
    lab, lab_len = E.padded_labels([labels[i] for i in idx])
    lp = F.log_softmax(logits[idx], dim=-1).transpose(0, 1)
    loss_live = F.ctc_loss(lp, torch.tensor(lab, dtype=torch.long), torch.tensor(seq_len[idx], dtype=torch.long),
                           torch.tensor(lab_len, dtype=torch.long), blank=logits.shape[2] - 1, reduction="none", zero_infinity=True)
    (loss_live.sum() / b).backward()
    loss = np.zeros(b)
    loss[idx] = loss_live.detach().numpy()
    return dict(loss=loss, logits=logits.detach().numpy(), grads=unflat(w, [v.grad.numpy() for _, v in flat(tw)]))


# ---- optimisers over the extended parameter set -------------------------------------------------------------------------------------

def global_norm(grads):
    return float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for _, g in flat(grads))))


class Optimizer(object):
    """train_model.Optimizer over flat(): ibeta and igamma take the same clip and the same update as every other tensor."""

    def __init__(self, w, kind, dtype=np.float64):
        self.kind, self.f, self.t = kind, dtype, 0
        self.m = [np.zeros_like(np.asarray(v, dtype)) for _, v in flat(w)]
        self.v = [np.zeros_like(np.asarray(v, dtype)) for _, v in flat(w)]

    def apply(self, w, grads, lr, max_grad_norm=-1.0):
        f = self.f
        gs = [np.asarray(g, f) for _, g in flat(grads)]
        if max_grad_norm > 0:
            s = max_grad_norm / max(global_norm(grads), max_grad_norm)
            gs = [g * f(s) if f is np.float32 else g * s for g in gs]
        self.t += 1
        out = []
        for i, ((_, theta), g) in enumerate(zip(flat(as_dtype(w, f)), gs)):
            if self.kind == "adam":
                lr_t = f(lr * np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t))
                self.m[i] = self.m[i] + (g - self.m[i]) * f(0.1)
                self.v[i] = self.v[i] + (g * g - self.v[i]) * f(0.001)
                out.append(theta - lr_t * self.m[i] / (np.sqrt(self.v[i]) + f(1e-8)))
            else:
                self.m[i] = f(0.9) * self.m[i] + g
                out.append(theta - f(lr) * g - f(lr) * f(0.9) * self.m[i])
        return unflat(w, out)


# ---- the case table: each at the smallest shape that reaches its path ----------------------------------------------------------------

_ODD = M.CASES["odd_mel"]
# name -> (layer norm, residual, (H, L, n_mel, C, B, T, seq_len, labels))
CASES = {
    # one frame: layer 0's dx^ product, which exists only under the layer norm
    "ln_t1": (True, False, M.CASES["t1"]),
    # one feature: v = 0, xn = 0 exactly, d in = 0
    "ln_mel1": (True, False, M.CASES["mel1"]),
    # ragged with one empty slot: dead rows in every layer-norm kernel
    "ln_odd_mel": (True, False, _ODD[:6] + ([9, 7, 0, 9, 3], _ODD[7])),
    # more than one value per lane, tail lanes
    "ln_mel70": (True, False, M.CASES["mel70"]),
    # the widest row: 16 values per lane
    "ln_mel1024": (True, False, M.CASES["mel1024"]),
    "res_l2": (False, True, (64, 2, 8, 6, 3, 8, [8, 5, 6], [[1, 2], [3], [2]])),
    # one layer: the residual has no effect, the plain handle's bits
    "res_l1": (False, True, M.CASES["t2"]),
    "both_ref_shape": (True, True, M.CASES["ref_shape"]),
    "both_h256": (True, True, M.CASES["h256"]),
    # every per-layer slot, seven residual adds
    "both_l8": (True, True, M.CASES["l8"]),
    # 660 rows: three chunks of the ibeta / igamma reduction, the last one partial
    "both_split_rows": (True, True, (64, 2) + M.CASES["split_rows"][2:]),
    # chunks of 512 rows
    "ln_rows_chunk512": (True, False, M.CASES["rows_chunk512"]),
    # one utterance without a valid path: its gradient is exactly 0
    "both_no_path": (True, True, M.CASES["no_path"]),
}


@functools.lru_cache(maxsize=None)
def make_problem(name, seed=0, var=False):
    """train_model.make_problem's recipe with the case's switches and random layer-norm tables (wrapped_cell_model.random_ln: with
    TF's initial ibeta = 0 the layer norm outputs igamma whatever x is, and a wrong mean or variance goes unseen)."""
    from keyword_spotting_amd import weights
    ln, res, (h, l, n_mel, c, b, t, seq_len, labels) = CASES[name]
    cfg = config_of(h, l, n_mel, c, ln, res, var)
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    w = weights.init_weights(cfg, seed=seed + 1)
    for lay in w["layers"]:
        lay["bg"] = (lay["bg"] + 0.3 * rng.standard_normal(lay["bg"].shape)).astype(np.float32)
        lay["bc"] = (0.3 * rng.standard_normal(lay["bc"].shape)).astype(np.float32)
    w["Wfc"] = (0.5 * w["Wfc"]).astype(np.float32)
    w["bfc"] = (0.5 * rng.standard_normal(c)).astype(np.float32)
    if ln:
        W.random_ln(w, n_mel, seed + 5)
    return dict(name=name, config=cfg, ln=ln, res=res, w=w, x=rng.standard_normal((b, t, n_mel)).astype(np.float32),
                seq_len=np.array(seq_len, np.int32), labels=[list(s) for s in labels], B=b, T=t)


def drop_masks(p, keep_prob, seed=7, variational=False):
    """uint8 [L,B,T,H], or [L,B,H] (variational), floor(keep_prob + U)."""
    cfg = p["config"]
    rng = np.random.default_rng(seed)
    shape = (cfg.num_layers, p["B"], cfg.hidden_size) if variational else (cfg.num_layers, p["B"], p["T"], cfg.hidden_size)
    return np.floor(keep_prob + rng.random(shape)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def reference(name, keep_prob=1.0):
    """(fp64 restatement, float32 torch) of the gradient call on a case, per-frame masks at keep_prob < 1: computed once, shared."""
    import torch
    p = make_problem(name)
    drop = drop_masks(p, keep_prob) if keep_prob < 1.0 else None
    return (loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], p["ln"], p["res"], drop, keep_prob),
            torch_reference(p["w"], p["x"], p["seq_len"], p["labels"], torch.float32, p["ln"], p["res"], drop, keep_prob))


@functools.lru_cache(maxsize=None)
def trajectory(name, kind, steps, lr, float32=False):
    """train_model.trajectory on CASES[name] with its switches."""
    import torch
    p = make_problem(name)
    w = p["w"] if float32 else as_dtype(p["w"], np.float64)
    opt = Optimizer(w, kind, np.float32 if float32 else np.float64)
    losses, path = [], []
    for _ in range(steps):
        if float32:
            r = torch_reference(w, p["x"], p["seq_len"], p["labels"], torch.float32, p["ln"], p["res"])
            loss, grads = r["loss"], r["grads"]
        else:
            loss, grads, _ = loss_and_grad(w, p["x"], p["seq_len"], p["labels"], p["ln"], p["res"])
        w = opt.apply(w, grads, lr)
        losses.append(np.asarray(loss, np.float64))
        path.append(blob_of(w))
    return np.array(losses), path


# ---- the toy task of train_model.toy_task at L = 2 with all three switches -----------------------------------------------------------

# Steps and learning rate chosen on the fp64 restatement (tests/test_train_wrapped_host.py), from TF's initial layer norm (ibeta = 0,
# igamma = 1: the input reaches the cell only once ibeta has moved).  The plain toy's 150 steps at 0.02 do: the loss falls from 24.9
# to 1.2 in 30 steps, 0.02 in 90 and 0.006 in 150, every utterance recognised.
TOY = dict(M.TOY, L=2, steps=150, lr=0.02, keep_prob=0.9)


def toy_task(seed=0):
    """train_model.toy_task's utterances for a two-layer model with layer norm, residual and variational dropout, from
    weights.init_weights (TF's initial ibeta = 0, igamma = 1)."""
    from keyword_spotting_amd import weights
    p = dict(M.toy_task(seed))
    cfg = config_of(TOY["H"], TOY["L"], TOY["n_mel"], TOY["C"], True, True, True)
    p.update(config=cfg, w=weights.init_weights(cfg, seed=seed + 3), ln=True, res=True)
    return p


@functools.lru_cache(maxsize=None)
def toy_trained(seed=0):
    """The restatement trained on the toy task with Adam and a fresh [L,B,H] mask per step -> (losses [steps + 1] of sum / B, the last
    one without dropout; final weights fp64; final logits without dropout)."""
    p = toy_task(seed)
    w = as_dtype(p["w"], np.float64)
    opt = Optimizer(w, "adam")
    rng = np.random.default_rng(seed + 17)
    losses = []
    for _ in range(TOY["steps"]):
        drop = np.floor(TOY["keep_prob"] + rng.random((TOY["L"], p["B"], TOY["H"]))).astype(np.uint8)
        loss, grads, _ = loss_and_grad(w, p["x"], p["seq_len"], p["labels"], True, True, drop, TOY["keep_prob"])
        losses.append(loss.sum() / p["B"])
        w = opt.apply(w, grads, TOY["lr"])
    loss, _, logits = loss_and_grad(w, p["x"], p["seq_len"], p["labels"], True, True)
    losses.append(loss.sum() / p["B"])
    return np.array(losses), w, logits
