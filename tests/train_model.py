"""TEST INFRASTRUCTURE ONLY -- the training graph of the GRU stack (models/rnn_ctc.py:34-101,179-284) restated twice:

  * forward / backward: hand-written numpy fp64 -- TF 1.x GRUCell under dynamic_rnn(sequence_length) and DropoutWrapper(output_keep_prob)
    from the zero state, the dense layer, the CTC loss of tests/enroll_model.py, loss = sum_b ctc_b / B, and back-propagation through
    time by the formulas of include/kws_amd.h;
  * torch_reference: the same graph in torch ops, so that autograd gives a float64 and a float32 reference.

Conventions of kws_train_grad: frames t >= seq_len copy the state and output 0; seq_len == 0 is an empty slot (adds 0, counts in B); an
utterance without a valid path has loss +inf and contributes a gradient of exactly 0.  Then TensorFlow's optimisers: Adam
(enroll_model.adam_step), momentum with use_nesterov, tf.clip_by_global_norm and the non-staircase exponential decay."""
import functools
import types

import numpy as np

import enroll_model as E


def config_of(h, l, n_mel, c):
    """The attribute bag weights.init_weights / to_blob / from_blob read."""
    return types.SimpleNamespace(hidden_size=h, num_layers=l, n_mel=n_mel, num_classes=c, use_relu=False, value_clip=-1.0, precision="fp32")


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def flat(w):
    """dict form -> [(name, array)] in blob order."""
    out = []
    for l, lay in enumerate(w["layers"]):
        out += [("l%d_%s" % (l, k), lay[k]) for k in ("Wg", "bg", "Wc", "bc")]
    return out + [("Wfc", w["Wfc"]), ("bfc", w["bfc"])]


def as_dtype(w, dtype):
    return dict(layers=[{k: np.asarray(v, dtype) for k, v in lay.items()} for lay in w["layers"]], Wfc=np.asarray(w["Wfc"], dtype),
                bfc=np.asarray(w["bfc"], dtype))


# ---- numpy fp64 ------------------------------------------------------------------------------------------------------------------

def forward(w, x, seq_len, drop=None, keep_prob=1.0):
    """-> (logits [B,T,C], tape): tape[l] = dict(a [B,T,I_l] the layer's input, r, u, c, h (the state each frame started from), live)."""
    w = as_dtype(w, np.float64)
    x = np.asarray(x, np.float64)
    b, t_len = x.shape[:2]
    live = np.arange(t_len)[None, :] < np.asarray(seq_len)[:, None]          # [B,T]
    a = np.where(live[:, :, None], x, 0.0)                                  # the padding may be anything, NaN included
    tape = []
    for l, lay in enumerate(w["layers"]):
        hid = lay["bc"].shape[0]
        h = np.zeros((b, hid))
        r, u, c, hs, y = (np.zeros((b, t_len, hid)) for _ in range(5))
        for t in range(t_len):
            g = sigmoid(np.concatenate([a[:, t], h], axis=1) @ lay["Wg"] + lay["bg"])
            r[:, t], u[:, t] = g[:, :hid], g[:, hid:]
            c[:, t] = np.tanh(np.concatenate([a[:, t], r[:, t] * h], axis=1) @ lay["Wc"] + lay["bc"])
            hs[:, t] = h
            hn = u[:, t] * h + (1.0 - u[:, t]) * c[:, t]
            on = live[:, t, None]
            y[:, t] = np.where(on, hn, 0.0)
            h = np.where(on, hn, h)
        if drop is not None:
            y = y * (np.asarray(drop[l]) != 0) / keep_prob
        tape.append(dict(a=a, r=r, u=u, c=c, h=hs, live=live))
        a = y
    return a @ w["Wfc"] + w["bfc"], dict(layers=tape, top=a)


def loss_and_grad(w, x, seq_len, labels, drop=None, keep_prob=1.0):
    """-> (loss [B] (+inf without a path), gradient of sum(loss) / B in the dict form, logits)."""
    w64 = as_dtype(w, np.float64)
    logits, tape = forward(w64, x, seq_len, drop, keep_prob)
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
        if drop is not None:
            dy = dy * (np.asarray(drop[l]) != 0) / keep_prob
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
        grads["layers"][l] = g
        dy = dx
    return loss, grads, logits


# ---- torch -----------------------------------------------------------------------------------------------------------------------

def torch_reference(w, x, seq_len, labels, dtype, drop=None, keep_prob=1.0):
    """The same graph in torch ops on the CPU in `dtype` -> dict(loss [B] (0 where torch zeroes an infinite loss), logits, grads (dict
    form, of sum(loss) / B)).  Empty slots are left out of the CTC call: they add nothing."""
    import torch
    import torch.nn.functional as F
    tw = dict(layers=[{k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in lay.items()} for lay in w["layers"]],
              Wfc=torch.tensor(np.asarray(w["Wfc"]), dtype=dtype, requires_grad=True), bfc=torch.tensor(np.asarray(w["bfc"]), dtype=dtype, requires_grad=True))
    seq_len = np.asarray(seq_len)
    b, t_len = x.shape[:2]
    live = torch.tensor(np.arange(t_len)[None, :] < seq_len[:, None])
    a = torch.where(live[:, :, None], torch.tensor(np.asarray(x), dtype=dtype), torch.zeros((), dtype=dtype))
    for l, lay in enumerate(tw["layers"]):
        hid = lay["bc"].shape[0]
        h = torch.zeros(b, hid, dtype=dtype)
        ys = []
        for t in range(t_len):
            g = torch.sigmoid(torch.cat([a[:, t], h], dim=1) @ lay["Wg"] + lay["bg"])
            r, u = g[:, :hid], g[:, hid:]
            c = torch.tanh(torch.cat([a[:, t], r * h], dim=1) @ lay["Wc"] + lay["bc"])
            hn = u * h + (1.0 - u) * c
            on = live[:, t, None]
            ys.append(torch.where(on, hn, torch.zeros((), dtype=dtype)))
            h = torch.where(on, hn, h)
        a = torch.stack(ys, dim=1)
        if drop is not None:
            a = a * torch.tensor((np.asarray(drop[l]) != 0).astype(np.float64), dtype=dtype) / keep_prob
    logits = a @ tw["Wfc"] + tw["bfc"]
    idx = [i for i in range(b) if seq_len[i] > 0]
    lab, lab_len = E.padded_labels([labels[i] for i in idx])
    lp = F.log_softmax(logits[idx], dim=-1).transpose(0, 1)
    loss_live = F.ctc_loss(lp, torch.tensor(lab, dtype=torch.long), torch.tensor(seq_len[idx], dtype=torch.long),
                           torch.tensor(lab_len, dtype=torch.long), blank=logits.shape[2] - 1, reduction="none", zero_infinity=True)
    (loss_live.sum() / b).backward()
    loss = np.zeros(b)
    loss[idx] = loss_live.detach().numpy()
    grads = dict(layers=[{k: v.grad.numpy() for k, v in lay.items()} for lay in tw["layers"]], Wfc=tw["Wfc"].grad.numpy(), bfc=tw["bfc"].grad.numpy())
    return dict(loss=loss, logits=logits.detach().numpy(), grads=grads)


# ---- optimisers ------------------------------------------------------------------------------------------------------------------

def global_norm(grads):
    return float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for _, g in flat(grads))))


def clip_by_global_norm(grads, clip):
    """tf.clip_by_global_norm: g * clip / max(norm, clip); clip <= 0: untouched (models/rnn_ctc.py:96-98)."""
    if not clip > 0:
        return grads
    s = clip / max(global_norm(grads), clip)
    return dict(layers=[{k: v * s for k, v in lay.items()} for lay in grads["layers"]], Wfc=grads["Wfc"] * s, bfc=grads["bfc"] * s)


def nesterov_step(theta, a, g, lr, momentum=0.9):
    """tf.train.MomentumOptimizer(use_nesterov=True): a <- 0.9 a + g; theta <- theta - lr g - lr 0.9 a."""
    a = momentum * a + g
    return theta - lr * g - lr * momentum * a, a


def exponential_decay(lr0, step, decay_step, decay):
    return lr0 * decay ** (step / decay_step)


class Optimizer(object):
    """The slots of one optimiser over the dict form, in `dtype` arithmetic (float32: every constant rounded as the kernel's)."""

    def __init__(self, w, kind, dtype=np.float64):
        self.kind, self.f, self.t = kind, dtype, 0
        self.m = [np.zeros_like(np.asarray(v, dtype)) for _, v in flat(w)]
        self.v = [np.zeros_like(np.asarray(v, dtype)) for _, v in flat(w)]

    def apply(self, w, grads, lr, max_grad_norm=-1.0):
        f = self.f
        grads = clip_by_global_norm(as_dtype(grads, f), max_grad_norm)
        self.t += 1
        out = []
        for i, ((_, theta), (_, g)) in enumerate(zip(flat(as_dtype(w, f)), flat(grads))):
            g = np.asarray(g, f)
            if self.kind == "adam":
                lr_t = f(lr * np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t))
                self.m[i] = self.m[i] + (g - self.m[i]) * f(0.1)          # the kernel's form: 1 - beta is the constant, not beta
                self.v[i] = self.v[i] + (g * g - self.v[i]) * f(0.001)
                out.append(theta - lr_t * self.m[i] / (np.sqrt(self.v[i]) + f(1e-8)))
            else:
                self.m[i] = f(0.9) * self.m[i] + g
                out.append(theta - f(lr) * g - f(lr) * f(0.9) * self.m[i])
        n = len(w["layers"])
        return dict(layers=[dict(zip(("Wg", "bg", "Wc", "bc"), out[4 * l:4 * l + 4])) for l in range(n)], Wfc=out[4 * n], bfc=out[4 * n + 1])


def blob_of(w):
    return np.concatenate([np.asarray(v, np.float64).ravel() for _, v in flat(w)])


TRAJECTORY_LR = {"adam": 0.01, "nesterov": 0.005}          # the twenty-step cases of both test files


@functools.lru_cache(maxsize=None)
def trajectory(name, kind, steps, lr, float32=False):
    """`steps` optimiser steps on CASES[name] -> (loss [steps, B], [parameter blob after each step] fp64 arrays).  float32: the torch
    graph and the optimiser in float32 (the yardstick trajectory); else the numpy fp64 restatement.  Cached: the host and the GPU
    tests share one evaluation."""
    import torch
    p = make_problem(name)
    w = p["w"] if float32 else as_dtype(p["w"], np.float64)
    opt = Optimizer(w, kind, np.float32 if float32 else np.float64)
    losses, path = [], []
    for _ in range(steps):
        if float32:
            r = torch_reference(w, p["x"], p["seq_len"], p["labels"], torch.float32)
            loss, grads = r["loss"], r["grads"]
        else:
            loss, grads, _ = loss_and_grad(w, p["x"], p["seq_len"], p["labels"])
        w = opt.apply(w, grads, lr)
        losses.append(np.asarray(loss, np.float64))
        path.append(blob_of(w))
    return np.array(losses), path


# ---- the case list both test files share: the smallest shapes at which the kernels can go wrong -----------------------------------

# name -> (H, L, n_mel, C, B, T, seq_len, labels); labels index classes 0..C-2, the blank is C-1
def _ragged(b, t, zero_at, full_at, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(max(6, t // 3), t, size=b)
    s[zero_at], s[full_at] = 0, t
    return s.tolist()


def _ragged_short(b, t, empty, full_at, seed):
    """As _ragged with a list of empty slots, for the short T of the cases below: lengths from max(3, t // 3)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(max(3, t // 3), t, size=b)
    s[list(empty)], s[full_at] = 0, t
    return s.tolist()


_REF_LABELS = [[1, 2, 3, 3], [0, 1, 0, 2, 0], [4], [], [1, 2, 3, 3], [2, 2], [0, 4, 0]]
_MEL_BATCH = (4, 4, 5, [5, 3, 4, 5], [[1], [0, 2], [2], [1, 1]])          # C, B, T, seq_len, labels of mel70 / mel72
CASES = {
    "t1": (64, 1, 4, 3, 1, 1, [1], [[1]]),
    "t2": (64, 1, 4, 3, 1, 2, [2], [[0, 1]]),
    "odd_mel": (64, 2, 13, 6, 5, 9, [9, 7, 5, 9, 3], [[1, 2], [0, 3, 0], [4], [2, 2, 1], [1]]),
    "mel1": (64, 1, 1, 4, 3, 7, [7, 4, 6], [[1, 2], [0], [2, 1, 0]]),
    # 17 utterances: the second stream group has one stream; one empty slot, one full length
    "ref_shape": (128, 2, 40, 6, 17, 23, _ragged(17, 23, 5, 16, 1), [_REF_LABELS[i % 7] for i in range(17)]),
    "mel60_l3": (128, 3, 60, 6, 33, 12, _ragged(33, 12, 20, 32, 2), [_REF_LABELS[(i + 2) % 7] for i in range(33)]),
    "c8_s_long": (64, 2, 8, 8, 4, 40, [40, 33, 40, 20], [[1, 1, 2, 3, 3, 4, 5, 5, 6, 0, 0, 1], [6, 5, 4, 3, 2, 1, 0], [0, 1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6], [2, 2, 2]]),
    # [3,3,3,3] needs 7 frames and has 5: no path, beside two utterances that have one
    "no_path": (64, 2, 8, 6, 3, 8, [8, 5, 6], [[1, 2], [3, 3, 3, 3], [2]]),
    # 20 x 33 = 660 rows: 2.58 chunks of the weight-gradient reduction's 256 rows
    "split_rows": (64, 1, 8, 4, 20, 33, _ragged(20, 33, 3, 19, 3), [[1, 2], [0, 1, 0], [2]] * 6 + [[1], [2, 2, 1]]),
    # ---- the paths the kernels specialise on outside the nine above, each at the smallest shape that reaches it ----
    # hidden 256: gru_train_forward<4> / gru_train_backward<4> (four tiles per wave), a second group of two streams, C = 5
    "h256": (256, 2, 24, 5, 18, 9, _ragged_short(18, 9, [4], 17, 4), [[1, 2, 3][:1 + i % 3] for i in range(18)]),
    # 8 layers: every slot of the handle's per-layer tables, 6 * 8 + 2 = 50 weight-gradient jobs, seven flips of the dy ping-pong, C = 7
    "l8": (64, 8, 8, 7, 3, 6, [6, 4, 5], [[1, 5], [0], [2, 2]]),
    # the x-part GEMM beyond its first pass over K (64 k a pass): n_mel % 4 = 2 -> scalar loads and a partial block behind a full pass
    "mel70": (64, 1, 70) + _MEL_BATCH,
    # ... the same on the 16-byte loads: at k = 64 lane groups 2 and 3 have k + 3 >= K
    "mel72": (64, 1, 72) + _MEL_BATCH,
    # three passes, n_mel % 4 = 1, nine k-units of the weight gradient with the last one partial
    "mel133": (128, 1, 133, 3, 2, 4, [4, 3], [[1], [0, 1]]),
    # the largest n_mel a handle accepts: 16 full passes
    "mel1024": (64, 1, 1024, 3, 2, 3, [3, 2], [[1], [0]]),
    # streams 16..31 are all empty: the middle workgroup has tmax == 0 and runs only its zero-fill tails
    "dead_group": (64, 2, 8, 4, 33, 7, _ragged_short(33, 7, range(16, 32), 32, 5), [[1, 2][:1 + i % 2] for i in range(33)]),
    # two whole groups at full length: no invalid lane, no dead frame
    "full_groups": (128, 1, 8, 6, 32, 6, [6] * 32, [_REF_LABELS[i % 7][:3] for i in range(32)]),
    # 66 x 250 = 16500 rows: the weight-gradient reduction's chunks grow to 512 rows, 33 chunks with the last one partial
    "rows_chunk512": (64, 1, 4, 3, 66, 250, _ragged_short(66, 250, [7], 65, 6), [[i % 2, 1, 0][:1 + i % 3] for i in range(66)]),
}
# the first nine: the cases whose full-length logits are also held against kws_step's at 2e-5 (tests/test_gpu_train.py)
FIRST_CASES = ("t1", "t2", "odd_mel", "mel1", "ref_shape", "mel60_l3", "c8_s_long", "no_path", "split_rows")


@functools.lru_cache(maxsize=None)
def make_problem(name, seed=0):
    """-> dict(config, w (float32 dict, non-zero biases), x [B,T,n_mel] float32, seq_len [B] int32, labels (list))."""
    from keyword_spotting_amd import weights
    h, l, n_mel, c, b, t, seq_len, labels = CASES[name]
    cfg = config_of(h, l, n_mel, c)
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    w = weights.init_weights(cfg, seed=seed + 1)
    for lay in w["layers"]:
        lay["bg"] = (lay["bg"] + 0.3 * rng.standard_normal(lay["bg"].shape)).astype(np.float32)
        lay["bc"] = (0.3 * rng.standard_normal(lay["bc"].shape)).astype(np.float32)
    w["Wfc"] = (0.5 * w["Wfc"]).astype(np.float32)
    w["bfc"] = (0.5 * rng.standard_normal(c)).astype(np.float32)
    return dict(name=name, config=cfg, w=w, x=rng.standard_normal((b, t, n_mel)).astype(np.float32), seq_len=np.array(seq_len, np.int32),
                labels=[list(s) for s in labels], B=b, T=t)


def drop_masks(p, keep_prob, seed=7):
    """uint8 [L,B,T,H], floor(keep_prob + U)."""
    cfg = p["config"]
    rng = np.random.default_rng(seed)
    return np.floor(keep_prob + rng.random((cfg.num_layers, p["B"], p["T"], cfg.hidden_size))).astype(np.uint8)


# ---- the end-to-end toy task: two words in order, each a bump on its own mel bins ------------------------------------------------

TOY = dict(H=64, L=1, n_mel=8, C=4, B=16, T=24, steps=150, lr=0.02, label="12")


def toy_task(seed=0, hidden=None):
    """16 utterances of 24 frames: word 1 lights bins 0..3 for six frames, then word 2 bins 4..7, at utterance-specific times, on noise.
    -> dict(config, w, x, seq_len, labels = ctc_label([1, 2]) for all).  hidden: TOY["H"], or 128 for the model that is also served
    by the f16x3 kernels (they take hidden 128 / 256 only); the utterances are the same."""
    from keyword_spotting_amd import weights
    cfg = config_of(hidden or TOY["H"], TOY["L"], TOY["n_mel"], TOY["C"])
    rng = np.random.default_rng(seed + 11)
    b, t = TOY["B"], TOY["T"]
    x = 0.1 * rng.standard_normal((b, t, TOY["n_mel"]))
    for i in range(b):
        s1 = int(rng.integers(1, 5))
        s2 = s1 + 6 + int(rng.integers(2, 5))
        x[i, s1:s1 + 6, :4] += 1.0
        x[i, s2:s2 + 6, 4:] += 1.0
    return dict(config=cfg, w=weights.init_weights(cfg, seed=seed + 3), x=x.astype(np.float32), seq_len=np.full(b, t, np.int32),
                labels=[[0, 1, 0, 2, 0]] * b, B=b, T=t)


@functools.lru_cache(maxsize=None)
def toy_trained(seed=0, hidden=None):
    """The restatement trained on the toy task with Adam -> (losses [steps] of sum / B, final weights fp64, final logits)."""
    p = toy_task(seed, hidden)
    w = as_dtype(p["w"], np.float64)
    opt = Optimizer(w, "adam")
    losses = []
    for _ in range(TOY["steps"]):
        loss, grads, _ = loss_and_grad(w, p["x"], p["seq_len"], p["labels"])
        losses.append(loss.sum() / p["B"])
        w = opt.apply(w, grads, TOY["lr"])
    loss, _, logits = loss_and_grad(w, p["x"], p["seq_len"], p["labels"])
    losses.append(loss.sum() / p["B"])
    return np.array(losses), w, logits
