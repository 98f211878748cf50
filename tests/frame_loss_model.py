"""TEST INFRASTRUCTURE ONLY -- frame-wise targets (include/kws_amd.h, "Frame-wise targets") restated:

  * frame_loss: the loss and its gradient with respect to the logits in numpy, in fp64 or -- the yardstick of the GPU tests -- with every
    operation in float32.  For utterance b with n = seq_len[b], targets y_t in {-1, 0..C-1} and class weights w:
        W_b = sum_{t<n, y_t>=0} w[y_t];   ce_b = sum w[y_t] (logsumexp(z_t) - z_t[y_t]) / W_b;   d ce_b / d z_t = w[y_t] / W_b (softmax - e_y)
    W_b == 0 gives 0 / 0.  A live target outside [-1, C) counts as -1 and makes ce_b NaN.  Nothing at t >= n is read.
  * gru_loss_and_grad: the mixed objective J = sum_b (ctc_weight ctc_b + frame_weight ce_b) / B + <dstate_out, state_out> through
    tests/train_state_model.py's forward (plain, wrapped, from a carried state) in numpy fp64.  Its backward is that file's
    loss_and_grad restated from a given gradient of the logits: with frame_weight 0 and ctc_weight 1 the numbers are equal, not close
    (tests/test_frame_loss_host.py holds that).
  * gru_torch / attention_torch: the trainer graphs of tests/train_state_model.py and tests/attention_train_model.py in torch on the
    CPU with F.cross_entropy(weight=, ignore_index=-1, reduction='mean') per utterance added, in a chosen dtype.
  * the case tables of tests/test_gpu_frame_loss.py and tests/test_gpu_train_frames.py, and the toy task trained on frame-wise targets."""
import functools

import numpy as np

import align_model as AL
import attention_train_model as AM
import enroll_model as E
import train_model as M
import train_state_model as SM
import train_wrapped_model as WM


# ---- the loss ----------------------------------------------------------------------------------------------------------------------

def frame_loss(logits, seq_len, targets, weight=None, dtype=np.float64):
    """logits [B,T,C], seq_len [B], targets [B,T] -> (ce [B], grad [B,T,C]) in `dtype` arithmetic."""
    f = dtype
    logits, targets = np.asarray(logits), np.asarray(targets)
    b_n, t_n, c = logits.shape
    w = np.ones(c, f) if weight is None else np.asarray(weight, f)
    ce, grad = np.zeros(b_n, f), np.zeros((b_n, t_n, c), f)
    for b in range(b_n):
        n = int(seq_len[b])
        y = targets[b, :n].astype(np.int64)
        bad = (y < -1) | (y >= c)
        on = (y >= 0) & ~bad
        if on.any():
            z = logits[b, :n][on].astype(f)
            yy = y[on]
            m = z.max(axis=1, keepdims=True)
            lse = (m[:, 0] + np.log(np.exp(z - m).sum(axis=1, dtype=f))).astype(f)
            wy = w[yy]
            total = wy.sum(dtype=f)
            if total > 0:
                ce[b] = (wy * (lse - z[np.arange(len(yy)), yy])).sum(dtype=f) / total
                g = np.exp(z - lse[:, None]).astype(f)
                g[np.arange(len(yy)), yy] -= f(1.0)
                rows = np.zeros((n, c), f)
                rows[on] = (wy / total)[:, None] * g
                grad[b, :n] = rows
        if bad.any():
            ce[b] = np.nan
    return ce, grad


def random_targets(rng, seq_len, t_n, c, none=0.3, garbage=False):
    """[B,T] int32: a class per live frame, runs of -1 (probability `none` of starting one, two to four frames long); past seq_len -1, or
    with `garbage` values far outside the classes (those frames are never read)."""
    out = np.full((len(seq_len), t_n), -1, np.int32)
    for b, n in enumerate(seq_len):
        t = 0
        while t < n:
            if rng.random() < none:
                t += int(rng.integers(2, 5))
            else:
                out[b, t] = rng.integers(0, c)
                t += 1
        if garbage:
            out[b, n:] = rng.integers(1000, 2 ** 30, size=t_n - n) * rng.choice([-1, 1], size=t_n - n)
    return out


# ---- the GRU trainers' graph, numpy fp64 ---------------------------------------------------------------------------------------------

def _backward(w64, tape, gl, dstate_out, ln, res, drop, keep_prob):
    """train_state_model.loss_and_grad's backward from gl = dJ / d logits [B,T,C] -> (grads, dstate_in)."""
    top = tape["top"]
    b, t_len = gl.shape[:2]
    n_layers = len(w64["layers"])
    grads = dict(layers=[None] * n_layers, Wfc=np.einsum("bth,btc->hc", top, gl), bfc=gl.sum(axis=(0, 1)))
    dstate_in = [None] * n_layers
    dy = gl @ w64["Wfc"].T
    for l in range(n_layers - 1, -1, -1):
        lay, tp = w64["layers"][l], tape["layers"][l]
        hid, n_in = lay["bc"].shape[0], tp["a"].shape[2]
        residual = res and l >= 1
        if residual:
            dy = SM.K * dy
        share = dy
        if drop is not None:
            dy = dy * WM._mask(drop, l, t_len) / keep_prob
        g = dict(Wg=np.zeros_like(lay["Wg"]), bg=np.zeros_like(lay["bg"]), Wc=np.zeros_like(lay["Wc"]), bc=np.zeros_like(lay["bc"]))
        dx = np.zeros_like(tp["a"])
        dh = np.zeros((b, hid)) if dstate_out is None else np.asarray(dstate_out[l], np.float64)
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
        dstate_in[l] = dh
        if ln:
            dn = dx * lay["ibeta"]
            mean_dn = dn.mean(axis=2, keepdims=True)
            mean_dn_xn = (dn * tp["xn"]).mean(axis=2, keepdims=True)
            g["ibeta"] = (dx * tp["xn"]).sum()
            g["igamma"] = dx.sum(axis=(0, 1))
            dx = tp["rstd"] * (dn - mean_dn - tp["xn"] * mean_dn_xn)
        grads["layers"][l] = g
        dy = dx + share if residual else dx
    return grads, np.stack(dstate_in)


def gru_loss_and_grad(w, x, seq_len, labels, targets, ctc_weight=1.0, frame_weight=0.0, class_weight=None, state_in=None, dstate_out=None,
                      ln=False, res=False, drop=None, keep_prob=1.0):
    """-> dict(loss [B] = ctc_weight ctc_b + frame_weight ce_b, ce [B], grads (dJ / d parameters, dict form), logits, state_out,
    dstate_in).  labels may be None at ctc_weight 0."""
    w64 = WM.as_dtype(w, np.float64)
    logits, tape, state_out = SM.forward(w64, x, seq_len, state_in, ln, res, drop, keep_prob)
    b = logits.shape[0]
    loss, gl, ce = np.zeros(b), np.zeros_like(logits), np.zeros(b)
    if ctc_weight > 0:
        for i in range(b):
            loss[i], gl[i] = E.ctc_loss_grad(logits[i], seq_len[i], labels[i])
        gl /= b
        if ctc_weight != 1.0:
            loss, gl = ctc_weight * loss, ctc_weight * gl
    if frame_weight > 0:
        ce, gce = frame_loss(logits, seq_len, targets, class_weight)
        loss = loss + frame_weight * ce
        gl = gl + (frame_weight / b) * gce
    grads, dstate_in = _backward(w64, tape, gl, dstate_out, ln, res, drop, keep_prob)
    return dict(loss=loss, ce=ce, grads=grads, logits=logits, state_out=state_out, dstate_in=dstate_in)


# ---- the trainers' graphs in torch ---------------------------------------------------------------------------------------------------

def _torch_ce(logits_b, n, targets_b, weight, dtype):
    """F.cross_entropy over the first n rows of one utterance -> a tensor (None where W_b == 0: torch would give NaN, the library 0)."""
    import torch
    import torch.nn.functional as F
    y = np.asarray(targets_b[:n], np.int64)
    w = None if weight is None else torch.tensor(np.asarray(weight, np.float64), dtype=dtype)
    total = float((y >= 0).sum()) if weight is None else float(np.asarray(weight, np.float64)[y[y >= 0]].sum())
    if n == 0 or total <= 0:
        return None
    return F.cross_entropy(logits_b[:n], torch.tensor(y), weight=w, ignore_index=-1, reduction="mean")


def gru_torch(w, x, seq_len, labels, targets, dtype, ctc_weight=1.0, frame_weight=0.0, class_weight=None, state_in=None, dstate_out=None,
              ln=False, res=False, drop=None, keep_prob=1.0):
    """train_state_model.torch_reference's graph with the frame term added -> dict(loss, ce, logits, grads, state_out, dstate_in)."""
    import torch
    tw = SM._leaves(w, dtype)
    n_layers, b, hid = len(w["layers"]), x.shape[0], w["layers"][0]["bc"].shape[0]
    s0 = torch.tensor(SM._states(state_in, n_layers, b, hid), dtype=dtype, requires_grad=True)
    ctc_labels = labels if ctc_weight > 0 else [[]] * b
    total, loss, logits, out = SM._torch_segment(tw, x, seq_len, ctc_labels, [s0[l] for l in range(n_layers)], dtype, ln, res, drop, keep_prob)
    total, loss = (ctc_weight * total, ctc_weight * loss) if ctc_weight > 0 else (torch.zeros((), dtype=dtype), np.zeros(b))
    ce = np.zeros(b)
    if frame_weight > 0:
        for i in range(b):
            term = _torch_ce(logits[i], int(seq_len[i]), targets[i], class_weight, dtype)
            if term is not None:
                total = total + (frame_weight / b) * term
                ce[i] = float(term.detach())
        loss = loss + frame_weight * ce
    state_out = torch.stack(out)
    if dstate_out is not None:
        total = total + (torch.tensor(np.asarray(dstate_out), dtype=dtype) * state_out).sum()
    total.backward()
    return dict(loss=loss, ce=ce, logits=logits.detach().numpy(), grads=SM._grads_of(w, tw), state_out=state_out.detach().numpy(),
                dstate_in=(s0.grad if s0.grad is not None else torch.zeros_like(s0)).numpy())


def attention_torch(cfg, w, x, seq_len, labels, targets, dtype, ctc_weight=1.0, frame_weight=0.0, class_weight=None, seed=0, keep_prob=1.0):
    """attention_train_model.torch_reference's graph with the frame term on the [B,T'] targets added -> dict(loss, ce, logits, grads)."""
    import torch
    import torch.nn.functional as F
    A = AM.A
    tw = AM.torch_params(w, dtype)
    B, T = x.shape[:2]
    C = cfg.num_classes
    loss, ce, logits, total = np.zeros(B), np.zeros(B), np.zeros((B, A.frames_out(T, cfg.combine_frame), C)), None
    for b in range(B):
        n = A.frames_out(int(seq_len[b]), cfg.combine_frame)
        if n == 0:
            continue
        lg = AM.torch_forward(cfg, tw, np.asarray(x[b, :int(seq_len[b])], np.float64), b, seed, keep_prob, dtype)
        logits[b, :n] = lg.detach().numpy()
        part = torch.zeros((), dtype=dtype)
        if ctc_weight > 0:
            lab = torch.tensor(np.asarray(labels[b], np.int64).reshape(1, -1))
            lb = F.ctc_loss(F.log_softmax(lg, dim=-1)[:, None, :], lab, torch.tensor([n]), torch.tensor([lab.shape[1]]), blank=C - 1,
                            reduction="none", zero_infinity=True)
            part = part + ctc_weight * lb.sum()
        term = _torch_ce(lg, n, targets[b], class_weight, dtype) if frame_weight > 0 else None
        if term is not None:
            part = part + frame_weight * term
            ce[b] = float(term.detach())
        loss[b] = float(part.detach())
        total = part if total is None else total + part
    if total is not None and total.requires_grad:
        (total / B).backward()
    grads = AM.unflat([(v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))) for _, v in AM.flat(tw)], len(w["layers"]))
    return dict(loss=loss, ce=ce, logits=logits, grads=grads)


# ---- case tables ---------------------------------------------------------------------------------------------------------------------

# the stand-alone kernel: name -> (B, T, C, class weights or None).  T around the workgroup's 32 frames per pass and its multiples, 1 and 2,
# one beyond any LDS limit of the CTC kernels; B = 17 has seq_len 0 at slot 3, full length at slot 16, an utterance of -1 only at slot 5
# and one of blanks only at slot 7
_ZERO_W = {3: [1.0, 0.0, 2.0], 5: [1.0, 0.0, 2.0, 0.5, 1.0], 6: [0.5, 1.0, 0.0, 2.0, 1.0, 1.5], 8: [1.0, 2.0, 0.0, 1.0, 0.5, 1.0, 3.0, 1.0]}
_SPREAD_W = {3: [50.0, 1.0, 5.0], 5: [1.0, 50.0, 2.0, 10.0, 1.0], 6: [1.0, 2.0, 50.0, 1.0, 25.0, 1.0], 8: [50.0, 1.0, 1.0, 2.0, 5.0, 1.0, 10.0, 1.0]}
KERNEL_CASES = {}
for _i, _t in enumerate((1, 2, 63, 64, 65, 255, 256, 257, 300)):
    _c = (3, 5, 6, 8)[_i % 4]
    KERNEL_CASES["t%d_c%d_b17" % (_t, _c)] = (17, _t, _c, (None, _ZERO_W[_c], _SPREAD_W[_c])[_i % 3])
    KERNEL_CASES["t%d_c%d_b1" % (_t, (5, 6, 8, 3)[_i % 4])] = (1, _t, (5, 6, 8, 3)[_i % 4], (_SPREAD_W, _ZERO_W)[_i % 2][(5, 6, 8, 3)[_i % 4]])
KERNEL_CASES["t4000_c6_b3"] = (3, 4000, 6, _SPREAD_W[6])
KERNEL_CASES["t33_c3_b17"] = (17, 33, 3, _ZERO_W[3])
KERNEL_CASES["t40_c8_b17"] = (17, 40, 8, None)


@functools.lru_cache(maxsize=None)
def kernel_problem(name):
    """-> dict(logits [B,T,C] float32, seq_len, targets, weight (float32 or None), ref64 / ref32 = frame_loss in fp64 / float32)."""
    b, t, c, weight = KERNEL_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    logits = (3.0 * rng.standard_normal((b, t, c))).astype(np.float32)
    seq_len = rng.integers(max(1, t // 3), t + 1, size=b).astype(np.int32)
    if b >= 17:
        seq_len[3], seq_len[16] = 0, t
    else:
        seq_len[0] = t
    targets = random_targets(rng, seq_len, t, c)
    if b >= 17:
        targets[5, :] = -1
        targets[7, :seq_len[7]] = c - 1
        for i in (0, 16):          # -1 at the first and at the last live frame; a class at their neighbours
            targets[i, 0], targets[i, seq_len[i] - 1] = -1, -1
            if seq_len[i] > 2:
                targets[i, 1], targets[i, seq_len[i] - 2] = 0, c - 1
    weight = None if weight is None else np.asarray(weight, np.float32)
    return dict(name=name, B=b, T=t, C=c, logits=logits, seq_len=seq_len, targets=targets, weight=weight,
                ref64=frame_loss(logits, seq_len, targets, weight), ref32=frame_loss(logits, seq_len, targets, weight, np.float32))


# the trainers: objective name -> (ctc_weight, frame_weight, with class weights)
OBJECTIVES = {"frames": (0.0, 1.0, False), "ctc": (1.0, 0.0, False), "mixed": (1.0, 0.5, True)}
GRU_CASES = ("t1", "odd_mel", "ref_shape", "h256", "dead_group", "split_rows")          # of train_model.CASES
ATTENTION_CASES = {"c2": ("frames", 1.0), "c4": ("mixed", 1.0), "head32": ("mixed", 0.9)}          # of attention_train_model.CASES: (objective, keep_prob)


def class_weights(c, on=True):
    """A fixed 8:1 spread over c classes in a shuffled order (float32, no two alike), or None."""
    return (1.0 + 7.0 * np.random.default_rng(c).permutation(c) / (c - 1)).astype(np.float32) if on else None


def gru_targets(p, seed=0):
    """[B,T] random targets with runs of -1 for a train_model / train_wrapped_model / train_state_model problem."""
    rng = np.random.default_rng(4242 + seed + sum(map(ord, p["name"])))
    return random_targets(rng, p["seq_len"], p["T"], p["config"].num_classes)


def attention_targets(p, seed=0):
    """[B,T'] random targets with runs of -1 for an attention_train_model problem."""
    cfg = p["config"]
    rng = np.random.default_rng(777 + seed + sum(map(ord, p["name"])))
    rows = [AM.A.frames_out(int(n), cfg.combine_frame) for n in p["seq_len"]]
    return random_targets(rng, rows, AM.A.frames_out(p["x"].shape[1], cfg.combine_frame), cfg.num_classes)


@functools.lru_cache(maxsize=None)
def gru_reference(name, objective):
    """(fp64 torch graph, float32 torch graph, targets, class weights) of a GRU case under an objective: computed once."""
    import torch
    p = M.make_problem(name)
    cw, fw, weighted = OBJECTIVES[objective]
    targets, weight = gru_targets(p), class_weights(p["config"].num_classes, weighted)
    args = (p["w"], p["x"], p["seq_len"], p["labels"], targets)
    kw = dict(ctc_weight=cw, frame_weight=fw, class_weight=weight)
    return gru_torch(*args, torch.float64, **kw), gru_torch(*args, torch.float32, **kw), targets, weight


TRAJECTORY = dict(name="ref_shape", objective="mixed", kind="adam", steps=20, lr=M.TRAJECTORY_LR["adam"])


@functools.lru_cache(maxsize=None)
def gru_trajectory(float32=False):
    """TRAJECTORY's steps of the mixed objective -> (loss [steps, B], [parameter blob after each step]): the numpy fp64 restatement, or
    the torch graph and the optimiser in float32 (the yardstick trajectory)."""
    import torch
    p = M.make_problem(TRAJECTORY["name"])
    cw, fw, weighted = OBJECTIVES[TRAJECTORY["objective"]]
    targets, weight = gru_targets(p), class_weights(p["config"].num_classes, weighted)
    w = p["w"] if float32 else M.as_dtype(p["w"], np.float64)
    opt = M.Optimizer(w, TRAJECTORY["kind"], np.float32 if float32 else np.float64)
    losses, path = [], []
    for _ in range(TRAJECTORY["steps"]):
        if float32:
            r = gru_torch(w, p["x"], p["seq_len"], p["labels"], targets, torch.float32, cw, fw, weight)
        else:
            r = gru_loss_and_grad(w, p["x"], p["seq_len"], p["labels"], targets, cw, fw, weight)
        w = opt.apply(w, r["grads"], TRAJECTORY["lr"])
        losses.append(np.asarray(r["loss"], np.float64))
        path.append(M.blob_of(w))
    return np.array(losses), path


# ---- the toy task on frame-wise targets ------------------------------------------------------------------------------------------------

# the settings tests/test_frame_loss_host.py establishes on the CPU and tests/test_gpu_train_frames.py trains with on the device: frames
# only, Adam, train_model.TOY's steps and learning rate, unit class weights
TOY_FRAMES = dict(steps=M.TOY["steps"], lr=M.TOY["lr"], class_weight=None)


def toy_targets(logits, p):
    """The frame-wise targets of the toy task: align_model's best path through each utterance's transcript on `logits`, as classes."""
    blank = p["config"].num_classes - 1
    return np.stack([AL.frame_classes(AL.align(logits[i], p["seq_len"][i], p["labels"][i])["states"], p["labels"][i], blank)
                     for i in range(p["B"])])


@functools.lru_cache(maxsize=None)
def toy_frames_trained(seed=0):
    """The restatement trained on the toy task's frame-wise targets alone (ctc_weight 0) from toy_task's initial weights
    -> (losses [steps + 1] of sum / B, final logits, targets)."""
    p = M.toy_task(seed)
    targets = toy_targets(M.toy_trained(seed)[2], p)
    w = M.as_dtype(p["w"], np.float64)
    opt = M.Optimizer(w, "adam")
    losses = []
    for _ in range(TOY_FRAMES["steps"]):
        r = gru_loss_and_grad(w, p["x"], p["seq_len"], None, targets, 0.0, 1.0, TOY_FRAMES["class_weight"])
        losses.append(r["loss"].sum() / p["B"])
        w = opt.apply(w, r["grads"], TOY_FRAMES["lr"])
    r = gru_loss_and_grad(w, p["x"], p["seq_len"], None, targets, 0.0, 1.0, TOY_FRAMES["class_weight"])
    losses.append(r["loss"].sum() / p["B"])
    return np.array(losses), r["logits"], targets
