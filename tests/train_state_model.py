"""TEST INFRASTRUCTURE ONLY -- the training graph of tests/train_model.py / tests/train_wrapped_model.py from and to carried states
(kws_train_grad_state, include/kws_amd.h), restated twice as there:

  * loss_and_grad: hand-written numpy fp64.  Every layer starts from state_in[l] (None: zeros) and state_out[l] is its state after
    frame seq_len[b] - 1; the backward's dh starts from dstate_out[l] (None: zeros) and what is left of it in front of frame 0 is
    dstate_in[l].  The objective is J = sum_b ctc_b / B + <dstate_out, state_out>; grads is dJ / d parameters, dstate_in dJ / d state_in.
    With state_in = dstate_out = None it performs train_wrapped_model.loss_and_grad's operations in its order (and so, with the
    switches off, train_model.loss_and_grad's): the numbers are equal, not close.
  * torch_reference: the same graph in torch ops with state_in.requires_grad and the inner product added to the loss -- autograd in
    float64 and float32.  torch_chain: several segments in ONE graph, each from the state the one before left, the objective the sum
    of the segments' sum_b ctc_b / B plus <dstate_out, the last state>: what chained calls have to reproduce.

Inputs per case name, fixed seed: state_in uniform in (-scale, scale) (scale 0.9: inside the cell's own range), dstate_out normal with
sigma = 1 / B, the scale of the loss gradient."""
import functools

import numpy as np

import enroll_model as E
import train_model as M
import train_wrapped_model as WM

K, EPS = WM.K, WM.EPS

# the case table of tests/test_gpu_train_state.py: id -> (module, case name, variational masks, scale of state_in)
TABLE = {
    "t1": (M, "t1", False, 0.9),                          # T = 1: state_out is one cell step, dstate_in one cell's backward
    "t2": (M, "t2", False, 0.9),
    "ref_shape": (M, "ref_shape", False, 0.9),            # 17 streams: a group of one, an empty slot
    "mel60_l3": (M, "mel60_l3", False, 0.9),
    "h256": (M, "h256", False, 0.9),                      # four tiles per wave
    "l8": (M, "l8", False, 0.9),                          # state [8,B,H]
    "dead_group": (M, "dead_group", False, 0.9),          # a workgroup that runs no frame
    "no_path": (M, "no_path", False, 0.9),
    "both_ref_shape": (WM, "both_ref_shape", False, 0.9),  # layer norm and residual
    "res_l2_var": (WM, "res_l2", True, 0.9),              # one mask per stream, keep 0.6
    "ref_shape_wide": (M, "ref_shape", False, 3.0),       # a state outside the cell's own range
}
VAR_KEEP = 0.6


@functools.lru_cache(maxsize=None)
def make_problem(key):
    """The case's problem (train_model / train_wrapped_model .make_problem) with ln, res, drop, keep_prob, state_in, dstate_out."""
    mod, name, var, scale = TABLE[key]
    p = dict(mod.make_problem(name, var=True) if var else mod.make_problem(name))
    p.setdefault("ln", False)
    p.setdefault("res", False)
    cfg = p["config"]
    rng = np.random.default_rng(77 + sum(map(ord, key)))
    shape = (cfg.num_layers, p["B"], cfg.hidden_size)
    p["state_in"] = rng.uniform(-scale, scale, shape).astype(np.float32)
    p["dstate_out"] = (rng.standard_normal(shape) / p["B"]).astype(np.float32)
    p["keep_prob"] = VAR_KEEP if var else 1.0
    p["drop"] = WM.drop_masks(p, VAR_KEEP, variational=True) if var else None
    p["key"] = key
    return p


def _states(v, n_layers, b, hid):
    return np.zeros((n_layers, b, hid)) if v is None else np.asarray(v, np.float64)


# ---- numpy fp64 ------------------------------------------------------------------------------------------------------------------

def forward(w, x, seq_len, state_in=None, ln=False, res=False, drop=None, keep_prob=1.0):
    """train_wrapped_model.forward from state_in -> (logits, tape, state_out [L,B,H])."""
    w = WM.as_dtype(w, np.float64)
    x = np.asarray(x, np.float64)
    b, t_len = x.shape[:2]
    live = np.arange(t_len)[None, :] < np.asarray(seq_len)[:, None]
    a = np.where(live[:, :, None], x, 0.0)
    tape, state_out = [], []
    for l, lay in enumerate(w["layers"]):
        ain, xn, rstd = a, None, None
        if ln:
            m = ain.mean(axis=2, keepdims=True)
            v = ((ain - m) ** 2).mean(axis=2, keepdims=True)
            rstd = np.where(live[:, :, None], 1.0 / np.sqrt(v + EPS), 0.0)
            xn = (ain - m) * rstd
            a = np.where(live[:, :, None], xn * lay["ibeta"] + lay["igamma"], 0.0)
        hid = lay["bc"].shape[0]
        h = np.zeros((b, hid)) if state_in is None else np.asarray(state_in[l], np.float64)
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
        state_out.append(h)
        if drop is not None:
            y = y * WM._mask(drop, l, t_len) / keep_prob
        tape.append(dict(a=a, r=r, u=u, c=c, h=hs, live=live, ain=ain, xn=xn, rstd=rstd))
        a = K * (y + ain) if res and l >= 1 else y
    return a @ w["Wfc"] + w["bfc"], dict(layers=tape, top=a), np.stack(state_out)


def loss_and_grad(w, x, seq_len, labels, state_in=None, dstate_out=None, ln=False, res=False, drop=None, keep_prob=1.0):
    """-> (loss [B] (+inf without a path), dJ / d parameters in the dict form, logits, state_out [L,B,H], dstate_in [L,B,H])."""
    w64 = WM.as_dtype(w, np.float64)
    logits, tape, state_out = forward(w64, x, seq_len, state_in, ln, res, drop, keep_prob)
    b, t_len, _ = logits.shape
    loss, gl = np.zeros(b), np.zeros_like(logits)
    for i in range(b):
        loss[i], gl[i] = E.ctc_loss_grad(logits[i], seq_len[i], labels[i])
    gl /= b
    top = tape["top"]
    n_layers = len(w64["layers"])
    grads = dict(layers=[None] * n_layers, Wfc=np.einsum("bth,btc->hc", top, gl), bfc=gl.sum(axis=(0, 1)))
    dstate_in = [None] * n_layers
    dy = gl @ w64["Wfc"].T
    for l in range(n_layers - 1, -1, -1):
        lay, tp = w64["layers"][l], tape["layers"][l]
        hid, n_in = lay["bc"].shape[0], tp["a"].shape[2]
        residual = res and l >= 1
        if residual:
            dy = K * dy
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
    return loss, grads, logits, state_out, np.stack(dstate_in)


def of_problem(p, **kw):
    """loss_and_grad on a make_problem() dict; kw overrides (state_in=None, ...)."""
    args = dict(state_in=p["state_in"], dstate_out=p["dstate_out"], ln=p["ln"], res=p["res"], drop=p["drop"], keep_prob=p["keep_prob"])
    args.update(kw)
    return loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], **args)


# ---- torch -----------------------------------------------------------------------------------------------------------------------

def _torch_segment(tw, x, seq_len, labels, h0, dtype, ln, res, drop, keep_prob):
    """One call's graph from the list of states h0 -> (sum_b ctc_b / B as a tensor, loss [B] numpy, logits, the list of final states)."""
    import torch
    import torch.nn.functional as F
    seq_len = np.asarray(seq_len)
    b, t_len = x.shape[:2]
    live = torch.tensor(np.arange(t_len)[None, :] < seq_len[:, None])
    zero = torch.zeros((), dtype=dtype)
    a = torch.where(live[:, :, None], torch.tensor(np.asarray(x), dtype=dtype), zero)
    out_states = []
    for l, lay in enumerate(tw["layers"]):
        ain = a
        if ln:
            m = ain.mean(dim=2, keepdim=True)
            v = ((ain - m) ** 2).mean(dim=2, keepdim=True)
            a = torch.where(live[:, :, None], (ain - m) / torch.sqrt(v + EPS) * lay["ibeta"] + lay["igamma"], zero)
        hid = lay["bc"].shape[0]
        h = h0[l]
        ys = []
        for t in range(t_len):
            g = torch.sigmoid(torch.cat([a[:, t], h], dim=1) @ lay["Wg"] + lay["bg"])
            r, u = g[:, :hid], g[:, hid:]
            c = torch.tanh(torch.cat([a[:, t], r * h], dim=1) @ lay["Wc"] + lay["bc"])
            hn = u * h + (1.0 - u) * c
            on = live[:, t, None]
            ys.append(torch.where(on, hn, zero))
            h = torch.where(on, hn, h)
        out_states.append(h)
        a = torch.stack(ys, dim=1)
        if drop is not None:
            a = a * torch.tensor(WM._mask(drop, l, t_len).astype(np.float64), dtype=dtype) / keep_prob
        if res and l >= 1:
            a = K * (a + ain)
    logits = a @ tw["Wfc"] + tw["bfc"]
    idx = [i for i in range(b) if seq_len[i] > 0]
    loss = np.zeros(b)
    total = torch.zeros((), dtype=dtype)
    if idx:
        lab, lab_len = E.padded_labels([labels[i] for i in idx])
        lp = F.log_softmax(logits[idx], dim=-1).transpose(0, 1)
        loss_live = F.ctc_loss(lp, torch.tensor(lab, dtype=torch.long), torch.tensor(seq_len[idx], dtype=torch.long),
                               torch.tensor(lab_len, dtype=torch.long), blank=logits.shape[2] - 1, reduction="none", zero_infinity=True)
        total = loss_live.sum() / b
        loss[idx] = loss_live.detach().numpy()
    return total, loss, logits, out_states


def _leaves(w, dtype):
    import torch
    return WM.unflat(w, [torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for _, v in WM.flat(w)])


def _grads_of(w, tw):
    import torch
    return WM.unflat(w, [(v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for _, v in WM.flat(tw)])


def torch_reference(w, x, seq_len, labels, dtype, state_in=None, dstate_out=None, ln=False, res=False, drop=None, keep_prob=1.0):
    """-> dict(loss [B] (0 where torch zeroes an infinite loss), logits, grads, state_out, dstate_in) of J in `dtype` on the CPU."""
    import torch
    tw = _leaves(w, dtype)
    n_layers, b, hid = len(w["layers"]), x.shape[0], w["layers"][0]["bc"].shape[0]
    s0 = torch.tensor(_states(state_in, n_layers, b, hid), dtype=dtype, requires_grad=True)
    total, loss, logits, out = _torch_segment(tw, x, seq_len, labels, [s0[l] for l in range(n_layers)], dtype, ln, res, drop, keep_prob)
    state_out = torch.stack(out)
    if dstate_out is not None:
        total = total + (torch.tensor(np.asarray(dstate_out), dtype=dtype) * state_out).sum()
    total.backward()
    return dict(loss=loss, logits=logits.detach().numpy(), grads=_grads_of(w, tw), state_out=state_out.detach().numpy(),
                dstate_in=(s0.grad if s0.grad is not None else torch.zeros_like(s0)).numpy())


def torch_of_problem(p, dtype, **kw):
    args = dict(state_in=p["state_in"], dstate_out=p["dstate_out"], ln=p["ln"], res=p["res"], drop=p["drop"], keep_prob=p["keep_prob"])
    args.update(kw)
    return torch_reference(p["w"], p["x"], p["seq_len"], p["labels"], dtype, **args)


def torch_chain(w, segments, dtype, state_in=None, dstate_out=None, ln=False, res=False):
    """segments: [(x, seq_len, labels), ...] run in ONE graph, each from the state the one before left; the objective is the sum of the
    segments' sum_b ctc_b / B + <dstate_out, the last segment's state_out> (a stream that ended in an earlier segment carries its part
    of dstate_out back through every later segment's seq_len = 0 and its own dead frames) -> dict(loss [segments, B], grads, state_out (the last segment's), dstate_in (w.r.t. state_in))."""
    import torch
    tw = _leaves(w, dtype)
    n_layers, b, hid = len(w["layers"]), segments[0][0].shape[0], w["layers"][0]["bc"].shape[0]
    s0 = torch.tensor(_states(state_in, n_layers, b, hid), dtype=dtype, requires_grad=True)
    h = [s0[l] for l in range(n_layers)]
    total, losses = torch.zeros((), dtype=dtype), []
    for x, seq_len, labels in segments:
        part, loss, _, h = _torch_segment(tw, x, seq_len, labels, h, dtype, ln, res, None, 1.0)
        total = total + part
        losses.append(loss)
    if dstate_out is not None:
        total = total + (torch.tensor(np.asarray(dstate_out), dtype=dtype) * torch.stack(h)).sum()
    total.backward()
    return dict(loss=np.array(losses), grads=_grads_of(w, tw), state_out=torch.stack(h).detach().numpy(),
                dstate_in=(s0.grad if s0.grad is not None else torch.zeros_like(s0)).numpy())


def add_grads(w, a, b):
    return WM.unflat(w, [np.asarray(u, np.float64) + np.asarray(v, np.float64) for (_, u), (_, v) in zip(WM.flat(a), WM.flat(b))])


# ---- shared, computed once ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference(key):
    """(fp64 restatement, float32 torch) of the state call on a TABLE case: computed once, shared by the tests that need it."""
    import torch
    p = make_problem(key)
    return of_problem(p), torch_of_problem(p, torch.float32)


# the two segments of the chained back-propagation tests: a case's utterances cut at CHAIN_CUT frames, each part with labels of its own
CHAIN_CUT = {"ref_shape": 9, "both_ref_shape": 9}


@functools.lru_cache(maxsize=None)
def chain_problem(key):
    """-> (p, [(x, seq_len, labels) of A, of B]): the case's frames [0, cut) and [cut, T) with train_model's labels cut to what fits."""
    from keyword_spotting_amd.training import segment_lengths
    p = make_problem(key)
    cut = CHAIN_CUT[key]
    segs = []
    for start, frames, shift in ((0, cut, 0), (cut, p["T"] - cut, 1)):
        sl = segment_lengths(p["seq_len"], start, frames)
        labels = [list(p["labels"][(i + shift) % p["B"]][:max(0, (int(sl[i]) - 1) // 2)]) for i in range(p["B"])]
        segs.append((p["x"][:, start:start + frames], sl, labels))
    return p, segs


@functools.lru_cache(maxsize=None)
def chain_reference(key):
    """(float64, float32) torch_chain of chain_problem(key) from the case's state_in, with its dstate_out on the last state."""
    import torch
    p, segs = chain_problem(key)
    return tuple(torch_chain(p["w"], segs, dt, p["state_in"], p["dstate_out"], p["ln"], p["res"]) for dt in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def trajectory(key, kind, steps, lr, float32=False):
    """`steps` optimiser steps on a TABLE case, step s from the state_out of step s - 1 (the first from zeros), dstate_out = None ->
    (loss [steps, B], [parameter blob after each step]).  float32: the torch graph and the optimiser in float32; else the restatement."""
    import torch
    p = make_problem(key)
    w = p["w"] if float32 else WM.as_dtype(p["w"], np.float64)
    opt = WM.Optimizer(w, kind, np.float32 if float32 else np.float64)
    state, losses, path = None, [], []
    for _ in range(steps):
        if float32:
            r = torch_of_problem(dict(p, w=w), torch.float32, state_in=state, dstate_out=None)
            loss, grads, state = r["loss"], r["grads"], r["state_out"]
        else:
            loss, grads, _, state, _ = of_problem(dict(p, w=w), state_in=state, dstate_out=None)
        w = opt.apply(w, grads, lr)
        losses.append(np.asarray(loss, np.float64))
        path.append(WM.blob_of(w))
    return np.array(losses), path
