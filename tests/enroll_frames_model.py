"""TEST INFRASTRUCTURE ONLY -- the enrolment fit on frame-wise targets (include/kws_amd.h, "Frame-wise targets": kws_enroll_fit_frames)
restated in fp64 numpy on top of tests/enroll_model.py (the CTC term, the splice, TensorFlow's Adam) and tests/frame_loss_model.py (the
frame cross-entropy):

    loss_b = ctc_weight ctc_b + frame_weight ce_b        on the spliced rows z_t = (logits1[.., 0..C-2] | nn_t Wn + bn | logits1[.., C-1])
    the step's gradient: that of sum_b loss_b / K with respect to Wn and bn -- the columns C-1 .. C+n-2 of d loss_b / d z_t

with the conventions of both: frames t >= seq_len add nothing; W_b == 0 gives ce 0 and gradient 0; a slot without a valid CTC path has
ctc +inf and CTC gradient 0 (and still its frame term); a live target outside [-1, C2) counts as -1 and makes the slot's losses NaN.
Also the same step as a torch graph (F.ctc_loss + F.cross_entropy, autograd with respect to Wn and bn only) in a chosen dtype, the case
table of tests/test_gpu_enroll_frames.py, and the two end-to-end flows with the settings the host test establishes on the CPU."""
import functools

import numpy as np

import align_model as AL
import enroll_model as M
import frame_loss_model as FL


def loss_grad(nn, logits1, seq_len, labels, label_len, targets, weight, wn, bn, ctc_weight=1.0, frame_weight=1.0):
    """One enrolment of K slots -> (loss [K], ce [K], gW [H,n], gb [n]); labels / label_len may be None at ctc_weight 0."""
    nn, logits1 = np.asarray(nn, np.float64), np.asarray(logits1, np.float64)
    wn, bn = np.asarray(wn, np.float64), np.asarray(bn, np.float64)
    k, c, n = nn.shape[0], logits1.shape[2], wn.shape[1]
    loss, ce, gw, gb = np.zeros(k), np.zeros(k), np.zeros_like(wn), np.zeros_like(bn)
    for i in range(k):
        z = M.splice(logits1[i], nn[i] @ wn + bn)
        g = np.zeros_like(z)
        if ctc_weight > 0:
            ctc, g_ctc = M.ctc_loss_grad(z, seq_len[i], labels[i][:label_len[i]])
            loss[i] = ctc_weight * ctc
            g = g + ctc_weight * g_ctc
        if frame_weight > 0:
            ce_i, g_ce = FL.frame_loss(z[None], seq_len[i:i + 1], np.asarray(targets)[i:i + 1], weight)
            ce[i] = ce_i[0]
            loss[i] = loss[i] + frame_weight * ce_i[0]
            g = g + frame_weight * g_ce[0]
        dz = g[:, c - 1:c - 1 + n]
        gw += nn[i].T @ dz
        gb += dz.sum(axis=0)
    return loss, ce, gw / k, gb / k


def fit(nn, logits1, seq_len, labels, label_len, targets, weight, wn, bn, steps, lr, ctc_weight=1.0, frame_weight=1.0):
    """-> (wn, bn, loss_trace [steps, K], ce_trace [steps, K], [(wn, bn) after each step]); Adam from zero moments."""
    wn, bn = np.array(wn, np.float64), np.array(bn, np.float64)
    mw, vw, mb, vb = np.zeros_like(wn), np.zeros_like(wn), np.zeros_like(bn), np.zeros_like(bn)
    trace, ces, path = [], [], []
    for t in range(1, steps + 1):
        loss, ce, gw, gb = loss_grad(nn, logits1, seq_len, labels, label_len, targets, weight, wn, bn, ctc_weight, frame_weight)
        trace.append(loss)
        ces.append(ce)
        wn, mw, vw = M.adam_step(wn, mw, vw, gw, t, lr)
        bn, mb, vb = M.adam_step(bn, mb, vb, gb, t, lr)
        path.append((wn.copy(), bn.copy()))
    return wn, bn, np.array(trace), np.array(ces), path


# ---- the same step as a torch graph ------------------------------------------------------------------------------------------------

def torch_reference(p, dtype, ctc_weight, frame_weight):
    """One fit step of problem p on the CPU in `dtype`: F.ctc_loss(blank = C2 - 1, zero_infinity=True) + F.cross_entropy(weight=,
    ignore_index=-1) per slot on the spliced logits, autograd with respect to Wn and bn only -> dict(loss [K] (the CTC part 0 where torch
    zeroes an infinite loss), ce [K], gW, gb of sum(loss) / K).  Empty slots and slots with W_b == 0 are left out of their term."""
    import torch
    import torch.nn.functional as F
    k = p["K"]
    nn = torch.tensor(p["nn"], dtype=dtype)
    l1 = torch.tensor(p["logits1"], dtype=dtype)
    wn = torch.tensor(p["wn"], dtype=dtype, requires_grad=True)
    bn = torch.tensor(p["bn"], dtype=dtype, requires_grad=True)
    z = torch.cat([l1[..., :-1], nn @ wn + bn, l1[..., -1:]], dim=-1)
    total, loss, ce = torch.zeros((), dtype=dtype), np.zeros(k), np.zeros(k)
    live = [i for i in range(k) if p["seq_len"][i] > 0]
    if ctc_weight > 0 and live:
        lab, lab_len = M.padded_labels([p["labels"][i] for i in live])
        lp = F.log_softmax(z[live], dim=-1).transpose(0, 1)
        ctc = F.ctc_loss(lp, torch.tensor(lab, dtype=torch.long), torch.tensor(p["seq_len"][live], dtype=torch.long),
                         torch.tensor(lab_len, dtype=torch.long), blank=p["C"] + p["n"] - 1, reduction="none", zero_infinity=True)
        total = total + ctc_weight * ctc.sum()
        loss[live] = ctc_weight * ctc.detach().numpy()
    if frame_weight > 0:
        for i in live:
            term = FL._torch_ce(z[i], int(p["seq_len"][i]), p["targets"][i], p["weight"], dtype)
            if term is not None:
                total = total + frame_weight * term
                ce[i] = float(term.detach())
        loss = loss + frame_weight * ce
    if total.requires_grad:
        (total / k).backward()
    zero = lambda v: np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy()          # noqa: E731
    return dict(loss=loss, ce=ce, gW=zero(wn), gb=zero(bn))


def torch_fit(p, steps, lr, ctc_weight, frame_weight, f=np.float32):
    """The fit as the torch graph and TensorFlow's Adam in float32 -> (loss_trace [steps, K], [(wn, bn) after each step]): the yardstick
    trajectory, as enroll_model.torch_fit_float32 (f = np.float64: the same graph in fp64, against which the restatement is checked)."""
    import torch
    q = dict(p)
    dtype = torch.float32 if f is np.float32 else torch.float64
    wn, bn = p["wn"].astype(f), p["bn"].astype(f)
    mw, vw, mb, vb = np.zeros_like(wn), np.zeros_like(wn), np.zeros_like(bn), np.zeros_like(bn)
    trace, path = [], []
    for t in range(1, steps + 1):
        q["wn"], q["bn"] = wn, bn
        r = torch_reference(q, dtype, ctc_weight, frame_weight)
        gw, gb = r["gW"].astype(f), r["gb"].astype(f)
        trace.append(r["loss"])
        lr_t = f(lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
        mw, vw = f(0.9) * mw + (f(1) - f(0.9)) * gw, f(0.999) * vw + (f(1) - f(0.999)) * gw * gw
        mb, vb = f(0.9) * mb + (f(1) - f(0.9)) * gb, f(0.999) * vb + (f(1) - f(0.999)) * gb * gb
        wn = wn - lr_t * mw / (np.sqrt(vw) + f(1e-8))
        bn = bn - lr_t * mb / (np.sqrt(vb) + f(1e-8))
        path.append((wn.copy(), bn.copy()))
    return np.array(trace), path


# ---- the case table ----------------------------------------------------------------------------------------------------------------

# objective name -> (ctc_weight, frame_weight)
OBJECTIVES = {"ce": (0.0, 1.0), "mixed": (1.0, 1.0), "mixed_03_2": (0.3, 2.0)}

# class weights over C2 = 8 classes: none, one zero among unequal ones, a 50 : 1 spread
WEIGHTS = {"unit": None, "zero": [1.0, 2.0, 0.0, 1.0, 0.5, 1.0, 3.0, 1.0], "spread": [50.0, 1.0, 1.0, 2.0, 5.0, 1.0, 10.0, 1.0]}

# name -> (H, C, n, T, [(seq_len, label)] per slot, class weights, slot whose targets are all -1 or None).  T in {1, 2, 9, 33, 300}, every
# hidden size, (C, n) in {(6, 2), (6, 1), (3, 5)}, K in {1, 3, 4}; seq_len < T; an empty slot among full ones; slots whose label has no
# valid path ([5, 5] in two frames, five labels in three frames); an empty label
CASES = {
    "t1_k1": (64, 6, 2, 1, [(1, [5])], "unit", None),
    "t2_k3_no_path": (128, 6, 1, 2, [(2, [5]), (2, [5, 5]), (1, [])], "zero", None),
    "t9_k4_empty_slot": (64, 3, 5, 9, [(9, [2, 3]), (5, [0, 4, 0]), (0, [1]), (9, [])], "spread", None),
    "t33_k4_c3": (256, 3, 5, 33, [(33, [0, 2, 0, 3, 0]), (20, [2, 3, 4, 5, 6]), (0, [1]), (3, [0, 2, 0, 3, 0])], "zero", 0),
    "t33_k3_all_none": (128, 6, 2, 33, [(33, [0, 5, 0, 6, 0]), (17, [6, 0, 0, 6]), (33, [5, 5, 6, 6, 5])], "unit", 2),
    "t300_k3": (128, 6, 2, 300, [(300, M._words(5, 5, 6)), (211, [0, 5, 0, 6, 0]), (300, [0, 4, 0])], "spread", None),
    "t300_k1_h256": (256, 6, 1, 300, [(300, [0, 5, 0])], "unit", None),
    "t300_k4_h64": (64, 6, 2, 300, [(300, [0, 5, 0, 6, 0]), (299, [5, 6]), (1, [6]), (150, [])], "zero", None),
}
# ctc_weight 0 only: no LDS per frame, so no limit on T (kws_enroll_fit refuses this T: 4000 x 9 floats of lp and alpha alone)
LONG_CASES = {"t4000_k1": (64, 6, 2, 4000, [(4000, [])], "spread", None)}


def make_problem(name, seed=0):
    """enroll_model.make_problem's dict (float32 arrays) with targets [K,T] int32 over the C + n classes (runs of -1; -1 past seq_len)
    and weight ([C + n] float32 or None)."""
    h, c, n, t, slots, weights, none_slot = CASES[name] if name in CASES else LONG_CASES[name]
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    k = len(slots)
    seq_len = np.array([s for s, _ in slots], np.int32)
    targets = FL.random_targets(rng, seq_len, t, c + n, none=0.3 if t > 2 else 0.0)          # T 1 and 2: every frame labelled
    if none_slot is not None:
        targets[none_slot] = -1
    w = WEIGHTS[weights]
    return dict(name=name, H=h, C=c, n=n, K=k, T=t,
                nn=(0.5 * rng.standard_normal((k, t, h))).astype(np.float32),
                logits1=(2.0 * rng.standard_normal((k, t, c))).astype(np.float32),
                seq_len=seq_len, labels=[list(l) for _, l in slots], targets=targets,
                weight=None if w is None else np.asarray(w[:c + n], np.float32),
                wn=(0.3 * rng.standard_normal((h, n))).astype(np.float32), bn=(0.5 * rng.standard_normal(n)).astype(np.float32))


def step64(p, objective):
    """loss_grad of a problem under an objective -> dict(loss, ce, gW, gb)."""
    cw, fw = OBJECTIVES[objective]
    _, lab_len = M.padded_labels(p["labels"])
    loss, ce, gw, gb = loss_grad(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, p["targets"], p["weight"], p["wn"], p["bn"], cw, fw)
    return dict(loss=loss, ce=ce, gW=gw, gb=gb)


@functools.lru_cache(maxsize=None)
def references(name, objective, seed=0):
    """(fp64 restatement, torch float32 graph) of one step: computed once, shared by the tests."""
    import torch
    p = make_problem(name, seed)
    return step64(p, objective), torch_reference(p, torch.float32, *OBJECTIVES[objective])


# ---- the end-to-end flows ----------------------------------------------------------------------------------------------------------

def extend_targets(targets, c, n):
    """custom_keyword.extend_targets restated: head 1's blank c-1 -> c+n-1."""
    a = np.asarray(targets)
    return np.where(a == c - 1, c + n - 1, a).astype(np.int32)


def frame_targets(nn, logits1, seq_len, labels, wn, bn):
    """Enroller.frame_targets restated: align the spliced logits with the labels, classes per frame with the extended head's blank."""
    z = M.splice(np.asarray(logits1, np.float64), np.asarray(nn, np.float64) @ wn + bn)
    blank = z.shape[2] - 1
    return np.stack([AL.frame_classes(AL.align(z[i], seq_len[i], labels[i])["states"], labels[i], blank) for i in range(len(z))]).astype(np.int32)


def features(w, mel, seq_len=None):
    """The frozen stack in fp64 (oracle.gru_oracle) -> (nn_outputs [B,T,H], logits1 [B,T,C])."""
    from oracle import gru_oracle as G
    hid = w["Wfc"].shape[0]
    top, _ = G.gru_forward(dict(w, Wfc=np.eye(hid), bfc=np.zeros(hid)), mel, seq_len=seq_len, dtype=np.float64)
    return top, top @ np.asarray(w["Wfc"], np.float64) + np.asarray(w["bfc"], np.float64)


def new_mass(nn, logits1, seq_len, wn, bn):
    """Per utterance the softmax mass of the new classes summed over its live frames."""
    z = M.splice(np.asarray(logits1, np.float64), np.asarray(nn, np.float64) @ wn + bn)
    c, n = logits1.shape[2], wn.shape[1]
    sm = np.exp(M.log_softmax(z))
    return np.array([sm[i, :seq_len[i], c - 1:c - 1 + n].sum() for i in range(len(z))])


# (a) frames only, from a fresh start: a model with ONE trained word (4 classes: space, the word, other, blank), so that the two new
# classes are 3 and 4 and lie inside the columns predict_ctc's ctc_decode reads (1..4; utils/prediction.py:21).  Settings established by
# tests/test_enroll_frames_host.py on the restatement; the device test runs with the same ones.
FLOW_A = dict(label_dict={"ni3": 1}, n_new=2, words=[3, 4], keyword="34", frames=48, ctc_steps=300, frame_steps=300, lr=0.03, seeds=(0, 2))
# (b) three positives and one negative, mixed 1 / 1 from the CTC result, against the CTC-only enrolment: the default 6-class model
FLOW_B = dict(n_new=2, words=[5, 6], frames=48, steps=300, refit_steps=100, lr=0.03, negative_label=[0, 4, 0], seeds=(0, 2))
