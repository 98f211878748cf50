"""TEST INFRASTRUCTURE ONLY -- fp64 numpy restatement of the customised-keyword enrolment (README "Customize keyword";
models/rnn_ctc.py:59-101): the CTC loss with the blank as the LAST class, its gradient with respect to the logits (softmax -
occupancy / P), the splice of n new logits between head 1's columns and its blank, the gradient with respect to the new columns
and their bias, and tf.train.AdamOptimizer's update.

Conventions of kws_ctc_loss / kws_enroll_fit (include/kws_amd.h): frames t >= seq_len contribute nothing; seq_len == 0 is an empty
slot (loss 0, gradient 0, label ignored); an utterance without a valid path has loss +inf and gradient exactly 0.
"""
import numpy as np

NEG = -np.inf


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _extended(label, blank):
    ext = np.full(2 * len(label) + 1, blank, np.int64)
    ext[1::2] = label
    skip = np.zeros(len(ext), bool)            # s-2 -> s: ext[s] is no blank and differs from ext[s-2]
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    return ext, skip


def ctc_loss_grad(logits, seq_len, label):
    """One utterance: logits [T, C] (blank = C-1), its first seq_len frames, label (a sequence over 0..C-2) -> (loss, grad [T, C])."""
    logits = np.asarray(logits, np.float64)
    t_len, c = logits.shape
    grad = np.zeros((t_len, c))
    n = int(seq_len)
    if n == 0:
        return 0.0, grad
    lp = log_softmax(logits[:n])
    ext, skip = _extended(np.asarray(label, np.int64), c - 1)
    ns = len(ext)
    alpha = np.full((n, ns), NEG)
    alpha[0, :2] = lp[0, ext[:2]]
    for t in range(1, n):
        a = alpha[t - 1]
        a1 = np.concatenate([[NEG], a])[:ns]
        a2 = np.where(skip, np.concatenate([[NEG, NEG], a])[:ns], NEG)
        alpha[t] = np.logaddexp(np.logaddexp(a, a1), a2) + lp[t, ext]
    log_p = np.logaddexp(alpha[n - 1, ns - 1], alpha[n - 1, ns - 2] if ns > 1 else NEG)
    if log_p == NEG:
        return np.inf, grad
    beta = np.full((n, ns), NEG)
    beta[n - 1, max(ns - 2, 0):] = lp[n - 1, ext[max(ns - 2, 0):]]
    skip_out = np.concatenate([skip, [False, False]])[2:]
    for t in range(n - 2, -1, -1):
        b = beta[t + 1]
        b1 = np.concatenate([b, [NEG]])[1:]
        b2 = np.where(skip_out, np.concatenate([b, [NEG, NEG]])[2:], NEG)
        beta[t] = np.logaddexp(np.logaddexp(b, b1), b2) + lp[t, ext]
    with np.errstate(invalid="ignore"):
        occ = np.exp(np.where((alpha > NEG) & (beta > NEG), alpha + beta - lp[:, ext] - log_p, NEG))
    grad[:n] = np.exp(lp)
    for s in range(ns):
        grad[:n, ext[s]] -= occ[:, s]
    return -log_p, grad


def splice(logits1, new_logits):
    """(space, words, garbage | new | blank): weights.extend_head's column order, on logits."""
    return np.concatenate([logits1[..., :-1], new_logits, logits1[..., -1:]], axis=-1)


def enroll_loss_grad(nn, logits1, seq_len, labels, label_len, wn, bn):
    """One enrolment of K slots: nn [K,T,H], logits1 [K,T,C], wn [H,n], bn [n] -> (loss [K], gW [H,n], gb [n]); the gradient of
    sum(loss) / K, as the reference's reduce_sum(ctc_loss) / config.batch_size (infeasible and empty slots add nothing)."""
    nn, logits1 = np.asarray(nn, np.float64), np.asarray(logits1, np.float64)
    wn, bn = np.asarray(wn, np.float64), np.asarray(bn, np.float64)
    k, c, n = nn.shape[0], logits1.shape[2], wn.shape[1]
    loss, gw, gb = np.zeros(k), np.zeros_like(wn), np.zeros_like(bn)
    for i in range(k):
        z = splice(logits1[i], nn[i] @ wn + bn)
        loss[i], g = ctc_loss_grad(z, seq_len[i], labels[i][:label_len[i]])
        dz = g[:, c - 1:c - 1 + n]
        gw += nn[i].T @ dz
        gb += dz.sum(axis=0)
    return loss, gw / k, gb / k


def adam_step(theta, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer at step t (1-based): epsilon outside the root, the bias corrections in the step size."""
    lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return theta - lr_t * m / (np.sqrt(v) + eps), m, v


def fit(nn, logits1, seq_len, labels, label_len, wn, bn, steps, lr):
    """-> (wn, bn, loss_trace [steps, K], [(wn, bn) after each step])."""
    wn, bn = np.array(wn, np.float64), np.array(bn, np.float64)
    mw, vw, mb, vb = np.zeros_like(wn), np.zeros_like(wn), np.zeros_like(bn), np.zeros_like(bn)
    trace, path = [], []
    for t in range(1, steps + 1):
        loss, gw, gb = enroll_loss_grad(nn, logits1, seq_len, labels, label_len, wn, bn)
        trace.append(loss)
        wn, mw, vw = adam_step(wn, mw, vw, gw, t, lr)
        bn, mb, vb = adam_step(bn, mb, vb, gb, t, lr)
        path.append((wn.copy(), bn.copy()))
    return wn, bn, np.array(trace), path


# ---- the case list both test files share: the smallest shapes at which the kernels can go wrong ---------------------------------

def _words(n, lo, hi):
    """ctc_label form of n words cycling through classes lo..hi: [0, w, 0, w', ..., 0] (2n + 1 entries, no adjacent repeat)."""
    out = [0]
    for i in range(n):
        out += [lo + i % (hi - lo + 1), 0]
    return out


# name -> (H, C, n, T, [(seq_len, label)] per slot); K = number of slots.  Labels index the C + n classes, blank = C + n - 1.
CASES = {
    "t1_empty_label": (64, 6, 2, 1, [(1, [])]),
    "t1_one_label": (64, 6, 2, 1, [(1, [5])]),
    # T == S exactly (one path); [5,5] needs three frames: feasible at 3, infeasible at 2
    "one_path_and_repeats": (128, 6, 1, 5, [(5, [0, 5, 0, 5, 0]), (3, [5, 5]), (2, [5, 5])]),
    # seq_len < T, an empty slot among full ones (its label is ignored), an empty label; three trained classes and five new ones
    "ragged_empty_slot": (256, 3, 5, 33, [(33, [0, 2, 0, 3, 0]), (20, [2, 3, 4, 5, 6]), (0, [1]), (33, [])]),
    # S = 31: all 63 states; the second slot has exactly as many frames as labels
    "s31": (128, 6, 2, 65, [(65, _words(15, 5, 6)), (31, _words(15, 1, 6)), (40, [0, 5, 0, 6, 0])]),
    "repeats_k4": (64, 6, 2, 33, [(33, [5, 5, 6, 6, 5]), (33, [0, 5, 0, 6, 0]), (17, [6, 0, 0, 6]), (9, [1, 2, 3, 3, 5, 6])]),
}


def make_problem(name, seed=0):
    """-> dict(H, C, n, K, T, nn [K,T,H], logits1 [K,T,C], seq_len [K], labels (list), wn [H,n], bn [n]); float32 arrays."""
    h, c, n, t, slots = CASES[name]
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    k = len(slots)
    return dict(name=name, H=h, C=c, n=n, K=k, T=t,
                nn=(0.5 * rng.standard_normal((k, t, h))).astype(np.float32),
                logits1=(2.0 * rng.standard_normal((k, t, c))).astype(np.float32),
                seq_len=np.array([s for s, _ in slots], np.int32), labels=[list(l) for _, l in slots],
                wn=(0.3 * rng.standard_normal((h, n))).astype(np.float32), bn=(0.5 * rng.standard_normal(n)).astype(np.float32))


def padded_labels(labels):
    s_max = max([len(l) for l in labels] + [1])
    out = np.zeros((len(labels), s_max), np.int32)
    for i, l in enumerate(labels):
        out[i, :len(l)] = l
    return out, np.array([len(l) for l in labels], np.int32)


def torch_reference(p, dtype):
    """The same fit step as a torch graph on the CPU in `dtype`: F.ctc_loss(blank = C2 - 1, reduction='none', zero_infinity=True)
    and autograd -> dict(loss [K] (0 where torch zeroes an infinite loss), logits2 [K,T,C2], grad_logits [K,T,C2] of sum(loss),
    gW [H,n], gb [n] of sum(loss) / K).  Empty slots (seq_len 0) are left out of the graph: they add nothing."""
    import torch
    import torch.nn.functional as F
    nn = torch.tensor(p["nn"], dtype=dtype)
    l1 = torch.tensor(p["logits1"], dtype=dtype)
    wn = torch.tensor(p["wn"], dtype=dtype, requires_grad=True)
    bn = torch.tensor(p["bn"], dtype=dtype, requires_grad=True)
    z = torch.cat([l1[..., :-1], nn @ wn + bn, l1[..., -1:]], dim=-1)
    z.retain_grad()
    live = [i for i in range(p["K"]) if p["seq_len"][i] > 0]
    lab, lab_len = padded_labels([p["labels"][i] for i in live])
    lp = F.log_softmax(z[live], dim=-1).transpose(0, 1)
    loss_live = F.ctc_loss(lp, torch.tensor(lab, dtype=torch.long), torch.tensor(p["seq_len"][live], dtype=torch.long),
                           torch.tensor(lab_len, dtype=torch.long), blank=p["C"] + p["n"] - 1, reduction="none", zero_infinity=True)
    (loss_live.sum() / p["K"]).backward()
    loss = np.zeros(p["K"])
    loss[live] = loss_live.detach().numpy()
    return dict(loss=loss, logits2=z.detach().numpy(), grad_logits=z.grad.numpy() * p["K"], gW=wn.grad.numpy(), gb=bn.grad.numpy())


def torch_ctc(logits, seq_len, labels, dtype):
    """F.ctc_loss and autograd on given logits [K,T,C2] (blank = C2 - 1) in `dtype` -> (loss [K], grad_logits [K,T,C2] of sum(loss));
    empty slots left out as in torch_reference."""
    import torch
    import torch.nn.functional as F
    k, c2 = logits.shape[0], logits.shape[2]
    z = torch.tensor(logits, dtype=dtype, requires_grad=True)
    live = [i for i in range(k) if seq_len[i] > 0]
    lab, lab_len = padded_labels([labels[i] for i in live])
    lp = F.log_softmax(z[live], dim=-1).transpose(0, 1)
    loss_live = F.ctc_loss(lp, torch.tensor(lab, dtype=torch.long), torch.tensor(np.asarray(seq_len)[live], dtype=torch.long),
                           torch.tensor(lab_len, dtype=torch.long), blank=c2 - 1, reduction="none", zero_infinity=True)
    loss_live.sum().backward()
    loss = np.zeros(k)
    loss[live] = loss_live.detach().numpy()
    return loss, z.grad.numpy()


def torch_fit_float32(p, steps, lr):
    """The fit as the torch graph in float32 with TensorFlow's Adam in float32 -> (loss_trace [steps, K], [(wn, bn) after each step]):
    the yardstick trajectory (how far float32 arithmetic alone drifts from the fp64 one)."""
    import torch
    q = dict(p)
    f = np.float32
    wn, bn = p["wn"].astype(f), p["bn"].astype(f)
    mw, vw, mb, vb = np.zeros_like(wn), np.zeros_like(wn), np.zeros_like(bn), np.zeros_like(bn)
    trace, path = [], []
    for t in range(1, steps + 1):
        q["wn"], q["bn"] = wn, bn
        r = torch_reference(q, torch.float32)
        trace.append(r["loss"])
        lr_t = f(lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
        mw, vw = f(0.9) * mw + (f(1) - f(0.9)) * r["gW"], f(0.999) * vw + (f(1) - f(0.999)) * r["gW"] * r["gW"]
        mb, vb = f(0.9) * mb + (f(1) - f(0.9)) * r["gb"], f(0.999) * vb + (f(1) - f(0.999)) * r["gb"] * r["gb"]
        wn = wn - lr_t * mw / (np.sqrt(vw) + f(1e-8))
        bn = bn - lr_t * mb / (np.sqrt(vb) + f(1e-8))
        path.append((wn.copy(), bn.copy()))
    return np.array(trace), path
