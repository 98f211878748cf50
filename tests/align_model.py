"""TEST INFRASTRUCTURE ONLY -- CTC forced alignment restated in numpy (fp64 by default, float32 with dtype=np.float32): the semantics
kws_ctc_align is held to (include/kws_amd.h).  The blank is the LAST class; the extended label blank, l_1, blank, ..., l_S, blank has
L = 2S + 1 states.  The best path is the Viterbi recursion over the log-softmax rows -- max where the loss has log-add-exp --, the
posteriors are alpha + beta - lp - log P of the loss.  The float32 run keeps the operation order of csrc/ctc_device.h:
((a (+) a1) (+) a2) + lp with (+) = max (a predecessor replaces the choice only when strictly greater, tried in the order stay, s-1,
s-2) or the guarded log-add-exp.

Pinned by tests/test_align_host.py to brute-force enumeration of all C^T paths and to torch's CTC loss and gradient in fp64."""
import itertools

import numpy as np

NEG = -np.inf


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    z = x - x.max(axis=-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=-1, keepdims=True, dtype=dtype))).astype(dtype)


def extended(label, blank, allow_repeat_skip=False):
    """-> (ext [L], skip [L]): skip[s] -- s-2 -> s is allowed: ext[s] is no blank and differs from ext[s-2].  allow_repeat_skip: the
    negative control (a repeated label is skipped into as any other)."""
    label = np.asarray(label, np.int64).ravel()
    ext = np.full(2 * len(label) + 1, blank, np.int64)
    ext[1::2] = label
    skip = np.zeros(len(ext), bool)
    skip[3::2] = True if allow_repeat_skip else ext[3::2] != ext[1:-2:2]
    return ext, skip


def _shift(a, d, fill):
    """a[s - d] at s (d > 0: from the states below; d < 0: from the states above), `fill` where there is none"""
    out = np.full_like(a, fill)
    if d > 0:
        out[d:] = a[:-d]
    else:
        out[:d] = a[-d:]
    return out


def spans_of(states, n_labels):
    """[S, 2] first and last frame (inclusive) spent in state 2k + 1; -1 where the path never is"""
    out = np.full((n_labels, 2), -1, np.int32)
    for k in range(n_labels):
        at = np.flatnonzero(np.asarray(states) == 2 * k + 1)
        if len(at):
            out[k] = at[0], at[-1]
    return out


def align(logits, seq_len, label, dtype=np.float64, allow_repeat_skip=False):
    """One utterance: logits [T, C], its first seq_len frames (None: all), label over 0..C-2 -> dict(
    score: log-probability of the best path (0 for an empty slot, -inf without a valid path),
    states [T] int32 (-1 past seq_len, and everywhere without a path), spans [S, 2] int32,
    loss: -log P(label) (0 for an empty slot, +inf without a valid path), post [T, S]: occupancy of state 2k + 1 at frame t,
    gap: the smallest margin between the chosen predecessor and the next one along the chosen path, the final choice included;
    occupancy [T, L]: the posterior of every state, blanks included; valid)."""
    logits = np.asarray(logits)
    t_all, c = logits.shape
    n = t_all if seq_len is None else min(max(int(seq_len), 0), t_all)
    label = np.asarray(label, np.int64).ravel()
    n_lab = len(label)
    out = dict(score=dtype(0.0), states=np.full(t_all, -1, np.int32), spans=np.full((n_lab, 2), -1, np.int32), loss=dtype(0.0),
               post=np.zeros((t_all, n_lab), dtype), gap=np.inf, valid=False)
    if n == 0:
        return out
    ninf = dtype(NEG)
    lp = log_softmax(logits[:n].astype(dtype), dtype)
    ext, skip = extended(label, c - 1, allow_repeat_skip)
    ns = len(ext)
    out["occupancy"] = np.zeros((t_all, ns), dtype)
    e = lp[:, ext]                                  # [n, L] the log-probability each state emits
    # ---- Viterbi
    v = np.full(ns, ninf)
    v[:2] = e[0, :2]
    back = np.zeros((n, ns), np.int8)
    margin = np.full((n, ns), np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(1, n):
            v1 = _shift(v, 1, ninf)
            v2 = np.where(skip, _shift(v, 2, ninf), ninf)
            m, src = v.copy(), np.zeros(ns, np.int8)
            take = v1 > m
            m, src = np.where(take, v1, m), np.where(take, 1, src).astype(np.int8)
            take = v2 > m
            m, src = np.where(take, v2, m), np.where(take, 2, src).astype(np.int8)
            cand = np.sort(np.stack([v, v1, v2]).astype(np.float64), axis=0)
            margin[t] = np.where(cand[1] > NEG, cand[2] - cand[1], np.inf)
            back[t] = src
            v = (m + e[t]).astype(dtype)
    end1, end2 = v[ns - 1], (v[ns - 2] if ns > 1 else ninf)
    last = ns - 2 if end2 > end1 else ns - 1
    score = end2 if end2 > end1 else end1
    out["score"] = dtype(score)
    # ---- loss: the alpha pass
    a = np.full(ns, ninf)
    a[:2] = e[0, :2]
    alpha = np.full((n, ns), ninf)
    alpha[0] = a
    for t in range(1, n):
        a1 = _shift(a, 1, ninf)
        a2 = np.where(skip, _shift(a, 2, ninf), ninf)
        a = (np.logaddexp(np.logaddexp(a, a1), a2) + e[t]).astype(dtype)
        alpha[t] = a
    log_p = np.logaddexp(a[ns - 1], a[ns - 2] if ns > 1 else ninf)
    out["loss"] = dtype(-log_p)
    if score == NEG:
        return out
    out["valid"] = True
    lo, hi = float(min(end1, end2)), float(max(end1, end2))
    gap = hi - lo if lo > NEG else np.inf
    s, states = last, np.zeros(n, np.int32)
    for t in range(n - 1, -1, -1):
        states[t] = s
        if t > 0:
            gap = min(gap, float(margin[t, s]))
            s -= int(back[t, s])
    out["gap"] = gap
    out["states"][:n] = states
    out["spans"] = spans_of(out["states"], n_lab)
    # ---- posteriors: the beta pass
    if log_p > NEG:
        nll = dtype(-log_p)
        skip_out = _shift(skip, -2, False)
        b = np.full(ns, ninf)
        b[max(ns - 2, 0):] = e[n - 1, max(ns - 2, 0):]
        for t in range(n - 1, -1, -1):
            if t < n - 1:
                b1 = _shift(b, -1, ninf)
                b2 = np.where(skip_out, _shift(b, -2, ninf), ninf)
                b = (np.logaddexp(np.logaddexp(b, b1), b2) + e[t]).astype(dtype)
            ab = (alpha[t] + b).astype(dtype)
            with np.errstate(invalid="ignore"):
                occ = np.where(ab > NEG, np.minimum(np.exp(((ab - e[t]).astype(dtype) + nll).astype(dtype)), dtype(1.0)), dtype(0.0))
            out["post"][t] = occ[1::2]
            out["occupancy"][t] = occ
    return out


def frame_classes(states, label, blank):
    """class per frame of a state row: odd states their label, even states the blank, -1 stays"""
    states = np.asarray(states)
    lab = np.concatenate([np.asarray(label, np.int64).ravel(), [blank]])
    return np.where(states < 0, -1, np.where(states % 2 == 1, lab[np.clip(states, 0, None) // 2 % len(lab)], blank)).astype(np.int32)


def collapse(path, blank):
    out, prev = [], blank
    for c in path:
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return tuple(out)


def path_states(path, blank):
    """the state of the extended label (of collapse(path)) at every frame of a class path"""
    out, prev, k = [], blank, 0          # k: labels begun so far
    for c in path:
        if c != blank and c != prev:
            k += 1
        out.append(2 * k if c == blank else 2 * k - 1)
        prev = c
    return out


def brute_force(logits, label):
    """all C^T class paths that collapse to `label` -> (best score, its states, occupancy [T, L] (posterior of each state), log P);
    (-inf, None, None, -inf) when there is none"""
    lp = log_softmax(logits, np.float64)
    t_all, c = lp.shape
    label = tuple(int(v) for v in label)
    ns = 2 * len(label) + 1
    best, best_states, scores, rows = NEG, None, [], []
    for path in itertools.product(range(c), repeat=t_all):
        if collapse(path, c - 1) != label:
            continue
        s = float(lp[np.arange(t_all), list(path)].sum())
        st = path_states(path, c - 1)
        scores.append(s)
        rows.append(st)
        if s > best:
            best, best_states = s, st
    if not scores:
        return NEG, None, None, NEG
    scores = np.array(scores)
    log_p = float(np.logaddexp.reduce(scores))
    w = np.exp(scores - log_p)
    occ = np.zeros((t_all, ns))
    for wi, st in zip(w, rows):
        occ[np.arange(t_all), st] += wi
    return best, np.array(best_states, np.int32), occ, log_p


def brute_force_scores(logits, label):
    """the log-probability of every class path that collapses to `label`"""
    lp = log_softmax(logits, np.float64)
    t_all, c = lp.shape
    label = tuple(int(v) for v in label)
    return [float(lp[np.arange(t_all), list(path)].sum()) for path in itertools.product(range(c), repeat=t_all)
            if collapse(path, c - 1) == label]


def make_logits(seed, t, c, peak=4.0):
    """the inputs of tests/test_gpu_align.py: N(0,1) plus `peak` on one random class per frame (beam_model.make_logits' form)"""
    rng = np.random.default_rng([seed, t, c, 77])
    x = rng.standard_normal((t, c))
    x[np.arange(t), rng.integers(0, c, t)] += peak
    return x.astype(np.float32)


def make_label(seed, t, c, s):
    """a random label of s entries over 0..c-2; with c = 3 every second pair repeats"""
    rng = np.random.default_rng([seed, t, c, s, 78])
    return [int(v) for v in rng.integers(0, c - 1, s)]
