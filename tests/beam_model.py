"""CTC prefix beam search restated in numpy (fp64 by default, float32 with dtype=np.float32): the semantics kws_ctc_beam_search is
held to (include/kws_amd.h).  The exact-candidate form: every stay and every extension of every beam entry is a candidate, candidates
with the same prefix merge by CONTENT whichever way they arose, the W best by lp_b (+) lp_nb survive.  The blank is the last class.

Pinned by tests/test_beam_host.py to brute-force enumeration of all C^T paths and to torch's CTC loss in fp64 -- not to TensorFlow,
whose decoder prunes further once the beam is full; with W >= the number of labellings the two coincide by construction."""
import itertools

import numpy as np


def log_softmax(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    z = x - x.max(axis=-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=-1, keepdims=True, dtype=dtype))).astype(dtype)


def _lae(a, b):
    """the guarded logaddexp of ctc_device.h, in the operands' dtype"""
    m = a if a > b else b
    if m == -np.inf:
        return m
    return m + np.log1p(np.exp(-abs(a - b)))


def beam_search(logits, seq_len=None, beam_width=None, top_paths=1, l_max=64, merge_repeated=True, dtype=np.float64,
                repeat_from_total=False):
    """logits [T,C] -> dict(paths: list of K tuples, scores: [K] (-inf past the prefixes that exist), gap: the smallest selection gap
    met (W-th kept against best dropped over all frames; neighbouring output ranks up to K + 1), reentries: how often a prefix came
    back into the beam as a new extension of its parent while one of its own extensions was resident, rejoined: how often that
    extension was kept beside it -- from the next frame on the two must merge by content --, raw: the paths before merge_repeated).
    repeat_from_total: the negative control (the extension by c == last(p) takes the total instead of lp_b)."""
    logits = np.asarray(logits)
    t_all, c_all = logits.shape
    blank = c_all - 1
    w = blank if beam_width is None else int(beam_width)
    n_frames = t_all if seq_len is None else min(max(int(seq_len), 0), t_all)
    lp = log_softmax(logits[:n_frames].astype(dtype), dtype) if n_frames else np.zeros((0, c_all), dtype)
    ninf = dtype(-np.inf)
    beam = [((), dtype(0.0), ninf)]
    gap, reentries, rejoined = np.inf, 0, 0
    for t in range(n_frames):
        row = lp[t]
        cand = {}              # prefix -> [lp_b', lp_nb'], insertion-ordered: the candidate index of the tie rule
        for p, b, nb in beam:
            tot = _lae(b, nb)
            e = cand.setdefault(p, [ninf, ninf])
            e[0] = _lae(e[0], tot + row[blank])
            if p:
                e[1] = _lae(e[1], nb + row[p[-1]])
            if len(p) >= l_max:
                continue
            for c in range(blank):
                src = b if (p and c == p[-1] and not repeat_from_total) else tot
                if src == -np.inf:
                    continue
                e = cand.setdefault(p + (c,), [ninf, ninf])
                e[1] = _lae(e[1], row[c] + src)
        order = sorted(((-_lae(v[0], v[1]), i, p) for i, (p, v) in enumerate(cand.items())))
        if len(order) > w:
            gap = min(gap, float(order[w][0]) - float(order[w - 1][0]))
        before = set(p for p, _, _ in beam)
        kept = [p for _, _, p in order[:w]]
        reentries += len(set(kept) - before & set(r[:-1] for r in before if r))
        rejoined += len(set(kept) - before & set(r[:-1] for r in kept if r and r in before))
        beam = [(p, cand[p][0], cand[p][1]) for p in kept]
    final = sorted(((-_lae(b, nb), i, p) for i, (p, b, nb) in enumerate(beam)))
    for a, nxt in zip(final[:top_paths], final[1:top_paths + 1]):
        gap = min(gap, float(nxt[0]) - float(a[0]))
    raw = [p for _, _, p in final[:top_paths]]
    scores = np.full(top_paths, -np.inf, dtype)
    scores[:len(raw)] = [-s for s, _, _ in final[:top_paths]]
    paths = [tuple(c for i, c in enumerate(p) if not (merge_repeated and i and c == p[i - 1])) for p in raw]
    pad = top_paths - len(raw)
    return {"paths": paths + [()] * pad, "raw": raw + [()] * pad, "scores": scores, "gap": gap, "reentries": reentries,
            "rejoined": rejoined}


def dense(paths, l_max):
    """the K paths as the device writes them: [K, l_max] int32 padded with -1, and the lengths"""
    out = np.full((len(paths), l_max), -1, np.int32)
    for k, p in enumerate(paths):
        out[k, :len(p)] = p
    return out, np.array([len(p) for p in paths], np.int32)


def collapse(path, blank):
    out, prev = [], blank
    for c in path:
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return tuple(out)


def brute_force(logits):
    """every labelling's exact log-probability: all C^T paths, collapsed and summed (fp64) -> {labelling: log P}"""
    lp = log_softmax(logits, np.float64)
    t_all, c_all = lp.shape
    acc = {}
    for path in itertools.product(range(c_all), repeat=t_all):
        acc.setdefault(collapse(path, c_all - 1), []).append(lp[np.arange(t_all), list(path)].sum())
    return {k: float(np.logaddexp.reduce(np.array(v))) for k, v in acc.items()}


def torch_log_prob(logits, labelling, seq_len=None):
    """log P(labelling | logits) = -torch.nn.functional.ctc_loss in fp64, blank = C - 1"""
    import torch
    x = torch.as_tensor(np.asarray(logits, np.float64))
    n = x.shape[0] if seq_len is None else int(seq_len)
    if n == 0:
        return 0.0 if len(labelling) == 0 else -np.inf
    lp = torch.log_softmax(x[:n], -1).unsqueeze(1)
    tgt = torch.tensor([list(labelling)], dtype=torch.long).reshape(1, len(labelling))
    loss = torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([n]), torch.tensor([len(labelling)]), blank=x.shape[1] - 1, reduction="none",
                                        zero_infinity=False)
    return -float(loss[0])


REJOIN_SEEDS = (10, 15, 21, 22, 27, 41)          # make_logits(seed, 24, 3, 3, peak=1.0) on which `rejoined` > 0


def make_logits(seed, t, c, w, peak=4.0):
    """the inputs of tests/test_gpu_beam.py: N(0,1) plus `peak` on one random class per frame.  A low peak keeps the beam contested:
    at 1.0 prefixes come back beside their surviving extensions (`rejoined`), which the peaked inputs never show."""
    rng = np.random.default_rng([seed, t, c, w] if peak == 4.0 else [seed, t, c, w, int(peak)])
    x = rng.standard_normal((t, c))
    x[np.arange(t), rng.integers(0, c, t)] += peak
    return x.astype(np.float32)
