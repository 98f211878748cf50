"""TEST INFRASTRUCTURE ONLY -- the two-head streaming policy (a stream manager on a customised-keyword model) stated twice, without
the device:

  * CoupledWindows / CoupledRescan: the fp-free window part on per-frame WORD traces.  Two tests/window_model.IncrementalWindow
    plus the cross-clear (what heads_window_kernel does) against two oracle SimpleQueues re-scanned with ctc_decode2 / ctc_predict
    plus the cross-clear (what the reference would do: detector.py:195-209 per head, README "decode respectively",
    server_demo.py:122-129's OR).
  * policy_loop: the whole loop in fp64 -- tests/heads_model.heads_forward for the stack and both heads, the oracle's queue and
    decoders per head, the coupled clear and restart -- with, per (chunk, stream), the decision margins and whether the coupling
    was OBSERVABLE there (head 1 alone would have fired had a head-2 hit not cleared its window).
Not imported by the product.
"""
import numpy as np

import heads_model as HM
from oracle import decode_oracle as D
from window_model import IncrementalWindow


class CoupledWindows(object):
    """Two incremental windows and the coupling of heads_window_kernel: a hit of either empties both."""

    def __init__(self, max_chunks, label1, label2, cross_clear=True):
        self.w = [IncrementalWindow(max_chunks, [int(c) for c in label1]), IncrementalWindow(max_chunks, [int(c) for c in label2])]
        self.cross_clear = cross_clear

    def step(self, words1, words2, clear_before=False):
        h1, h2 = self.w[0].step(words1, clear_before), self.w[1].step(words2, clear_before)
        if (h1 or h2) and self.cross_clear:
            self.w[0].ring, self.w[1].ring = [], []
        return h1 | (h2 << 1)


def rows_for(words, classes):
    """Softmax-like rows that decode to `words` (-1: the blank class wins)."""
    r = np.full((len(words), classes), 0.02, np.float32)
    for i, w in enumerate(words):
        r[i, classes - 1 if w < 0 else w + 1] = 0.9
    return r


class CoupledRescan(object):
    """The reference's re-scan per head with the oracle's pinned functions, and the coupled clear."""

    def __init__(self, max_chunks, label1, label2, classes=(6, 8)):
        self.q = [D.SimpleQueue(max_chunks), D.SimpleQueue(max_chunks)]
        self.labels, self.classes = (label1, label2), classes

    def step(self, words1, words2, clear_before=False):
        mask = 0
        for k, words in enumerate((words1, words2)):
            if clear_before:
                self.q[k].clear()
            self.q[k].add(rows_for(words, self.classes[k]))
            window = np.concatenate(self.q[k].get_all(), 0)
            mask |= int(bool(D.ctc_predict(D.ctc_decode2(window, self.classes[k]), self.labels[k]))) << k
        if mask:
            self.q[0].clear()
            self.q[1].clear()
        return mask


def _margin_ok(sm, classes, thres, eps=1e-4):
    """tests/test_gpu_detector.py's rule on the rows of one chunk: no frame's largest word class within eps of the threshold or of
    the runner-up (a head with one word class has no runner-up)."""
    if sm.shape[0] == 0:
        return True
    p = np.sort(sm[:, 1:classes - 1], axis=1)
    ok = (np.abs(p[:, -1] - thres) > eps).all()
    if p.shape[1] > 1:
        ok = ok and (p[:, -1] - p[:, -2] > eps).all()
    return bool(ok)


def policy_loop(w, mel, chunks, speech, labels, thres, window_chunks=15):
    """The two-head loop in fp64 for mel [B, sum(chunks), n_mel]; speech [len(chunks), B] bool (False: a silent chunk).
    -> dict(mask [chunks, B] hit_1 | hit_2 << 1, margin_ok [chunks, B], observable [chunks, B]: head 1 did not fire here but
    would have, had an earlier head-2-only hit left its window alone)."""
    b = mel.shape[0]
    c = (w["Wfc"].shape[1], w["Wfc2"].shape[1])
    nl, hdim = len(w["layers"]), w["Wfc"].shape[0]
    state = np.zeros((nl, b, hdim), np.float64)
    queues = [[D.SimpleQueue(window_chunks) for _ in range(b)] for _ in range(2)]
    shadow = [None] * b                     # head 1's window as it would be without the cross-clear, while that differs
    mask = np.zeros((len(chunks), b), np.int32)
    margin = np.ones((len(chunks), b), bool)
    observable = np.zeros((len(chunks), b), bool)
    restart = np.zeros(b, bool)
    pos = 0
    for ci, n in enumerate(chunks):
        silent = ~np.asarray(speech[ci], bool)
        state[:, silent | restart] = 0
        restart[:] = False
        for s in np.nonzero(silent)[0]:
            queues[0][s].clear()
            queues[1][s].clear()
            shadow[s] = None
        r = HM.heads_forward(w, mel[:, pos:pos + n], state)
        state = r["state"]
        for s in range(b):
            hit = [0, 0]
            for k in range(2):
                sm = r["softmax%d" % (k + 1)][s]
                margin[ci, s] &= _margin_ok(sm, c[k], thres[k])
                queues[k][s].add(sm)
                hit[k] = int(bool(D.ctc_predict(D.ctc_decode2(np.concatenate(queues[k][s].get_all(), 0), c[k], thres[k]), labels[k])))
            if shadow[s] is not None:
                shadow[s].add(r["softmax1"][s])
                would = bool(D.ctc_predict(D.ctc_decode2(np.concatenate(shadow[s].get_all(), 0), c[0], thres[0]), labels[0]))
                if would and not hit[0]:
                    observable[ci, s] = True
                    shadow[s] = None
            mask[ci, s] = hit[0] | (hit[1] << 1)
            if mask[ci, s]:
                if mask[ci, s] == 2 and shadow[s] is None:       # head 2 alone: remember what head 1's window held
                    shadow[s] = D.SimpleQueue(window_chunks)
                    for chunk in queues[0][s].get_all():
                        shadow[s].add(chunk)
                elif mask[ci, s] != 2:
                    shadow[s] = None
                queues[0][s].clear()
                queues[1][s].clear()
                restart[s] = True
        pos += n
    return dict(mask=mask, margin_ok=margin, observable=observable)
