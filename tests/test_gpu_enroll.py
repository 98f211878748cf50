"""Customised-keyword enrolment on the device: kws_ctc_loss and kws_enroll_fit against torch's CTC loss in fp64 on the SAME float32
arrays, with the deviation of the identical torch graph in float32 (CPU) as the yardstick -- bound = 4 x that deviation (the factor
tests/test_gpu_mfcc.py uses for the same kind of comparison), floored at 16 * 2^-23 * max|reference| where float32 torch happens to
be exact.  Then the fit: trajectory against the fp64 restatement (tests/enroll_model.py), bit-exactness across call splits and
batch composition, the end-to-end README flow, the refusals that need a device."""
import ctypes

import numpy as np
import pytest
import torch

import enroll_model as M

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -23


def _bound(ref64, ref32):
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    return max(4.0 * dev, FLOOR * (float(np.abs(ref64).max()) if np.size(ref64) else 0.0)), dev


def _report(what, name, got, ref64, ref32):
    bound, dev = _bound(ref64, ref32)
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    ratio = err / bound if bound > 0 else 0.0
    print("ENROLL-RATIO %s %s: kernel %.3e  float32-CPU %.3e  bound %.3e  kernel/bound %.3f" % (what, name, err, dev, bound, ratio))
    return err, bound


class Handle(object):
    """kws_enroll_* on E problems of one shape (tests/enroll_model.make_problem)."""

    def __init__(self, problems):
        from keyword_spotting_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        p = problems[0]
        self.E, self.K, self.H, self.C, self.n, self.T = len(problems), p["K"], p["H"], p["C"], p["n"], p["T"]
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.kws_enroll_create(self.H, self.C, self.n, self.E, self.K, ctypes.byref(self.h)))
        dev = lambda key: torch.from_numpy(np.concatenate([q[key] for q in problems])).cuda().contiguous()   # noqa: E731
        self.nn, self.logits1 = dev("nn"), dev("logits1")
        self.labels, self.label_len = M.padded_labels([l for q in problems for l in q["labels"]])
        self.seq_len = np.concatenate([q["seq_len"] for q in problems]).astype(np.int32)
        self.wn = torch.from_numpy(np.stack([q["wn"] for q in problems])).cuda()
        self.bn = torch.from_numpy(np.stack([q["bn"] for q in problems])).cuda()
        self.set()

    def set(self):
        self._lib.check(self.lib.kws_enroll_set(self.h, self._lib.ptr(self.wn), self._lib.ptr(self.bn), None))

    def fit(self, iterations, lr, trace=True, seq_len=None, labels=None, s_max=None):
        b = self.E * self.K
        out = torch.full((iterations, b), -1.0, device="cuda") if trace else None
        sl = np.ascontiguousarray(self.seq_len if seq_len is None else seq_len, np.int32)
        lab = np.ascontiguousarray(self.labels if labels is None else labels, np.int32)
        rc = self.lib.kws_enroll_fit(self.h, self._lib.ptr(self.nn), self._lib.ptr(self.logits1), sl.ctypes.data_as(ctypes.c_void_p),
                                     lab.ctypes.data_as(ctypes.c_void_p), self.label_len.ctypes.data_as(ctypes.c_void_p), self.T,
                                     int(lab.shape[1]) if s_max is None else s_max, lr, iterations, self._lib.ptr(out), None)
        self._lib.check(rc)
        torch.cuda.synchronize()
        return None if out is None else out.cpu().numpy()

    def get(self):
        w, b = torch.empty_like(self.wn), torch.empty_like(self.bn)
        self._lib.check(self.lib.kws_enroll_get(self.h, self._lib.ptr(w), self._lib.ptr(b), None))
        torch.cuda.synchronize()
        return w.cpu().numpy(), b.cpu().numpy()

    def moments(self):
        nm = self.E * (self.H + 1) * self.n
        m, v = torch.empty(nm, device="cuda"), torch.empty(nm, device="cuda")
        self._lib.check(self.lib.kws_enroll_moments(self.h, self._lib.ptr(m), self._lib.ptr(v), None))
        torch.cuda.synchronize()
        nw = self.E * self.H * self.n
        m = m.cpu().numpy()
        return m[:nw].reshape(self.E, self.H, self.n), m[nw:].reshape(self.E, self.n)

    def stats(self):
        nbytes, allocs, steps = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
        self._lib.check(self.lib.kws_enroll_stats(self.h, ctypes.byref(nbytes), ctypes.byref(allocs), ctypes.byref(steps)))
        return nbytes.value, allocs.value, steps.value

    def close(self):
        self.lib.kws_enroll_destroy(self.h)
        self.h = ctypes.c_void_p()


def test_new_entry_points_exist():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_ctc_loss", "kws_enroll_create", "kws_enroll_destroy", "kws_enroll_set", "kws_enroll_fit", "kws_enroll_get"):
        assert hasattr(lib, sym), sym


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_ctc_loss_and_gradient_against_torch_fp64(name):
    from keyword_spotting_amd.custom_keyword import ctc_loss
    p = M.make_problem(name)
    logits2 = M.torch_reference(p, torch.float32)["logits2"].astype(np.float32)         # ONE float32 array for all three
    loss64, grad64 = M.torch_ctc(logits2, p["seq_len"], p["labels"], torch.float64)
    loss32, grad32 = M.torch_ctc(logits2, p["seq_len"], p["labels"], torch.float32)
    want_inf = np.array([M.ctc_loss_grad(logits2[i], p["seq_len"][i], p["labels"][i])[0] == np.inf for i in range(p["K"])])
    loss, grad = ctc_loss(torch.from_numpy(logits2), p["seq_len"], p["labels"])
    loss_only, none = ctc_loss(torch.from_numpy(logits2), p["seq_len"], p["labels"], want_grad=False)
    torch.cuda.synchronize()
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    assert none is None and np.array_equal(loss_only.cpu().numpy(), loss)
    assert np.array_equal(np.isinf(loss), want_inf) and (loss[want_inf] > 0).all()       # no path: +inf (torch: zeroed) ...
    assert not grad[want_inf].any()                                                     # ... and a gradient of exactly 0
    for i in range(p["K"]):
        assert not grad[i, p["seq_len"][i]:].any()                                      # zeros past seq_len, empty slots included
    assert (loss[p["seq_len"] == 0] == 0).all()
    err, bound = _report("ctc_loss loss", name, np.where(want_inf, 0.0, loss), loss64, loss32)
    assert err <= bound
    err, bound = _report("ctc_loss grad", name, grad, grad64, grad32)
    assert err <= bound


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_one_fit_iteration_implies_the_gradient(name):
    """m after the first Adam step from zero moments is (1 - 0.9f) g: the gradient the kernel computed, to one rounding."""
    p = M.make_problem(name)
    ref64, ref32 = M.torch_reference(p, torch.float64), M.torch_reference(p, torch.float32)
    h = Handle([p])
    try:
        trace = h.fit(1, 0.01)
        mw, mb = h.moments()
    finally:
        h.close()
    scale = np.float32(1.0) - np.float32(0.9)
    gw, gb = mw[0] / scale, mb[0] / scale
    inf = np.isinf(trace[0])
    err, bound = _report("fit loss", name, np.where(inf, 0.0, trace[0]), ref64["loss"], ref32["loss"])
    assert err <= bound
    err, bound = _report("fit gW", name, gw, ref64["gW"], ref32["gW"])
    assert err <= bound
    err, bound = _report("fit gb", name, gb, ref64["gb"], ref32["gb"])
    assert err <= bound


@pytest.mark.parametrize("name", ["repeats_k4", "s31", "ragged_empty_slot"])
def test_twenty_step_fit_follows_the_restatement(name):
    """loss_trace and (Wn, bn) after every step against the fp64 restatement.  The yardstick at step s is the largest deviation
    the float32 torch trajectory has shown from the fp64 one up to s (rounding differences accumulate along a trajectory, they
    do not shrink); bound_s = max(4 x that, s x floor)."""
    steps, lr = 20, 0.01
    p = M.make_problem(name)
    _, lab_len = M.padded_labels(p["labels"])
    _, _, trace64, path64 = M.fit(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, p["wn"], p["bn"], steps, lr)
    trace32, path32 = M.torch_fit_float32(p, steps, lr)
    h = Handle([p])
    try:
        got_trace, got_path = [], []
        for _ in range(steps):
            got_trace.append(h.fit(1, lr)[0])
            got_path.append(h.get())
    finally:
        h.close()
    fin = np.isfinite(trace64[0])
    dev_l = dev_w = worst = 0.0
    for s in range(steps):
        assert np.array_equal(np.isfinite(got_trace[s]), fin)
        ref_w = np.concatenate([path64[s][0].ravel(), path64[s][1].ravel()])
        dev_l = max(dev_l, float(np.abs(trace32[s][fin] - trace64[s][fin]).max()))
        dev_w = max(dev_w, float(np.abs(np.concatenate([path32[s][0].ravel(), path32[s][1].ravel()]) - ref_w).max()))
        b_l = max(4 * dev_l, (s + 1) * FLOOR * float(np.abs(trace64[s][fin]).max()))
        b_w = max(4 * dev_w, (s + 1) * FLOOR * float(np.abs(ref_w).max()))
        e_l = float(np.abs(got_trace[s][fin] - trace64[s][fin]).max())
        e_w = float(np.abs(np.concatenate([got_path[s][0].ravel(), got_path[s][1].ravel()]) - ref_w).max())
        worst = max(worst, e_l / b_l, e_w / b_w)
        assert e_l <= b_l and e_w <= b_w, (s, e_l, b_l, e_w, b_w)
    print("ENROLL-RATIO fit20 %s: worst kernel/bound %.3f (float32-CPU drift: loss %.3e, parameters %.3e)" % (name, worst, dev_l, dev_w))


def test_split_calls_and_batch_composition_leave_the_bits_alone():
    steps, lr = 20, 0.01
    problems = [M.make_problem("repeats_k4", seed) for seed in range(5)]
    h = Handle(problems)
    try:
        trace_once = h.fit(steps, lr)
        once = h.get()
        assert h.stats()[1:] == (1, steps)
        h.set()                                  # ... zeroes the moments and the step count
        assert h.stats()[2] == 0
        trace_split = np.concatenate([h.fit(1, lr) for _ in range(steps)])
        split = h.get()
        assert h.stats()[1:] == (1, steps)       # nothing allocated after the first call at this shape
        # one slot of enrolment 2 emptied: nothing changes for the other enrolments
        h.set()
        seq = h.seq_len.copy()
        seq[2 * h.K + 1] = 0
        trace_gap = h.fit(steps, lr, seq_len=seq)
        gap = h.get()
    finally:
        h.close()
    assert np.array_equal(trace_once, trace_split) and all(np.array_equal(a, b) for a, b in zip(once, split))
    others = [0, 1, 3, 4]
    assert all(np.array_equal(a[others], b[others]) for a, b in zip(once, gap))
    assert not np.array_equal(once[0][2], gap[0][2]) and (trace_gap[:, 2 * 4 + 1] == 0).all()
    for e in (0, 3):                             # an enrolment alone: the bits it has inside E = 5
        one = Handle([problems[e]])
        try:
            trace = one.fit(steps, lr)
            w, b = one.get()
        finally:
            one.close()
        assert np.array_equal(w[0], once[0][e]) and np.array_equal(b[0], once[1][e])
        assert np.array_equal(trace, trace_once[:, e * 4:e * 4 + 4])


@pytest.mark.parametrize("seed", [0, 2])
def test_enrolled_keyword_is_decoded_on_its_training_utterances(seed):
    """The README flow: enroll() on three utterances (300 steps, lr 0.03), the result served through kws_create_heads; ctc_decode2
    of softmax2 emits the two new words in label order on every training utterance (seeds on which the fp64 restatement does)."""
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.custom_keyword import enroll
    from keyword_spotting_amd.prediction import ctc_decode2, ctc_label
    from keyword_spotting_amd.rnn_ctc import FEED_INPUT, FEED_STATE, FETCH_SOFTMAX2, DeployModel
    from oracle import gru_oracle as G
    cfg = get_config()
    model = DeployModel(cfg, weights.init_weights(cfg, seed=seed))
    mel = G.synthetic_mel(3, 48, cfg.n_mel, seed=seed + 10)
    w2 = enroll(model, [mel[i] for i in range(3)], ctc_label([5, 6]), n_new=2, steps=300, lr=0.03, seed=seed)
    assert w2["Wfc2"].shape == (cfg.hidden_size, 8) and np.array_equal(w2["Wfc2"][:, :5], w2["Wfc"][:, :5])
    assert np.array_equal(w2["Wfc2"][:, 7], w2["Wfc"][:, 5])
    cfg2 = get_config()
    cfg2.num_classes2 = 8
    served = DeployModel(cfg2, w2)
    for i in range(3):
        sm2 = served.run(FETCH_SOFTMAX2, {FEED_INPUT: torch.from_numpy(mel[i]), FEED_STATE: served.zero_state(1)})
        words = [int(w) for w in ctc_decode2(sm2, 8)[1::2]]
        assert 5 in words and 6 in words[words.index(5) + 1:], (i, words)
    served.close()
    model.close()


def test_refusals_behind_the_device_check():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.custom_keyword import ctc_loss
    lib = _lib.load()
    with pytest.raises(_lib.UnsupportedError, match=r"198800 bytes exceed the 163840"):
        ctc_loss(torch.zeros(1, 700, 6), [700], [list(range(5)) * 6 + [0]])             # 700 x (8 + 63) floats
    p = M.make_problem("repeats_k4")
    h = Handle([p])
    try:
        h.T, keep = 300, h.T                                                            # 4 x 300 x 71 floats; refused before anything is read
        try:
            with pytest.raises(_lib.UnsupportedError, match=r"LDS: \d+ bytes exceed the 163840"):
                h.fit(1, 0.01, s_max=31, labels=np.zeros((4, 31), np.int32))
        finally:
            h.T = keep
        blank = h.labels.copy()
        blank[1, 0] = 7
        with pytest.raises(_lib.InvalidArgumentError, match=r"labels\[1\]\[0\]=7"):
            h.fit(1, 0.01, labels=blank)
        with pytest.raises(_lib.InvalidArgumentError, match="iterations"):
            h.fit(0, 0.01, trace=False)
        with pytest.raises(_lib.InvalidArgumentError, match="lr="):
            h.fit(1, 0.0)
        with pytest.raises(_lib.InvalidArgumentError, match="S_max=32"):
            h.fit(1, 0.01, s_max=32)
        assert h.stats()[1:] == (0, 0)                                                  # nothing ran, nothing was allocated
        assert lib.kws_enroll_set(h.h, None, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    finally:
        h.close()
