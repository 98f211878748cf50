"""CPU checks of the CTC forced alignment: the restatement tests/align_model.py against brute-force enumeration of all C^T paths
(best score, best path, per-state occupancy) and against torch's CTC loss and gradient in fp64, the greedy identity, the negative
control on repeated labels, every refusal kws_ctc_align raises before it touches a device, and the host side of the Python wrappers."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import align_model as M
from conftest import have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (T, C, label): every label length a short utterance takes, repeats included
SMALL = [(1, 3, []), (1, 3, [1]), (2, 3, [0]), (3, 3, [0, 0]), (4, 3, [0, 1]), (5, 3, [1, 1]), (6, 3, [0, 0, 1]), (7, 3, [0, 1, 1]), (7, 3, [1, 1, 1]),
         (5, 4, [2, 0]), (6, 4, [1, 1, 2]), (7, 4, [0, 2, 2])]


@pytest.mark.parametrize("t,c,label", SMALL, ids=lambda v: str(v).replace(" ", ""))
def test_restatement_is_brute_force(t, c, label):
    for seed in range(3):
        x = M.make_logits(seed, t, c, peak=2.0)
        best, states, occ, log_p = M.brute_force(x, label)
        r = M.align(x, t, label)
        assert r["valid"] and abs(float(r["score"]) - best) <= 1e-10
        assert np.array_equal(r["states"], states)
        assert abs(float(r["loss"]) + log_p) <= 1e-10
        assert np.abs(r["occupancy"] - occ).max() <= 1e-10
        assert np.array_equal(r["post"], r["occupancy"][:, 1::2])
        assert np.abs(r["occupancy"].sum(axis=1) - 1.0).max() <= 1e-10            # a frame is in exactly one state
        assert np.array_equal(r["spans"], M.spans_of(states, len(label)))
        # the gap is best - second-best path score
        scores = sorted(M.brute_force_scores(x, label), reverse=True)
        if len(scores) > 1:
            assert abs(r["gap"] - (scores[0] - scores[1])) <= 1e-10
        else:
            assert r["gap"] == np.inf


def test_no_path_and_empty_slot():
    x = M.make_logits(0, 2, 3)
    r = M.align(x, 2, [1, 1])                           # a repeat needs a blank between: three frames
    assert not r["valid"] and r["score"] == -np.inf and r["loss"] == np.inf
    assert (r["states"] == -1).all() and (r["spans"] == -1).all() and not r["post"].any()
    assert M.brute_force(x, [1, 1])[0] == -np.inf
    r = M.align(x, 0, [1])
    assert r["score"] == 0 and r["loss"] == 0 and (r["states"] == -1).all() and (r["spans"] == -1).all() and not r["post"].any()
    r = M.align(M.make_logits(0, 6, 3), 4, [0])         # seq_len < T: -1 and zeros past it, the first frames as the short utterance's
    s = M.align(M.make_logits(0, 6, 3)[:4], 4, [0])
    assert (r["states"][4:] == -1).all() and not r["post"][4:].any() and np.array_equal(r["states"][:4], s["states"]) and r["score"] == s["score"]


@pytest.mark.parametrize("t,c,s", [(5, 4, 2), (9, 6, 4), (40, 6, 4), (63, 8, 31), (64, 3, 8)])
def test_loss_and_posteriors_are_torchs(t, c, s):
    import torch
    import torch.nn.functional as F
    for seed in range(3):
        x, label = M.make_logits(seed, t, c), M.make_label(seed, t, c, s)
        r = M.align(x, t, label)
        z = torch.tensor(x.astype(np.float64), requires_grad=True)
        loss = F.ctc_loss(F.log_softmax(z, -1).unsqueeze(1), torch.tensor([label], dtype=torch.long).reshape(1, s), torch.tensor([t]),
                          torch.tensor([s]), blank=c - 1, reduction="none")[0]
        loss.backward()
        assert r["valid"] and abs(float(r["loss"]) - float(loss.detach())) <= 1e-10
        want = torch.softmax(z.detach(), -1).numpy() - z.grad.numpy()           # per class: the occupancy of the states that emit it
        got = np.zeros((t, c))
        for k, l in enumerate(label):
            got[:, l] += r["post"][:, k]
        assert np.abs(got[:, :c - 1] - want[:, :c - 1]).max() <= 1e-10
        assert np.abs((1.0 - r["post"].sum(axis=1)) - want[:, c - 1]).max() <= 1e-10      # the blank states: what the labels leave
        assert r["post"].min() >= 0 and r["post"].max() <= 1


@pytest.mark.parametrize("t,c", [(1, 3), (7, 3), (40, 6), (150, 8)])
def test_greedy_identity(t, c):
    """on rows with a unique argmax, aligning the collapsed argmax labelling returns the argmax path, score = sum of the row maxima"""
    for seed in range(3):
        x = M.make_logits(seed, t, c)
        lp = M.log_softmax(x)
        assert (np.sort(lp, axis=1)[:, -1] > np.sort(lp, axis=1)[:, -2]).all()
        path = lp.argmax(axis=1)
        label = M.collapse(path, c - 1)
        r = M.align(x, t, label)
        assert np.array_equal(r["states"], M.path_states(path, c - 1))
        assert abs(float(r["score"]) - lp.max(axis=1).sum()) <= 1e-10
        assert np.array_equal(M.frame_classes(r["states"], label, c - 1), path)


def test_negative_control_fails_on_repeated_labels():
    """the slip of tools/patches/mutant_align_allows_repeat_skip.patch (s-2 -> s between equal labels) in the restatement: on repeated labels
    it returns paths that do not collapse to the label, and only there"""
    patch = open(os.path.join(ROOT, "tools", "patches", "mutant_align_allows_repeat_skip.patch")).read()
    assert "ctc_viterbi" in patch and "MUTANT" in patch
    wrong = {True: 0, False: 0}
    for t, c, s in ((3, 3, 2), (5, 4, 2), (9, 6, 4), (40, 6, 4), (64, 3, 8)):
        for seed in range(12):
            x, label = M.make_logits(seed, t, c), M.make_label(seed, t, c, s)
            good, slip = M.align(x, t, label), M.align(x, t, label, allow_repeat_skip=True)
            repeats = any(a == b for a, b in zip(label, label[1:]))
            differs = not np.array_equal(good["states"], slip["states"])
            if differs:
                assert repeats and slip["score"] > good["score"]
                classes = M.frame_classes(slip["states"], label, c - 1)
                assert M.collapse(classes, c - 1) != tuple(label)                # the slip's path spells another labelling
            wrong[repeats] += differs
    assert wrong[False] == 0 and wrong[True] >= 10, wrong


def test_float32_restatement_stays_close():
    x, label = M.make_logits(0, 150, 6), M.make_label(0, 150, 6, 9)
    r64, r32 = M.align(x, 150, label), M.align(x, 150, label, dtype=np.float32)
    assert r32["score"].dtype == np.float32 and r32["post"].dtype == np.float32
    assert abs(float(r32["score"]) - float(r64["score"])) <= 1e-3 and np.abs(r32["post"] - r64["post"]).max() <= 1e-3


def test_the_cases_of_the_device_tests_are_mostly_decided():
    """the caps tests/test_gpu_align.py holds its undecided share to, checked where no device is needed"""
    import test_gpu_align as G
    total = 0
    for shape in G.SHAPES:
        undecided = sum(not G.case(seed, shape)["decided"] for seed in G.SEEDS)
        print("ALIGN-UNDECIDED T=%d C=%d S=%d: %d of %d" % (shape + (undecided, len(G.SEEDS))))
        assert undecided <= 4, (shape, undecided)
        total += undecided
    assert total <= 0.15 * len(G.SHAPES) * len(G.SEEDS)


_KEEP = []        # the arrays behind the pointers below


def _i32(*v):
    a = np.array(v, np.int32)
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def test_entry_point_and_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert "kws_ctc_align" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "kws_ctc_align")
    assert len(lib.kws_ctc_align.argtypes) == 14
    x = ctypes.c_void_p(256)            # a non-null, aligned address that is never read: every refusal below comes first
    sl, ll, lab = _i32(4, 4), _i32(2, 1), _i32(1, 4, 0, 0)

    def call(logits=x, seq=sl, labels=lab, lens=ll, b=2, t=4, c=6, s_max=2, states=x, spans=x, score=x, loss=x, post=x):
        return lib.kws_ctc_align(logits, seq, labels, lens, b, t, c, s_max, states, spans, score, loss, post, None)
    bad = _lib.KWS_ERR_INVALID_ARGUMENT
    assert call(c=2) == bad and b"C=2 out of range [3,8]" in lib.kws_last_error()
    assert call(c=9) == bad and b"C=9" in lib.kws_last_error()
    assert call(s_max=32) == bad and b"S_max=32 out of range [0,31]" in lib.kws_last_error()
    assert call(t=0) == bad and b"bad shape B=2 T=0 S_max=2" in lib.kws_last_error()
    assert call(b=-1) == bad and call(s_max=-1) == bad
    for kw in ({"logits": None}, {"seq": None}, {"labels": None}, {"lens": None}, {"score": None}):
        assert call(**kw) == bad and b"null pointer argument" in lib.kws_last_error(), kw
    assert call(logits=ctypes.c_void_p(258)) == bad and b"4-byte aligned" in lib.kws_last_error()
    for kw in ("states", "spans", "score", "loss", "post"):
        assert call(**{kw: ctypes.c_void_p(257)}) == bad and b"4-byte aligned" in lib.kws_last_error(), kw
    assert call(c=5) == bad and b"labels[0][1]=4 outside [0,3] (the blank is class 4)" in lib.kws_last_error()
    assert call(labels=_i32(1, -1, 0, 0)) == bad
    assert call(seq=_i32(4, 5)) == bad and b"seq_len[1]=5 outside [0,4]" in lib.kws_last_error()
    assert call(lens=_i32(3, 1)) == bad and b"label_len[0]=3 outside [0,2]" in lib.kws_last_error()
    # the LDS bound of the header, 4 T (13 + A) <= 160 KiB, at S_max = 4: A = 9 with the loss or the posteriors, 0 without
    unsupported = _lib.KWS_ERR_UNSUPPORTED
    lab4, len4 = _i32(*([0] * 8)), _i32(4, 4)
    for alpha, t_max in ((9, 1861), (0, 3150)):
        assert 4 * t_max * (13 + alpha) <= 160 * 1024 < 4 * (t_max + 1) * (13 + alpha)
        outs = [{"loss": x, "post": x}, {"loss": x, "post": None}, {"loss": None, "post": x}] if alpha else [{"loss": None, "post": None}]
        for kw in outs:
            assert call(t=t_max + 1, s_max=4, labels=lab4, lens=len4, **kw) == unsupported
            assert ("%d bytes exceed the 163840" % (4 * (t_max + 1) * (13 + alpha))).encode() in lib.kws_last_error()
            if not have_gpu():          # accepted past the check: the next thing that can fail is the device probe
                assert call(t=t_max, s_max=4, labels=lab4, lens=len4, **kw) == _lib.KWS_ERR_NO_DEVICE
    assert call(t=2 ** 31 - 1, s_max=31, seq=_i32(0, 0)) == unsupported
    if not have_gpu():
        assert call(b=0) == _lib.KWS_OK
        assert call() == _lib.KWS_ERR_NO_DEVICE
        assert call(states=None, spans=None, loss=None, post=None) == _lib.KWS_ERR_NO_DEVICE      # the optional outputs
        assert call(labels=None, s_max=0, lens=_i32(0, 0)) == _lib.KWS_ERR_NO_DEVICE
        assert call(labels=_i32(9, 9, 0, 0), seq=_i32(0, 4)) == _lib.KWS_ERR_NO_DEVICE             # an empty slot's label is ignored


def test_python_wrappers_host_side():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd import custom_keyword as K
    assert list(inspect.signature(K.ctc_align).parameters) == ["logits", "seq_len", "labels", "want_post"]
    assert inspect.signature(K.ctc_align).parameters["want_post"].default is False
    assert K.Alignment._fields == ("states", "spans", "score", "loss", "post")
    assert list(inspect.signature(K.Enroller.align).parameters)[:6] == ["self", "inputs", "lengths", "labels", "new_columns", "new_bias"]
    assert list(inspect.signature(K.frame_labels).parameters) == ["states", "labels", "blank"]
    states = np.array([[0, 1, 1, 2, 3, 4, -1], [1, 1, 2, 2, 2, -1, -1]], np.int32)
    got = K.frame_labels(states, [[3, 4], [2]], 5)
    assert got.dtype == np.int32 and got.tolist() == [[5, 3, 3, 5, 4, 5, -1], [2, 2, 5, 5, 5, -1, -1]]
    assert K.frame_labels(states[:1], [3, 4], 5).tolist() == got[:1].tolist()                      # one sequence for all
    for t, c, s in ((9, 6, 4), (64, 3, 8)):                                                        # ... and the restatement's form of it
        x, label = M.make_logits(1, t, c), M.make_label(1, t, c, s)
        st = M.align(x, t - 2, label)["states"]
        assert np.array_equal(K.frame_labels(st[None], [label], c - 1)[0], M.frame_classes(st, label, c - 1))
    with pytest.raises(_lib.InvalidArgumentError, match="outside"):
        K.frame_labels(np.array([[5]]), [[1, 2]], 5)
    with pytest.raises(_lib.InvalidArgumentError, match=r"\[B,T\]"):
        K.frame_labels(np.zeros(3, np.int32), [[1]], 5)
