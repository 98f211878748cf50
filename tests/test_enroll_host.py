"""CPU checks of the customised-keyword enrolment: the fp64 restatement tests/enroll_model.py against torch's CTC loss and autograd,
TensorFlow's Adam against a hand-computed example, prediction.ctc_label, and every refusal the new entry points raise before they
touch a device."""
import ctypes
import types

import numpy as np
import pytest

import enroll_model as M
from conftest import have_gpu


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_restatement_matches_torch_fp64(name):
    import torch
    p = M.make_problem(name)
    want = M.torch_reference(p, torch.float64)
    _, lab_len = M.padded_labels(p["labels"])
    loss, gw, gb = M.enroll_loss_grad(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, p["wn"], p["bn"])
    finite = np.isfinite(loss)
    assert np.abs(np.where(finite, loss, 0.0) - want["loss"]).max() <= 1e-10
    assert np.abs(gw - want["gW"]).max() <= 1e-10 and np.abs(gb - want["gb"]).max() <= 1e-10
    for i in range(p["K"]):                 # ... and the gradient with respect to the logits, utterance by utterance
        _, g = M.ctc_loss_grad(want["logits2"][i], p["seq_len"][i], p["labels"][i])
        assert np.abs(g - want["grad_logits"][i]).max() <= 1e-10
        if not finite[i]:
            assert loss[i] == np.inf and not g.any()
    if name == "one_path_and_repeats":
        assert list(finite) == [True, True, False]        # [5,5] in two frames has no path
        # T == S: the one path's probability is the product of its frames' softmax entries
        lp = M.log_softmax(want["logits2"][0])
        assert abs(loss[0] + lp[np.arange(5), [0, 5, 0, 5, 0]].sum()) <= 1e-10
    if name == "ragged_empty_slot":
        assert loss[2] == 0.0


def test_adam_step_is_tensorflows():
    """theta 1, lr 0.1, gradients 0.5 then -0.25, by hand:
    t=1: m = 0.05, v = 0.00025, lr_t = 0.1 sqrt(0.001) / 0.1 -> theta = 1 - 0.0316227766 * 0.05 / (0.0158113883 + 1e-8)
    t=2: m = 0.02, v = 0.00031225, lr_t = 0.1 sqrt(0.001999) / 0.19 -> theta -= 0.0235316725 * 0.02 / (0.0176705971 + 1e-8)"""
    theta, m, v = M.adam_step(1.0, 0.0, 0.0, 0.5, 1, 0.1)
    assert abs(m - 0.05) < 1e-15 and abs(v - 0.00025) < 1e-15 and abs(theta - 0.9000000632455132) < 1e-12
    theta, m, v = M.adam_step(theta, m, v, -0.25, 2, 0.1)
    assert abs(m - 0.02) < 1e-15 and abs(v - 0.00031225) < 1e-15 and abs(theta - 0.8733663743517929) < 1e-12
    # epsilon sits outside the root: with torch's placement (sqrt(v / (1 - b2^t)) + eps) the first step would be 0.1 / (1 + 1e-7)
    assert abs((1.0 - 0.9000000632455132) - 0.1 / (1 + 1e-8 / np.sqrt(0.00025))) < 1e-12


def test_ctc_label_is_the_datasets_form():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.prediction import ctc_label
    assert ctc_label([5, 6]).tolist() == [0, 5, 0, 6, 0] and ctc_label([1]).tolist() == [0, 1, 0]
    assert ctc_label([1, 2, 3, 3]).tolist() == [0, 1, 0, 2, 0, 3, 0, 3, 0] and ctc_label([2]).dtype == np.int32
    for bad in ([], [0], [1, -2]):
        with pytest.raises(_lib.InvalidArgumentError):
            ctc_label(bad)


_KEEP = []        # the arrays behind the pointers below


def _i32(*v):
    a = np.array(v, np.int32)
    _KEEP.append(a)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_ctc_loss_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    x = ctypes.c_void_p(256)            # a non-null, aligned address that is never read: every refusal below comes first
    sl, sl_p = _i32(4, 4)
    ll, ll_p = _i32(2, 1)
    lab, lab_p = _i32(1, 4, 0, 0)

    def call(logits=x, seq=sl_p, labels=lab_p, lens=ll_p, b=2, t=4, c=6, s_max=2, loss=x, grad=None):
        return lib.kws_ctc_loss(logits, seq, labels, lens, b, t, c, s_max, loss, grad, None)
    bad = _lib.KWS_ERR_INVALID_ARGUMENT
    assert call(c=2) == bad and b"C=2" in lib.kws_last_error()
    assert call(c=9) == bad
    assert call(s_max=32) == bad and b"S_max=32" in lib.kws_last_error()
    assert call(t=0) == bad and call(b=-1) == bad
    assert call(logits=None) == bad and call(seq=None) == bad and call(labels=None) == bad and call(lens=None) == bad and call(loss=None) == bad
    assert call(logits=ctypes.c_void_p(258)) == bad and b"aligned" in lib.kws_last_error()
    assert call(grad=ctypes.c_void_p(257)) == bad
    assert call(c=5) == bad and b"labels[0][1]=4" in lib.kws_last_error()          # 4 is the blank of a 5-class head
    _, neg = _i32(1, -1, 0, 0)
    assert call(labels=neg) == bad
    _, long_seq = _i32(4, 5)
    assert call(seq=long_seq) == bad and b"seq_len[1]=5" in lib.kws_last_error()
    _, long_lab = _i32(3, 1)
    assert call(lens=long_lab) == bad and b"label_len[0]=3" in lib.kws_last_error()
    _, empty = _i32(0, 4)
    if not have_gpu():
        assert call(b=0) == _lib.KWS_OK
        assert call() == _lib.KWS_ERR_NO_DEVICE
        assert call(labels=_i32(9, 9, 0, 0)[1], seq=empty) == _lib.KWS_ERR_NO_DEVICE      # an empty slot's label is ignored


def test_enroll_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    bad = _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_enroll_create(128, 6, 2, 1, 3, None) == bad
    assert lib.kws_enroll_create(100, 6, 2, 1, 3, ctypes.byref(h)) == _lib.KWS_ERR_UNSUPPORTED and b"hidden=100" in lib.kws_last_error()
    for c, n in ((6, 3), (2, 1), (6, 0), (8, 1)):
        assert lib.kws_enroll_create(128, c, n, 1, 3, ctypes.byref(h)) == bad, (c, n)
    assert lib.kws_enroll_create(128, 6, 2, 0, 3, ctypes.byref(h)) == bad
    assert lib.kws_enroll_create(128, 6, 2, 1, 5, ctypes.byref(h)) == bad and b"K=5" in lib.kws_last_error()
    assert lib.kws_enroll_create(128, 6, 2, 1, 0, ctypes.byref(h)) == bad
    assert not h.value
    if not have_gpu():
        assert lib.kws_enroll_create(128, 6, 2, 1, 3, ctypes.byref(h)) == _lib.KWS_ERR_NO_DEVICE
    assert lib.kws_enroll_destroy(None) == _lib.KWS_OK
    assert lib.kws_enroll_set(None, None, None, None) == bad
    assert lib.kws_enroll_fit(None, None, None, None, None, None, 4, 2, 0.01, 1, None, None) == bad
    assert lib.kws_enroll_get(None, None, None, None) == bad
    assert lib.kws_enroll_moments(None, None, None, None) == bad
    assert lib.kws_enroll_stats(None, None, None, None) == bad


def _fake_model(**kw):
    from keyword_spotting_amd import get_config
    num_classes2 = kw.pop("num_classes2", 0)
    return types.SimpleNamespace(config=get_config(**kw), num_classes2=num_classes2, wrappers=(False, False), device="cuda:0")


def test_enroller_refuses_models_it_cannot_train_on():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.custom_keyword import Enroller
    with pytest.raises(_lib.UnsupportedError, match="use_relu"):
        Enroller(_fake_model(use_relu=True), 2)
    with pytest.raises(_lib.UnsupportedError, match="use_relu"):
        Enroller(_fake_model(use_relu=True, value_clip=20.0), 2)
    with pytest.raises(_lib.InvalidArgumentError, match="second head"):
        Enroller(_fake_model(num_classes2=8), 2)
    for precision in ("bf16", "int8", "f16x3"):
        with pytest.raises(_lib.UnsupportedError, match="fp32"):
            Enroller(_fake_model(precision=precision), 2)
