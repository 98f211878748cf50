"""CPU-only checks of the customised-keyword surface (a second class head and nn_outputs): the fp64 restatement against the
oracle, the C ABI's sizes and pre-device refusals, the weight containers, predict_ctc's decode-and-OR logic and run()'s fetch
names.  None of it needs a GPU."""
import ctypes

import numpy as np
import pytest

import heads_model as HM
from oracle import decode_oracle as D
from oracle import gru_oracle as G


def _cfg(n_mel=40, hidden=128, layers=2, classes=6, relu=0, clip=-1.0, precision=0):
    from keyword_spotting_amd import _lib
    return _lib.KwsConfig(n_mel, hidden, layers, classes, relu, clip, precision)


def _canonical_floats(n_mel, hidden, layers, classes):
    n, i = 0, n_mel
    for _ in range(layers):
        n += (i + hidden) * 3 * hidden + 3 * hidden
        i = hidden
    return n + hidden * classes + classes


@pytest.mark.parametrize("relu,clip", [(False, -1.0), (True, 20.0)])
def test_restatement_head1_equals_the_oracle(relu, clip):
    w = HM.random_heads_weights(13, 64, 3, 6, 8, seed=5, scale=8.0 if relu else 1.0)
    mel = G.synthetic_mel(5, 9, 13, seed=6)
    st = 0.3 * np.random.default_rng(7).standard_normal((3, 5, 64))
    lens = np.array([0, 1, 8, 9, 4])
    r = HM.heads_forward(w, mel, st, lens, use_relu=relu, value_clip=clip)
    want, want_state = G.gru_forward(w, mel, st, lens, dtype=np.float64, use_relu=relu, value_clip=clip)
    assert np.abs(r["logits1"] - want).max() <= 1e-12
    assert np.abs(r["state"] - want_state).max() <= 1e-12
    # the second head is the same function of the same rows; rows past the length are the zero row
    lg2 = r["top"] @ w["Wfc2"].astype(np.float64) + w["bfc2"]
    if relu:
        lg2 = np.clip(lg2, 0.0, 20.0)
    assert np.array_equal(r["logits2"], lg2)
    for b, n in enumerate(lens):
        assert not r["top"][b, n:].any()
    assert np.abs(r["softmax2"].sum(-1) - 1).max() < 1e-12


def test_weights_nbytes_heads():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for (i, h, l, c, c2) in [(40, 128, 2, 6, 8), (13, 64, 1, 5, 3), (60, 256, 4, 6, 6)]:
        assert lib.kws_weights_nbytes_heads(ctypes.byref(_cfg(i, h, l, c)), c2) == 4 * (_canonical_floats(i, h, l, c) + h * c2 + c2)
        assert lib.kws_weights_nbytes_heads(ctypes.byref(_cfg(i, h, l, c)), c2) == lib.kws_weights_nbytes(ctypes.byref(_cfg(i, h, l, c))) + 4 * (h * c2 + c2)
    for bad in (2, 9, 0, -1):
        assert lib.kws_weights_nbytes_heads(ctypes.byref(_cfg()), bad) == 0
        assert b"num_classes2=%d" % bad in lib.kws_last_error()
    assert lib.kws_weights_nbytes_heads(ctypes.byref(_cfg(hidden=100)), 8) == 0
    assert b"hidden=100" in lib.kws_last_error()
    assert lib.kws_weights_nbytes_heads(None, 8) == 0
    assert lib.kws_weights_nbytes_heads(ctypes.byref(_cfg(precision=_lib.BF16)), 8) == 0


def test_create_heads_refusals_come_before_the_device():
    """Every refusal by code and message; none of them reaches hipGetDeviceCount (this test runs without a GPU, where a probe
    would answer KWS_ERR_NO_DEVICE)."""
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    blob = np.zeros(_canonical_floats(40, 128, 2, 6) + 128 * 8 + 8, np.float32)

    def create(cfg, c2, nbytes=None):
        return lib.kws_create_heads(ctypes.byref(cfg), c2, blob.ctypes.data_as(ctypes.c_void_p),
                                    blob.nbytes if nbytes is None else nbytes, ctypes.byref(out))
    for bad in (2, 9):
        assert create(_cfg(), bad) == _lib.KWS_ERR_UNSUPPORTED
        assert b"num_classes2=%d unsupported (3..8)" % bad in lib.kws_last_error()
    for prec, word in ((_lib.BF16, b"bf16"), (_lib.INT8, b"int8"), (_lib.F16X3, b"f16x3")):
        assert create(_cfg(precision=prec), 8) == _lib.KWS_ERR_UNSUPPORTED
        msg = lib.kws_last_error()
        assert b"second class head needs precision fp32" in msg and word in msg
    # a canonical blob without the second head, and one float short
    assert create(_cfg(), 8, 4 * _canonical_floats(40, 128, 2, 6)) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert b"weights_blob has 657432 bytes, config needs 661560" in lib.kws_last_error()
    assert create(_cfg(), 8, blob.nbytes - 4) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert create(_cfg(hidden=100), 8) == _lib.KWS_ERR_UNSUPPORTED
    assert lib.kws_create_heads(ctypes.byref(_cfg()), 8, None, blob.nbytes, ctypes.byref(out)) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_create_heads(ctypes.byref(_cfg()), 8, blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert not out.value
    assert lib.kws_step_heads(None, None, None, None, None, None, None, None, None, 1, 1, None) == _lib.KWS_ERR_INVALID_ARGUMENT


def test_head_io_struct_size():
    from keyword_spotting_amd import _lib
    assert _lib.load().kws_sizeof_head_io() == ctypes.sizeof(_lib.KwsHeadIo) == 40


def test_to_blob_appends_the_second_head_and_extend_head_inserts_columns():
    from keyword_spotting_amd import get_config, weights
    cfg = get_config(n_mel=4, hidden_size=64, num_layers=1)
    w = weights.init_weights(cfg, seed=3)
    plain = weights.to_blob(cfg, w)
    h, c = 64, 6
    new_cols = np.arange(2 * h, dtype=np.float32).reshape(h, 2) + 1000.0
    wfc2, bfc2 = weights.extend_head(w["Wfc"], np.arange(6, dtype=np.float32), new_cols, np.array([70.0, 80.0], np.float32))
    assert wfc2.shape == (h, 8) and wfc2.dtype == np.float32
    assert np.array_equal(wfc2[:, :5], w["Wfc"][:, :5])            # space, three words, garbage: untouched, in place
    assert np.array_equal(wfc2[:, 5:7], new_cols)                   # the new words in front of ...
    assert np.array_equal(wfc2[:, 7], w["Wfc"][:, 5])               # ... the ctc blank
    assert bfc2.tolist() == [0, 1, 2, 3, 4, 70, 80, 5]
    with pytest.raises(ValueError):
        weights.extend_head(w["Wfc"], np.zeros(6), np.zeros((h + 1, 2)), np.zeros(2))
    # the blob: canonical part unchanged, then Wfc2 row-major, then bfc2
    cfg.num_classes2 = 8
    w2 = dict(w, Wfc2=wfc2, bfc2=bfc2)
    blob = weights.to_blob(cfg, w2)
    assert blob.dtype == np.float32 and blob.size == plain.size + h * 8 + 8
    assert np.array_equal(blob[:plain.size], plain)
    assert np.array_equal(blob[plain.size:plain.size + h * 8], wfc2.ravel())
    assert np.array_equal(blob[plain.size + h * 8:], bfc2)
    back = weights.from_blob(cfg, blob)
    assert np.array_equal(back["Wfc2"], wfc2) and np.array_equal(back["bfc2"], bfc2) and np.array_equal(back["Wfc"], w["Wfc"])
    from keyword_spotting_amd import _lib
    assert blob.nbytes == _lib.load().kws_weights_nbytes_heads(ctypes.byref(_cfg(4, 64, 1, 6)), 8)
    with pytest.raises(ValueError):
        weights.to_blob(cfg, w)                                     # num_classes2 set, no second head
    with pytest.raises(ValueError):
        weights.to_blob(cfg, dict(w2, bfc2=np.zeros(7, np.float32)))
    del cfg.num_classes2
    with pytest.raises(ValueError):
        weights.to_blob(cfg, w2)                                    # a second head the config does not announce


class _StubModel(object):
    """What predict_ctc needs of a DeployModel: the class counts, a zero state, and run() on the three fetch names."""

    def __init__(self, sm1, sm2):
        from keyword_spotting_amd import get_config
        self.config = get_config()
        self.num_classes2 = sm2.shape[1]
        self.sm = (sm1, sm2)
        self.calls = []

    def zero_state(self, batch=1):
        return np.zeros((2, batch, 128), np.float32)

    def run(self, fetches, feed_dict):
        self.calls.append((list(fetches), sorted(feed_dict)))
        return [self.sm[0], self.sm[1], np.zeros((len(self.sm[0]), 128), np.float32)]


class _Decoders(object):
    """The oracle's decoders (pinned to the reference by tests/test_oracle_decode.py) behind the names and argument order of
    keyword_spotting_amd.prediction, recording how they were called."""

    def __init__(self):
        self.calls = []

    def ctc_decode_strict(self, softmax, classnum):
        self.calls.append(("strict", softmax.shape[1], classnum))
        return D.ctc_decode_strict(softmax, classnum)

    def ctc_decode(self, softmax, lockout):
        self.calls.append(("decode", softmax.shape[1], lockout))
        return D.ctc_decode(softmax, lockout)

    def ctc_predict(self, seq, label):
        return D.ctc_predict(seq, label)


def _eight_columns(sm6):
    """A stored 6-class softmax as the 8-class one of a head whose two new words (extend_head: in front of the blank) never fire."""
    return np.concatenate([sm6[:, :5], np.zeros((len(sm6), 2), np.float32), sm6[:, 5:]], axis=1)


def test_predict_ctc_decodes_each_head_and_ors(golden):
    """Head 1: the reference's stored 6-class cases (decode_golden.npz) and its own stored ctc_decode_strict answers.  Head 2: those
    cases widened to 8 classes, and the hand-built 8-class cases of heads_golden.npz (make_heads_golden.py), whose peaks are far
    enough apart to survive a lockout of 8."""
    from keyword_spotting_amd.custom_keyword import predict_ctc
    from keyword_spotting_amd.rnn_ctc import FEED_INPUT, FEED_STATE
    from conftest import ROOT
    import os
    hg = np.load(os.path.join(ROOT, "tests", "golden", "heads_golden.npz"))
    cases = [k for k in range(int(golden["n_cases"])) if len(golden["c%d_softmax" % k]) >= 10]
    second = [_eight_columns(golden["c%d_softmax" % k]) for k in cases[::6]] + [hg[k] for k in sorted(hg.files)]
    seen = set()
    for a in cases:
        for sm2 in second:
            sm1 = golden["c%d_softmax" % a]
            model, dec = _StubModel(sm1, sm2), _Decoders()
            result, out1, out2 = predict_ctc(model, np.zeros(16000, np.float32), "1233", decoders=dec)
            assert model.calls == [(["model/softmax1:0", "model/softmax2:0", "model/nn_outputs:0"], sorted([FEED_INPUT, FEED_STATE]))]
            # head 1: ctc_decode_strict with its 6 classes -- the reference's own stored answer
            assert np.array_equal(out1, golden["c%d_strict" % a])
            # head 2: ctc_decode, its class count in the lockout position as the server passes it
            assert dec.calls == [("strict", 6, 6), ("decode", 8, 8)]
            assert np.array_equal(out2, D.ctc_decode(sm2, lockout=8))
            p1, p2 = D.ctc_predict(out1, "1233"), D.ctc_predict(out2, "1233")
            assert result == (p1 | p2)
            seen.add((p1, p2))
    assert seen == {(0, 0), (1, 0), (0, 1), (1, 1)}, seen          # the OR is exercised from every side
    # the lockout of 8 is what decides h1 (peaks 4 frames apart): under ctc_decode's default it would be a hit
    assert D.ctc_predict(D.ctc_decode(hg["h1_softmax"], lockout=8)) == 0 and D.ctc_predict(D.ctc_decode(hg["h1_softmax"])) == 1


def test_run_refuses_the_heads_fetches_on_a_one_head_model():
    """run() validates its fetch list before any device work; a DeployModel needs a device to be created, so the instance is
    made without __init__."""
    from keyword_spotting_amd import _lib, get_config
    from keyword_spotting_amd import rnn_ctc
    m = rnn_ctc.DeployModel.__new__(rnn_ctc.DeployModel)
    m.config, m.num_classes2, m._frontend, m._handle = get_config(), 0, None, None
    for name in ("model/softmax1:0", "model/softmax2:0", "model/nn_outputs:0"):
        with pytest.raises(_lib.InvalidArgumentError) as e:
            m.run([name], {rnn_ctc.FEED_INPUT: np.zeros((3, 40), np.float32), rnn_ctc.FEED_STATE: np.zeros((2, 1, 128), np.float32)})
        assert "unknown fetch %r (graph exports model/softmax:0, model/logit:0, model/rnn_states:0)" % name in str(e.value)
    with pytest.raises(_lib.InvalidArgumentError) as e:
        m.forward_heads(np.zeros((1, 3, 40), np.float32), np.zeros((2, 1, 128), np.float32))
    assert "num_classes2" in str(e.value)
