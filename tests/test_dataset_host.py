"""The dataset front-end (process_wav.py:38-44,69-78 -> reader.py:264-269) without a GPU: the restatement the kernels are tested
against (tests/dataset_model.py) pinned by two third-party implementations of librosa.stft's transform and by np.pad's reflection,
the frame count, and the host-side checks of kws_frontend_create_dataset / kws_frontend_frames_of / kws_frontend_window
(include/kws_amd.h).  The kernels' side is tests/test_gpu_dataset.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import dataset_model as D
from conftest import ROOT, have_gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "dataset_golden.npz")
LENGTHS, PRE = (201, 360, 1234), (0.0, 0.97)


@pytest.mark.parametrize("pre", PRE)
@pytest.mark.parametrize("n", LENGTHS)
def test_restatement_matches_both_third_party_pins(n, pre):
    """scipy.signal.stft on the reflect-padded signal computes in float64: 1e-12.  transformers.audio_utils.spectrogram computes in
    complex64: 1e-6 of the largest value, four times the 2.5e-7 absolute it was measured at on spectra of scale 3-8."""
    g = np.load(GOLDEN)
    got = D.linearspec(g["pcm_%d" % n], pre)
    sc, tr = g["scipy_%d_pre%g" % (n, pre)], g["transformers_%d_pre%g" % (n, pre)]
    assert got.shape == sc.shape == tr.shape == (D.num_frames(n), 201)
    e_sc, e_tr, scale = np.abs(got - sc).max(), np.abs(got - tr).max(), np.abs(got).max()
    print("n=%d pre=%g: |restatement - scipy| = %.2e  |restatement - transformers| = %.2e (max %.2f)" % (n, pre, e_sc, e_tr, scale))
    assert e_sc < 1e-12
    assert e_tr < 1e-6 * scale
    assert np.abs(D.window() - g["window"]).max() < 1e-15


@pytest.mark.parametrize("n", [201, 359, 360, 3601])
def test_index_formula_is_np_pads_reflection(n):
    y = np.random.default_rng(n).standard_normal(n)
    idx = D.source_index(n)
    assert idx.shape == (1 + n // 160, 400) and idx.min() >= 0 and idx.max() < n
    padded = np.pad(y, 200, mode="reflect")
    want = padded[160 * np.arange(idx.shape[0])[:, None] + np.arange(400)[None]]
    assert np.array_equal(y[idx], want)


def test_pre_emphasis_is_float32_with_two_roundings():
    x = (np.random.default_rng(1).standard_normal(1000) * 0.3).astype(np.float32)
    y = D.pre_emphasis(x, 0.97)
    assert y.dtype == np.float32 and y[0] == x[0]
    want = x[1:] - (np.float32(0.97) * x[:-1]).astype(np.float32)
    assert np.array_equal(y[1:], want)
    fused = (x[1:].astype(np.float64) - np.float64(np.float32(0.97)) * x[:-1].astype(np.float64)).astype(np.float32)
    assert not np.array_equal(y[1:], fused)              # an FMA would round once: the signal tells the two apart
    assert D.pre_emphasis(x, 0.0) is not None and np.array_equal(D.pre_emphasis(x, 0.0), x)


def _dataset(framing=1, pre=0.0, kind=0, power=1, n_mfcc=0, fft=400, n_mel=40):
    from keyword_spotting_amd import _lib
    feat = _lib.KwsFeatureConfig(_lib.KwsFrontendConfig(16000, fft, 160, n_mel, 300.0, 8000.0), kind, power, n_mfcc)
    return _lib.KwsDatasetConfig(feat, framing, pre)


def test_frame_count_of_the_model_and_struct_sizes():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert [D.num_frames(n) for n in (0, 200, 201, 319, 320)] == [0, 0, 2, 2, 3]
    assert lib.kws_sizeof_dataset_config() == ctypes.sizeof(_lib.KwsDatasetConfig) == 44
    assert lib.kws_sizeof_feature_config() == ctypes.sizeof(_lib.KwsFeatureConfig) == 36          # unchanged
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kws_amd.h")).read(), flags=re.S)
    for sym in ("kws_sizeof_dataset_config", "kws_frontend_create_dataset", "kws_frontend_frames_of", "kws_frontend_window"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTED_SYMBOLS
    assert re.search(r"KWS_FRAMES_DEPLOY\s*=\s*0\s*,\s*KWS_FRAMES_DATASET\s*=\s*1", text)
    # kws_frontend_frames keeps its meaning: the deploy rule
    base = _lib.KwsFrontendConfig(16000, 400, 160, 40, 300.0, 8000.0)
    assert [lib.kws_frontend_frames(ctypes.byref(base), n) for n in (201, 399, 400, 560)] == [0, 0, 1, 2]


def test_create_dataset_validates_before_any_device_work(monkeypatch):
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()

    def create(cfg):
        rc = lib.kws_frontend_create_dataset(ctypes.byref(cfg), ctypes.byref(h))
        assert rc != _lib.KWS_OK and not h.value
        return rc, lib.kws_last_error().decode()

    assert lib.kws_frontend_create_dataset(None, ctypes.byref(h)) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_frontend_create_dataset(ctypes.byref(_dataset()), None) == _lib.KWS_ERR_INVALID_ARGUMENT
    for framing in (2, -1):
        rc, msg = create(_dataset(framing=framing))
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "framing=%d" % framing in msg, msg
    for pre in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        rc, msg = create(_dataset(pre=pre))
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "pre_emphasis" in msg, msg
    rc, msg = create(_dataset(framing=_lib.FRAMES_DEPLOY, pre=0.97))          # the deploy graph has no pre-emphasis
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "pre_emphasis" in msg and "DEPLOY" in msg, msg
    for kw in (dict(), dict(kind=_lib.FEAT_MFCC, n_mfcc=13), dict(power=2)):
        rc, msg = create(_dataset(fft=256, **kw))
        assert rc == _lib.KWS_ERR_UNSUPPORTED and "fft_size=256" in msg, msg
    rc, msg = create(_dataset(fft=256, pre=0.97))
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "fft_size=256" in msg and "KWS_FRAMES_DATASET" in msg, msg
    # the feature config's own checks, as kws_frontend_create_features makes them
    rc, msg = create(_dataset(kind=_lib.FEAT_MFCC, n_mfcc=33, n_mel=60))
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "n_mfcc=33" in msg, msg
    rc, msg = create(_dataset(power=3))
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "power=3" in msg, msg
    rc, msg = create(_dataset(kind=2))
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "kind=2" in msg, msg
    rc, msg = create(_dataset(n_mel=65))
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "n_mel" in msg, msg
    # the dense-DFT kernel frames as the deploy graph only (the switch is read at create)
    monkeypatch.setenv("KWS_FRONTEND_DENSE", "1")
    rc, msg = create(_dataset())
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "KWS_FRONTEND_DENSE=1" in msg and "KWS_FRAMES_DATASET" in msg, msg
    monkeypatch.delenv("KWS_FRONTEND_DENSE")
    if not have_gpu():
        # {feat, KWS_FRAMES_DEPLOY, 0} passes exactly what kws_frontend_create_features passes, fft sizes other than 400 included
        for cfg in (_dataset(), _dataset(pre=0.97), _dataset(kind=_lib.FEAT_MFCC, n_mfcc=20, n_mel=60, pre=0.5), _dataset(power=2),
                    _dataset(framing=_lib.FRAMES_DEPLOY), _dataset(framing=_lib.FRAMES_DEPLOY, fft=256)):
            assert create(cfg)[0] == _lib.KWS_ERR_NO_DEVICE
            assert lib.kws_frontend_create_features(ctypes.byref(cfg.feat), ctypes.byref(h)) == _lib.KWS_ERR_NO_DEVICE


def test_deploy_framing_refuses_what_create_features_refuses():
    """The {feat, KWS_FRAMES_DEPLOY, 0} identity at the argument-check level: the same code and message for the same feature config."""
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    for kw in (dict(kind=_lib.FEAT_MFCC, n_mfcc=0), dict(power=0), dict(kind=3), dict(fft=256, power=2), dict(fft=250), dict(n_mel=0)):
        cfg = _dataset(framing=_lib.FRAMES_DEPLOY, **kw)
        rc_d = lib.kws_frontend_create_dataset(ctypes.byref(cfg), ctypes.byref(h))
        msg_d = lib.kws_last_error()
        rc_f = lib.kws_frontend_create_features(ctypes.byref(cfg.feat), ctypes.byref(h))
        assert rc_d == rc_f and rc_d != _lib.KWS_OK and msg_d == lib.kws_last_error(), kw


def test_null_handles_are_refused():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert lib.kws_frontend_frames_of(None, 400) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_frontend_window(None, None) == _lib.KWS_ERR_INVALID_ARGUMENT


def test_attention_config_has_the_pre_emphasis_switch():
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.config import get_attention_config
    assert get_attention_config().pre_emphasis is False and get_attention_config(pre_emphasis=True).pre_emphasis is True
    with pytest.raises(AttributeError):                  # config/rnn_config.py has no such field
        get_config(pre_emphasis=True)
