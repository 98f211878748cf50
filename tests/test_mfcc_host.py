"""The MFCC feature path (utils/mfcc.py:20-99) without a GPU: the restatement the kernels are tested against
(tests/mfcc_model.py) pinned by a third-party implementation, the delta quirks it keeps, the config and blob widths that
follow config.mfcc, and the host-side checks of the kws_frontend_*features* entry points (include/kws_amd.h).

test_dct_is_scipys_orthonormal_dct2, test_delta_quirks and test_no_top_db_and_the_floor check the ORACLE (tests/mfcc_model.py)
only: they say nothing about the library and need no feature in it.  Their library-side counterparts need a GPU and are in
tests/test_gpu_mfcc.py: kws_frontend_dct_basis against scipy, the delta edges and one-frame utterances of the kernels' output, and
the exact-zeros signal (-100 dB in every filter)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mfcc_model as M
from conftest import ROOT, have_gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("noise_3600", "noise_loud_3840", "tone_8000", "chirp_8000", "int16_like_3600", "exact_400", "short_559")
SHAPES = ((60, 20), (40, 13))


def test_fixture_covers_every_front_end_signal_at_both_shapes():
    g, src = np.load(os.path.join(GOLDEN, "mfcc_golden.npz")), np.load(os.path.join(GOLDEN, "frontend_golden.npz"))
    assert sorted(k[4:] for k in src.files if k.startswith("pcm_")) == sorted(CASES)
    for name in CASES:
        for n_mel, n_mfcc in SHAPES:
            t = 1 + (src["pcm_" + name].shape[0] - 400) // 160
            assert g["mfcc%d_%d_%s" % (n_mel, n_mfcc, name)].shape == (t, n_mfcc)
    assert not any(k.startswith("pcm_") for k in g.files)            # the signals live in frontend_golden.npz only


@pytest.mark.parametrize("n_mel,n_mfcc", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_restatement_static_coefficients_match_the_third_party_pin(name, n_mel, n_mfcc):
    """transformers' power/dB mel spectrogram + scipy's orthonormal DCT-II.  The gap (3.5e-6 at worst: the chirp, coefficients up
    to 322) is the float32 rounding of D, which the pin does not have."""
    g, src = np.load(os.path.join(GOLDEN, "mfcc_golden.npz")), np.load(os.path.join(GOLDEN, "frontend_golden.npz"))
    got = M.mfcc(src["pcm_" + name], n_mel, n_mfcc)
    want = g["mfcc%d_%d_%s" % (n_mel, n_mfcc, name)]
    assert got.shape == (want.shape[0], 3 * n_mfcc)
    err = np.abs(got[:, :n_mfcc] - want).max()
    print("%s n_mel=%d n_mfcc=%d: |restatement - pin| = %.2e (max|c| = %.1f)" % (name, n_mel, n_mfcc, err, np.abs(want).max()))
    assert err < 1e-5


@pytest.mark.parametrize("n", [1, 13, 20, 40])
def test_dct_is_scipys_orthonormal_dct2(n):
    import scipy.fft
    D = M.dct(n, 40)
    x = np.random.default_rng(n).standard_normal((5, 40))
    assert np.abs(x @ D - scipy.fft.dct(x, type=2, norm="ortho", axis=-1)[:, :n]).max() < 1e-13
    assert np.abs(D.T @ D - np.eye(n)).max() < 1e-13


def test_delta_quirks():
    """_delta_order shifts by ONE frame whatever its order (utils/mfcc.py:58-69), so with d[t] = c[min(t+1, T-1)] - c[max(t-1, 0)]
    delta(c, 1) = d / 2, delta(c, 2) = (d + 2 d) / 10 = 0.3 d = 0.6 delta(c, 1); one frame gives zero deltas."""
    rng = np.random.default_rng(3)
    for T in (1, 2, 3, 7):
        c = rng.standard_normal((T, 5))
        f = M.features_from_static(c)
        assert f.shape == (T, 15) and np.array_equal(f[:, :5], c)
        d1, d2 = f[:, 5:10], f[:, 10:]
        d = c[np.minimum(np.arange(T) + 1, T - 1)] - c[np.maximum(np.arange(T) - 1, 0)]
        assert np.abs(d1 - d / 2).max() < 1e-15 and np.abs(d2 - 0.3 * d).max() < 1e-15
        assert np.abs(d2 - 0.6 * d1).max() < 1e-15
        if T == 1:
            assert not d1.any() and not d2.any()
        if T == 2:          # both rows see the same difference
            assert np.allclose(d1[0], (c[1] - c[0]) / 2) and np.allclose(d1[1], (c[1] - c[0]) / 2)
        if T >= 3:          # edges are one-sided, the interior is the central difference
            assert np.allclose(d1[0], (c[1] - c[0]) / 2) and np.allclose(d1[-1], (c[-1] - c[-2]) / 2)
            assert np.allclose(d1[1], (c[2] - c[0]) / 2)
    assert M.features_from_static(np.zeros((0, 4))).shape == (0, 12)
    assert M.mfcc(np.zeros(399), 40, 13).shape == (0, 39)


def test_no_top_db_and_the_floor():
    """Silence is -100 dB in every filter, not max - 80: c0 = -100 sqrt(n_mel) and every other coefficient 0."""
    f = M.mfcc(np.zeros(720), 60, 20)
    assert f.shape == (3, 60)
    assert np.abs(f[:, 0] + 100.0 * np.sqrt(60.0)).max() < 1e-4 and np.abs(f[:, 1:]).max() < 1e-4
    x = np.zeros(400 + 160 * 5)
    x[:400] = np.random.default_rng(0).standard_normal(400)
    S = M.mfcc(x, 60, 20, with_db=True)[1]
    assert S[0].max() > 0.0 and (S[-1] == -100.0).all()     # a top_db of 80 would have lifted the silent frame to max - 80


def test_attention_config_follows_the_mfcc_switch():
    from keyword_spotting_amd import attention_weights as AW
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.config import get_attention_config
    cfg = get_attention_config(mfcc=True)
    assert cfg.n_mfcc == 20 and cfg.n_mel == 60 and cfg.freq_size == 60 and cfg.power == 1
    assert get_attention_config().freq_size == 60 and get_attention_config(n_mel=40).freq_size == 40 and not get_attention_config().mfcc
    c13 = get_attention_config(mfcc=True, n_mfcc=13, n_mel=40)
    assert c13.freq_size == 39
    top, _ = AW.shapes(c13)
    assert top["W_in"] == (39 * c13.combine_frame, c13.hidden_size)
    w = AW.init(c13, 0)
    blob = AW.to_blob(c13, w)
    plain = AW.to_blob(get_attention_config(n_mel=40), AW.init(get_attention_config(n_mel=40), 0))
    assert plain.size - blob.size == (40 - 39) * c13.combine_frame * c13.hidden_size
    with pytest.raises(AttributeError):                  # the RNN deploy graph has no MFCC branch (models/rnn_ctc.py:139-149)
        get_config(mfcc=True)
    with pytest.raises(AttributeError):
        get_config(n_mfcc=20)


def test_blob_size_of_the_abi_follows_freq_size():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd import attention_weights as AW
    from keyword_spotting_amd.config import get_attention_config
    lib = _lib.load()
    for kw in (dict(mfcc=True), dict(mfcc=True, n_mfcc=13, n_mel=40)):
        cfg = get_attention_config(**kw)
        abi = _lib.KwsAttentionConfig(cfg.freq_size, cfg.combine_frame, cfg.hidden_size, cfg.multi_head_num, cfg.feed_forward_inner_size,
                                      cfg.num_layers, cfg.num_classes, int(cfg.use_relu), cfg.max_frames)
        assert lib.kws_attention_weights_nbytes(ctypes.byref(abi)) == AW.to_blob(cfg, AW.init(cfg, 1)).nbytes


def test_converter_takes_the_mfcc_width(tmp_path):
    import subprocess
    import sys
    from keyword_spotting_amd import attention_weights as AW
    from keyword_spotting_amd.config import get_attention_config
    cfg = get_attention_config(mfcc=True, n_mfcc=13, n_mel=40)
    w = AW.init(cfg, 2)
    np.savez(tmp_path / "vars.npz", **AW.to_tf_variables(cfg, w))
    tool = os.path.join(ROOT, "tools", "convert_weights.py")
    ok = subprocess.run([sys.executable, tool, str(tmp_path / "vars.npz"), "--model", "attention", "--n-mel", "40", "--mfcc", "--n-mfcc", "13",
                         "--out", str(tmp_path / "m")], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert np.array_equal(np.fromfile(tmp_path / "m.blob", np.float32), AW.to_blob(cfg, w))
    bad = subprocess.run([sys.executable, tool, str(tmp_path / "vars.npz"), "--model", "attention", "--n-mel", "40", "--out", str(tmp_path / "n")],
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "input_linear_trans/kernel" in bad.stderr


def test_struct_size_and_declared_symbols():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert lib.kws_sizeof_feature_config() == ctypes.sizeof(_lib.KwsFeatureConfig) == 36
    assert lib.kws_sizeof_frontend_config() == ctypes.sizeof(_lib.KwsFrontendConfig) == 24          # unchanged
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kws_amd.h")).read(), flags=re.S)
    for sym in ("kws_sizeof_feature_config", "kws_frontend_create_features", "kws_frontend_feature_size", "kws_frontend_run_lengths",
                "kws_frontend_dct_basis"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTED_SYMBOLS
    assert re.search(r"KWS_FEAT_MEL\s*=\s*0\s*,\s*KWS_FEAT_MFCC\s*=\s*1", text)


def _feat(kind, power, n_mfcc, fft=400, n_mel=60):
    from keyword_spotting_amd import _lib
    return _lib.KwsFeatureConfig(_lib.KwsFrontendConfig(16000, fft, 160, n_mel, 300.0, 8000.0), kind, power, n_mfcc)


def test_create_features_validates_before_any_device_work():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()

    def create(cfg):
        rc = lib.kws_frontend_create_features(ctypes.byref(cfg), ctypes.byref(h))
        assert rc != _lib.KWS_OK and not h.value
        return rc, lib.kws_last_error().decode()

    assert lib.kws_frontend_create_features(None, ctypes.byref(h)) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_frontend_create_features(ctypes.byref(_feat(1, 2, 20)), None) == _lib.KWS_ERR_INVALID_ARGUMENT
    for n_mfcc, n_mel in ((0, 60), (-1, 60), (33, 60), (21, 20), (14, 13)):
        rc, msg = create(_feat(_lib.FEAT_MFCC, 2, n_mfcc, n_mel=n_mel))
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "n_mfcc=%d" % n_mfcc in msg, msg
    for power in (0, 3, -2):
        rc, msg = create(_feat(_lib.FEAT_MEL, power, 0))
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "power=%d" % power in msg, msg
    rc, msg = create(_feat(2, 1, 0))
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "kind=2" in msg
    rc, msg = create(_feat(_lib.FEAT_MFCC, 1, 20, fft=256))
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "fft_size=256" in msg and "MFCC" in msg, msg
    rc, msg = create(_feat(_lib.FEAT_MEL, 2, 0, fft=256))
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "fft_size=256" in msg and "power=2" in msg, msg
    rc, msg = create(_feat(_lib.FEAT_MFCC, 2, 20, n_mel=65))          # the base config's own checks still come first
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "n_mel" in msg
    if not have_gpu():
        # MFCC ignores `power`; the valid configs get as far as the device
        for cfg in (_feat(_lib.FEAT_MFCC, 7, 20), _feat(_lib.FEAT_MFCC, 2, 32, n_mel=64), _feat(_lib.FEAT_MEL, 2, 0), _feat(_lib.FEAT_MEL, 1, 99)):
            assert create(cfg)[0] == _lib.KWS_ERR_NO_DEVICE


def test_null_handles_are_refused():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert lib.kws_frontend_run_lengths(None, None, None, 1, 400, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_frontend_feature_size(None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_frontend_dct_basis(None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
