"""The reader's noise augmentation (reader.py:207-280) without a GPU: the restatement the kernels are tested against
(tests/augment_model.py) against its closed form, the argument checks of kws_frontend_run_linear / kws_frontend_augment
(include/kws_amd.h) that are decided before the device is touched, and NoiseAugmenter's draws.  The kernels' side is
tests/test_gpu_augment.py and tests/test_gpu_enroll_augmented.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import augment_model as A
import dataset_model as D
from conftest import ROOT, have_gpu


def _pair(seed=5):
    rng = np.random.default_rng(seed)
    clean = (rng.standard_normal(1600) * 0.1).astype(np.float32)
    noise = (rng.standard_normal(4000) * 0.3).astype(np.float32)
    return D.linearspec(clean), D.linearspec(noise)


@pytest.mark.parametrize("gain", [-5.0, -15.0, 0.0, 3.5])
def test_factor_is_the_root_of_the_mean_energy_ratio(gain):
    clean, noise = _pair()
    e_a, e_n = np.square(clean).sum(), np.square(noise).sum()
    want = np.sqrt((e_a / clean.shape[0]) / (e_n / noise.shape[0])) * 10 ** (gain / 20)
    got = A.factor(clean, noise, gain)
    assert abs(got - want) <= 1e-12 * want, (got, want)
    # the mixed noise then lies `gain` dB from the utterance's level, as config/rnn_config.py:71-72 means it
    assert abs(A.compute_db(got * noise, noise.shape[0]) - A.compute_db(clean, clean.shape[0]) - gain) < 1e-9


def test_factor_edge_cases_follow_the_header():
    clean, noise = _pair()
    assert A.factor(np.zeros_like(clean), noise, -5.0) == 0.0          # 10 ** -inf
    assert A.factor(clean, np.zeros_like(noise), -5.0) == 0.0          # the reference: NaN
    assert A.factor(clean, noise[:0], -5.0) == 0.0


def test_mix_is_linear_in_the_noise_at_a_fixed_factor():
    clean, noise = _pair()
    other = D.linearspec((np.random.default_rng(6).standard_normal(4000) * 0.2).astype(np.float32))
    f = A.factor(clean, noise, -5.0)
    for start in (0, 3, 20, 40):
        a, b, both = A.mix(clean, noise, start, f), A.mix(clean, other, start, f), A.mix(clean, 2.0 * noise + 0.5 * other, start, f)
        assert np.abs((both - clean) - (2.0 * (a - clean) + 0.5 * (b - clean))).max() <= 1e-12 * np.abs(both).max()
    # a slice past the clip's end adds zeros; a negative start reads as 0
    assert np.array_equal(A.mix(clean, noise, noise.shape[0], f), clean)
    assert np.array_equal(A.mix(clean, noise, -3, f), A.mix(clean, noise, 0, f))
    assert np.array_equal(A.noise_slice(noise, noise.shape[0] - 2, 5)[2:], np.zeros((3, 201)))


def test_entry_points_are_declared_and_bound():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kws_amd.h")).read(), flags=re.S)
    for sym in ("kws_frontend_linear_size", "kws_frontend_run_linear", "kws_frontend_augment"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert hasattr(lib, sym) and sym in _lib.EXPORTED_SYMBOLS


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_refusals_are_decided_before_the_device_is_touched():
    """Sizes first, then the pointers (the handle among them): all of it refused on a machine without a GPU."""
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, np.float32)            # host memory: never dereferenced by a refused call
    p = _ptr(buf)

    def linear(h, pcm, B, n_max, spec, frames, energy):
        rc = lib.kws_frontend_run_linear(h, pcm, None, B, n_max, spec, frames, energy, None)
        return rc, lib.kws_last_error().decode()

    for B, n_max in ((0, 1600), (-1, 1600), (2, 0), (2, -5)):
        rc, msg = linear(None, p, B, n_max, p, p, p)
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "B=%d n_max=%d" % (B, n_max) in msg, msg
    rc, msg = linear(None, p, 2, 1600, p, p, p)
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "handle is null" in msg, msg

    def augment(h, R=3, B=2, T=11, K=2, Tn=51, null=None):
        args = dict(spec=p, frames=p, energy=p, noise_spec=p, noise_frames=p, noise_energy=p, src=p, noise=p, start=p, gain_db=p, out=p)
        if null:
            args[null] = None
        rc = lib.kws_frontend_augment(h, args["spec"], args["frames"], args["energy"], B, T, args["noise_spec"], args["noise_frames"],
                                      args["noise_energy"], K, Tn, args["src"], args["noise"], args["start"], args["gain_db"], R,
                                      args["out"], None)
        return rc, lib.kws_last_error().decode()

    for kw in (dict(R=0), dict(R=-2), dict(B=0), dict(T=0), dict(K=0), dict(Tn=0)):
        rc, msg = augment(None, **kw)
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "must be positive" in msg, msg
        assert "%s=%d" % ({"T": "T_max", "Tn": "Tn_max"}.get(list(kw)[0], list(kw)[0]), list(kw.values())[0]) in msg, msg
    rc, msg = augment(None)
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "handle is null" in msg, msg
    assert lib.kws_frontend_linear_size(None) == _lib.KWS_ERR_INVALID_ARGUMENT and b"handle is null" in lib.kws_last_error()

    if not have_gpu():
        return
    # with a handle (which needs a device to exist): every null pointer by name of its group, and a handle without the FFT kernel
    base = _lib.KwsFrontendConfig(16000, 400, 160, 40, 300.0, 8000.0)
    h = ctypes.c_void_p()
    _lib.check(lib.kws_frontend_create(ctypes.byref(base), ctypes.byref(h)))
    assert lib.kws_frontend_linear_size(h) == 201
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        rc, msg = linear(h, args[0], 2, 1600, *args[1:])
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "null pointer" in msg, msg
    rc, msg = linear(h, p, 2, 399, p, p, p)
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "n_max=399" in msg and "no frame" in msg, msg
    for name in ("spec", "frames", "energy", "noise_spec", "noise_frames", "noise_energy"):
        rc, msg = augment(h, null=name)
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "null pointer" in msg and "noise set" in msg, (name, msg)
    for name in ("src", "noise", "start", "gain_db", "out"):
        rc, msg = augment(h, null=name)
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "null pointer" in msg and "gain_db" in msg, (name, msg)
    lib.kws_frontend_destroy(h)
    small = _lib.KwsFrontendConfig(16000, 256, 128, 40, 300.0, 8000.0)
    _lib.check(lib.kws_frontend_create(ctypes.byref(small), ctypes.byref(h)))
    assert lib.kws_frontend_linear_size(h) == _lib.KWS_ERR_UNSUPPORTED and b"fft_size=256" in lib.kws_last_error()
    rc, msg = linear(h, p, 2, 1600, p, p, p)
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "fft_size=256" in msg and "kws_frontend_run_linear" in msg, msg
    rc, msg = augment(h)
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "fft_size=256" in msg and "kws_frontend_augment" in msg, msg
    lib.kws_frontend_destroy(h)


def _augmenter(**kw):
    from keyword_spotting_amd.custom_keyword import NoiseAugmenter
    return NoiseAugmenter(**kw)


def test_augmenter_defaults_are_the_shipped_config():
    a = _augmenter()
    assert (a.bg_noise_prob, a.bg_decay_min_db, a.bg_decay_max_db, a.max_sequence_length, a.per_row) == (0.5, -15.0, -5.0, 2000, False)


@pytest.mark.parametrize("per_row", [False, True])
def test_augmenter_draws(per_row):
    rows, n_noise, T = 7, 3, 34
    a, b, c = (_augmenter(seed=s, per_row=per_row) for s in (11, 11, 12))
    seen_on, seen_off, differs = False, False, False
    for _ in range(40):
        da, db, dc = a.draw(rows, n_noise, T), b.draw(rows, n_noise, T), c.draw(rows, n_noise, T)
        assert all(np.array_equal(x, y) for x, y in zip(da, db))                  # the same seed: the same draws
        differs = differs or not all(np.array_equal(x, y) for x, y in zip(da, dc))
        src, noise, start, gain = da
        assert [x.dtype for x in da] == [np.int32, np.int32, np.int32, np.float32] and all(x.shape == (rows,) for x in da)
        assert np.array_equal(src, np.arange(rows))
        assert (start >= 0).all() and (start < 2000 - T).all()
        assert (gain >= -15.0).all() and (gain < -5.0).all()
        on = noise >= 0
        assert np.array_equal(noise[on], (np.arange(rows) % n_noise)[on]) and (noise[~on] == -1).all()
        if not per_row:                        # one decay, one start, one flag per batch (reader.py:229-253)
            assert len(set(start)) == 1 and len(set(gain)) == 1 and (on.all() or not on.any())
        seen_on, seen_off = seen_on or on.any(), seen_off or not on.all()
    assert differs and seen_on and seen_off
    if per_row:
        assert len(set(a.draw(64, n_noise, T)[2])) > 1 and len(set(a.draw(64, n_noise, T)[3])) > 1


def test_augmenter_probability_bounds_and_refusals():
    from keyword_spotting_amd import _lib
    for per_row in (False, True):
        off, on = _augmenter(bg_noise_prob=0.0, per_row=per_row, seed=2), _augmenter(bg_noise_prob=1.0, per_row=per_row, seed=2)
        for _ in range(20):
            assert (off.draw(5, 2, 10)[1] == -1).all()
            assert np.array_equal(on.draw(5, 2, 10)[1], np.arange(5) % 2)
    a = _augmenter(max_sequence_length=100)
    assert (a.draw(3, 1, 99)[2] == 0).all()                     # the one start there is
    for T in (100, 101, 5000):
        with pytest.raises(_lib.InvalidArgumentError, match="max_sequence_length"):
            a.draw(3, 1, T)
    with pytest.raises(_lib.InvalidArgumentError):
        a.draw(0, 1, 10)
    with pytest.raises(_lib.InvalidArgumentError):
        a.draw(3, 0, 10)
    with pytest.raises(_lib.InvalidArgumentError):
        _augmenter(bg_noise_prob=1.5)
    with pytest.raises(_lib.InvalidArgumentError):
        _augmenter(bg_decay_min_db=-5, bg_decay_max_db=-15)
