"""The dataset front-end's kernels (kws_frontend_create_dataset / kws_frontend_run_lengths; the DatasetFrames instantiations of
csrc/fft_frontend.hip) against the fp64 restatement tests/dataset_model.py, which tests/test_dataset_host.py pins to scipy and
transformers: every epilogue at both tile counts with and without pre-emphasis, the per-utterance lengths, the delta edges, the
window, the identity of {feat, KWS_FRAMES_DEPLOY, 0} with kws_frontend_create_features, the refusals, and the RNN DeployModel fed
from PCM.

Bounds (dataset_model.tolerance; no constant of their own): mel of |X| 2e-5 of the largest value as tests/test_gpu_frontend.py, of
|X|^2 twice that as tests/test_gpu_mfcc.py, MFCC max(4 x float32-CPU deviation, DCT floor) per case as mfcc_model.tolerance.  Every
case prints kernel error / bound (DATASET-RATIO, DATASET-E2E) for DESIGN.md section 9, which has no figures yet: these tests had not
run on an MI355X when they were written."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dataset_model as D

pytestmark = pytest.mark.gpu

PRE = (0.0, 0.97)
KINDS = [("mel", 0), ("power", 0), ("mfcc", None)]        # n_mfcc None: 13 on the 40-filter bank, 20 on the 60-filter one
N_MFCC = {40: 13, 60: 20}


def _config(kind, n_mel, n_mfcc=0, **kw):
    from keyword_spotting_amd.config import get_attention_config
    return get_attention_config(n_mel=n_mel, mfcc=kind == "mfcc", power=2 if kind == "power" else 1, n_mfcc=n_mfcc or 20, **kw)


def _fe(kind, n_mel, n_mfcc=0, pre=0.0, **kw):
    from keyword_spotting_amd.frontend import DatasetFrontend
    return DatasetFrontend(_config(kind, n_mel, n_mfcc, **kw), pre_emphasis=pre)


@functools.lru_cache(maxsize=None)
def _signals():
    """The smallest utterances that take each path: two frames that reflect on both sides; a hop boundary (three frames, each
    an edge); 23 frames (interior waves, a second 16-frame block); a quiet one (the dB range of the MFCC bound); silence."""
    rng = np.random.default_rng(41)
    return (("noise_201", (rng.standard_normal(201) * 0.1).astype(np.float32)),
            ("noise_360", (rng.standard_normal(360) * 0.1).astype(np.float32)),
            ("noise_3600", (rng.standard_normal(3600) * 0.1).astype(np.float32)),
            ("noise_1e-4_3600", (rng.standard_normal(3600) * 1e-4).astype(np.float32)),
            ("zeros_3600", np.zeros(3600, np.float32)))


@functools.lru_cache(maxsize=None)
def _reference(name, kind, n_mel, n_mfcc, pre):
    """(restatement, bound) of one signal, computed once for every test that asks."""
    pcm = dict(_signals())[name]
    want, tol = D.features(pcm, kind, n_mel, n_mfcc, pre), D.tolerance(pcm, kind, n_mel, n_mfcc, pre)
    want.setflags(write=False)
    return want, tol


def _check(tag, got, want, tol):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not want.size:
        return
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("DATASET-RATIO %s: kernel %.3e  bound %.3e  kernel/bound %s" % (tag, err, tol, "%.3f" % (err / tol) if tol else "-"))
    assert err <= tol, (tag, err, tol)


@pytest.mark.parametrize("pre", PRE)
@pytest.mark.parametrize("kind,n_mfcc", KINDS)
@pytest.mark.parametrize("n_mel", [40, 60])
def test_features_match_the_restatement(n_mel, kind, n_mfcc, pre):
    n_mfcc = N_MFCC[n_mel] if n_mfcc is None else n_mfcc
    fe = _fe(kind, n_mel, n_mfcc, pre)
    assert fe.feature_size == (3 * n_mfcc if kind == "mfcc" else n_mel)
    for name, pcm in _signals():
        got = fe.forward(torch.from_numpy(pcm)).cpu().numpy()
        assert got.shape[0] == fe.num_frames(pcm.shape[0]) == 1 + pcm.shape[0] // 160
        want, tol = _reference(name, kind, n_mel, n_mfcc, pre)
        _check("%s %s n_mel=%d pre=%g" % (name, kind, n_mel, pre), got, want, tol)
        if name == "zeros_3600" and kind != "mfcc":
            assert not got.any()
    fe.close()


N_MAX = 1600
LENS = [200, 201, 559, 560, 1234, N_MAX]      # no frames; both-sided reflection; left- and right-edge frames sharing taps; the longest row


def _ragged(seed):
    rng = np.random.default_rng(seed)
    pcm = np.full((len(LENS), N_MAX), np.nan, np.float32)           # whatever lies past n_b is never read into a result
    for b, n in enumerate(LENS):
        pcm[b, :n] = rng.standard_normal(n) * (0.05 + 0.02 * b)
    return pcm


@pytest.mark.parametrize("kind,n_mel,n_mfcc,pre", [("mel", 40, 0, 0.97), ("power", 60, 0, 0.0), ("mfcc", 60, 20, 0.97), ("mfcc", 40, 13, 0.0)])
def test_every_utterance_has_its_own_length(kind, n_mel, n_mfcc, pre):
    fe = _fe(kind, n_mel, n_mfcc, pre)
    pcm = _ragged(7)
    lens = torch.tensor(LENS, dtype=torch.int32)
    whole = fe.forward(torch.from_numpy(pcm), lens)
    again = fe.forward(torch.from_numpy(pcm), lens)
    assert whole.shape == (len(LENS), 1 + N_MAX // 160, fe.feature_size)
    assert torch.equal(whole, again) and not torch.isnan(whole).any()
    assert [fe.num_frames(n) for n in (0, 200, 201, 319, 320)] == [0, 0, 2, 2, 3]
    for b, n in enumerate(LENS):
        tb = fe.num_frames(n)
        assert tb == D.num_frames(n)
        assert not whole[b, tb:].any(), (b, n)                      # rows past T(n_b) are written as 0; the n = 200 utterance is all zeros
        alone = fe.forward(torch.from_numpy(pcm[b, :n].copy()))     # its own rows, its own grid
        assert alone.shape == (tb, fe.feature_size)
        assert torch.equal(alone, whole[b, :tb]), (b, n)
        if tb:
            _check("utt%d(n=%d) %s n_mel=%d pre=%g" % (b, n, kind, n_mel, pre), whole[b, :tb].cpu().numpy(),
                   D.features(pcm[b, :n], kind, n_mel, n_mfcc, pre), D.tolerance(pcm[b, :n], kind, n_mel, n_mfcc, pre))
    # no lengths: every row is n_max samples long
    clean = np.nan_to_num(pcm[-2:], nan=0.01)
    full = fe.forward(torch.from_numpy(clean))
    for b in range(2):
        _check("full%d %s" % (b, kind), full[b].cpu().numpy(), D.features(clean[b], kind, n_mel, n_mfcc, pre),
               D.tolerance(clean[b], kind, n_mel, n_mfcc, pre))
    fe.close()


@pytest.mark.parametrize("pre", PRE)
def test_mfcc_delta_edges_are_the_utterances_own(pre):
    """d[t] = c[min(t + 1, T_b - 1)] - c[max(t - 1, 0)] with T_b = 1 + n_b // hop: T = 2, T = 3 and longer ones side by side in one
    batch, and T = 1 (a hop longer than the utterance): zero deltas."""
    n_mfcc = 13
    fe = _fe("mfcc", 40, n_mfcc, pre)
    lens = [250, 320, 479, 480, 1000, 201]
    rng = np.random.default_rng(9)
    pcm = np.full((len(lens), 1000), np.nan, np.float32)
    for b, n in enumerate(lens):
        pcm[b, :n] = rng.standard_normal(n) * 0.1
    got = fe.forward(torch.from_numpy(pcm), torch.tensor(lens, dtype=torch.int32)).cpu().numpy()
    two = np.float32(2)
    for b, n in enumerate(lens):
        tb = 1 + n // 160
        c, d1, d2 = got[b, :tb, :n_mfcc], got[b, :tb, n_mfcc:2 * n_mfcc], got[b, :tb, 2 * n_mfcc:]
        d = c[np.minimum(np.arange(tb) + 1, tb - 1)] - c[np.maximum(np.arange(tb) - 1, 0)]
        assert np.array_equal(d1, d / two) and np.array_equal(d2, (d + two * d) / np.float32(10)), (b, n)
        assert np.array_equal(d1[-1], (c[-1] - c[-2]) / two) and np.array_equal(d1[0], (c[1] - c[0]) / two)
        assert not got[b, tb:].any()
        _check("delta utt%d(n=%d,T=%d) pre=%g" % (b, n, tb, pre), got[b, :tb], D.features(pcm[b, :n], "mfcc", 40, n_mfcc, pre),
               D.tolerance(pcm[b, :n], "mfcc", 40, n_mfcc, pre))
    fe.close()
    one = _fe("mfcc", 40, n_mfcc, pre, hop_size=512)                # T(300) = 1 + 300 // 512 = 1
    assert one.num_frames(300) == 1
    row = one.forward(torch.from_numpy(pcm[4, :300].copy())).cpu().numpy()
    assert row.shape == (1, 3 * n_mfcc) and not row[0, n_mfcc:].any()
    want = D.features(pcm[4, :300], "mfcc", 40, n_mfcc, pre)[:1, :n_mfcc]           # frame 0 does not depend on the hop
    assert np.abs(row[0, :n_mfcc] - want[0]).max() <= D.tolerance(pcm[4, :300], "mfcc", 40, n_mfcc, pre)
    one.close()


def _raw(lib, create, cfg):
    h = ctypes.c_void_p()
    return h, getattr(lib, create)(ctypes.byref(cfg), ctypes.byref(h))


def _feature_config(kind=0, power=1, n_mfcc=0, n_mel=40):
    from keyword_spotting_amd import _lib
    return _lib.KwsFeatureConfig(_lib.KwsFrontendConfig(16000, 400, 160, n_mel, 300.0, 8000.0), kind, power, n_mfcc)


def test_window_is_scipys_periodic_hann():
    import scipy.signal
    fe = _fe("mel", 40)
    w = fe.window()
    assert w.shape == (400,) and w.dtype == np.float32
    assert np.abs(w.astype(np.float64) - scipy.signal.get_window("hann", 400, fftbins=True)).max() <= 2.0 ** -24 * 1.01
    fe.close()


@pytest.mark.parametrize("kind,power,n_mfcc", [(0, 1, 0), (0, 2, 0), (1, 2, 13)])
def test_deploy_framing_is_create_features_bit_for_bit(kind, power, n_mfcc):
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    feat = _feature_config(kind, power, n_mfcc)
    hd, rc = _raw(lib, "kws_frontend_create_dataset", _lib.KwsDatasetConfig(feat, _lib.FRAMES_DEPLOY, 0.0))
    _lib.check(rc)
    hf, rc = _raw(lib, "kws_frontend_create_features", feat)
    _lib.check(rc)
    width = lib.kws_frontend_feature_size(hf)
    assert lib.kws_frontend_feature_size(hd) == width
    for n in (0, 399, 400, 3600):
        assert lib.kws_frontend_frames_of(hd, n) == lib.kws_frontend_frames_of(hf, n) == lib.kws_frontend_frames(ctypes.byref(feat.base), n)
    x = torch.from_numpy((np.random.default_rng(3).standard_normal((3, 3600)) * 0.1).astype(np.float32)).cuda()
    lens = torch.tensor([3600, 400, 1999], dtype=torch.int32, device="cuda")
    a, b = torch.full((3, 21, width), float("nan"), device="cuda"), torch.full((3, 21, width), float("nan"), device="cuda")
    _lib.check(lib.kws_frontend_run(hd, _lib.ptr(x), 3, 3600, _lib.ptr(a), _lib.current_stream_ptr()))
    _lib.check(lib.kws_frontend_run(hf, _lib.ptr(x), 3, 3600, _lib.ptr(b), _lib.current_stream_ptr()))
    assert torch.equal(a, b)
    _lib.check(lib.kws_frontend_run_lengths(hd, _lib.ptr(x), _lib.ptr(lens), 3, 3600, _lib.ptr(a), _lib.current_stream_ptr()))
    _lib.check(lib.kws_frontend_run_lengths(hf, _lib.ptr(x), _lib.ptr(lens), 3, 3600, _lib.ptr(b), _lib.current_stream_ptr()))
    assert torch.equal(a, b)
    buf = np.zeros(400, np.float32)
    assert lib.kws_frontend_window(hd, buf.ctypes.data_as(ctypes.c_void_p)) == _lib.KWS_ERR_INVALID_ARGUMENT      # no window on deploy frames
    torch.cuda.synchronize()
    lib.kws_frontend_destroy(hd)
    lib.kws_frontend_destroy(hf)


def test_run_on_a_dataset_handle_is_run_lengths_without_lengths():
    from keyword_spotting_amd import _lib
    fe = _fe("mel", 40, pre=0.97)
    x = torch.from_numpy(np.stack([dict(_signals())["noise_3600"]] * 2)).cuda()
    a, b = torch.empty(2, 23, 40, device="cuda"), torch.empty(2, 23, 40, device="cuda")
    _lib.check(fe._lib.kws_frontend_run(fe._handle, _lib.ptr(x), 2, 3600, _lib.ptr(a), _lib.current_stream_ptr()))
    _lib.check(fe._lib.kws_frontend_run_lengths(fe._handle, _lib.ptr(x), None, 2, 3600, _lib.ptr(b), _lib.current_stream_ptr()))
    assert torch.equal(a, b) and torch.equal(a[0], a[1])
    fe.close()


def test_refusals(monkeypatch):
    from keyword_spotting_amd import _lib, get_config, weights
    from keyword_spotting_amd.rnn_ctc import DeployModel as RnnModel
    lib = _lib.load()
    for feat in (_feature_config(), _feature_config(1, 2, 13)):
        h, rc = _raw(lib, "kws_frontend_create_dataset", _lib.KwsDatasetConfig(feat, _lib.FRAMES_DATASET, 0.0))
        _lib.check(rc)
        x, out = torch.zeros(2, 800, device="cuda"), torch.zeros(2, 6, 64, device="cuda")
        rc = lib.kws_frontend_run_carry(h, None, 0, _lib.ptr(x), 800, 2, _lib.ptr(out), None, 0, None)
        assert rc == _lib.KWS_ERR_UNSUPPORTED and b"KWS_FRAMES_DATASET" in lib.kws_last_error() and b"utterance's end" in lib.kws_last_error()
        cfg = get_config()
        model = RnnModel(cfg, weights.init_weights(cfg, seed=0))
        win = ctypes.c_void_p()
        _lib.check(lib.kws_window_create(2, 15, 32, 6, 0.4, ctypes.byref(win)))
        state, restart = torch.zeros(2, 2, 128, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda")
        s = ctypes.c_void_p()
        rc = lib.kws_stream_create(model._handle, h, win, 2, 3600, 30.0, b"1233", _lib.ptr(state), _lib.ptr(restart), ctypes.byref(s))
        assert rc == _lib.KWS_ERR_UNSUPPORTED and not s.value and b"utterance's end" in lib.kws_last_error()
        lib.kws_window_destroy(win)
        lib.kws_frontend_destroy(h)
        model.close()
    # a handle whose launches would go to the dense-DFT kernel cannot frame the dataset's way (the switch is read at create)
    monkeypatch.setenv("KWS_FRONTEND_DENSE", "1")
    h, rc = _raw(lib, "kws_frontend_create_dataset", _lib.KwsDatasetConfig(_feature_config(), _lib.FRAMES_DATASET, 0.0))
    assert rc == _lib.KWS_ERR_UNSUPPORTED and not h.value and b"KWS_FRONTEND_DENSE=1" in lib.kws_last_error()
    h, rc = _raw(lib, "kws_frontend_create_dataset", _lib.KwsDatasetConfig(_feature_config(), _lib.FRAMES_DEPLOY, 0.0))
    _lib.check(rc)                                                   # ... while deploy frames still take it
    lib.kws_frontend_destroy(h)
    monkeypatch.delenv("KWS_FRONTEND_DENSE")
    torch.cuda.synchronize()


def test_rnn_deploy_model_on_dataset_features_end_to_end():
    """PCM -> DatasetFrontend -> the GRU kernels (the DeployModel's mel-input form) -> softmax, against oracle.gru_oracle fed the
    restatement's features, within the parity bounds of tests/test_gpu_parity.py (logits and state 1e-4, softmax 2e-5)."""
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.frontend import DatasetFrontend
    from keyword_spotting_amd.rnn_ctc import DeployModel
    from oracle import gru_oracle as G
    cfg = get_config()
    w = weights.init_weights(cfg, seed=0)
    model, fe = DeployModel(cfg, w), DatasetFrontend(cfg, pre_emphasis=0.97)
    pcm = (np.random.default_rng(12).standard_normal((2, 16000)) * 0.1).astype(np.float32)
    mel = fe.forward(torch.from_numpy(pcm))
    assert mel.shape == (2, 101, cfg.n_mel)
    r = model.forward(mel, model.zero_state(2))
    want_mel = np.stack([D.features(p, "mel", cfg.n_mel, pre=0.97) for p in pcm])
    want_l, want_s = G.gru_forward(w, want_mel, dtype=np.float64)
    err_l = np.abs(r["logits"].cpu().numpy() - want_l).max()
    err_s = np.abs(r["state"].cpu().numpy() - want_s).max()
    err_sm = np.abs(r["softmax"].cpu().numpy() - G.softmax(want_l)).max()
    print("DATASET-E2E logits %.3e  state %.3e  softmax %.3e" % (err_l, err_s, err_sm))
    assert err_l < 1e-4 and err_s < 1e-4 and err_sm < 2e-5
    fe.close()
    model.close()
