"""The MFCC feature kernels (kws_frontend_create_features / kws_frontend_run_lengths; csrc/fft_frontend.hip) against the fp64
restatement of utils/mfcc.py (tests/mfcc_model.py), the third-party pin of the static coefficients, their per-utterance length
handling, and the attention DeployModel served from PCM with config.mfcc.

Tolerance (tests/mfcc_model.py:tolerance): the error of S = 10 log10(m) is 4.34 dm/m, so it follows the signal's dynamic range
and no constant fits every signal.  Per case the bound is 4 x the deviation of a float32 CPU evaluation of the same formula from
the restatement -- computed from the restatement, never from the kernel -- with the floor n_mel * max|S| * 2^-23 * max|D|.  Every
case prints kernel error / bound; DESIGN.md section 9 records them."""
import ctypes

import numpy as np
import pytest
import torch

import attention_model as AM
import mfcc_model as M
from conftest import ROOT
from oracle import frontend_oracle as F

pytestmark = pytest.mark.gpu

SHAPES = [(n_mel, n_mfcc) for n_mel in (13, 40, 60, 64) for n_mfcc in (1, 13, 20, 32) if n_mfcc <= n_mel]
GOLDEN_CASES = ("noise_3600", "noise_loud_3840", "tone_8000", "chirp_8000", "int16_like_3600", "exact_400", "short_559")


def _cfg(**kw):
    from keyword_spotting_amd.config import get_attention_config
    return get_attention_config(mfcc=True, **kw)


def _fe(n_mel, n_mfcc):
    from keyword_spotting_amd.frontend import MfccFrontend
    return MfccFrontend(_cfg(n_mel=n_mel, n_mfcc=n_mfcc))


def _golden():
    import os
    return (np.load(os.path.join(ROOT, "tests", "golden", "frontend_golden.npz")),
            np.load(os.path.join(ROOT, "tests", "golden", "mfcc_golden.npz")))


def _signals():
    src, _ = _golden()
    sig = {name: src["pcm_" + name] for name in GOLDEN_CASES}
    rng = np.random.default_rng(77)
    sig["noise_1e-4_3600"] = (rng.standard_normal(3600) * 1e-4).astype(np.float32)
    sig["zeros_3600"] = np.zeros(3600, np.float32)
    sig["noise_300_frames"] = (rng.standard_normal(400 + 160 * 299) * 0.1).astype(np.float32)
    t = np.arange(400 + 160 * 299) / 16000.0
    sig["speechlike_300_frames"] = (0.3 * np.sin(2 * np.pi * (200.0 + 150.0 * np.sin(2 * np.pi * 3.0 * t)) * t) * (0.55 + 0.45 * np.sin(2 * np.pi * 2.0 * t))
                                    + 0.01 * rng.standard_normal(t.size)).astype(np.float32)
    return sig


def _check(tag, got, pcm, n_mel, n_mfcc):
    want = M.mfcc(pcm, n_mel, n_mfcc)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    if not want.size:
        return 0.0
    tol, dev, floor = M.tolerance(pcm, n_mel, n_mfcc)
    err = float(np.abs(got - want).max())
    print("MFCC-RATIO %s n_mel=%d n_mfcc=%d: kernel %.3e  float32-CPU %.3e  floor %.3e  bound %.3e  kernel/bound %.3f"
          % (tag, n_mel, n_mfcc, err, dev, floor, tol, err / tol))
    assert err <= tol, (tag, n_mel, n_mfcc, err, tol)
    return err / tol


@pytest.mark.parametrize("n_mel,n_mfcc", SHAPES)
def test_features_match_the_restatement(n_mel, n_mfcc):
    fe = _fe(n_mel, n_mfcc)
    assert fe.feature_size == 3 * n_mfcc
    for name, pcm in _signals().items():
        got = fe.forward(torch.from_numpy(pcm)).cpu().numpy().astype(np.float64)
        assert got.shape[0] == fe.num_frames(pcm.shape[0])
        _check(name, got, pcm, n_mel, n_mfcc)
    fe.close()


@pytest.mark.parametrize("n_mel,n_mfcc", [(60, 20), (40, 13)])
def test_bases_are_the_float32_constants_of_the_graph(n_mel, n_mfcc):
    fe = _fe(n_mel, n_mfcc)
    d = fe.dct_basis()
    assert d.shape == (n_mel, n_mfcc) and d.dtype == np.float32
    import scipy.fft
    # the library's basis is scipy's orthonormal DCT-II (columns of the transform of the identity) rounded to float32 ...
    ortho = scipy.fft.dct(np.eye(n_mel), type=2, norm="ortho", axis=-1)[:, :n_mfcc]
    assert np.abs(d.astype(np.float64) - ortho).max() <= 2.0 ** -24 * np.abs(ortho).max() * 1.01
    # ... and of the restatement's; the cosine of two libms may differ in the last place of the double
    assert np.abs(d.astype(np.float64) - M.dct(n_mfcc, n_mel)).max() <= 2.0 ** -24 * np.abs(M.dct(n_mfcc, n_mel)).max() * 1.01
    np.testing.assert_allclose(fe.mel_basis(), F.mel_basis(16000, 400, n_mel, 300.0, 8000.0), rtol=2e-6, atol=1e-9)
    fe.close()


@pytest.mark.parametrize("n_mel,n_mfcc", [(60, 20), (40, 13)])
def test_static_columns_match_the_third_party_pin(n_mel, n_mfcc):
    src, g = _golden()
    fe = _fe(n_mel, n_mfcc)
    for name in GOLDEN_CASES:
        pcm = src["pcm_" + name]
        got = fe.forward(torch.from_numpy(pcm)).cpu().numpy().astype(np.float64)[:, :n_mfcc]
        want = g["mfcc%d_%d_%s" % (n_mel, n_mfcc, name)]
        tol = M.tolerance(pcm, n_mel, n_mfcc)[0] + 1e-5          # + the pin's own distance from the restatement (tests/test_mfcc_host.py)
        err = np.abs(got - want).max()
        print("MFCC-PIN %s n_mel=%d n_mfcc=%d: %.3e (bound %.3e)" % (name, n_mel, n_mfcc, err, tol))
        assert err <= tol, (name, err, tol)
    fe.close()


def _power_handle(n_mel, power, kind=0, n_mfcc=0, fft=400):
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    cfg = _lib.KwsFeatureConfig(_lib.KwsFrontendConfig(16000, fft, 160, n_mel, 300.0, 8000.0), kind, power, n_mfcc)
    h = ctypes.c_void_p()
    rc = lib.kws_frontend_create_features(ctypes.byref(cfg), ctypes.byref(h))
    return lib, h, rc


@pytest.mark.parametrize("n_mel,batch,n", [(40, 3, 3600), (60, 2, 4000), (40, 1, 400), (13, 2, 8000), (64, 5, 16000)])
def test_power_two_mel_matches_the_oracle_squared(n_mel, batch, n):
    """reader.py:267-268: |rfft|^2 through the same mel bank.  Bound: twice the relative bound of the magnitude front-end
    (tests/test_gpu_frontend.py: 2e-5 of the largest value), since d(x^2) / x^2 = 2 dx / x."""
    from keyword_spotting_amd import _lib
    lib, h, rc = _power_handle(n_mel, 2)
    _lib.check(rc)
    assert lib.kws_frontend_feature_size(h) == n_mel
    pcm = (np.random.default_rng(300 + n).standard_normal((batch, n)) * 0.1).astype(np.float32)
    x = torch.from_numpy(pcm).cuda()
    t = 1 + (n - 400) // 160
    out = torch.full((batch, t, n_mel), float("nan"), device="cuda")
    _lib.check(lib.kws_frontend_run(h, _lib.ptr(x), batch, n, _lib.ptr(out), _lib.current_stream_ptr()))
    P = np.abs(np.fft.rfft(F.frames(pcm.astype(np.float64)), 400, axis=-1)) ** 2
    want = P @ F.mel_basis(16000, 400, n_mel, 300.0, 8000.0).astype(np.float32).astype(np.float64).T
    got = out.cpu().numpy()
    err, scale = np.abs(got - want).max(), np.abs(want).max()
    print("POWER2 n_mel=%d: %.3e of %.3e" % (n_mel, err, scale))
    assert err < 4e-5 * scale
    # ... and power 1 through the lengths entry point is the magnitude front-end, bit for bit
    lib1, h1, rc1 = _power_handle(n_mel, 1)
    _lib.check(rc1)
    a, b = torch.empty_like(out), torch.empty_like(out)
    _lib.check(lib.kws_frontend_run(h1, _lib.ptr(x), batch, n, _lib.ptr(a), _lib.current_stream_ptr()))
    _lib.check(lib.kws_frontend_run_lengths(h1, _lib.ptr(x), None, batch, n, _lib.ptr(b), _lib.current_stream_ptr()))
    assert torch.equal(a, b)
    lib.kws_frontend_destroy(h)
    lib.kws_frontend_destroy(h1)


def _ragged_batch(n_max, lens, seed, pad=0.0):
    rng = np.random.default_rng(seed)
    pcm = np.full((len(lens), n_max), pad, np.float32)
    for b, n in enumerate(lens):
        n = min(max(n, 0), n_max)
        pcm[b, :n] = rng.standard_normal(n) * (0.02 + 0.01 * b)
    return pcm


# 33 utterances in rows of 45 frames: the lengths the issue names, frame counts on both sides of the 16-frame blocks of the
# flattened [B * T_max] index (utterance b starts at frame 45 b: every residue mod 16 occurs), out-of-range lengths (clamped)
N_MAX = 400 + 160 * 44
LENS33 = [0, 399, 400, 559, 560, 720, N_MAX] + [400 + 160 * (t - 1) + r for t, r in
          ((15, 0), (16, 0), (17, 159), (31, 0), (32, 1), (33, 0), (2, 0), (3, 80), (44, 0), (45, 0), (1, 159), (7, 0), (8, 0), (9, 0),
           (24, 0), (40, 0), (12, 5), (20, 0), (28, 0), (36, 0), (5, 0), (43, 159))] + [-5, N_MAX + 1000, 1, 6000]
assert len(LENS33) == 33


@pytest.mark.parametrize("n_mel,n_mfcc", [(60, 20), (40, 13), (64, 32)])
def test_every_utterance_has_its_own_length(n_mel, n_mfcc):
    fe = _fe(n_mel, n_mfcc)
    pcm = _ragged_batch(N_MAX, LENS33, 5, pad=float("nan"))           # whatever lies past n_b is never read into a result
    got = fe.forward(torch.from_numpy(pcm), torch.tensor(LENS33, dtype=torch.int32)).cpu().numpy().astype(np.float64)
    assert got.shape == (33, 45, 3 * n_mfcc)
    for b, n in enumerate(LENS33):
        n = min(max(n, 0), N_MAX)
        tb = fe.num_frames(n)
        assert not got[b, tb:].any(), (b, n)                           # rows past T_b are written as 0 (NaN would show here)
        _check("utt%d(n=%d,T=%d)" % (b, n, tb), got[b, :tb], pcm[b, :n], n_mel, n_mfcc)
        if tb > 1:       # the right-hand delta edge is the utterance's own last frame
            assert np.array_equal(got[b, tb - 1, n_mfcc:2 * n_mfcc], (got[b, tb - 1, :n_mfcc] - got[b, tb - 2, :n_mfcc]).astype(np.float32) / np.float32(2))
        if tb == 1:
            assert not got[b, 0, n_mfcc:].any()
    # no lengths: every row is n_max samples long (NaN-free input)
    clean = _ragged_batch(N_MAX, [N_MAX] * 3, 6)
    full = fe.forward(torch.from_numpy(clean)).cpu().numpy().astype(np.float64)
    for b in range(3):
        _check("full%d" % b, full[b], clean[b], n_mel, n_mfcc)
    fe.close()


def test_an_utterance_alone_equals_it_among_33_others_and_repeats_bitwise():
    fe = _fe(60, 20)
    pcm = _ragged_batch(N_MAX, LENS33, 9, pad=float("nan"))
    lens = torch.tensor(LENS33, dtype=torch.int32)
    whole = fe.forward(torch.from_numpy(pcm), lens)
    again = fe.forward(torch.from_numpy(pcm), lens)
    assert torch.equal(whole, again)                                   # (NaN-free: every row past T_b is 0)
    assert not torch.isnan(whole).any()
    for b, n in enumerate(LENS33):
        n = min(max(n, 0), N_MAX)
        alone = fe.forward(torch.from_numpy(pcm[b, :n].copy()))        # its own T_b rows, its own grid
        tb = fe.num_frames(n)
        assert alone.shape == (tb, 60)
        assert torch.equal(alone, whole[b, :tb]), (b, n)
    # another stream, another neighbourhood: the same bits again
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        third = fe.forward(torch.from_numpy(pcm[5:12].copy()), lens[5:12])
    other.synchronize()
    assert torch.equal(third, whole[5:12])
    fe.close()


def _model(cfg, seed):
    from keyword_spotting_amd import attention_weights as AW
    from keyword_spotting_amd.attention_ctc import DeployModel
    w = AW.init(cfg, seed)
    return w, DeployModel(cfg, w)


def test_deploy_model_run_is_the_front_end_followed_by_forward():
    from keyword_spotting_amd.attention_ctc import FETCH_LENGTHS, FETCH_LOGIT, FETCH_SOFTMAX
    from keyword_spotting_amd.frontend import MfccFrontend
    cfg = _cfg()
    w, m = _model(cfg, 21)
    assert isinstance(m.frontend, MfccFrontend)
    rng = np.random.default_rng(22)
    pcms = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n in (16000, 5000, 399, 400, 7777)]
    sm, lg, n = m.run([FETCH_SOFTMAX, FETCH_LOGIT, FETCH_LENGTHS], {"model/inputX:0": pcms})
    fe = MfccFrontend(cfg)
    n_max = max(p.shape[0] for p in pcms)
    batch = torch.zeros(len(pcms), n_max)
    for b, p in enumerate(pcms):
        batch[b, :p.shape[0]] = torch.from_numpy(p)
    feats = fe.forward(batch, torch.tensor([p.shape[0] for p in pcms], dtype=torch.int32))
    frames = torch.tensor([fe.num_frames(p.shape[0]) for p in pcms], dtype=torch.int32)
    r = m.forward(feats, frames)
    assert torch.equal(sm, r["softmax"]) and torch.equal(lg, r["logits"]) and torch.equal(n.cpu(), r["lengths_out"].cpu())
    # the zero-padded tail does not enter an utterance's last delta: each utterance alone gives the same rows
    for b, p in enumerate(pcms):
        one = m.run(FETCH_SOFTMAX, {"model/inputX:0": p})
        assert torch.equal(one[0], sm[b, :one.shape[1]]), b
    with pytest.raises(Exception):
        m.forward(torch.zeros(1, 10, cfg.n_mel + 1))
    fe.close()
    m.close()


@pytest.mark.parametrize("kw", [dict(), dict(n_mel=40, n_mfcc=13)])
def test_deploy_model_run_matches_the_restatements_end_to_end(kw):
    """PCM -> MFCC kernels -> attention kernels against tests/attention_model.py fed tests/mfcc_model.py's features.  The bound is
    derived as for the features: the float32 CPU features and the fp64 features both through the fp64 attention model, x 4, and
    as there never less than the rounding of the last product's own sum -- H * max|x| * 2^-23 * max|W_out| for the logits (x: the
    last layer norm's output, from the restatement; 7e-6 .. 1.1e-5), half of that for the softmax (its slope is at most 1/2 in the
    max norm).  The floor is what the attention kernels' own fp32 arithmetic needs, which the propagated deviation does not see
    (they agree with a torch-eager fp32 build to 2.4e-6 / 6.6e-7).  Measured against 4 x the deviation ALONE:
    n_mel 60: 0.09 .. 0.31 (logits) / 0.04 .. 0.43 (softmax) on the T' > 1 utterances; the one-row utterance (T' = 1, whose layer norm
    cancels a feature perturbation almost entirely) 4.1e-7 / 1.2e-7 against 2.2e-7 / 5.3e-8 = 1.9 x / 2.2 x.  n_mel 40: 0.01 .. 0.97
    (logits) / 0.01 .. 0.95 (softmax), and the 1-second noise utterance 5.31e-7 against 5.24e-7 = 1.012 x in the softmax.  The two
    cases over 1 x are 9 ulp or less of the outputs; with the floor the kernels use at most 0.61 of a bound."""
    from keyword_spotting_amd.attention_ctc import FETCH_LOGIT, FETCH_SOFTMAX
    cfg = _cfg(**kw)
    w, m = _model(cfg, 31)
    src, _ = _golden()
    rng = np.random.default_rng(32)
    pcms = [src["pcm_noise_3600"], src["pcm_tone_8000"], src["pcm_chirp_8000"], rng.uniform(-0.5, 0.5, 16000).astype(np.float32),
            src["pcm_exact_400"]]
    sm, lg = m.run([FETCH_SOFTMAX, FETCH_LOGIT], {"model/inputX:0": [torch.from_numpy(p) for p in pcms]})
    sm, lg = sm.cpu().numpy().astype(np.float64), lg.cpu().numpy().astype(np.float64)
    for b, p in enumerate(pcms):
        seen = []

        def ln(x, gamma, beta):
            seen.append(AM.layer_norm(x, gamma, beta))
            return seen[-1]

        want_l, want_s = AM.forward(cfg, w, M.mfcc(p, cfg.n_mel, cfg.n_mfcc), ln=ln)
        floor_l = cfg.hidden_size * np.abs(seen[-1]).max() * 2.0 ** -23 * np.abs(w["W_out"]).max()
        f32_l, f32_s = AM.forward(cfg, w, M.mfcc_float32(p, cfg.n_mel, cfg.n_mfcc).astype(np.float64))
        dev_l, dev_s = np.abs(f32_l - want_l).max(), np.abs(f32_s - want_s).max()
        t1 = want_l.shape[0]
        tol_l, tol_s = max(4.0 * dev_l, floor_l), max(4.0 * dev_s, 0.5 * floor_l)
        err_l, err_s = np.abs(lg[b, :t1] - want_l).max(), np.abs(sm[b, :t1] - want_s).max()
        print("MFCC-E2E utt%d n_mel=%d T'=%d: logits %.3e (4 x float32-CPU %.3e, floor %.3e) / bound = %.3f   softmax %.3e (4 x %.3e) / bound = %.3f"
              % (b, cfg.n_mel, t1, err_l, 4.0 * dev_l, floor_l, err_l / tol_l, err_s, 4.0 * dev_s, err_s / tol_s))
        assert err_l <= tol_l and err_s <= tol_s, (b, err_l, tol_l, err_s, tol_s)
        assert not lg[b, t1:].any() and not sm[b, t1:].any()
    m.close()


def test_refusals():
    from keyword_spotting_amd import _lib, get_config, weights
    from keyword_spotting_amd.rnn_ctc import DeployModel as RnnModel
    for kind, power, n_mfcc, word in ((_lib.FEAT_MFCC, 2, 20, "MFCC"), (_lib.FEAT_MEL, 2, 0, "power=2")):
        lib, h, rc = _power_handle(40, power, kind, n_mfcc, fft=256)
        assert rc == _lib.KWS_ERR_UNSUPPORTED and not h.value and b"fft_size=256" in lib.kws_last_error()
        lib, h, rc = _power_handle(40, power, kind, n_mfcc)
        _lib.check(rc)
        x, out = torch.zeros(2, 800, device="cuda"), torch.zeros(2, 3, 64, device="cuda")
        rc = lib.kws_frontend_run_carry(h, None, 0, _lib.ptr(x), 800, 2, _lib.ptr(out), None, 0, None)
        assert rc == _lib.KWS_ERR_UNSUPPORTED and word.encode() in lib.kws_last_error()
        # kws_stream_create refuses it too, before it looks at anything else
        cfg = get_config()
        model = RnnModel(cfg, weights.init_weights(cfg, seed=0))
        win = ctypes.c_void_p()
        _lib.check(lib.kws_window_create(2, 15, 32, 6, 0.4, ctypes.byref(win)))
        state, restart = torch.zeros(2, 2, 128, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda")
        s = ctypes.c_void_p()
        rc = lib.kws_stream_create(model._handle, h, win, 2, 3600, 30.0, b"1233", _lib.ptr(state), _lib.ptr(restart), ctypes.byref(s))
        assert rc == _lib.KWS_ERR_UNSUPPORTED and not s.value and word.encode() in lib.kws_last_error()
        lib.kws_window_destroy(win)
        lib.kws_frontend_destroy(h)
    # the plain handle still streams, and takes lengths only where the FFT kernel runs
    lib, h, rc = _power_handle(40, 1, fft=256)
    _lib.check(rc)
    x, out = torch.zeros(2, 800, device="cuda"), torch.zeros(2, 4, 40, device="cuda")
    lens = torch.tensor([800, 300], dtype=torch.int32, device="cuda")
    assert lib.kws_frontend_run_lengths(h, _lib.ptr(x), _lib.ptr(lens), 2, 800, _lib.ptr(out), None) == _lib.KWS_ERR_UNSUPPORTED
    assert b"fft_size=256" in lib.kws_last_error()
    _lib.check(lib.kws_frontend_run_lengths(h, _lib.ptr(x), None, 2, 800, _lib.ptr(out), None))
    assert lib.kws_frontend_dct_basis(h, out.cpu().numpy().ctypes.data_as(ctypes.c_void_p)) == _lib.KWS_ERR_INVALID_ARGUMENT
    lib.kws_frontend_destroy(h)
    torch.cuda.synchronize()
