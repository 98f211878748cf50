"""The self-attention CTC model on the GPU (kws_attention_*, attention_ctc.DeployModel) against the fp64 restatement
(tests/attention_model.py), and bitwise against itself across batch composition, T_max padding and repeated runs."""
import ctypes
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest
import torch

import attention_model as AM
from conftest import ROOT

pytestmark = pytest.mark.gpu

LOGIT_TOL, SOFTMAX_TOL = 1e-4, 2e-5


def _cfg(**kw):
    from keyword_spotting_amd.config import get_attention_config
    return get_attention_config(**kw)


def _weights(cfg, seed):
    from keyword_spotting_amd import attention_weights as AW
    return AW.init(cfg, seed)


def _model(cfg, w):
    from keyword_spotting_amd.attention_ctc import DeployModel
    return DeployModel(cfg, w)


def _mel(B, T, F, seed):
    return np.random.default_rng(seed).standard_normal((B, T, F)).astype(np.float32)


def _check(cfg, w, mel, lengths, r):
    lg, sm = r["logits"].cpu().numpy(), r["softmax"].cpu().numpy()
    for b in range(mel.shape[0]):
        tb = min(max(int(lengths[b]), 0), mel.shape[1])
        want_l, want_s = AM.forward(cfg, w, mel[b, :tb])
        n = want_l.shape[0]
        assert n == AM.frames_out(tb, cfg.combine_frame) == int(r["lengths_out"][b])
        assert np.abs(lg[b, :n] - want_l).max(initial=0.0) < LOGIT_TOL, (b, tb)
        assert np.abs(sm[b, :n] - want_s).max(initial=0.0) < SOFTMAX_TOL, (b, tb)
        assert not lg[b, n:].any() and not sm[b, n:].any(), (b, tb)     # rows past T'_b are written as 0


@pytest.mark.parametrize("B", [1, 7, 64])
def test_reference_shape_against_the_restatement(B):
    cfg = _cfg()
    w = _weights(cfg, B)
    T = 300
    mel = _mel(B, T, cfg.n_mel, B + 1)
    lengths = np.random.default_rng(B).integers(1, T + 1, B).astype(np.int32)
    lengths[0] = T
    _check(cfg, w, mel, lengths, _model(cfg, w).forward(mel, lengths))


def test_edge_lengths_in_one_batch():
    """0 frames (one all-pad row at c = 2), 1, 2, T mod c == 0 and != 0, and max_frames itself."""
    cfg = _cfg(max_frames=1200)
    w = _weights(cfg, 3)
    lengths = np.array([0, 1, 2, 37, 38, 300, 1200], np.int32)
    mel = _mel(len(lengths), 1200, cfg.n_mel, 4)
    _check(cfg, w, mel, lengths, _model(cfg, w).forward(mel, lengths))


def test_max_frames_at_the_reference_default():
    cfg = _cfg()
    w = _weights(cfg, 5)
    mel = _mel(2, cfg.max_frames, cfg.n_mel, 6)
    lengths = np.array([cfg.max_frames, 5], np.int32)
    _check(cfg, w, mel, lengths, _model(cfg, w).forward(mel, lengths))


# (combine_frame, n_mel, hidden, heads, ffn_inner, layers, classes, relu): every value of every axis of the issue's grid
# (c 1/2/3, d 16/32, H 64/128/256, Fi 256/1024, L 1/6, C 3/8, relu on/off) appears, with each H at both head sizes
GRID = [
    (1, 40, 64, 4, 256, 1, 3, True),
    (2, 60, 64, 2, 1024, 6, 8, False),
    (3, 13, 128, 8, 256, 6, 3, False),
    (1, 60, 128, 4, 1024, 1, 8, True),
    (2, 40, 256, 16, 1024, 1, 3, True),
    (3, 60, 256, 8, 256, 6, 8, True),
    (2, 100, 128, 8, 256, 1, 8, False),
    (1, 512, 64, 4, 1024, 6, 6, True),
    (3, 170, 256, 16, 256, 1, 5, False),
    (2, 256, 128, 4, 1024, 6, 3, True),
]


@pytest.mark.parametrize("c,F,H,heads,Fi,L,C,relu", GRID)
def test_config_grid(c, F, H, heads, Fi, L, C, relu):
    cfg = _cfg(combine_frame=c, n_mel=F, hidden_size=H, multi_head_num=heads, feed_forward_inner_size=Fi, num_layers=L,
               use_relu=relu, max_frames=200, label_dict={str(i): i for i in range(1, C - 2)})
    assert cfg.num_classes == C
    w = _weights(cfg, c * 1000 + H + L)
    lengths = np.array([75, 1, 33, 64, 70], np.int32)
    mel = _mel(len(lengths), 75, F, H + Fi)
    _check(cfg, w, mel, lengths, _model(cfg, w).forward(mel, lengths))


def test_an_utterance_alone_equals_it_inside_a_mixed_batch_and_ignores_padding():
    """Bitwise: batch composition, T_max and whatever lies in the padding past T_b (NaN here) change nothing."""
    cfg = _cfg()
    w = _weights(cfg, 8)
    m = _model(cfg, w)
    rng = np.random.default_rng(9)
    lengths = np.array([130, 7, 299, 64, 1, 200, 131], np.int32)
    T = 320
    mel = rng.standard_normal((len(lengths), T, cfg.n_mel)).astype(np.float32)
    for b, tb in enumerate(lengths):
        mel[b, tb:] = np.nan
    r = m.forward(mel, lengths)
    lg, sm = r["logits"].cpu().numpy(), r["softmax"].cpu().numpy()
    for b, tb in enumerate(lengths):
        n = AM.frames_out(int(tb), cfg.combine_frame)
        for pad in (0, 41):
            alone = np.full((1, tb + pad, cfg.n_mel), np.nan, np.float32)
            alone[0, :tb] = mel[b, :tb]
            ra = m.forward(alone, np.array([tb], np.int32))
            assert np.array_equal(ra["logits"].cpu().numpy()[0, :n], lg[b, :n]), (b, pad)
            assert np.array_equal(ra["softmax"].cpu().numpy()[0, :n], sm[b, :n]), (b, pad)
    assert np.isfinite(lg).all() and np.isfinite(sm).all()


def test_two_runs_are_identical_and_lengths_are_clamped():
    cfg = _cfg()
    w = _weights(cfg, 10)
    m = _model(cfg, w)
    mel = _mel(16, 150, cfg.n_mel, 11)
    lengths = np.array([150, -5, 400, 3] * 4, np.int32)          # clamped to [0, T_max]
    r1, r2 = m.forward(mel, lengths), m.forward(mel, lengths)
    assert torch.equal(r1["logits"], r2["logits"]) and torch.equal(r1["softmax"], r2["softmax"])
    _check(cfg, w, mel, np.clip(lengths, 0, 150), r1)


def test_pe_table_is_the_float_rounding_of_the_double_op():
    cfg = _cfg(max_frames=500)
    m = _model(cfg, _weights(cfg, 12))
    pe = m.pe_table()
    assert pe.shape == (251, 128)
    assert np.array_equal(pe, AM.pe_table(251, 128))


def test_pcm_run_matches_the_restatement_on_the_front_end_mel():
    from keyword_spotting_amd.attention_ctc import FETCH_LENGTHS, FETCH_LOGIT, FETCH_SOFTMAX
    from keyword_spotting_amd.frontend import MelFrontend
    cfg = _cfg()
    w = _weights(cfg, 13)
    m = _model(cfg, w)
    rng = np.random.default_rng(14)
    pcms = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n in (16000, 5000, 399)]
    fe = MelFrontend(cfg)
    sm1 = m.run([FETCH_SOFTMAX], {"model/inputX:0": pcms[0]})[0].cpu().numpy()
    mel0 = fe.forward(torch.from_numpy(pcms[0])).cpu().numpy()
    assert sm1.shape == (1, AM.frames_out(mel0.shape[0], 2), 6)
    assert np.abs(sm1[0] - AM.forward(cfg, w, mel0)[1]).max() < SOFTMAX_TOL
    sm, lg, n = m.run([FETCH_SOFTMAX, FETCH_LOGIT, FETCH_LENGTHS], {"model/inputX:0": pcms})
    sm, lg, n = sm.cpu().numpy(), lg.cpu().numpy(), n.cpu().numpy()
    for b, p in enumerate(pcms):
        mel = fe.forward(torch.from_numpy(p)).cpu().numpy()
        want_l, want_s = AM.forward(cfg, w, mel)
        assert n[b] == want_l.shape[0]
        assert np.abs(sm[b, :n[b]] - want_s).max() < SOFTMAX_TOL
        assert np.abs(lg[b, :n[b]] - want_l).max() < LOGIT_TOL
        assert not sm[b, n[b]:].any()
    fe.close()


def test_decode_equals_the_host_decoder_per_utterance():
    from oracle import decode_oracle as D
    cfg = _cfg()
    w = _weights(cfg, 15)
    w["W_out"] = w["W_out"] * 6.0                 # peaky posteriors: words are emitted
    m = _model(cfg, w)
    lengths = np.array([300, 120, 40, 299, 2, 250], np.int32)
    mel = _mel(len(lengths), 300, cfg.n_mel, 16)
    r = m.forward(mel, lengths)
    seqs, hits = m.decode(r["softmax"], r["lengths_out"])
    sm = r["softmax"].cpu().numpy()
    emitted = 0
    for b in range(len(lengths)):
        n = int(r["lengths_out"][b])
        want = D.ctc_decode(sm[b, :n])
        assert np.array_equal(seqs[b], want), b
        assert hits[b] == D.ctc_predict(want, cfg.label_seqs)
        emitted += len(want) // 2
    assert emitted > 0


def test_selftest_passes_and_runs_at_create_under_the_environment_switch():
    for kw in ({}, dict(combine_frame=1, hidden_size=256, multi_head_num=8, num_layers=2, max_frames=40)):
        cfg = _cfg(**kw)
        _model(cfg, _weights(cfg, 17)).selftest()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from keyword_spotting_amd.config import get_attention_config\n"
            "from keyword_spotting_amd import attention_weights as AW\n"
            "from keyword_spotting_amd.attention_ctc import DeployModel\n"
            "cfg = get_attention_config(); DeployModel(cfg, AW.init(cfg, 1)); print('created')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KWS_SELFTEST="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "created" in r.stdout, r.stderr[-2000:]


def test_bad_arguments_return_the_documented_codes():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    cfg = _cfg(max_frames=100)
    m = _model(cfg, _weights(cfg, 18))
    h = m._handle
    mel = torch.zeros(2, 100, cfg.n_mel, device="cuda")
    out = torch.empty(2, 51, 6, device="cuda")
    st = _lib.current_stream_ptr()
    P = _lib.ptr
    assert lib.kws_attention_run(None, P(mel), None, 2, 100, P(out), None, st) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_run(h, P(mel), None, -1, 100, P(out), None, st) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_run(h, P(mel), None, 2, 101, P(out), None, st) == _lib.KWS_ERR_UNSUPPORTED
    assert b"max_frames" in lib.kws_last_error()
    assert lib.kws_attention_run(h, P(mel), None, 2, 100, None, None, st) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_run(h, None, None, 2, 100, P(out), None, st) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_run(h, P(mel), None, 0, 100, P(out), None, st) == _lib.KWS_OK
    assert lib.kws_attention_reserve(h, 2, 101) == _lib.KWS_ERR_UNSUPPORTED
    assert lib.kws_attention_pe_table(h, None) == _lib.KWS_ERR_INVALID_ARGUMENT


def test_a_second_thread_inside_the_handle_gets_busy():
    """Thread A holds the handle while a scratch growth waits for queued work; a run from this thread meanwhile returns
    KWS_ERR_BUSY and launches nothing; afterwards the handle serves correct results."""
    from keyword_spotting_amd import _lib
    cfg = _cfg(max_frames=2000)
    w = _weights(cfg, 19)
    m = _model(cfg, w)
    big = torch.randn(2048, 1000, cfg.n_mel, device="cuda")
    for _ in range(3):
        m.forward(big, want_logits=False)                        # tens of ms of queued device work
    t = threading.Thread(target=m.reserve, args=(4096, 2000))   # grows the scratch: waits for the device inside the call
    t.start()
    time.sleep(0.005)
    mel = _mel(3, 50, cfg.n_mel, 20)
    with pytest.raises(_lib.BusyError):
        m.forward(mel)
    t.join()
    _check(cfg, w, mel, np.array([50, 50, 50]), m.forward(mel))
