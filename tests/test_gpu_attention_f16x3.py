"""The self-attention CTC model with precision="f16x3" (kws_attention_create_precision, csrc/attention_f16x3.hip) on the GPU: against
the fp64 restatement (tests/attention_model.py) at the fp32 path's tolerances, bitwise against itself across batch composition,
padding, repeated runs and HIP streams, and the fp32 entry bitwise against what it was."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_model as AM
from conftest import ROOT

pytestmark = pytest.mark.gpu

LOGIT_TOL, SOFTMAX_TOL = 1e-4, 2e-5            # tests/test_gpu_attention.py's, unchanged

# tests/test_gpu_attention.py's GRID: (combine_frame, n_mel, hidden, heads, ffn_inner, layers, classes, relu).  c * n_mel is not
# a multiple of 32 in rows 0, 2 (39), 3, 4 (80), 5, 6 (200), 8; n_mel 512 is row 7
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


def _cfg(**kw):
    from keyword_spotting_amd.config import get_attention_config
    return get_attention_config(**kw)


def _grid_cfg(c, F, H, heads, Fi, L, C, relu):
    return _cfg(combine_frame=c, n_mel=F, hidden_size=H, multi_head_num=heads, feed_forward_inner_size=Fi, num_layers=L,
                use_relu=relu, max_frames=200, label_dict={str(i): i for i in range(1, C - 2)})


def _weights(cfg, seed):
    from keyword_spotting_amd import attention_weights as AW
    return AW.init(cfg, seed)


def _model(cfg, w, **kw):
    from keyword_spotting_amd.attention_ctc import DeployModel
    return DeployModel(cfg, w, **kw)


def _f16x3(cfg, w):
    return _model(cfg, w, precision="f16x3")


def _mel(B, T, F, seed):
    return np.random.default_rng(seed).standard_normal((B, T, F)).astype(np.float32)


def _check(cfg, w, mel, lengths, r, want=None, skip=()):
    """Every utterance against the restatement (`want`: precomputed [(logits, softmax)]); rows past T'_b are exactly 0.
    -> (max logit deviation, max softmax deviation)."""
    lg, sm = r["logits"].cpu().numpy(), r["softmax"].cpu().numpy()
    dl = ds = 0.0
    for b in range(mel.shape[0]):
        tb = min(max(int(lengths[b]), 0), mel.shape[1])
        n = AM.frames_out(tb, cfg.combine_frame)
        assert n == int(r["lengths_out"][b])
        assert not lg[b, n:].any() and not sm[b, n:].any(), (b, tb)
        if b in skip:
            continue
        want_l, want_s = want[b] if want is not None else AM.forward(cfg, w, mel[b, :tb])
        assert want_l.shape[0] == n
        dl = max(dl, np.abs(lg[b, :n] - want_l).max(initial=0.0))
        ds = max(ds, np.abs(sm[b, :n] - want_s).max(initial=0.0))
    print("max deviation from fp64: logits %.3g, softmax %.3g" % (dl, ds))
    assert dl < LOGIT_TOL and ds < SOFTMAX_TOL, (dl, ds)
    return dl, ds


@pytest.mark.parametrize("c,F,H,heads,Fi,L,C,relu", GRID)
def test_config_grid(c, F, H, heads, Fi, L, C, relu):
    cfg = _grid_cfg(c, F, H, heads, Fi, L, C, relu)
    assert cfg.num_classes == C
    w = _weights(cfg, c * 1000 + H + L)
    lengths = np.array([75, 1, 33, 64, 70], np.int32)
    mel = _mel(len(lengths), 75, F, H + Fi)
    _check(cfg, w, mel, lengths, _f16x3(cfg, w).forward(mel, lengths))


@pytest.fixture(scope="module")
def reference_case():
    """The reference shape, B = 7, T = 300, and its fp64 results: computed once, read by two tests."""
    cfg = _cfg()
    w = _weights(cfg, 7)
    mel = _mel(7, 300, cfg.n_mel, 8)
    lengths = np.random.default_rng(7).integers(1, 301, 7).astype(np.int32)
    lengths[0] = 300
    want = [AM.forward(cfg, w, mel[b, :lengths[b]]) for b in range(7)]
    return cfg, w, mel, lengths, want


def test_reference_shape_against_the_restatement(reference_case):
    cfg, w, mel, lengths, want = reference_case
    _check(cfg, w, mel, lengths, _f16x3(cfg, w).forward(mel, lengths), want)


def test_deviation_from_the_fp32_handle_at_the_reference_shape(reference_case):
    """Printed for DESIGN section 9; the assertion is only that both meet the tolerances."""
    cfg, w, mel, lengths, want = reference_case
    r16, r32 = _f16x3(cfg, w).forward(mel, lengths), _model(cfg, w).forward(mel, lengths)
    _check(cfg, w, mel, lengths, r16, want)
    _check(cfg, w, mel, lengths, r32, want)
    print("max |f16x3 - fp32 handle|: logits %.3g, softmax %.3g" % (float((r16["logits"] - r32["logits"]).abs().max()),
                                                                     float((r16["softmax"] - r32["softmax"]).abs().max())))


def test_edge_lengths_in_one_batch():
    """0 frames (one all-pad row at c = 2), 1, 2, T mod c != 0 and == 0."""
    cfg = _cfg(max_frames=38)
    w = _weights(cfg, 3)
    lengths = np.array([0, 1, 2, 37, 38], np.int32)
    mel = _mel(len(lengths), 38, cfg.n_mel, 4)
    _check(cfg, w, mel, lengths, _f16x3(cfg, w).forward(mel, lengths))


@pytest.mark.parametrize("scale,shift", [(1e-4, 0.0), (300.0, -50.0)])
def test_input_range(scale, shift):
    cfg = _cfg(max_frames=64)
    w = _weights(cfg, 21)
    mel = (_mel(4, 64, cfg.n_mel, 22) * np.float32(scale) + np.float32(shift)).astype(np.float32)
    lengths = np.array([64, 17, 40, 63], np.int32)
    _check(cfg, w, mel, lengths, _f16x3(cfg, w).forward(mel, lengths))


def test_a_frame_beyond_the_fp16_range_saturates_and_stays_in_its_utterance():
    cfg = _cfg(max_frames=64)
    w = _weights(cfg, 23)
    mel = _mel(4, 64, cfg.n_mel, 24)
    mel[1, 0] = 1e8
    lengths = np.array([64, 64, 40, 63], np.int32)
    r = _f16x3(cfg, w).forward(mel, lengths)
    assert torch.isfinite(r["logits"]).all() and torch.isfinite(r["softmax"]).all()
    _check(cfg, w, mel, lengths, r, skip=(1,))         # the other utterances do not see it


def test_mfcc_sized_features_with_the_mfcc_config():
    cfg = _cfg(mfcc=True, max_frames=64)
    assert cfg.freq_size == 3 * cfg.n_mfcc
    w = _weights(cfg, 25)
    mel = np.random.default_rng(26).uniform(-300.0, 300.0, (4, 64, cfg.freq_size)).astype(np.float32)
    lengths = np.array([64, 17, 40, 63], np.int32)
    _check(cfg, w, mel, lengths, _f16x3(cfg, w).forward(mel, lengths))


def test_bitwise_alone_in_a_mixed_batch_twice_and_on_a_second_stream():
    """Batch composition, T_max, NaN in the padding past T_b, a repeated run and another HIP stream change no bit."""
    cfg = _cfg(max_frames=200)
    w = _weights(cfg, 8)
    m = _f16x3(cfg, w)
    lengths = np.array([130, 7, 64, 1], np.int32)
    T = 160
    mel = np.random.default_rng(9).standard_normal((len(lengths), T, cfg.n_mel)).astype(np.float32)
    for b, tb in enumerate(lengths):
        mel[b, tb:] = np.nan
    dmel, dlen = torch.from_numpy(mel).cuda(), torch.from_numpy(lengths).cuda()
    r = m.forward(dmel, dlen)
    lg, sm = r["logits"].cpu().numpy(), r["softmax"].cpu().numpy()
    assert np.isfinite(lg).all() and np.isfinite(sm).all()
    for b, tb in enumerate(lengths):
        n = AM.frames_out(int(tb), cfg.combine_frame)
        alone = np.full((1, tb + 41, cfg.n_mel), np.nan, np.float32)
        alone[0, :tb] = mel[b, :tb]
        ra = m.forward(alone, np.array([tb], np.int32))
        assert np.array_equal(ra["logits"].cpu().numpy()[0, :n], lg[b, :n]), b
        assert np.array_equal(ra["softmax"].cpu().numpy()[0, :n], sm[b, :n]), b
    r2 = m.forward(dmel, dlen)
    assert torch.equal(r["logits"], r2["logits"]) and torch.equal(r["softmax"], r2["softmax"])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r3 = m.forward(dmel, dlen)
    side.synchronize()
    assert torch.equal(r["logits"], r3["logits"]) and torch.equal(r["softmax"], r3["softmax"])
    _check(cfg, w, np.nan_to_num(mel), lengths, r)


@pytest.mark.parametrize("grid_row", [None, 6])
def test_the_fp32_entry_is_what_it_was(grid_row):
    """DeployModel's default, precision="fp32" and the old C entry kws_attention_create are one path: bitwise-equal results."""
    cfg = _cfg() if grid_row is None else _grid_cfg(*GRID[grid_row])
    w = _weights(cfg, 31)
    lengths = np.array([75, 1, 33, 64, 70], np.int32)
    mel = _mel(len(lengths), 75, cfg.n_mel, 32)
    a, b = _model(cfg, w).forward(mel, lengths), _model(cfg, w, precision="fp32").forward(mel, lengths)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["softmax"], b["softmax"])
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd import attention_weights as AW
    import ctypes
    # ... and a handle of the entry without a precision argument behind the same Python object
    m = _model(cfg, w)
    lib, blob, h = _lib.load(), AW.to_blob(cfg, w), ctypes.c_void_p()
    _lib.check(lib.kws_attention_create(ctypes.byref(m._cfg), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ctypes.byref(h)))
    old, m._handle = m._handle, h
    c = m.forward(mel, lengths)
    lib.kws_attention_destroy(old)
    assert torch.equal(a["logits"], c["logits"]) and torch.equal(a["softmax"], c["softmax"])


def test_selftest_passes_and_runs_at_create_under_the_environment_switch():
    for kw in ({}, dict(combine_frame=1, hidden_size=256, multi_head_num=8, num_layers=2, max_frames=40)):
        cfg = _cfg(**kw)
        _f16x3(cfg, _weights(cfg, 17)).selftest()
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from keyword_spotting_amd.config import get_attention_config\n"
            "from keyword_spotting_amd import attention_weights as AW\n"
            "from keyword_spotting_amd.attention_ctc import DeployModel\n"
            "cfg = get_attention_config(); DeployModel(cfg, AW.init(cfg, 1), precision='f16x3'); print('created')\n"
            ) % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KWS_SELFTEST="1"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "created" in r.stdout, r.stderr[-2000:]
