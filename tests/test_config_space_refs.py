"""CPU companion of tests/test_gpu_config_space.py: (1) the references that file compares the kernels with agree with each
other on its grid, so that a failure there points at a kernel, not at a reference; (2) the grid lies inside the space
kws_create accepts and the boundaries of that space are where api_model.hip:config_ok puts them (config_ok runs before any
device call, so this needs no GPU)."""
import ctypes

import numpy as np
import pytest

from conftest import have_gpu
from oracle import gru_oracle as G
from tests import config_space_grid as S

MI355X_CUS = 256


@pytest.mark.parametrize("n_mel,hidden,layers,classes,batch", [
    (1024, 256, 2, 8, 4), (257, 256, 5, 4, 5), (13, 64, 8, 8, 5), (100, 128, 6, 3, 4), (1, 64, 1, 3, 5), (65, 64, 7, 5, 4)])
def test_c_oracle_agrees_with_float64_on_the_grid(oracle_c, n_mel, hidden, layers, classes, batch):
    w = G.random_weights(n_mel, hidden, layers, classes, seed=n_mel + layers)
    t = 6
    mel = G.synthetic_mel(batch, t, n_mel, seed=7)
    st0 = (0.5 * np.random.default_rng(8).standard_normal((layers, batch, hidden))).astype(np.float32)
    lens = np.array([t, 0, 3, 1, t][:batch], np.int32)
    want_l, want_s = G.gru_forward(w, mel, st0, seq_len=lens, dtype=np.float64)
    c_l, c_sm, c_s = oracle_c.gru_forward((n_mel, hidden, layers, classes, 0, -1.0), G.weights_to_blob(w), mel, st0, seq_len=lens)
    assert np.abs(c_l - want_l).max() < 5e-5 and np.abs(c_s - want_s).max() < 5e-5
    assert np.abs(c_sm - G.softmax(want_l)).max() < 2e-5


@pytest.mark.parametrize("clip", [-1.0, 0.0, 0.5, 20.0])
def test_relu_clip_means_clip_to_20_whenever_value_clip_is_positive(oracle_c, clip):
    """models/rnn_ctc.py:280-283: relu, then clip to [0, 20] if value_clip > 0 -- whatever the value of value_clip."""
    w = G.random_weights(13, 64, 2, 5, seed=3)
    w["Wfc"] *= 20
    mel = G.synthetic_mel(3, 9, 13, seed=4)
    plain, _ = G.gru_forward(w, mel, dtype=np.float64)
    want, _ = G.gru_forward(w, mel, dtype=np.float64, use_relu=True, value_clip=clip)
    assert plain.max() > 20 and plain.min() < 0
    np.testing.assert_array_equal(want, np.clip(plain, 0, 20) if clip > 0 else np.maximum(plain, 0))
    c_l, _, _ = oracle_c.gru_forward((13, 64, 2, 5, 1, clip), G.weights_to_blob(w), mel, np.zeros((2, 3, 64), np.float32))
    assert np.abs(c_l - want).max() < 5e-5 * 20
    assert (c_l.max() == 20.0) == (clip > 0)


@pytest.mark.parametrize("n_mel,layers,classes", [(13, 2, 3), (100, 2, 8), (13, 1, 8), (100, 5, 3)])
def test_bf16_and_octbit_references_at_other_class_counts_and_widths(n_mel, layers, classes):
    w = G.random_weights(n_mel, 128, layers, classes, seed=5)
    b, t = 3, 7
    mel = G.synthetic_mel(b, t, n_mel, seed=6)
    ref_l, ref_s = G.gru_forward(w, mel, dtype=np.float64)
    fwds = [G.gru_forward_octbit] + ([G.gru_forward_bf16] if layers <= 2 else [])
    for fwd in fwds:
        lg, st = fwd(w, mel, seq_len=np.array([t, 0, 4]))
        assert lg.shape == (b, t, classes) and st.shape == (layers, b, 128)
        assert np.isfinite(lg).all() and np.isfinite(st).all()
        np.testing.assert_array_equal(lg[1], np.broadcast_to(w["bfc"], (t, classes)))     # zero output rows: the bias
        full, _ = fwd(w, mel)
        # the same model in coarser arithmetic: int8 moves a logit by a few percent of its size, bf16 by less
        assert np.abs(full - ref_l).mean() < 0.2 * np.abs(ref_l).mean(), fwd.__name__


def test_grid_rows_take_the_layout_they_were_written_for():
    """On the MI355X's CU count; the GPU test re-checks against the count of the device it runs on."""
    names = [r.name for r in S.ROWS]
    assert len(names) == len(set(names))
    for r in S.ROWS:
        assert S.layout_of(r, r.batch, r.frames, MI355X_CUS) == r.layout, r.name
        assert len(S.expected_names(r, r.batch, r.frames, MI355X_CUS)) == r.layers
        if r.twin:
            assert S.layout_of(r, S.sequential_batch(r.layers, MI355X_CUS), r.frames if r.layout == "ovl" else r.twin,
                               MI355X_CUS) == "seq", r.name
    layouts = {(r.prec, r.layout) for r in S.ROWS}
    for want in [("fp32", "single"), ("fp32", "pipe"), ("fp32", "seq"), ("fp32", "ovl"), ("f16x3", "f16x3"), ("f16x3", "pipe"),
                 ("bf16", "bf16"), ("int8", "int8")]:
        assert want in layouts
    assert {r.classes for r in S.ROWS} == {3, 4, 5, 7, 8}
    assert {r.layers for r in S.ROWS} == set(range(1, 9))
    assert {(r.relu, r.clip > 0) for r in S.ROWS if r.prec == "fp32"} == {(0, False), (1, False), (1, True)}


def _create(prec, n_mel, hidden, layers, classes, relu=0, clip=-1.0):
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    cfg = _lib.KwsConfig(n_mel, hidden, layers, classes, relu, clip, S.PRECISION[prec])
    nbytes = lib.kws_weights_nbytes(ctypes.byref(cfg))
    blob = np.full(max(nbytes // 4, 1), 0.01, np.float32)       # not zeros: the int8 quantiser refuses an all-zero matrix (scale 0)
    h = ctypes.c_void_p()
    rc = lib.kws_create(ctypes.byref(cfg), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ctypes.byref(h))
    if h.value:
        lib.kws_destroy(h)
    return rc, nbytes


@pytest.mark.parametrize("row", S.ROWS, ids=[r.name for r in S.ROWS])
def test_grid_row_is_accepted(row):
    from keyword_spotting_amd import _lib
    rc, nbytes = _create(row.prec, row.n_mel, row.hidden, row.layers, row.classes, row.relu, row.clip)
    assert nbytes > 0
    assert rc == (_lib.KWS_OK if have_gpu() else _lib.KWS_ERR_NO_DEVICE), _lib.load().kws_last_error()


@pytest.mark.parametrize("cfg", S.OUTSIDE, ids=["%s-%d-%d-%d-%d" % c for c in S.OUTSIDE])
def test_just_outside_the_space_is_refused(cfg):
    from keyword_spotting_amd import _lib
    rc, nbytes = _create(*cfg)
    assert nbytes == 0
    assert rc in (_lib.KWS_ERR_UNSUPPORTED, _lib.KWS_ERR_INVALID_ARGUMENT), rc
