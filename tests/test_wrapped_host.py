"""CPU checks of the cell wrappers (ResidualWrapper(LayerNormalizer(GRUCell)), models/rnn_ctc.py:179-199): the fp64
restatement itself, the weights' round trips with the layer norm's variables, the checkpoint-name checks, and the C ABI's
blob sizes and argument validation (all before any device work)."""
import ctypes

import numpy as np
import pytest

from oracle import gru_oracle as G
from wrapped_cell_model import layer_norm, random_ln, wrapped_forward


def _cfg(**kw):
    from keyword_spotting_amd import get_config
    base = dict(n_mel=13, hidden_size=64, num_layers=3)
    base.update(kw)
    return get_config(**base)


def _weights(cfg, seed=1):
    from keyword_spotting_amd import weights as W
    w = G.random_weights(cfg.n_mel, cfg.hidden_size, cfg.num_layers, cfg.num_classes, seed)
    if cfg.use_layer_norm:
        random_ln(w, cfg.n_mel, seed)
    W.check_shapes(cfg, w)
    return w


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_layer_norm_with_tf_initial_values_ignores_the_input():
    rng = np.random.default_rng(0)
    w = G.random_weights(13, 64, 2, 6, 3)
    for lay, i_l in zip(w["layers"], (13, 64)):
        lay["ibeta"], lay["igamma"] = np.zeros((), np.float32), rng.standard_normal(i_l).astype(np.float32)
    a = rng.standard_normal((4, 7, 13)) * 5 + 3
    b = rng.standard_normal((4, 7, 13))
    la, sa = wrapped_forward(w, a, True, False)
    lb, sb = wrapped_forward(w, b, True, False)
    assert np.allclose(la, lb, atol=1e-12) and np.allclose(sa, sb, atol=1e-12)


def test_residual_on_one_layer_is_the_plain_cell():
    w = G.random_weights(13, 64, 1, 6, 4)
    mel = G.synthetic_mel(5, 9, 13, seed=2)
    want_l, want_s = G.gru_forward(w, mel, dtype=np.float64)
    got_l, got_s = wrapped_forward(w, mel, False, True)
    assert np.array_equal(got_l, want_l) and np.array_equal(got_s, want_s)


def test_layer_norm_is_invariant_to_a_constant_shift():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 40))
    gm = rng.standard_normal(40)
    assert np.allclose(layer_norm(x, 1.3, gm), layer_norm(x + 50.0, 1.3, gm), atol=1e-9)
    w = random_ln(G.random_weights(40, 64, 2, 6, 6), 40, 6)
    mel = G.synthetic_mel(3, 5, 40, seed=3).astype(np.float64)
    a, _ = wrapped_forward(w, mel, True, True)
    b, _ = wrapped_forward(w, mel + 50.0, True, False)
    c, _ = wrapped_forward(w, mel + 50.0, True, True)
    assert not np.allclose(a, b)                        # the residual of layer 1 sees the layer's raw input ...
    assert np.allclose(a, c, atol=1e-9)                 # ... which is the layer below's output, not the shifted mel


def test_residual_reaches_the_dense_layer_but_not_the_state():
    w = G.random_weights(13, 64, 2, 6, 7)
    mel = G.synthetic_mel(2, 4, 13, seed=4)
    l_res, s_res = wrapped_forward(w, mel, False, True)
    l_pl, s_pl = wrapped_forward(w, mel, False, False)
    assert np.array_equal(s_res, s_pl)
    assert not np.allclose(l_res, l_pl)


# ---- weights --------------------------------------------------------------------------------------------------------------
def test_init_weights_uses_the_tf_initial_values():
    from keyword_spotting_amd import weights as W
    cfg = _cfg(use_layer_norm=True)
    w = W.init_weights(cfg)
    for lay, i_l in zip(w["layers"], W.layer_in_dims(cfg)):
        assert lay["ibeta"].shape == () and float(lay["ibeta"]) == 0.0
        assert lay["igamma"].shape == (i_l,) and (lay["igamma"] == 1.0).all()
    assert "ibeta" not in W.init_weights(_cfg())["layers"][0]


@pytest.mark.parametrize("new_names", [True, False])
@pytest.mark.parametrize("prefix", ["model/", ""])
def test_round_trips_with_layer_norm(tmp_path, new_names, prefix):
    from keyword_spotting_amd import weights as W
    cfg = _cfg(use_layer_norm=True, use_residual=True)
    w = _weights(cfg)
    blob = W.to_blob(cfg, w)
    plain = W.to_blob(_cfg(), {**w, "layers": [{k: v for k, v in lay.items() if k in ("Wg", "bg", "Wc", "bc")} for lay in w["layers"]]})
    assert blob.size == plain.size + sum(1 + i for i in W.layer_in_dims(cfg))
    assert np.array_equal(blob[:plain.size], plain)                          # the canonical blob, unchanged, comes first
    assert float(blob[plain.size]) == float(w["layers"][0]["ibeta"])
    assert np.array_equal(W.to_blob(cfg, W.from_blob(cfg, blob)), blob)
    W.save_npz(str(tmp_path / "w.npz"), w)
    assert np.array_equal(W.to_blob(cfg, W.load_npz(str(tmp_path / "w.npz"))), blob)
    tf = W.to_tf_variables(w, new_names=new_names, prefix=prefix)
    assert prefix + "drnn/multi_rnn_cell/cell_2/LayerNormalizer/igamma" in tf
    assert np.array_equal(W.to_blob(cfg, W.from_tf_variables(cfg, tf)), blob)
    # an extra scope before LayerNormalizer/, a ":0" suffix and optimiser slots
    tf2 = {k.replace("cell_1/LayerNormalizer", "cell_1/wrapper/LayerNormalizer") + ":0": v for k, v in tf.items()}
    tf2[prefix + "drnn/multi_rnn_cell/cell_0/LayerNormalizer/ibeta/Adam"] = np.float32(7.0)
    assert np.array_equal(W.to_blob(cfg, W.from_tf_variables(cfg, tf2)), blob)


def test_from_tf_variables_rejects_a_layer_norm_mismatch():
    from keyword_spotting_amd import weights as W
    cfg = _cfg(use_layer_norm=True)
    tf = W.to_tf_variables(_weights(cfg))
    with pytest.raises(ValueError, match="cell_0/LayerNormalizer/ibeta"):
        W.from_tf_variables(_cfg(), tf)                                      # present, but use_layer_norm is off
    missing = {k: v for k, v in tf.items() if "cell_1/LayerNormalizer/igamma" not in k}
    with pytest.raises(ValueError, match="cell_1/LayerNormalizer/igamma"):
        W.from_tf_variables(cfg, missing)                                    # missing while it is on
    with pytest.raises(ValueError, match="use_layer_norm is off"):
        W.to_blob(_cfg(), _weights(cfg))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def _kc(n_mel=40, hidden=128, layers=2, precision=0):
    from keyword_spotting_amd import _lib
    return _lib.KwsConfig(n_mel, hidden, layers, 6, 0, -1.0, precision)


def test_wrapped_blob_sizes():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert lib.kws_sizeof_cell_wrappers() == ctypes.sizeof(_lib.KwsCellWrappers) == 8
    for n_mel, hidden, layers in ((40, 128, 2), (60, 256, 4), (13, 64, 1), (1024, 64, 8)):
        cfg = _kc(n_mel, hidden, layers)
        plain = lib.kws_weights_nbytes(ctypes.byref(cfg))
        assert plain > 0
        ln = lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(1, 0)))
        assert ln == plain + 4 * sum(1 + (n_mel if l == 0 else hidden) for l in range(layers))
        assert lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(1, 1))) == ln
        assert lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(0, 1))) == plain
        assert lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), None) == plain
        assert lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(0, 0))) == plain
    from keyword_spotting_amd import weights as W
    cfg = _cfg(n_mel=40, hidden_size=128, num_layers=2, use_layer_norm=True)
    assert W.to_blob(cfg, W.init_weights(cfg)).nbytes == \
        lib.kws_weights_nbytes_wrapped(ctypes.byref(_kc()), ctypes.byref(_lib.KwsCellWrappers(1, 0)))


def test_wrapped_create_validates_before_any_device_work():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    blob = np.zeros(1 << 20, np.float32)
    ptr = blob.ctypes.data_as(ctypes.c_void_p)
    for prec, name in ((1, b"bf16"), (3, b"f16x3"), (2, b"int8")):
        cfg = _kc(40, 128, 2, prec)
        for wrap, opt in (((1, 0), b"use_layer_norm"), ((0, 1), b"use_residual")):
            rc = lib.kws_create_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(*wrap)), ptr, 4, ctypes.byref(h))
            assert rc == _lib.KWS_ERR_UNSUPPORTED, (prec, wrap)
            err = lib.kws_last_error()
            assert opt in err and name in err, err
            assert lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(*wrap))) == 0
        # no wrapper at all: the plain create's own checks (here: the blob size)
        assert lib.kws_create_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(0, 0)), ptr, 4,
                                      ctypes.byref(h)) == _lib.KWS_ERR_INVALID_ARGUMENT
    cfg = _kc()
    for wrap in ((2, 0), (0, -1), (1, 7)):
        rc = lib.kws_create_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(*wrap)), ptr, blob.nbytes, ctypes.byref(h))
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT, wrap
        assert b"must be 0 or 1" in lib.kws_last_error()
        assert lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(*wrap))) == 0
    need = lib.kws_weights_nbytes_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(1, 1)))
    plain = lib.kws_weights_nbytes(ctypes.byref(cfg))
    for nbytes in (plain, need - 4, need + 4):
        rc = lib.kws_create_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(1, 1)), ptr, nbytes, ctypes.byref(h))
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and b"config needs %d" % need in lib.kws_last_error()
    assert lib.kws_create_wrapped(ctypes.byref(cfg), ctypes.byref(_lib.KwsCellWrappers(1, 1)), None, need,
                                  ctypes.byref(h)) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert not h.value


def test_convert_weights_takes_layer_norm_checkpoints_only_with_the_flag(tmp_path):
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from keyword_spotting_amd import weights as W
    cfg = _cfg(n_mel=40, hidden_size=128, num_layers=2, use_layer_norm=True, use_residual=True)
    w = _weights(cfg)
    src = str(tmp_path / "vars.npz")
    np.savez(src, **{k + ":0": v for k, v in W.to_tf_variables(w).items()})
    tool = [sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), src, "--n-mel", "40", "--hidden", "128", "--layers", "2"]
    ok = subprocess.run(tool + ["--out", str(tmp_path / "m"), "--layer-norm", "--residual"], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert np.array_equal(np.fromfile(str(tmp_path / "m.blob"), np.float32), W.to_blob(cfg, w))
    bad = subprocess.run(tool + ["--out", str(tmp_path / "p")], capture_output=True, text=True)
    assert bad.returncode != 0 and "drnn/multi_rnn_cell/cell_0/LayerNormalizer/ibeta" in bad.stderr
    assert not os.path.exists(str(tmp_path / "p.blob"))
