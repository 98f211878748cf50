"""CPU checks of the self-attention CTC model: the fp64 restatement (tests/attention_model.py) against an independent torch
build, its stacking / layer-norm / positional rules on hand cases, the weight converter, and the C ABI's host-side answers
(blob size, config refusals) through ctypes without a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import attention_model as AM
from conftest import ROOT


def _cfg(**kw):
    from keyword_spotting_amd.config import get_attention_config
    return get_attention_config(**kw)


def _torch_forward(cfg, w, mel):
    """The same model built from torch's own float64 CPU operators: F.layer_norm over (T', H), scaled_dot_product_attention."""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    c, H, heads = cfg.combine_frame, cfg.hidden_size, cfg.multi_head_num
    x = t(mel)
    if c > 1:
        x = torch.cat([x, torch.zeros(c - x.shape[0] % c, x.shape[1], dtype=torch.float64)]).reshape(-1, c * x.shape[1])
    T1 = x.shape[0]
    pos = torch.arange(T1, dtype=torch.float64)[:, None] / torch.pow(torch.tensor(10000.0, dtype=torch.float64),
                                                                     2.0 * torch.arange(H // 2, dtype=torch.float64) / H)
    pe = torch.stack([torch.sin(pos), torch.cos(pos)], -1).reshape(T1, H).float().double()
    x = x @ t(w["W_in"]) + t(w["b_in"]) + pe
    for lay in w["layers"]:
        q, k, v = (x @ t(lay["W_qkv"]) + t(lay["b_qkv"])).split(H, 1)
        split = lambda a: a.reshape(T1, heads, H // heads).transpose(0, 1)
        att = F.scaled_dot_product_attention(split(q), split(k), split(v)).transpose(0, 1).reshape(T1, H)
        y = F.layer_norm(att + x, (T1, H), eps=1e-12) * t(lay["ln_a_gamma"]) + t(lay["ln_a_beta"])
        z = torch.relu(y @ t(lay["W1"]) + t(lay["b1"])) @ t(lay["W2"]) + t(lay["b2"])
        x = F.layer_norm(z + y, (T1, H), eps=1e-12) * t(lay["ln_b_gamma"]) + t(lay["ln_b_beta"])
    logits = x @ t(w["W_out"]) + t(w["b_out"])
    if cfg.use_relu:
        logits = torch.relu(logits)
    return logits.numpy(), torch.softmax(logits, 1).numpy()


@pytest.mark.parametrize("kw,T", [({}, 300), ({}, 37), (dict(combine_frame=1, hidden_size=64, multi_head_num=2, use_relu=False), 20),
                                  (dict(combine_frame=3, n_mel=13, hidden_size=256, multi_head_num=16, num_layers=2), 41)])
def test_restatement_agrees_with_an_independent_torch_build(kw, T):
    from keyword_spotting_amd import attention_weights as AW
    cfg = _cfg(**kw)
    w = AW.init(cfg, 3)
    mel = np.random.default_rng(T).standard_normal((T, cfg.n_mel)).astype(np.float32)
    l1, s1 = AM.forward(cfg, w, mel)
    l2, s2 = _torch_forward(cfg, w, mel)
    assert np.abs(l1 - l2).max() < 1e-10 and np.abs(s1 - s2).max() < 1e-10


def test_stacking_and_padding_rule():
    mel = np.arange(12 * 3, dtype=np.float64).reshape(12, 3) + 1
    s = AM.stack_frames(mel, 3)                        # T % c == 0: c pad frames, one whole extra row of zeros
    assert s.shape == (5, 9) and not s[4].any() and np.array_equal(s[0], mel[:3].ravel())
    s = AM.stack_frames(mel[:11], 3)                   # one pad frame
    assert s.shape == (4, 9) and np.array_equal(s[3], np.r_[mel[9], mel[10], np.zeros(3)])
    assert np.array_equal(AM.stack_frames(mel, 1), mel)           # c == 1: nothing appended
    assert AM.stack_frames(np.zeros((0, 3)), 2).shape == (1, 6)    # T == 0 at c > 1: one all-pad row
    assert [AM.frames_out(T, 2) for T in (0, 1, 2, 3, 300)] == [1, 1, 2, 2, 151]
    assert [AM.frames_out(T, 1) for T in (0, 5)] == [0, 5]


def test_whole_block_layer_norm_differs_from_per_row():
    x = np.array([[1.0, 3.0], [10.0, 30.0]])
    g, b = np.ones(2), np.zeros(2)
    whole = AM.layer_norm(x, g, b)
    rows = AM.layer_norm_rows(x, g, b)
    mu, sd = x.mean(), x.std()
    assert np.allclose(whole, (x - mu) / sd) and np.allclose(rows, [[-1, 1], [-1, 1]])
    assert np.abs(whole - rows).max() > 0.5


def test_pe_table_rows_and_float_rounding():
    pe = AM.pe_table(50, 128)
    assert pe.dtype == np.float32
    assert np.array_equal(pe[0], np.tile([0.0, 1.0], 64))
    p, i = 7, 5
    assert pe[p, 2 * i] == np.float32(np.sin(p / 10000.0 ** (2.0 * i / 128)))
    assert pe[p, 2 * i + 1] == np.float32(np.cos(p / 10000.0 ** (2.0 * i / 128)))


def test_converter_names_shapes_and_refusals(tmp_path):
    from keyword_spotting_amd import attention_weights as AW
    cfg = _cfg(num_layers=2)
    w = AW.init(cfg, 4)
    blob = AW.to_blob(cfg, w)
    for prefix, conv4d, suffix in (("model/", True, ":0"), ("", False, ""), ("model/", False, "")):
        v = {k + suffix: a for k, a in AW.to_tf_variables(cfg, w, prefix=prefix, conv4d=conv4d).items()}
        assert np.array_equal(AW.to_blob(cfg, AW.from_tf_variables(cfg, v)), blob)
    v = AW.to_tf_variables(cfg, w)
    assert "model/layer_1/feed_forward/conv2/kernel" in v and v["model/layer_1/feed_forward/conv2/kernel"].shape == (1, 1, 512, 128)
    assert "model/layer_0/LayerNorm_1/gamma" in v and "model/input_linear_trans/bias" in v
    missing = dict(v)
    del missing["model/layer_1/LayerNorm/beta"]
    with pytest.raises(ValueError, match="layer_1/LayerNorm/beta"):
        AW.from_tf_variables(cfg, missing)
    with pytest.raises(ValueError, match="model/global_step"):
        AW.from_tf_variables(cfg, dict(v, **{"model/global_step": np.zeros(())}))
    with pytest.raises(ValueError, match="layer_2"):
        AW.from_tf_variables(cfg, dict(v, **{"model/layer_2/LayerNorm/beta": np.zeros(128)}))
    bad = dict(v)
    bad["model/output_linear_trans/kernel"] = np.zeros((1, 1, 128, 5), np.float32)
    with pytest.raises(ValueError, match="output_linear_trans/kernel"):
        AW.from_tf_variables(cfg, bad)
    src = str(tmp_path / "vars.npz")
    np.savez(src, **v)
    tool = [sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), src, "--model", "attention", "--layers", "2"]
    ok = subprocess.run(tool + ["--out", str(tmp_path / "m")], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    assert np.array_equal(np.fromfile(str(tmp_path / "m.blob"), np.float32), blob)
    np.savez(src, **missing)
    bad_run = subprocess.run(tool + ["--out", str(tmp_path / "p")], capture_output=True, text=True)
    assert bad_run.returncode != 0 and "layer_1/LayerNorm/beta" in bad_run.stderr
    assert not os.path.exists(str(tmp_path / "p.blob"))


def _abi_cfg(cfg):
    from keyword_spotting_amd import _lib
    return _lib.KwsAttentionConfig(cfg.n_mel, cfg.combine_frame, cfg.hidden_size, cfg.multi_head_num,
                                   cfg.feed_forward_inner_size, cfg.num_layers, cfg.num_classes, int(cfg.use_relu), cfg.max_frames)


@pytest.mark.parametrize("kw", [{}, dict(combine_frame=1, n_mel=13, hidden_size=256, multi_head_num=8, num_layers=8,
                                         feed_forward_inner_size=1024, label_dict={"a": 1, "b": 2, "c": 3, "d": 4, "e": 5})])
def test_weights_nbytes_equals_the_python_blob(kw):
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd import attention_weights as AW
    cfg = _cfg(**kw)
    lib = _lib.load()
    assert lib.kws_attention_weights_nbytes(ctypes.byref(_abi_cfg(cfg))) == AW.to_blob(cfg, AW.init(cfg, 0)).nbytes
    assert lib.kws_sizeof_attention_config() == ctypes.sizeof(_lib.KwsAttentionConfig) == 36


@pytest.mark.parametrize("field,value", [("n_mel", 0), ("combine_frame", 5), ("combine_frame", 0), ("n_mel", 257),
                                         ("hidden", 96), ("num_heads", 2), ("num_heads", 16), ("num_heads", 3),
                                         ("ffn_inner", 500), ("ffn_inner", 1088), ("num_layers", 9), ("num_layers", 0),
                                         ("num_classes", 2), ("num_classes", 9), ("use_relu", 2), ("max_frames", 8193),
                                         ("max_frames", 0)])
def test_config_refusals_name_the_field(field, value):
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    c = _abi_cfg(_cfg())
    setattr(c, field, value)
    if field == "n_mel" and value == 257:
        want = b"n_mel*combine_frame"
    else:
        want = field.encode()
    assert lib.kws_attention_weights_nbytes(ctypes.byref(c)) == 0
    assert want in lib.kws_last_error()
    h = ctypes.c_void_p()
    blob = np.zeros(16, np.float32)
    assert lib.kws_attention_create(ctypes.byref(c), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ctypes.byref(h)) == \
        _lib.KWS_ERR_UNSUPPORTED
    assert want in lib.kws_last_error() and not h.value


def test_create_checks_the_blob_before_the_device_and_frames_out():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    c = _abi_cfg(_cfg())
    n = lib.kws_attention_weights_nbytes(ctypes.byref(c))
    blob = np.zeros(n // 4 - 1, np.float32)
    h = ctypes.c_void_p()
    assert lib.kws_attention_create(ctypes.byref(c), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ctypes.byref(h)) == \
        _lib.KWS_ERR_INVALID_ARGUMENT
    assert b"config needs %d" % n in lib.kws_last_error()
    assert lib.kws_attention_create(ctypes.byref(c), None, n, ctypes.byref(h)) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert [lib.kws_attention_frames_out(ctypes.byref(c), T) for T in (0, 1, 2, 300, 8192)] == [1, 1, 2, 151, 4097]
    c.combine_frame = 1
    assert [lib.kws_attention_frames_out(ctypes.byref(c), T) for T in (0, 7)] == [0, 7]
    assert lib.kws_attention_frames_out(ctypes.byref(c), -1) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_frames_out(None, 3) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_run(None, None, None, 1, 1, None, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_selftest(None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_destroy(None) == _lib.KWS_OK
