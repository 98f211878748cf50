"""The f16x3 attention path without a GPU: the rounding model of its arithmetic (tests/attention_f16x3_model.py) against the fp64
restatement, and the validation of kws_attention_create_precision, which runs before the device is probed."""
import ctypes

import numpy as np
import pytest

import attention_f16x3_model as FM
import attention_model as AM
from conftest import have_gpu

# half the GPU tests' tolerances (tests/test_gpu_attention.py: 1e-4 / 2e-5): the model has no ordering noise of its own to spend
LOGIT_BOUND, SOFTMAX_BOUND = 5e-5, 1e-5

# tests/test_gpu_attention.py's GRID: (combine_frame, n_mel, hidden, heads, ffn_inner, layers, classes, relu)
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


def _weights(cfg, seed):
    from keyword_spotting_amd import attention_weights as AW
    return AW.init(cfg, seed)


def _grid_cfg(c, F, H, heads, Fi, L, C, relu):
    return _cfg(combine_frame=c, n_mel=F, hidden_size=H, multi_head_num=heads, feed_forward_inner_size=Fi, num_layers=L,
                use_relu=relu, max_frames=200, label_dict={str(i): i for i in range(1, C - 2)})


def _cases():
    """(name, cfg, weights, [utterances]): the ten grid shapes at T = 75 (lengths 75 / 1 / 33), the reference shape at T = 300 as it is,
    with peaky posteriors (W_out x 6) and with tiny and MFCC-sized inputs."""
    for i, g in enumerate(GRID):
        cfg = _grid_cfg(*g)
        mel = np.random.default_rng(g[2] + g[4]).standard_normal((3, 75, g[1])).astype(np.float32)
        yield "grid%d" % i, cfg, _weights(cfg, g[0] * 1000 + g[2] + g[5]), [mel[0], mel[1, :1], mel[2, :33]]
    cfg = _cfg()
    w = _weights(cfg, 1)
    mel = np.random.default_rng(2).standard_normal((300, cfg.n_mel)).astype(np.float32)
    yield "reference", cfg, w, [mel]
    yield "reference, W_out x 6", cfg, dict(w, W_out=w["W_out"] * np.float32(6.0)), [mel]
    yield "reference, mel x 1e-4", cfg, w, [mel * np.float32(1e-4)]
    yield "reference, mel x 300 - 50", cfg, w, [mel * np.float32(300.0) - np.float32(50.0)]


@pytest.fixture(scope="module")
def deviations():
    """name -> (max |logit - fp64|, max |softmax - fp64|) of the scaled-lo model and of the one-piece model (lo products dropped)."""
    out = {}
    for name, cfg, w, utts in _cases():
        d = np.zeros((2, 2))
        for mel in utts:
            want = AM.forward(cfg, w, mel)
            for i, pieces in enumerate((2, 1)):
                got = FM.forward(cfg, w, mel, pieces=pieces)
                d[i] = np.maximum(d[i], [np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max()])
        out[name] = d
        print("%-28s f16x3 %.2e / %.2e   one piece %.2e / %.2e" % (name, d[0, 0], d[0, 1], d[1, 0], d[1, 1]))
    return out


def test_three_products_with_scaled_lo_pieces_stay_within_half_the_tolerances(deviations):
    for name, d in deviations.items():
        assert d[0, 0] < LOGIT_BOUND and d[0, 1] < SOFTMAX_BOUND, (name, d[0])


def test_one_fp16_piece_per_operand_does_not_meet_the_logit_tolerance(deviations):
    """Why three products: with the lo products dropped the logits leave the GPU tests' 1e-4."""
    assert max(d[1, 0] for d in deviations.values()) > 1e-4


def _create(cfg, precision, blob, cfg_null=False, blob_null=False, out_null=False):
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    c = _lib.KwsAttentionConfig(int(cfg.freq_size), int(cfg.combine_frame), int(cfg.hidden_size), int(cfg.multi_head_num),
                                int(cfg.feed_forward_inner_size), int(cfg.num_layers), int(cfg.num_classes), int(bool(cfg.use_relu)),
                                int(cfg.max_frames))
    h = ctypes.c_void_p()
    rc = lib.kws_attention_create_precision(None if cfg_null else ctypes.byref(c), precision,
                                            None if blob_null else blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes,
                                            None if out_null else ctypes.byref(h))
    msg = lib.kws_last_error().decode()
    if rc == _lib.KWS_OK:
        lib.kws_attention_destroy(h)
    return rc, msg


def test_create_precision_returns_the_documented_codes_before_it_looks_for_a_device():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd import attention_weights as AW
    cfg = _cfg(max_frames=64)
    w = _weights(cfg, 3)
    blob = AW.to_blob(cfg, w)
    for prec, name in ((_lib.BF16, "KWS_BF16"), (_lib.INT8, "KWS_INT8")):
        rc, msg = _create(cfg, prec, blob)
        assert rc == _lib.KWS_ERR_UNSUPPORTED and name in msg, (rc, msg)
    assert _create(cfg, 17, blob)[0] == _lib.KWS_ERR_UNSUPPORTED
    w["layers"][1]["W1"][3, 5] = 64.0
    rc, msg = _create(cfg, _lib.F16X3, AW.to_blob(cfg, w))
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "W1" in msg and "layer 1" in msg and "64" in msg, (rc, msg)
    w["layers"][1]["W1"][3, 5] = np.nan
    assert _create(cfg, _lib.F16X3, AW.to_blob(cfg, w))[0] == _lib.KWS_ERR_UNSUPPORTED
    for kw in (dict(cfg_null=True), dict(blob_null=True), dict(out_null=True)):
        assert _create(cfg, _lib.F16X3, blob, **kw)[0] == _lib.KWS_ERR_INVALID_ARGUMENT, kw
    assert _create(cfg, _lib.F16X3, blob[:-1])[0] == _lib.KWS_ERR_INVALID_ARGUMENT
    # a valid request gets as far as the device
    for prec in (_lib.FP32, _lib.F16X3):
        assert _create(cfg, prec, blob)[0] == (_lib.KWS_OK if have_gpu() else _lib.KWS_ERR_NO_DEVICE)


def test_deploy_model_refuses_an_unknown_precision_before_anything_else():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.attention_ctc import DeployModel
    cfg = _cfg(max_frames=64)
    with pytest.raises(_lib.UnsupportedError):
        DeployModel(cfg, _weights(cfg, 4), precision="bf16")
