"""The cell wrappers on the GPU (kws_create_wrapped: ResidualWrapper(LayerNormalizer(GRUCell)), models/rnn_ctc.py:179-199)
against the fp64 restatement (tests/wrapped_cell_model.py), and bitwise against themselves across launch layouts, chunking,
masks and the plain path.  The layouts are restated from tests/config_space_grid.py (a wrapped handle is never resident)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import config_space_grid as CS
from conftest import ROOT
from oracle import decode_oracle as D
from oracle import gru_oracle as G
from wrapped_cell_model import random_ln, wrapped_forward

pytestmark = pytest.mark.gpu

WRAPS = {"ln": (True, False), "res": (False, True), "ln_res": (True, True)}
# (n_mel, hidden, layers, batch): the first three fit the chip as one layer-pipelined grid, (13,64,1) is a single launch,
# (100,64,5) at 900 streams is past the pipelined launch's size (sequential launches)
SHAPES = [(40, 128, 2, 1024), (60, 128, 3, 1024), (60, 256, 4, 1024), (13, 64, 1, 64), (100, 64, 5, 900)]
T = 20
SAMPLE = 48


def _cfg(n_mel, hidden, layers, ln, res):
    from keyword_spotting_amd import get_config
    return get_config(n_mel=n_mel, hidden_size=hidden, num_layers=layers, use_layer_norm=ln, use_residual=res)


def _weights(n_mel, hidden, layers, seed, ln):
    w = G.random_weights(n_mel, hidden, layers, 6, seed)
    return random_ln(w, n_mel, seed) if ln else w


def _mel(batch, frames, n_mel, seed):
    mel = G.synthetic_mel(batch, frames, n_mel, seed=seed)
    mel[: batch // 2] += 50.0                       # a large DC part: mean first, then the variance around it
    return np.ascontiguousarray(mel, np.float32)


def _layout(n_mel, hidden, layers, batch, frames):
    row = CS.R("wrapped", "fp32", "generic", n_mel, hidden, layers, 6, batch, frames, "")
    return CS.layout_of(row, batch, frames, torch.cuda.get_device_properties(0).multi_processor_count)


def _names(n_mel, hidden, layers, batch, frames):
    lay = _layout(n_mel, hidden, layers, batch, frames)
    if lay == "pipe":
        return [""] * (layers - 1) + ["gru_stack_generic_pipelined<%d, wrapped> (all %d layers, one launch)" % (hidden // 64, layers)]
    return ["gru_layer_generic<%d, %s, %s, wrapped>" % (hidden // 64, CS._tf(l == 0), CS._tf(l == layers - 1)) for l in range(layers)]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _run(model, mel, state, **kw):
    pw = model.fresh_prev_word(mel.shape[0])
    r = model.forward(torch.from_numpy(mel), torch.from_numpy(state) if isinstance(state, np.ndarray) else state, prev_word=pw, **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("wrap", list(WRAPS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_h%d_L%d_B%d" % s)
def test_wrapped_against_the_restatement(shape, wrap):
    from keyword_spotting_amd.rnn_ctc import DeployModel
    n_mel, hidden, layers, batch = shape
    ln, res = WRAPS[wrap]
    seed = 300 + SHAPES.index(shape) * 3 + list(WRAPS).index(wrap)
    cfg = _cfg(n_mel, hidden, layers, ln, res)
    w = _weights(n_mel, hidden, layers, seed, ln)
    model = DeployModel(cfg, w)
    rng = np.random.default_rng(seed)
    mel = _mel(batch, T, n_mel, seed)
    state = (0.5 * rng.standard_normal((layers, batch, hidden))).astype(np.float32)
    r = _run(model, mel, state)
    assert model.kernel_names() == _names(n_mel, hidden, layers, batch, T)
    pick = np.sort(rng.choice(batch, min(SAMPLE, batch), replace=False))
    want_l, want_s = wrapped_forward(w, mel[pick], ln, res, state=state[:, pick])
    lg, sm = r["logits"].cpu().numpy()[pick], r["softmax"].cpu().numpy()[pick]
    assert np.abs(lg - want_l).max() < 1e-4, (shape, wrap, np.abs(lg - want_l).max())
    assert np.abs(r["state"].cpu().numpy()[:, pick] - want_s).max() < 1e-4
    want_sm = G.softmax(want_l)
    assert np.abs(sm - want_sm).max() < 2e-5
    # fused ctc_decode2 tokens: the restatement's softmax decoded, on the streams that are not within 1e-4 of a decision
    from keyword_spotting_amd.prediction import tokens_to_seq
    tokens = r["tokens"].cpu().numpy()[pick]
    checked = 0
    for k in range(len(pick)):
        p = np.sort(want_sm[k][:, 1:5], axis=1)
        if (np.abs(p[:, -1] - 0.4) > 1e-4).all() and (p[:, -1] - p[:, -2] > 1e-4).all():
            assert np.array_equal(tokens_to_seq(tokens[k]), D.ctc_decode2(want_sm[k], 6)), (shape, wrap, k)
            checked += 1
    assert checked > 0

    # bitwise: chunked == one call; rows past seq_len emit bfc and hold the state; reset_mask == a zero state
    a = _run(model, mel[:, :9].copy(), state)
    b = _run(model, mel[:, 9:].copy(), a["state"])
    assert torch.equal(_bits(torch.cat([a["logits"], b["logits"]], 1)), _bits(r["logits"]))
    assert torch.equal(_bits(b["state"]), _bits(r["state"]))
    seq = rng.integers(0, T + 1, batch).astype(np.int32)
    m = _run(model, mel, state, seq_len=torch.from_numpy(seq))
    dead = np.arange(T)[None, :] >= seq[:, None]
    bfc = np.broadcast_to(w["bfc"], (batch, T, 6))
    assert np.array_equal(m["logits"].cpu().numpy()[dead].view(np.int32), bfc[dead].view(np.int32))
    held = _run(model, mel, m["state"], seq_len=torch.zeros(batch, dtype=torch.int32))
    assert torch.equal(_bits(held["state"]), _bits(m["state"]))
    assert np.array_equal(held["logits"].cpu().numpy().view(np.int32), bfc.view(np.int32))
    mask = (rng.random(batch) < 0.3).astype(np.uint8)
    z = state.copy()
    z[:, mask.astype(bool)] = 0.0
    got = _run(model, mel, state, reset_mask=torch.from_numpy(mask))
    want = _run(model, mel, z)
    assert torch.equal(_bits(got["logits"]), _bits(want["logits"])) and torch.equal(_bits(got["state"]), _bits(want["state"]))
    assert torch.equal(got["tokens"], want["tokens"])

    if _layout(n_mel, hidden, layers, batch, T) == "pipe":
        # the same streams in a batch past the pipelined launch's size: sequential launches, the same bits
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        big = CS.sequential_batch(layers, cus)
        mel2 = np.concatenate([mel, _mel(big - batch, T, n_mel, seed + 1)])
        st2 = np.concatenate([state, np.zeros((layers, big - batch, hidden), np.float32)], 1)
        r2 = _run(model, mel2, st2)
        assert _layout(n_mel, hidden, layers, big, T) == "seq"
        assert model.kernel_names() == _names(n_mel, hidden, layers, big, T)
        assert torch.equal(_bits(r2["logits"][:batch]), _bits(r["logits"]))
        assert torch.equal(_bits(r2["state"][:, :batch]), _bits(r["state"]))
    model.close()


_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
from keyword_spotting_amd.rnn_ctc import DeployModel
import test_gpu_wrapped as TW
out = {}
for name, (n_mel, hidden, layers, batch, frames) in %(cases)r:
    ln, res = True, True
    cfg = TW._cfg(n_mel, hidden, layers, ln, res)
    w = TW._weights(n_mel, hidden, layers, 77, ln)
    model = DeployModel(cfg, w)                   # KWS_SELFTEST=1: the create runs kws_selftest on the wrapped kernels
    mel = TW._mel(batch, frames, n_mel, 78)
    st = np.zeros((layers, batch, hidden), np.float32)
    r = TW._run(model, mel, st)
    out[name] = dict(names=model.kernel_names(), logits=r["logits"].cpu().numpy().tolist(), state=r["state"].cpu().numpy().tolist())
    model.close()
json.dump(out, open(sys.argv[1], "w"))
"""


def test_overlapped_layout_and_selftest_hook_in_a_child(tmp_path):
    """KWS_NO_PIPELINE=1 (a device without fine-grained memory): a batch that fits the chip runs its layers overlapped on HIP
    streams when T >= 64.  The same bits as the layer-pipelined launch of this process.  KWS_SELFTEST=1 makes every create
    prove the wrapped kernels first."""
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cases = [("ovl", (40, 128, 2, 256, 64)), ("ovl4", (60, 256, 4, 64, 70))]
    env = dict(os.environ, KWS_NO_PIPELINE="1", KWS_SELFTEST="1")
    out = tmp_path / "child.json"
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, cases=cases), str(out)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.load(open(out))
    for name, (n_mel, hidden, layers, batch, frames) in cases:
        assert child[name]["names"] == ["gru_layer_generic<%d, %s, %s, wrapped>" % (hidden // 64, CS._tf(l == 0), CS._tf(l == layers - 1))
                                        for l in range(layers)]
        w = _weights(n_mel, hidden, layers, 77, True)
        model = DeployModel(_cfg(n_mel, hidden, layers, True, True), w)
        mel = _mel(batch, frames, n_mel, 78)
        got = _run(model, mel, np.zeros((layers, batch, hidden), np.float32))
        assert _layout(n_mel, hidden, layers, batch, frames) == "pipe"
        assert model.kernel_names() == _names(n_mel, hidden, layers, batch, frames)
        assert np.array_equal(np.asarray(child[name]["logits"], np.float32).view(np.int32), got["logits"].cpu().numpy().view(np.int32))
        assert np.array_equal(np.asarray(child[name]["state"], np.float32).view(np.int32), got["state"].cpu().numpy().view(np.int32))
        model.close()


def test_null_wrappers_and_single_layer_residual_are_the_plain_path():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg = _cfg(13, 64, 1, False, False)
    w = G.random_weights(13, 64, 1, 6, 9)
    mel = _mel(33, 24, 13, 10)
    st = np.zeros((1, 33, 64), np.float32)
    plain = DeployModel(cfg, w)
    want = _run(plain, mel, st)
    res1 = DeployModel(_cfg(13, 64, 1, False, True), w)
    got = _run(res1, mel, st)
    assert torch.equal(_bits(got["logits"]), _bits(want["logits"])) and torch.equal(_bits(got["state"]), _bits(want["state"]))
    assert res1.kernel_names() == ["gru_layer_generic<1, true, true, wrapped>"]
    # kws_create_wrapped(NULL) and all-zero wrappers: kws_create exactly, kernels included
    for shape in ((13, 64, 1), (40, 128, 2)):
        cfgp = _cfg(*shape, False, False)
        wp = G.random_weights(*shape, 6, 11)
        melp = _mel(40, 24, shape[0], 12)
        stp = np.zeros((shape[2], 40, shape[1]), np.float32)
        ref = DeployModel(cfgp, wp)
        want = _run(ref, melp, stp)
        for wrap in (None, _lib.KwsCellWrappers(0, 0)):
            m = DeployModel(cfgp, wp)
            lib = m._lib
            lib.kws_destroy(m._handle)
            blob = G.weights_to_blob(wp)
            m._handle = ctypes.c_void_p()
            _lib.check(lib.kws_create_wrapped(ctypes.byref(m._cfg), None if wrap is None else ctypes.byref(wrap),
                                              blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ctypes.byref(m._handle)))
            got = _run(m, melp, stp)
            assert m.kernel_names() == ref.kernel_names()
            assert torch.equal(_bits(got["logits"]), _bits(want["logits"])) and torch.equal(_bits(got["state"]), _bits(want["state"]))
            m.close()
        ref.close()
    plain.close()
    res1.close()


def test_resident_refused_auto_generic_and_selftest():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.rnn_ctc import DeployModel
    for ln, res in WRAPS.values():
        w = _weights(40, 128, 2, 21, ln)
        m = DeployModel(_cfg(40, 128, 2, ln, res), w)
        with pytest.raises(_lib.UnsupportedError, match="resident"):
            m.set_kernel("resident")
        m.set_kernel("auto")
        _run(m, _mel(16 * 300, 4, 40, 22), np.zeros((2, 16 * 300, 128), np.float32))     # past the pipelined size
        assert m.kernel_names() == ["gru_layer_generic<2, true, false, wrapped>", "gru_layer_generic<2, false, true, wrapped>"]
        m.selftest()
        m.close()
    for shape in ((13, 64, 1), (100, 256, 3)):
        m = DeployModel(_cfg(*shape, True, True), _weights(*shape, 23, True))
        m.selftest()
        m.close()


def test_stream_manager_equals_the_host_mirror():
    """LN + residual at (40,128,2): 64 streams x 12 ragged periods through kws_stream_feed_ragged (window_inc_kernel behind
    the wrapped GRU launches) against a HotwordDetector per stream fed its own chunks: hits, state and carry bit for bit."""
    from keyword_spotting_amd.detector import HotwordDetector, StreamManager
    from keyword_spotting_amd.frontend import MelFrontend
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg = _cfg(40, 128, 2, True, True)
    fe = MelFrontend(cfg)
    rng = np.random.default_rng(8200)
    B, periods = 64, 12
    noise = torch.from_numpy((rng.standard_normal((48, 16000)) * 0.2).astype(np.float32))
    for seed in range(7200, 7260):                  # as test_gpu_serve.py::_emitting: a model that says something on noise
        w = _weights(40, 128, 2, seed, True)
        w["Wfc"] = (w["Wfc"] * 2.0).astype(np.float32)
        model = DeployModel(cfg, w)
        sm = model.forward(fe.forward(noise), model.zero_state(48), want_logits=False)["softmax"].cpu().numpy()
        words = np.concatenate([D.ctc_decode2(sm[k], 6)[1::2] for k in range(48)])
        if words.size >= 96:
            label = str(int(np.bincount(words).argmax()))
            break
        model.close()
    else:
        raise AssertionError("no seed gives a wrapped model that emits words")
    lens = rng.choice([0, 150, 1800, 3600, 5000], size=(B, periods), p=[0.15, 0.1, 0.2, 0.4, 0.15]).astype(np.int32)
    pcm = [rng.integers(-6000, 6000, (B, 5000)).astype(np.int16) for _ in range(periods)]
    for p in range(periods):
        pcm[p][rng.random(B) < 0.05] //= 4096
    mgr = StreamManager(model, B, label=label, window_chunks=4)
    hits = np.zeros((B, periods), np.int32)
    for p in range(periods):
        hits[:, p] = mgr.feed_pcm(torch.from_numpy(pcm[p]).cuda(), fe, lengths=torch.from_numpy(lens[:, p])).cpu().numpy()
    torch.cuda.synchronize()
    assert hits.sum() > 0, "no trigger: the run does not cover reset-on-trigger"
    samples, clen = mgr.carry()
    for b in range(B):
        det = HotwordDetector(model, 1, window_chunks=4, label=label)
        for p in range(periods):
            n = int(lens[b, p])
            if n == 0:
                assert hits[b, p] == 0
                continue
            fired = det.feed_pcm(torch.from_numpy(pcm[p][b:b + 1, :n].copy()), fe)
            assert hits[b, p] == (1 if fired else 0), (b, p)
        torch.cuda.synchronize()
        assert torch.equal(_bits(mgr.state[:, b]), _bits(det.state[:, 0])), b
        n_c = int(clen[b])
        assert n_c == det.res.shape[1] and torch.equal(_bits(samples[b, :n_c]), _bits(det.res[0])), b
    mgr.close()
    model.close()


def test_converted_checkpoint_through_model_and_stream_manager(tmp_path):
    """A TF-variable .npz with LayerNormalizer entries -> tools/convert_weights.py --layer-norm --residual -> the blob through
    DeployModel and StreamManager.feed, within 1e-4 of the restatement."""
    from keyword_spotting_amd import weights as W
    from keyword_spotting_amd.detector import StreamManager
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg = _cfg(40, 128, 2, True, True)
    w = _weights(40, 128, 2, 31, True)
    src = str(tmp_path / "vars.npz")
    np.savez(src, **W.to_tf_variables(w))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), src, "--out", str(tmp_path / "m"),
                        "--layer-norm", "--residual"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blob = np.fromfile(str(tmp_path / "m.blob"), np.float32)
    model = DeployModel(cfg, blob)
    B, chunks = 40, (22, 9, 30)
    mel = _mel(B, sum(chunks), 40, 32)
    got = _run(model, mel, np.zeros((2, B, 128), np.float32))
    want_l, want_s = wrapped_forward(w, mel, True, True)
    assert np.abs(got["logits"].cpu().numpy() - want_l).max() < 1e-4
    assert np.abs(got["state"].cpu().numpy() - want_s).max() < 1e-4
    mgr = StreamManager(model, B, label="9", window_chunks=4)        # words are 1..4 here: "9" never triggers, no reset
    t0 = 0
    for n in chunks:
        mgr.feed(torch.from_numpy(mel[:, t0:t0 + n].copy()).cuda())
        t0 += n
    torch.cuda.synchronize()
    assert np.abs(mgr.state.cpu().numpy() - want_s).max() < 1e-4
    mgr.close()
    model.close()
