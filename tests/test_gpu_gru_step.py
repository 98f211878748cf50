"""The fp32 and f16x3 GRU kernels frame by frame at a measured bound: ONE-FRAME calls against tests/gru_step_model.py, which is
fed the device's own carried state and lower-layer output, so that the recurrence does not widen the comparison (the multi-frame
tests -- test_gpu_parity.py, test_gpu_config_space.py, test_gpu_resident_*.py, test_gpu_soak.py -- hold a flat 1e-4, some 25 times
what the kernels achieve).  One long call must then equal the chain of one-frame calls bit for bit -- logits, softmax, tokens,
state and prev_word, with and without lengths -- which brings the steady-state frame loop, the 16-frame epilogue ring and the fused
tokens under the same bound.  Every call asserts kernel_names(): a plan change that moves a case onto another kernel fails here
instead of leaving a family unchecked.

Each case prints `GRU-STEP <case> <kernel names>: worst err/bound state .., logits .., softmax ..`."""
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import config_space_grid as CS
import gru_step_model as M
from oracle import gru_oracle as G
from wrapped_cell_model import random_ln

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "family prec kernel n_mel hidden layers batch frames wrap relu clip wfc")


def C(family, prec, kernel, n_mel, hidden, layers, batch, frames, wrap=(False, False), relu=0, clip=-1.0, wfc=1.0):
    return Case(family, prec, kernel, n_mel, hidden, layers, batch, frames, wrap, relu, clip, wfc)


# the smallest shapes that reach each instantiation
CASES = [
    # fp32 resident: one layer (FIRST && LAST), a ragged second group, a middle layer, a single stream, past the 16-frame ring
    C("fp32_res", "fp32", "auto", 32, 128, 1, 16, 6), C("fp32_res", "fp32", "auto", 40, 128, 2, 17, 8),
    C("fp32_res", "fp32", "auto", 48, 128, 3, 33, 8), C("fp32_res", "fp32", "auto", 60, 128, 2, 1, 8),
    C("fp32_res", "fp32", "auto", 64, 128, 2, 16, 18),
    # fp32 generic / mixed: a single launch, a generic first layer under a resident one, the layer-pipelined launches
    C("fp32_gen", "fp32", "auto", 13, 64, 1, 17, 6), C("fp32_gen", "fp32", "auto", 100, 128, 2, 17, 8),
    C("fp32_gen", "fp32", "generic", 40, 128, 2, 33, 8), C("fp32_gen", "fp32", "auto", 60, 256, 2, 17, 6),
    C("fp32_gen", "fp32", "auto", 60, 256, 4, 16, 6),
    # wrapped (kws_create_wrapped): layer norm and residual, layer norm only, residual only
    C("wrapped", "fp32", "generic", 40, 128, 3, 17, 6, wrap=(True, True)), C("wrapped", "fp32", "generic", 13, 64, 2, 16, 6, wrap=(True, False)),
    C("wrapped", "fp32", "generic", 60, 256, 2, 17, 6, wrap=(False, True)),
    # f16x3 resident
    C("f16x3_res", "f16x3", "auto", 4, 128, 1, 1, 6), C("f16x3_res", "f16x3", "auto", 36, 128, 2, 17, 8),
    C("f16x3_res", "f16x3", "auto", 40, 128, 2, 16, 18), C("f16x3_res", "f16x3", "auto", 64, 128, 3, 33, 8),
    # f16x3 streaming (hidden 256): a single launch, the pipelined launch
    C("f16x3_gen", "f16x3", "auto", 60, 256, 1, 16, 6), C("f16x3_gen", "f16x3", "auto", 60, 256, 2, 17, 6),
    # relu + value_clip 20, Wfc scaled by 20 as the relu rows of config_space_grid.py
    C("relu_clip", "fp32", "auto", 40, 128, 2, 17, 8, relu=1, clip=20.0, wfc=20.0),
]


def case_id(c):
    tag = {(False, False): "", (True, True): "_ln_res", (True, False): "_ln", (False, True): "_res"}[tuple(c.wrap)]
    return "%s_%s_n%d_h%d_L%d_B%d_T%d%s" % (c.family, c.kernel, c.n_mel, c.hidden, c.layers, c.batch, c.frames, tag)


def _seed(c):
    return zlib.crc32(case_id(c)[:case_id(c).rindex("_B")].encode()) & 0x3FFFFFFF      # the case alone, whatever the batch


def _inputs(c):
    seed = _seed(c)
    w = G.random_weights(c.n_mel, c.hidden, c.layers, 6, seed=seed)
    if c.wrap[0]:
        random_ln(w, c.n_mel, seed + 3)
    w["Wfc"] = w["Wfc"] * np.float32(c.wfc)
    mel = G.synthetic_mel(c.batch, c.frames, c.n_mel, seed=seed + 1)
    st0 = (0.5 * np.random.default_rng(seed + 2).standard_normal((c.layers, c.batch, c.hidden))).astype(np.float32)
    return w, mel, st0


def _model(c, w):
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg = get_config(n_mel=c.n_mel, hidden_size=c.hidden, num_layers=c.layers, precision=c.prec, use_relu=bool(c.relu),
                     value_clip=c.clip, use_layer_norm=c.wrap[0], use_residual=c.wrap[1])
    return DeployModel(cfg, w, kernel="auto" if any(c.wrap) else c.kernel)


def _names(c, frames):
    """kernel_names() after a call of `frames` frames: config_space_grid.py's restatement of the plan; a wrapped handle takes
    the generic kernels' wrapped instantiations (tests/test_gpu_wrapped.py)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row = CS.R(case_id(c), c.prec, c.kernel, c.n_mel, c.hidden, c.layers, 6, c.batch, frames, "")
    names = CS.expected_names(row, c.batch, frames, cus)
    if any(c.wrap):
        names = [n.replace(">", ", wrapped>", 1) if n else n for n in names]
    return names


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _call(model, mel, state, pw, seq=None, reset=None):
    r = model.forward(torch.from_numpy(np.ascontiguousarray(mel)), state, prev_word=pw,
                      seq_len=None if seq is None else torch.from_numpy(seq), reset_mask=None if reset is None else torch.from_numpy(reset))
    torch.cuda.synchronize()
    return r


def _chain(model, c, w, mel, st0, seqs=None, resets=None):
    """T one-frame calls with the state and prev_word carried on the device, each through check_call.  seqs / resets: [T, B] or
    None.  -> dict(logits [B,T,C], softmax, tokens [B,T], state [L,B,H], prev_word [B], report)."""
    names = _names(c, 1)
    state = torch.from_numpy(st0).cuda()
    pw = model.fresh_prev_word(mel.shape[0])
    out = dict(logits=[], softmax=[], tokens=[], report=M.Report())
    before = st0
    for t in range(mel.shape[1]):
        seq = None if seqs is None else np.ascontiguousarray(seqs[t], np.int32)
        reset = None if resets is None else np.ascontiguousarray(resets[t], np.uint8)
        r = _call(model, mel[:, t:t + 1], state, pw, seq, reset)
        assert model.kernel_names() == names, (model.kernel_names(), names)
        new, lg, sm = _np(r["state"]), _np(r["logits"])[:, 0], _np(r["softmax"])[:, 0]
        out["report"].add(M.check_call(w, mel[:, t], before, new, lg, sm, seq, reset, precision=c.prec, wrap=c.wrap,
                                       use_relu=bool(c.relu), value_clip=c.clip))
        out["logits"].append(lg)
        out["softmax"].append(sm)
        out["tokens"].append(_np(r["tokens"])[:, 0])
        before, state = new, r["state"]
    for k in ("logits", "softmax", "tokens"):
        out[k] = np.stack(out[k], axis=1)
    out["state"], out["prev_word"] = before, _np(pw)
    return out


def _long_equals_chain(model, c, mel, st0, chain, lens=None):
    pw = model.fresh_prev_word(mel.shape[0])
    r = _call(model, mel, torch.from_numpy(st0).cuda(), pw, lens)
    assert model.kernel_names() == _names(c, mel.shape[1])
    for k in ("logits", "softmax", "tokens", "state"):
        assert np.array_equal(_bits(_np(r[k])), _bits(chain[k])), k
    assert np.array_equal(_np(pw), chain["prev_word"])


def _lens(b, t_len, seed):
    """Random lengths in [0, T] that include 0, 1 and T where the batch has room for them."""
    lens = np.random.default_rng(seed).integers(0, t_len + 1, b).astype(np.int32)
    for k, v in enumerate((t_len, 1, 0)[:b]):
        lens[(5 * k) % b if b >= 11 else k] = v
    return lens


def _report(c, rep, tag=""):
    print(rep.line(case_id(c) + tag, _names(c, 1)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_frame_chain_against_the_restatement_and_long_call_equals_chain(case):
    c = case
    w, mel, st0 = _inputs(c)
    model = _model(c, w)
    plain = _chain(model, c, w, mel, st0)
    _report(c, plain["report"])
    if c.relu:
        assert plain["logits"].min() == 0.0 and plain["logits"].max() == 20.0       # both ends of the clip are reached
    _long_equals_chain(model, c, mel, st0, plain)
    rng = np.random.default_rng(_seed(c) + 5)
    seqs = rng.integers(0, 2, (c.frames, c.batch)).astype(np.int32)
    seqs[0, 0] = 1
    resets = (rng.random((c.frames, c.batch)) < 0.3).astype(np.uint8)
    masked = _chain(model, c, w, mel, st0, seqs, resets)
    _report(c, masked["report"], " masked")
    lens = _lens(c.batch, c.frames, _seed(c) + 6)
    by_len = _chain(model, c, w, mel, st0, seqs=(np.arange(c.frames)[:, None] < lens[None, :]).astype(np.int32))
    _report(c, by_len["report"], " lengths")
    _long_equals_chain(model, c, mel, st0, by_len, lens)
    model.close()


def test_sequential_generic_launches():
    """hidden 128, two layers on the generic kernels, a batch whose layers x groups workgroups no longer fit the chip at once: one
    gru_layer_generic launch per layer through the seam in memory.  Every stream is checked."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = C("fp32_seq", "fp32", "generic", 40, 128, 2, CS.sequential_batch(2, cus), 2)
    assert CS.groups(c.batch) * c.layers > cus and _names(c, 1) == ["gru_layer_generic<2, true, false>", "gru_layer_generic<2, false, true>"]
    w, mel, st0 = _inputs(c)
    model = _model(c, w)
    chain = _chain(model, c, w, mel, st0)
    _report(c, chain["report"])
    _long_equals_chain(model, c, mel, st0, chain)
    model.close()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_persistent_workgroups_every_stream_checked(prec):
    """B = 16 x CUs + 17: every workgroup of the resident kernels walks a second stream group, one a third (ragged) one."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = C("%s_persistent" % prec, prec, "auto", 40, 128, 2, 16 * cus + 17, 2)
    assert all(("gru_layer_resident" if prec == "fp32" else "gru_layer_f16x3<") in n for n in _names(c, 1))
    w, mel, st0 = _inputs(c)
    model = _model(c, w)
    chain = _chain(model, c, w, mel, st0)
    _report(c, chain["report"])
    _long_equals_chain(model, c, mel, st0, chain)
    lens = _lens(c.batch, c.frames, _seed(c) + 6)
    by_len = _chain(model, c, w, mel, st0, seqs=(np.arange(c.frames)[:, None] < lens[None, :]).astype(np.int32))
    _report(c, by_len["report"], " lengths")
    _long_equals_chain(model, c, mel, st0, by_len, lens)
    model.close()
