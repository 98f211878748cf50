"""tests/gru_step_model.py on the CPU: its fp64 run IS the oracle, its bound accepts a correct float32 / split-fp16 cell with
room to spare, and it rejects three numeric slips that all stay below the 1e-4 the multi-frame GPU tests hold."""
import numpy as np
import pytest

import gru_step_model as M
from oracle import gru_oracle as G
from wrapped_cell_model import random_ln, wrapped_forward

SHAPES = [(40, 128, 2), (60, 256, 2), (13, 64, 1)]          # n_mel, hidden, layers
B = 33
OLD_TOL = 1e-4            # TOL of test_gpu_parity.py, test_gpu_config_space.py, test_gpu_resident_*.py, test_gpu_soak.py


def _ids(s):
    return "n%d_h%d_L%d" % s


def _inputs(shape, frames=1, ln=False):
    n_mel, hidden, layers = shape
    seed = 7100 + 10 * SHAPES.index(shape)
    w = G.random_weights(n_mel, hidden, layers, 6, seed=seed)
    if ln:
        random_ln(w, n_mel, seed + 3)
    mel = G.synthetic_mel(B, frames, n_mel, seed=seed + 1)
    st0 = (0.5 * np.random.default_rng(seed + 2).standard_normal((layers, B, hidden))).astype(np.float32)
    return w, mel, st0


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fp64_chain_is_the_oracle(shape):
    w, mel, st0 = _inputs(shape, frames=20)
    state = st0.astype(np.float64)
    logits = []
    for t in range(20):
        state, top = M.stack_step(w, mel[:, t], state, "f64")
        logits.append(M.project(top, w, "f64"))
    want_l, want_s = G.gru_forward(w, mel, state=st0, dtype=np.float64)
    assert np.abs(state - want_s).max() <= 1e-12
    assert np.abs(np.stack(logits, 1) - want_l).max() <= 1e-12


@pytest.mark.parametrize("wrap", [(True, False), (False, True), (True, True)], ids=["ln", "res", "ln_res"])
@pytest.mark.parametrize("shape", [(40, 128, 3), (13, 64, 2)], ids=_ids)
def test_fp64_chain_of_a_wrapped_stack_is_wrapped_forward(shape, wrap):
    n_mel, hidden, layers = shape
    w = G.random_weights(n_mel, hidden, layers, 6, seed=7200)
    if wrap[0]:
        random_ln(w, n_mel, 7203)
    mel = G.synthetic_mel(B, 20, n_mel, seed=7201)
    st0 = (0.5 * np.random.default_rng(7202).standard_normal((layers, B, hidden))).astype(np.float32)
    state = st0.astype(np.float64)
    logits = []
    for t in range(20):
        state, top = M.stack_step(w, mel[:, t], state, "f64", wrap)
        logits.append(M.project(top, w, "f64"))
    want_l, want_s = wrapped_forward(w, mel, wrap[0], wrap[1], state=st0)
    assert np.abs(state - want_s).max() <= 1e-12
    assert np.abs(np.stack(logits, 1) - want_l).max() <= 1e-12


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_check_call_accepts_the_yardstick_run(shape, precision):
    w, mel, st0 = _inputs(shape)
    state, logits, softmax = M.emulate_call(w, mel[:, 0], st0, precision)
    res = M.check_call(w, mel[:, 0], st0, state, logits, softmax, precision=precision)
    print("GRU-STEP host %s %s: err/bound state %.3f, logits %.3f, softmax %.3f" % (_ids(shape), precision, res["state"], res["logits"], res["softmax"]))
    assert res["state"] <= 0.25 and res["logits"] <= 0.25 and res["softmax"] <= 0.25, res


def test_check_call_accepts_a_wrapped_relu_masked_call():
    """Layer norm and residual, relu with the clip, rows with seq_len 0 and reset rows through the same bound."""
    w, mel, st0 = _inputs((40, 128, 2), ln=True)
    w["Wfc"] = w["Wfc"] * np.float32(20.0)
    rng = np.random.default_rng(7)
    seq = rng.integers(0, 2, B).astype(np.int32)
    reset = (rng.random(B) < 0.3).astype(np.uint8)
    kw = dict(wrap=(True, True), use_relu=True, value_clip=20.0, seq_len=seq, reset=reset)
    state, logits, softmax = M.emulate_call(w, mel[:, 0], st0, "fp32", **kw)
    assert logits.min() == 0.0 and logits.max() == 20.0
    res = M.check_call(w, mel[:, 0], st0, state, logits, softmax, precision="fp32", **kw)
    assert res["state"] <= 0.25 and res["logits"] <= 0.25 and res["softmax"] <= 0.25, res
    moved = state.copy()
    moved[1, np.flatnonzero(seq == 0)[0], 5] += np.float32(1e-6)
    with pytest.raises(AssertionError, match="seq_len 0"):
        M.check_call(w, mel[:, 0], st0, moved, logits, softmax, precision="fp32", **kw)


# (name, precision, mutant, err / bound that check_call must exceed)
MUTANTS = [("lo_chunk_zeroed", "f16x3", dict(zero_lo_chunk=1), 2.0),
           ("sigmoid_2e-5", "fp32", dict(sigmoid_eps=2e-5), 2.0),
           ("sigmoid_2e-5", "f16x3", dict(sigmoid_eps=2e-5), 2.0),
           ("sigmoid_5e-6", "fp32", dict(sigmoid_eps=5e-6), 1.2),
           ("sigmoid_5e-6", "f16x3", dict(sigmoid_eps=5e-6), 1.2)]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: "%s_%s" % (m[0], m[1]))
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_power_a_mutant_below_the_old_tolerance_is_rejected(shape, mutant):
    name, precision, mut, must_exceed = mutant
    w, mel, st0 = _inputs(shape)
    state, logits, softmax = M.emulate_call(w, mel[:, 0], st0, precision, **mut)
    # the fp64 stack on ITS OWN values: what the multi-frame tests compare with
    want_s, top = M.stack_step(w, mel[:, 0], st0, "f64")
    want_l = M.project(top, w, "f64")
    err_s, err_l = np.abs(state - want_s).max(), np.abs(logits - want_l).max()
    res = M.check_call(w, mel[:, 0], st0, state, logits, softmax, precision=precision, enforce=False)
    print("GRU-STEP host mutant %s %s %s: max err state %.2e logits %.2e, err/bound state %.2f logits %.2f" % (
        name, precision, _ids(shape), err_s, err_l, res["state"], res["logits"]))
    assert err_s < OLD_TOL and res["err_state"] < OLD_TOL, (err_s, res["err_state"])
    assert res["state"] > must_exceed, res
    with pytest.raises(AssertionError, match="outside the bound"):
        M.check_call(w, mel[:, 0], st0, state, logits, softmax, precision=precision)


def test_a_tanh_slip_and_a_scaled_logit_are_rejected():
    """tanh_eps and the logits bound: 2e-5 on the tanh moves h' by (1 - u) 2e-5; one wave's share of the logits off by 1e-5
    (the relative slip of a scaled partial sum) leaves the state alone and fails the logits."""
    w, mel, st0 = _inputs((40, 128, 2))
    state, logits, softmax = M.emulate_call(w, mel[:, 0], st0, "fp32", tanh_eps=2e-5)
    assert M.check_call(w, mel[:, 0], st0, state, logits, softmax, enforce=False)["state"] > 2.0
    state, logits, softmax = M.emulate_call(w, mel[:, 0], st0, "fp32")
    part = state[-1][:, :32].astype(np.float64) @ w["Wfc"][:32].astype(np.float64)
    off = (logits + 1e-5 * part).astype(np.float32)
    assert np.abs(off - logits).max() < OLD_TOL
    res = M.check_call(w, mel[:, 0], st0, state, off, M.softmax32(off), enforce=False)
    assert res["logits"] > 2.0 and res["state"] <= 0.25, res
