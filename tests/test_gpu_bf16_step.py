"""The bf16 GRU stack (csrc/gru_bf16.hip) frame by frame at fp32 accuracy: ONE-FRAME calls against tests/bf16_step_model.py,
which is fed the device's own carried state and lower-layer output, so that neither the recurrence nor a bf16 tie widens the
comparison (the multi-frame tests -- test_gpu_bf16.py, the bf16 rows of test_gpu_config_space.py, test_gpu_fullsize.py,
test_gpu_parity.py -- hold 6e-2 on the logits for that reason).  One long call must then equal the chain of one-frame calls
bit for bit, which brings the skewed steady state of the two-layer kernels (layer 1 of frame i beside layer 0 of frame i+1,
never executed by a one-frame call) and the later rounds of a persistent workgroup under the same tight check.  The 4-wave
two-layer kernel gru_stack_bf16<KX0, 2> (KWS_BF16_WAVES=4, read once per process) runs in a child process.

Each case prints `BF16-STEP <case> <kernel>: worst err/bound plain .., with allowance .., allowance rows .. %`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_step_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

TWO_LAYER = [c for c in M.CASES if c[1] == 2]


def _model(w, n_mel, layers):
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    return DeployModel(get_config(n_mel=n_mel, num_layers=layers, precision="bf16"), w)


def _names(n_mel, layers, four=False):
    kx = (n_mel + 31) // 32
    if layers == 1:
        return ["gru_stack_bf16<%d, 1>" % kx]
    if four:
        return ["gru_stack_bf16<%d, 2> (both layers, one launch, 4 waves)" % kx, ""]
    return ["gru_stack_bf16_ls<%d> (both layers, one launch, 8 waves)" % kx, ""]


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


def _chain(model, w, mel, st0, names, seqs=None, resets=None, check=True):
    """T one-frame calls with the state (and prev_word) carried on the device, each through check_call.
    seqs / resets: [T, B] or None.  -> dict(logits [B,T,C], softmax, tokens [B,T], state [L,B,H], states [T+1,L,B,H], report,
    checks [T] (check_call's results))."""
    b, t_len = mel.shape[:2]
    state = torch.from_numpy(st0).cuda()
    pw = model.fresh_prev_word(b)
    out = dict(logits=[], softmax=[], tokens=[], states=[st0], report=M.Report(), checks=[])
    for t in range(t_len):
        seq = None if seqs is None else np.ascontiguousarray(seqs[t], np.int32)
        reset = None if resets is None else np.ascontiguousarray(resets[t], np.uint8)
        r = _call(model, mel[:, t:t + 1], state, pw, seq, reset)
        assert model.kernel_names() == names
        new, lg = _np(r["state"]), _np(r["logits"])[:, 0]
        if check:
            res = M.check_call(w, mel[:, t], out["states"][-1], new, lg, seq, reset)
            out["report"].add(res)
            out["checks"].append(res)
        out["logits"].append(lg)
        out["softmax"].append(_np(r["softmax"])[:, 0])
        out["tokens"].append(_np(r["tokens"])[:, 0])
        out["states"].append(new)
        state = r["state"]
    for k in ("logits", "softmax", "tokens"):
        out[k] = np.stack(out[k], axis=1)
    out["state"], out["states"], out["prev_word"] = out["states"][-1], np.stack(out["states"]), _np(pw)
    return out


def _long_equals_chain(model, mel, st0, chain, names, lens=None):
    pw = model.fresh_prev_word(mel.shape[0])
    r = _call(model, mel, torch.from_numpy(st0).cuda(), pw, lens)
    assert model.kernel_names() == names
    for k in ("logits", "softmax", "tokens", "state"):
        assert np.array_equal(_bits(_np(r[k])), _bits(chain[k])), k
    assert np.array_equal(_np(pw), chain["prev_word"])


def _lens(b, t_len, seed):
    """Random lengths in [0, T] that include 0, 1 and T where the batch has room for them."""
    lens = np.random.default_rng(seed).integers(0, t_len + 1, b).astype(np.int32)
    for k, v in enumerate((t_len, 1, 0)[:b]):
        lens[(5 * k) % b if b >= 11 else k] = v
    return lens


def _run_case(case, names, tag=""):
    """Everything of one case on one kernel: the plain chain, the masked chain, long == chain with and without lengths.
    -> (plain chain, masked chain)."""
    n_mel, layers, b, t_len = case
    w, mel, st0 = M.case_inputs(case)
    model = _model(w, n_mel, layers)
    plain = _chain(model, w, mel, st0, names)
    rep = plain["report"]
    print(rep.line(M.case_id(case) + tag, names[0]) + " (logits %.3f, largest allowance %.1e)" % (rep.logits, rep.max_allow))
    rep.check_condition()
    _long_equals_chain(model, mel, st0, plain, names)
    rng = np.random.default_rng(4000 + b)
    seqs = rng.integers(0, 2, (t_len, b)).astype(np.int32)
    seqs[0, 0] = 1
    resets = (rng.random((t_len, b)) < 0.3).astype(np.uint8)
    masked = _chain(model, w, mel, st0, names, seqs, resets)
    rep = masked["report"]
    print(rep.line(M.case_id(case) + tag + " masked", names[0]) + " (logits %.3f, largest allowance %.1e)" % (rep.logits, rep.max_allow))
    rep.check_condition()
    lens = _lens(b, t_len, 4200 + b)
    by_len = _chain(model, w, mel, st0, names, seqs=(np.arange(t_len)[:, None] < lens[None, :]).astype(np.int32))
    _long_equals_chain(model, mel, st0, by_len, names, lens)
    model.close()
    return plain, masked


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_one_frame_chain_against_the_restatement_and_long_call_equals_chain(case):
    _run_case(case, _names(case[0], case[1]))


def test_persistent_rounds_long_call_equals_chain_and_every_stream_checked():
    """B = 16 x CUs + 17: every workgroup of gru_stack_bf16_ls walks a second stream group, one a third (ragged) one.  T = 2:
    the long call runs the skewed iteration, the one-frame calls are checked on ALL streams."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = (36, 2, 16 * cus + 17, 2)
    w, mel, st0 = M.case_inputs(case)
    names = _names(36, 2)
    model = _model(w, 36, 2)
    chain = _chain(model, w, mel, st0, names)
    rep = chain["report"]
    print(rep.line(M.case_id(case), names[0]) + " (logits %.3f, largest allowance %.1e)" % (rep.logits, rep.max_allow))
    rep.check_condition()
    _long_equals_chain(model, mel, st0, chain, names)
    model.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import test_gpu_bf16_step as TS
out = {}
for case in TS.TWO_LAYER:
    names = TS._names(case[0], case[1], four=True)
    plain, masked = TS._run_case(case, names, " child")
    out[TS.M.case_id(case) + "/states"] = plain["states"]
    out[TS.M.case_id(case) + "/logits"] = plain["logits"]
np.savez(sys.argv[1], **out)
"""


def test_four_wave_kernel_in_a_child_process(tmp_path):
    """KWS_BF16_WAVES=4: gru_stack_bf16<KX0, 2>.  The child runs the two-layer cases through the same chain, bitwise and
    check_call checks and hands over every one-frame call's state and logits.  Here each of those calls is checked again and
    repeated on the 8-wave kernel FROM THE CHILD'S INPUT STATE.  Both kernels round the same arithmetic, so on the same input
    they differ by no more than the sum of their two check_call bounds -- plus, above layer 0, the distance of their two fp64
    references, each of which was evaluated on its own kernel's lower-layer output."""
    env = dict(os.environ, KWS_BF16_WAVES="4")
    path = tmp_path / "four_waves.npz"
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT), str(path)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.count("4 waves") == 2 * len(TWO_LAYER)
    child = np.load(str(path))
    for case in TWO_LAYER:
        n_mel, layers, b, t_len = case
        w, mel, _ = M.case_inputs(case)
        names = _names(n_mel, layers)
        model = _model(w, n_mel, layers)
        states, logits = child[M.case_id(case) + "/states"], child[M.case_id(case) + "/logits"]
        assert states.shape == (t_len + 1, layers, b, 128) and logits.shape == (b, t_len, 6)
        for t in range(t_len):
            four = M.check_call(w, mel[:, t], states[t], states[t + 1], logits[:, t])
            got = _call(model, mel[:, t:t + 1], torch.from_numpy(states[t]).cuda(), model.fresh_prev_word(b))
            assert model.kernel_names() == names
            s8, l8 = _np(got["state"]), _np(got["logits"])[:, 0]
            eight = M.check_call(w, mel[:, t], states[t], s8, l8)
            apart = np.abs(four["ref"] - eight["ref"])
            assert apart[0].max() == 0.0                       # layer 0: the same inputs, one reference
            assert (np.abs(s8.astype(np.float64) - states[t + 1]) <= four["bound"] + eight["bound"] + apart).all(), (case, t)
            lapart = np.abs(four["ref_logits"] - eight["ref_logits"])
            assert (np.abs(l8.astype(np.float64) - logits[:, t]) <= four["bound_logits"] + eight["bound_logits"] + lapart).all(), (case, t)
        model.close()
