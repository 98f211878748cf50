"""The int8 ("octbit") GRU stack frame by frame: ONE-FRAME calls against tests/octbit_step_model.py, which is fed the device's own
carried state and lower-layer output, so that neither the recurrence nor a quantiser flip widens the comparison (the multi-frame
tests -- test_gpu_octbit_gru.py, the int8 rows of test_gpu_config_space.py -- allow 0.1 on a logit and 2e-2 on the state).

  bounded   the cell of a quantised layer: within the activation error on the rows whose quantised inputs are DECIDED, plus the
            modelled cost of the possible flips on the others (few, and capped); layer 0 (fp32 kernels) and the softmax under
            gru_step_model's bounds
  bitwise   the class projection -- at T = 1 in every call of every chain, at T > 1 (the per-call range over all frames and zero
            rows, the 32-frame blocks of octbit_fc_kernel with their halo, octbit_top_range_kernel for one-layer models) against
            logits_of the rows a one-frame chain returned; the state of one long call against the chain's; rows with seq_len 0

Every call asserts kernel_names().  Each case prints
`OCTBIT-STEP <case> <family>: worst err/bound decided .., allowed .., allowance rows .. %, clipped .. %`."""
import numpy as np
import pytest
import torch

import config_space_grid as CS
import octbit_step_model as M
from oracle import decode_oracle as D

pytestmark = pytest.mark.gpu

THRES = 0.4


def _model(c, w):
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg = get_config(n_mel=c.n_mel, num_layers=c.layers, precision="int8", use_relu=bool(c.relu), value_clip=c.clip)
    cfg.label_dict = {str(k): k for k in range(1, c.classes - 2)}
    assert cfg.num_classes == c.classes
    return DeployModel(cfg, w)


def _names(c, frames):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    row = CS.R(M.case_id(c), "int8", "auto", c.n_mel, M.HID, c.layers, c.classes, c.batch, frames, "int8")
    return CS.expected_names(row, c.batch, frames, cus)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _call(model, mel, state, pw, seq=None, reset=None):
    r = model.forward(_dev(mel), state, prev_word=pw, seq_len=None if seq is None else _dev(seq),
                      reset_mask=None if reset is None else _dev(reset))
    torch.cuda.synchronize()
    return r


def _chain(model, c, w, mel, st0, seqs=None, resets=None, check=True):
    """T one-frame calls with the state and prev_word carried on the device, each through check_call.  seqs / resets: [T, B] or
    None.  -> dict(top [B,T,H]: the top layer's state after every call, state [L,B,H], report)."""
    names = _names(c, 1)
    state = _dev(st0)
    pw = model.fresh_prev_word(mel.shape[0])
    rep, tops, before = M.Report(), [], st0
    for t in range(mel.shape[1]):
        seq = None if seqs is None else np.ascontiguousarray(seqs[t], np.int32)
        reset = None if resets is None else np.ascontiguousarray(resets[t], np.uint8)
        r = _call(model, mel[:, t:t + 1], state, pw, seq, reset)
        assert model.kernel_names() == names, (model.kernel_names(), names)
        new = _np(r["state"])
        if check:
            rep.add(M.check_call(w, mel[:, t], before, new, _np(r["logits"])[:, 0], _np(r["softmax"])[:, 0], seq, reset,
                                 bool(c.relu), c.clip))
        tops.append(new[-1])
        before, state = new, r["state"]
    return dict(top=np.stack(tops, axis=1), state=before, report=rep)


def _decode_ok(sm_row, classes, eps=1e-5):
    """ctc_decode2's frame word (first maximum of classes 1..C-2, strictly above the threshold) is decided with room to spare."""
    p = np.sort(np.asarray(sm_row)[1:classes - 1])
    return abs(p[-1] - THRES) > eps and (p[-1] < THRES or len(p) < 2 or p[-1] - p[-2] > eps)


def _long_call(model, c, w, mel, st0, chain, lens=None):
    """One call of all T frames: the state equals the chain's bit for bit; the logits equal logits_of the rows the chain returned
    (zero rows past seq_len) bit for bit; the softmax holds its bound; tokens and prev_word are ctc_decode2 of the call's own
    softmax on the streams no frame of which sits on the threshold.  (prev_word is NOT compared with the chain's: it follows the
    last frame's logits, and those are quantised with the call's range here and with the frame's own range in the chain.)"""
    from keyword_spotting_amd.prediction import tokens_to_seq
    pw = model.fresh_prev_word(mel.shape[0])
    r = _call(model, mel, _dev(st0), pw, lens)
    assert model.kernel_names() == _names(c, mel.shape[1]), model.kernel_names()
    assert np.array_equal(_bits(_np(r["state"])), _bits(chain["state"])), "state of the long call != state of the chain"
    logits, sm, toks, pw = _np(r["logits"]), _np(r["softmax"]), _np(r["tokens"]), _np(pw)
    detail = M.check_projection(w, chain["top"], lens, logits, bool(c.relu), c.clip)
    ratio = M.softmax_ratio(logits, sm)
    assert ratio <= 1.0, "softmax: worst err/bound %.3f" % ratio
    checked = 0
    for k in range(mel.shape[0]):
        if all(_decode_ok(f, c.classes) for f in sm[k]):
            assert np.array_equal(tokens_to_seq(toks[k]), D.ctc_decode2(sm[k].astype(np.float64), c.classes)), "tokens of stream %d" % k
            assert int(pw[k]) == int(D.frame_words(sm[k, -1:].astype(np.float64), 1, c.classes - 1, THRES)[0]), "prev_word of stream %d" % k
            checked += 1
    assert checked > 0
    return detail, logits


def _finish(c, rep, tag="", plain=True):
    print(rep.line(M.case_id(c) + tag, c.family))
    rep.check_condition(c.family, plain)
    assert rep.decided <= 1.0 and rep.allowed <= 1.0 and rep.layer0 <= 1.0 and rep.softmax <= 1.0


def _lens(b, t_len, seed):
    """Random lengths in [0, T] that include 0, 1, T - 1 and T where the batch has room for them."""
    lens = np.random.default_rng(seed).integers(0, t_len + 1, b).astype(np.int32)
    for k, v in enumerate((t_len, 1, 0, t_len - 1)[:b]):
        lens[(5 * k) % b if b >= 16 else k] = v
    return lens


def _one_case(c):
    w, mel, st0 = M.case_inputs(c)
    model = _model(c, w)
    plain = _chain(model, c, w, mel, st0)
    _finish(c, plain["report"])
    if c.family == "ties":
        assert plain["report"].ties > 0
    _long_call(model, c, w, mel, st0, plain)
    rng = np.random.default_rng(M.seed_of(c) + 5)
    seqs = rng.integers(0, 2, (c.frames, c.batch)).astype(np.int32)
    seqs[0, 0] = 1
    resets = ((rng.random((c.frames, c.batch)) < 0.3) | M.zero_streams(c)[None, :]).astype(np.uint8)
    masked = _chain(model, c, w, mel, st0, seqs, resets)
    _finish(c, masked["report"], " masked", plain=False)
    lens = _lens(c.batch, c.frames, M.seed_of(c) + 6)
    by_len = _chain(model, c, w, mel, st0, seqs=(np.arange(c.frames)[:, None] < lens[None, :]).astype(np.int32))
    _finish(c, by_len["report"], " lengths", plain=False)
    _long_call(model, c, w, mel, st0, by_len, lens)
    model.close()


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_one_frame_chain_against_the_restatement_and_long_call_equals_chain(case):
    _one_case(case)


def test_every_stream_of_several_groups_is_checked():
    """B = 16 x 3 + 5 at T = 2: four workgroups, the last one ragged, every stream through check_call."""
    _one_case(M.PERSISTENT)


# (family, T, layers, classes, relu, clip): both sides of a 32-frame block of octbit_fc_kernel and a third block, with their halos;
# one layer (the range from octbit_top_range_kernel) and two (from the layer kernel); glorot: signed ranges, nonneg: every row of
# every stream positive -- the unsigned projection at len == T, and at len < T zero rows that decide nothing
PROJECTION = [("glorot", 31, 2, 3, 0, -1.0), ("glorot", 32, 1, 8, 1, -1.0), ("glorot", 33, 2, 8, 1, 20.0), ("glorot", 65, 1, 3, 0, -1.0),
              ("glorot", 65, 2, 8, 0, -1.0), ("nonneg", 33, 2, 3, 0, -1.0), ("nonneg", 32, 1, 8, 1, 20.0), ("nonneg", 65, 2, 8, 0, -1.0)]


@pytest.mark.parametrize("family,frames,layers,classes,relu,clip", PROJECTION,
                         ids=["%s_T%d_L%d_C%d%s%s" % (p[0], p[1], p[2], p[3], "_relu" if p[4] else "", "_clip" if p[5] > 0 else "") for p in PROJECTION])
def test_projection_of_a_long_call_bit_for_bit(family, frames, layers, classes, relu, clip):
    c = M.Case(family, 40, layers, classes, 19, frames, relu, clip)
    w, mel, st0 = M.case_inputs(c)
    model = _model(c, w)
    lens = _lens(c.batch, frames, M.seed_of(c) + 6)
    assert {0, 1, frames - 1, frames} <= set(lens.tolist())
    chain = _chain(model, c, w, mel, st0, seqs=(np.arange(frames)[:, None] < lens[None, :]).astype(np.int32), check=False)
    detail, logits = _long_call(model, c, w, mel, st0, chain, lens)
    signed = detail["signed"].reshape(c.batch, frames)[:, 0]
    live = lens > 0
    if family == "nonneg":
        assert not signed.any() and (chain["top"][lens == frames] > 0).all()
    else:
        assert signed[live].all()
    if relu:
        assert logits.min() == 0.0 and (clip < 0 or logits.max() == 20.0)
    model.close()
