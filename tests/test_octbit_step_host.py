"""tests/octbit_step_model.py on the CPU: the restatement is gru_forward_octbit's arithmetic, its bound holds the float32 oracle's own
one-frame outputs on every case and family, its allowance stays rare and small, the families do what they promise, and the check
rejects every mutant of the restatement -- with what the older tolerances make of each mutant measured and asserted beside it."""
import numpy as np
import pytest

import octbit_step_model as M
from oracle import gru_oracle as G
from oracle import octbit_oracle as Q

F32 = np.float32


def _case(family, **kw):
    hit = [c for c in M.CASES if c.family == family and all(getattr(c, k) == v for k, v in kw.items())]
    assert hit, (family, kw)
    return hit[0]


def _two(family):
    """The family's first two-layer case with a full stream group."""
    return [c for c in M.CASES if c.family == family and c.layers == 2 and c.batch >= 16 and not c.relu][0]


def _masks(c, rng):
    seq = rng.integers(0, 2, c.batch).astype(np.int32)
    reset = ((rng.random(c.batch) < 0.3) | M.zero_streams(c)).astype(np.uint8)
    return seq, reset


def _chain(c, w, mel, st0, masked=False, mut=None, check=True):
    """T emulated one-frame calls carried on their own outputs -> (report, state [L,B,H], top rows [B,T,H], first call's state)."""
    rng = np.random.default_rng(7)
    rep, state, tops, first = M.Report(), st0, [], None
    for t in range(c.frames):
        seq, reset = _masks(c, rng) if masked else (None, None)
        new, logits, sm = M.emulate_call(w, mel[:, t], state, seq, reset, bool(c.relu), c.clip, mut)
        if check:
            rep.add(M.check_call(w, mel[:, t], state, new, logits, sm, seq, reset, bool(c.relu), c.clip))
        tops.append(new[-1])
        first = new if first is None else first
        state = new
    return rep, state, np.stack(tops, axis=1), first


def test_matmul_is_octbit_rows():
    rng = np.random.default_rng(11)
    wq, sw, b127 = Q.octize_weight_int8_signed(rng.uniform(-0.2, 0.2, (256, 24)).astype(F32))
    x = rng.standard_normal((12, 256)).astype(F32)
    x[3] = np.abs(x[3])                     # the unsigned branch
    x[4] = 0                                # the all-zero call
    for groups in (None, np.repeat(np.arange(4), 3)):
        want = Q.octbit_rows(x, wq, sw, b127, groups=groups)
        got = M.matmul(x, wq, sw, b127, groups=groups)
        assert np.array_equal(got["out"].view(np.int32), want.view(np.int32))
    got = M.matmul(x, wq, sw, b127)
    assert not got["signed"][3] and not got["signed"][4] and got["bscale"][4] == 0 and not got["out"][4].any() and got["signed"][0]


@pytest.mark.parametrize("case", [_case("glorot", batch=37), _case("clip", batch=17), _case("glorot", layers=3)], ids=M.case_id)
def test_float32_chain_is_the_oracle(case):
    """cell_step chained in float32 on its own values, and logits_of on the rows of the call: gru_forward_octbit bit for bit."""
    w, mel, st0 = M.case_inputs(case)
    lens = np.random.default_rng(3).integers(0, case.frames + 1, case.batch)
    for seq_len in (None, lens):
        want_l, want_s = G.gru_forward_octbit(w, mel, st0, seq_len=seq_len)
        state, tops = st0, []
        for t in range(case.frames):
            seq = None if seq_len is None else (t < seq_len).astype(np.int32)
            state = M.emulate_call(w, mel[:, t], state, seq)[0]
            tops.append(state[-1])
        assert np.array_equal(state.view(np.int32), want_s.view(np.int32))
        M.check_projection(w, np.stack(tops, axis=1), seq_len, want_l)


@pytest.mark.parametrize("case", M.CASES + [M.PERSISTENT], ids=M.case_id)
def test_oracle_chain_stays_inside_the_bound_and_the_conditions_hold(case):
    """check_call accepts the float32 oracle's own one-frame outputs; the allowance caps and what the family promises (clip shares,
    pre-activations inside [-30, 30], the unsigned branch everywhere, all-zero calls, exact ties) hold on the reference alone."""
    c = case
    w, mel, st0 = M.case_inputs(c)
    for masked in (False, True):
        rep, _, _, first = _chain(c, w, mel, st0, masked)
        print(rep.line(M.case_id(c) + (" masked" if masked else ""), "float32 oracle"))
        rep.check_condition(c.family, not masked)
        assert rep.rows > 0 or c.layers == 1
        if c.family == "ties":
            assert rep.ties >= 12 * c.batch // 2, rep.ties
        if c.family == "allzero":
            z = M.zero_streams(c)
            assert z.any() and not first[0][z].any()                     # x == 0: with h == 0 the quantised calls are all-zero
            if c.layers > 1 and not masked:
                lay = w["layers"][1]
                want = (1.0 - 1.0 / (1.0 + np.exp(-lay["bg"][M.HID:].astype(np.float64)))) * np.tanh(lay["bc"].astype(np.float64))
                assert np.abs(first[1][z] - want).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# power
def _today_single_step(err):
    """test_gpu_octbit_gru.py::test_single_step_is_exact_given_the_same_fp32_inputs at wscale 1."""
    return bool(np.mean(err < 2e-6) > 0.99 and err.max() < 5e-3)


def _today_multi_frame(el, es):
    """test_gpu_octbit_gru.py::test_int8_matches_oracle and the int8 rows of test_gpu_config_space.py."""
    return bool(el.mean() < 2e-3 and el.max() < 0.1 and es.mean() < 2e-4 and es.max() < 2e-2)


# mutant -> (the family whose case shows it, does it pass BOTH of today's criteria), the criteria evaluated on today's kind of inputs
# (glorot weights, a random signed state) with the mutant at work in every stream and frame.  Measured, and asserted as measured:
#   * half-even rounding and the correction in the unsigned branch change NOTHING on such inputs (no exact tie, no unsigned call):
#     today's tests cannot see them, only the ties and the nonnegative family do;
#   * every other mutant, at work in EVERY frame, misses one of today's criteria: a fault of one unit (the clamp mutants, the
#     swapped couple, the zeroed K-eighth) stays inside the free 1 % of the single-step criterion but moves that unit by more than
#     its 5e-3, and the chain's mean |dlogit| exceeds 2e-3; a fault of the quantiser proper (the offset, the range) touches every
#     unit of a stream.  What those tolerances cannot do is tell a rare fault from the quantiser flips they were sized for, or say
#     which layer, stream and unit is wrong.  check_call rejects every mutant on its first call and names them.
CELL_MUTANTS = {
    "no_clamp": ("clip", False), "clamp_high_only": ("clip", False), "half_even": ("ties", True), "offset_128": ("glorot", False),
    "range_h_only": ("glorot", False), "swap_couple": ("glorot", False), "unsigned_corrected": ("nonneg", True),
    "zero_k_eighth": ("glorot", False),
}


@pytest.mark.parametrize("mut", sorted(CELL_MUTANTS))
def test_check_call_rejects_every_cell_mutant_on_its_first_call(mut):
    family, passes_today = CELL_MUTANTS[mut]
    c = _two(family)
    w, mel, st0 = M.case_inputs(c)
    # rejected: on the first call already
    new, logits, sm = M.emulate_call(w, mel[:, 0], st0, mut=mut)
    with pytest.raises(AssertionError, match="layer 1"):
        M.check_call(w, mel[:, 0], st0, new, logits, sm)
    # today's tolerances, on today's kind of inputs (glorot weights, a random state): the multi-frame ones on the chain against the
    # oracle, the single-step one on the first call
    c = _two("glorot")
    w, mel, st0 = M.case_inputs(c)
    want_l, want_s = G.gru_forward_octbit(w, mel, st0)
    _, state, tops, first = _chain(c, w, mel, st0, mut=mut, check=False)
    clean = M.emulate_call(w, mel[:, 0], st0)[0]
    el, es = np.abs(M.logits_of(tops, w) - want_l), np.abs(state - want_s)
    err1 = np.abs(first[1] - clean[1])
    print("mutant %s on %s: first call max |dh'| %.2e, %.2f %% of the values within 2e-6; chain max |dlogit| %.2e mean %.2e, max |dstate| %.2e mean %.2e"
          % (mut, M.case_id(c), err1.max(), 100 * np.mean(err1 < 2e-6), el.max(), el.mean(), es.max(), es.mean()))
    assert (_today_multi_frame(el, es) and _today_single_step(err1)) == passes_today
    if passes_today:
        assert not err1.any() and not el.any() and not es.any()


def _ragged_block(family):
    c = _two(family)
    w, mel, st0 = M.case_inputs(c)
    lens = np.random.default_rng(5).integers(1, c.frames, c.batch)
    tops = _chain(c, w, mel, st0, check=False)[2]
    live = np.arange(c.frames)[None, :] < lens[:, None]
    tops[~live] = 0.0
    return c, w, tops, lens, live


def test_check_projection_rejects_a_per_frame_range():
    """The projection's range taken per frame instead of per call.  At T = 1 -- where today's bit-for-bit projection check stands
    -- it changes nothing; at T > 1 today's 0.1 on a logit is what stands (the mutant exceeds it where a frame's range is far from the
    call's)."""
    c, w, tops, lens, live = _ragged_block("glorot")
    good = M.logits_of(tops, w)
    M.check_projection(w, tops, lens, good)
    bad = M.logits_of(tops, w, mut="fc_range_per_frame")
    with pytest.raises(AssertionError, match="projection"):
        M.check_projection(w, tops, lens, bad)
    one = tops[:, :1]
    assert np.array_equal(M.logits_of(one, w, mut="fc_range_per_frame"), M.logits_of(one, w))


@pytest.mark.parametrize("family", ["glorot", "nonneg"])
def test_leaving_the_zero_rows_out_of_the_projection_range_changes_nothing(family):
    """An EQUIVALENT mutant, recorded so that nobody looks for a test of it: the zero rows past seq_len can move the call's minimum
    up to 0 or its maximum down to 0, and neither changes the branch (min < 0) or the scale (max(-min, max) / 127, max / 254)."""
    c, w, tops, lens, live = _ragged_block(family)
    assert np.array_equal(M.logits_of(tops, w, mut="fc_range_live_rows", live_rows=live), M.logits_of(tops, w))


def test_check_call_refuses_a_moved_dead_row_a_wrong_logit_bit_and_a_wrong_unit():
    c = _two("glorot")
    w, mel, st0 = M.case_inputs(c)
    seq = np.ones(c.batch, np.int32)
    seq[9] = 0
    new, logits, sm = M.emulate_call(w, mel[:, 0], st0, seq)
    M.check_call(w, mel[:, 0], st0, new, logits, sm, seq)
    moved = new.copy()
    moved[1, 9, 0] = np.nextafter(moved[1, 9, 0], F32(2))
    with pytest.raises(AssertionError, match="seq_len 0"):
        M.check_call(w, mel[:, 0], st0, moved, logits, sm, seq)
    lbad = logits.copy()
    lbad[2, 1] = np.nextafter(lbad[2, 1], F32(100))
    with pytest.raises(AssertionError, match="logits"):
        M.check_call(w, mel[:, 0], st0, new, lbad, sm, seq)
    bad = new.copy()
    bad[1, 3, 77] += F32(2e-5)
    with pytest.raises(AssertionError, match="layer 1"):
        M.check_call(w, mel[:, 0], st0, bad, M.emulate_call(w, mel[:, 0], st0, seq)[1], sm, seq)
