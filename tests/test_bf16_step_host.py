"""tests/bf16_step_model.py on the CPU: the single-step restatement is gru_forward_bf16's arithmetic, its bounds hold a float32
stand-in for the device, its allowance stays rare and small, and its tie classification does what it says."""
import numpy as np
import pytest

import bf16_step_model as M
from oracle import gru_oracle as G


def _standin_step(lay, x, h):
    """A float32 'device': the same roundings as cell_step, written in the concatenated-matmul form (another summation order)."""
    f = np.float32
    wg, wc = G.bf16_round(lay["Wg"]), G.bf16_round(lay["Wc"])
    xb, hb = G.bf16_round(x), G.bf16_round(h)
    g = (f(1) / (f(1) + np.exp(-(np.concatenate([xb, hb], 1) @ wg + lay["bg"])))).astype(f)
    r, u = g[:, :128], g[:, 128:]
    rh = G.bf16_round((r * h).astype(f))
    c = np.tanh(np.concatenate([xb, rh], 1) @ wc + lay["bc"]).astype(f)
    return (u * h + (f(1) - u) * c).astype(f)


def _standin_call(w, mel_row, state, seq_len=None, reset=None):
    state = state.copy()
    if reset is not None:
        state[:, reset.astype(bool)] = 0.0
    live = np.ones(mel_row.shape[0], bool) if seq_len is None else seq_len > 0
    out, x = [], mel_row
    for l, lay in enumerate(w["layers"]):
        hn = _standin_step(lay, x, state[l])
        out.append(np.where(live[:, None], hn, state[l]))
        x = hn
    top = np.where(live[:, None], out[-1], np.float32(0))
    logits = (G.bf16_round(top) @ G.bf16_round(w["Wfc"]) + w["bfc"]).astype(np.float32)
    return np.stack(out), logits


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_float32_chain_stays_inside_the_bounds_and_the_allowance_stays_rare(case):
    w, mel, st0 = M.case_inputs(case)
    b, t_len = mel.shape[:2]
    for masked in (False, True):
        rng = np.random.default_rng(7)
        rep, state = M.Report(), st0
        for t in range(t_len):
            seq = rng.integers(0, 2, b).astype(np.int32) if masked else None
            reset = (rng.random(b) < 0.3).astype(np.uint8) if masked else None
            new, logits = _standin_call(w, mel[:, t], state, seq, reset)
            rep.add(M.check_call(w, mel[:, t], state, new, logits, seq, reset))
            state = new
        print(rep.line(M.case_id(case) + (" masked" if masked else ""), "float32 stand-in") + ", largest allowance %.1e" % rep.max_allow)
        rep.check_condition()
        assert rep.rows > 0


@pytest.mark.parametrize("case", [(40, 2, 48, 24), (64, 1, 48, 24), (4, 2, 48, 24)], ids=M.case_id)
def test_fp64_chain_is_the_rounding_oracle(case):
    """cell_step chained in fp64 on its own values: gru_forward_bf16 exactly, the same arithmetic."""
    n_mel, layers, b, t_len = case
    w = G.random_weights(n_mel, 128, layers, 6, seed=31)
    mel = G.synthetic_mel(b, t_len, n_mel, seed=32)
    st0 = (0.5 * np.random.default_rng(33).standard_normal((layers, b, 128))).astype(np.float32)
    want_l, want_s = G.gru_forward_bf16(w, mel, st0)
    h = [st0[l].astype(np.float64) for l in range(layers)]
    logits = np.zeros((b, t_len, 6))
    for t in range(t_len):
        x = mel[:, t]
        for l in range(layers):
            h[l] = M.cell_step(w["layers"][l], x, h[l], np.float64)["h_new"]
            x = h[l]
        logits[:, t] = M.logits_of(h[-1], w)
    assert np.array_equal(np.stack(h), want_s)
    assert np.array_equal(logits, want_l)


def test_bf16_ulp_and_tie_distance():
    assert M.bf16_ulp(1.0) == 2.0 ** -7 and M.bf16_ulp(1.99) == 2.0 ** -7 and M.bf16_ulp(2.0) == 2.0 ** -6
    assert M.bf16_ulp(-0.75) == 2.0 ** -8
    assert M.tie_distance(1.0 + 2.0 ** -8) == 0.0 and M.tie_distance(-(1.0 + 2.0 ** -8)) == 0.0
    assert M.tie_distance(1.0 + 2.0 ** -7) == 2.0 ** -8 and M.tie_distance(0.0) == np.inf
    # around a power of two the nearest boundary is the last one of the LOWER binade, half of its ulp below
    assert M.tie_distance(1.0) == 2.0 ** -9 and M.tie_distance(1.0 + 2.0 ** -10) == 2.0 ** -9 + 2.0 ** -10
    assert M.tie_distance(2.0 - 2.0 ** -8) == 0.0
    for v in np.random.default_rng(1).standard_normal(2000):
        d = M.tie_distance(v)
        if d < 1e-5:                                        # the probes below are float32 values: keep clear of their spacing
            continue
        lo, hi = G.bf16_round(np.float32(v - 0.99 * d)), G.bf16_round(np.float32(v + 0.99 * d))
        assert lo == hi, v                                  # no boundary strictly inside (v - d, v + d) ...
        assert G.bf16_round(np.float32(v - 1.01 * d)) != G.bf16_round(np.float32(v + 1.01 * d)), v   # ... one at d


def test_hand_made_ties_are_classified_and_a_flip_stays_inside_the_allowance():
    """Unit 5's v = r*h exactly on a bf16 tie, unit 6's just inside the window, unit 7's just outside; unit 5's r*h then
    rounded to the other neighbour moves h' by no more than the allowance."""
    w = G.random_weights(8, 128, 1, 6, seed=41)
    lay = w["layers"][0]
    x = G.synthetic_mel(1, 1, 8, seed=42)[0]
    h = (0.5 * np.random.default_rng(43).standard_normal((1, 128))).astype(np.float32)
    s = M.cell_step(lay, x, h, np.float64)
    dev_r = 1e-7
    window = M.MARGIN * np.abs(h.astype(np.float64)) * (M.ACT_ERR + dev_r)
    v = s["v"].copy()
    tie = (np.floor(np.abs(v) / M.bf16_ulp(v)) + 0.5) * M.bf16_ulp(v) * np.sign(v)         # the boundary of each v's own cell
    v[0, 5] = tie[0, 5]
    v[0, 6] = tie[0, 6] + 0.9 * window[0, 6]
    v[0, 7] = tie[0, 7] - 1.1 * window[0, 7]
    wc_abs = np.abs(G.bf16_round(lay["Wc"])[8:].astype(np.float64))
    near, allow = M.near_allow(v, h, s["u"], wc_abs, dev_r)
    assert near[0, 5] and near[0, 6] and not near[0, 7]
    near5 = np.zeros_like(near)
    near5[0, 5] = True
    allow5 = ((near5 * M.bf16_ulp(v)) @ wc_abs) * (1.0 - s["u"])
    assert (allow >= allow5).all() and allow5.max() > 0 and allow5.max() <= M.MAX_ALLOW
    # the flip: unit 5's rounded r*h one bf16 step down and one up around the tie
    wc = G.bf16_round(lay["Wc"]).astype(np.float64)
    xb = G.bf16_round(x).astype(np.float64)
    rh = G.bf16_round(v.astype(np.float32)).astype(np.float64)
    outs = []
    for side in (-0.5, 0.5):
        rh2 = rh.copy()
        rh2[0, 5] = tie[0, 5] + side * M.bf16_ulp(v)[0, 5] * np.sign(v[0, 5])
        assert G.bf16_round(np.float32(rh2[0, 5])) == np.float32(rh2[0, 5])               # both are bf16 values
        c = np.tanh(xb @ wc[:8] + rh2 @ wc[8:] + lay["bc"].astype(np.float64))
        outs.append(s["u"] * h + (1.0 - s["u"]) * c)
    moved = np.abs(outs[0] - outs[1])
    assert moved.max() > 0 and (moved <= allow5 * (1 + 1e-12)).all()


def test_check_call_refuses_what_the_loose_tolerances_let_through():
    """A wrong bias on one unit (1e-3), a truncating r*h, a moved dead row: each far below 6e-2, each refused."""
    case = (36, 2, 33, 8)
    w, mel, st0 = M.case_inputs(case)
    new, logits = _standin_call(w, mel[:, 0], st0)
    M.check_call(w, mel[:, 0], st0, new, logits)
    bad = new.copy()
    bad[1, 3, 77] += 1e-3
    with pytest.raises(AssertionError, match="layer 1"):
        M.check_call(w, mel[:, 0], st0, bad, logits)
    lbad = logits.copy()
    lbad[2, 4] += 1e-4
    with pytest.raises(AssertionError, match="logits"):
        M.check_call(w, mel[:, 0], st0, new, lbad)
    seq = np.ones(33, np.int32)
    seq[9] = 0
    new, logits = _standin_call(w, mel[:, 0], st0, seq)
    M.check_call(w, mel[:, 0], st0, new, logits, seq)
    moved = new.copy()
    moved[0, 9, 0] = np.nextafter(moved[0, 9, 0], np.float32(2))
    with pytest.raises(AssertionError, match="seq_len 0"):
        M.check_call(w, mel[:, 0], st0, moved, logits, seq)
