"""Single-step restatement of the bf16 GRU stack (csrc/gru_bf16.hip) for frame-by-frame checks at fp32 accuracy.

The multi-frame bf16 tolerances (6e-2 on the logits) are wide because a value that rounds to the other side of a bf16 tie
than it does in oracle.gru_oracle.gru_forward_bf16 costs 2^-8 on that value and the recurrence carries the difference on.
A ONE-FRAME call takes both out of the comparison: it returns the fp32 h' of every layer, layer l+1's input is bf16(h'_l)
and the projection's input is bf16(h'_top) -- exact functions of numbers the call returns.  Fed the device's own carried state
and the device's own lower-layer output, the only rounding this restatement cannot see is bf16(r*h), 128 values per stream and
layer, and it knows which of them lie close enough to a tie to flip (`near`) and what a flip can cost each unit (`allow`).

cell_step rounds exactly where gru_forward_bf16 rounds (weights, x, h for the gates, r*h, all to bf16, nearest even; products
exact, everything else in `dtype`); chained in fp64 on its own values it IS gru_forward_bf16 (tests/test_bf16_step_host.py).

  window[b, j] = 4 * |h_j| * (3e-7 + dev_r)      3e-7: the activation error csrc/gru_device.h states for sigmoid_f / tanh_f;
                                                 dev_r: max |r32 - r64| of the two CPU runs of the call; 4: the usual margin
                                                 over a float32-CPU deviation (test_gpu_beam.py, test_gpu_enroll.py)
  near[b, j]   = v[b, j] = r*h lies within window[b, j] of a bf16 rounding boundary (the midpoint of two bf16 neighbours)
  allow[b, i]  = sum_j near[b, j] * ulp_bf16(v[b, j]) * |Wc_bf16[I + j, i]| * (1 - u[b, i])        (|tanh'| <= 1)
  bound[b, i]  = 4 * max |h'32 - h'64| over rows with no near tie, floored at 16 * 2^-23 * max(1, max |h'|)
                 + 4 * 3e-7 * (|h - c| + 1)[b, i] + allow[b, i]
The projection has no ties (bf16 products are exact in fp32): 4 x the float32-vs-fp64 deviation, floored at
16 * 2^-23 * max |reference|."""
import numpy as np

from oracle.gru_oracle import bf16_round

ACT_ERR = 3e-7          # csrc/gru_device.h: sigmoid_f / tanh_f, absolute
MARGIN = 4.0
FLOOR = 16.0 * 2.0 ** -23
MAX_ALLOW_SHARE = 0.25  # the cap on (stream, layer, frame) rows that carry an allowance ...
MAX_ALLOW = 2e-3        # ... and on any single allowance: they keep the allowance from hiding a failure


# (n_mel, layers, B, T): both KX0 values on both sides of 32, the widest and the narrowest mel row, a single, a full, a ragged
# and several stream groups
CASES = [(4, 1, 1, 6), (28, 1, 17, 6), (32, 2, 16, 8), (36, 1, 15, 6), (36, 2, 33, 8), (60, 2, 17, 8), (64, 2, 1, 8), (64, 1, 33, 6)]


def case_id(case):
    return "n%d_L%d_B%d_T%d" % tuple(case)


def case_inputs(case, batch=None):
    """(weights, mel [B,T,I], state [L,B,H]) of a case; the seeds depend on the case alone."""
    from oracle import gru_oracle as G
    n_mel, layers, b, t = case
    b = batch or b
    seed = 4100 + 10 * (CASES.index(tuple(case)) if tuple(case) in CASES else len(CASES))
    w = G.random_weights(n_mel, 128, layers, 6, seed=seed)
    mel = G.synthetic_mel(b, t, n_mel, seed=seed + 1)
    st0 = (0.5 * np.random.default_rng(seed + 2).standard_normal((layers, b, 128))).astype(np.float32)
    return w, mel, st0


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def bf16_ulp(v):
    """Spacing of the bf16 values around v (8 significand bits): 2^(e - 7) for 2^e <= |v| < 2^(e+1)."""
    _, ex = np.frexp(np.abs(np.asarray(v, np.float64)))            # |v| = m * 2^ex, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(ex, -125) - 8)


def tie_distance(v):
    """Distance of v from the nearest bf16 rounding boundary: (k + 1/2) * ulp inside its binade, and below the binade's first
    value 2^e the last boundary of the binade underneath, 2^e - ulp / 4; inf at 0."""
    a = np.abs(np.asarray(v, np.float64))
    ulp = bf16_ulp(a)
    q = a / ulp
    d = np.abs(q - np.floor(q) - 0.5) * ulp
    d = np.minimum(d, a - 128.0 * ulp + 0.25 * ulp)
    return np.where(a == 0.0, np.inf, d)


def near_allow(v, h, u, wc_h_abs, dev_r):
    """(near [B,H], allow [B,H]) of one layer: v = r*h unrounded, h the carried state, u the update gate, wc_h_abs =
    |Wc_bf16[I:, :]|."""
    window = MARGIN * np.abs(np.asarray(h, np.float64)) * (ACT_ERR + dev_r)
    near = tie_distance(v) <= window
    allow = ((near * bf16_ulp(v)) @ wc_h_abs) * (1.0 - np.asarray(u, np.float64))
    return near, allow


def cell_step(lay, x, h, dtype=np.float64, dev_r=0.0):
    """One bf16 GRU cell step.  x [B,I]: the float32 mel row, or the float32 lower-layer output as the device returned it;
    h [B,H]: the float32 state the call was given.  -> dict(h_new, r, u, c, v, near, allow)."""
    hdim = np.shape(h)[1]
    wg, wc = bf16_round(lay["Wg"]).astype(dtype), bf16_round(lay["Wc"]).astype(dtype)
    bg, bc = lay["bg"].astype(dtype), lay["bc"].astype(dtype)
    xb = bf16_round(np.asarray(x, np.float32)).astype(dtype)
    i_l = xb.shape[1]
    h = np.asarray(h, dtype)
    hb = bf16_round(h.astype(np.float32)).astype(dtype)
    g = _sigmoid(xb @ wg[:i_l] + hb @ wg[i_l:] + bg)
    r, u = g[:, :hdim], g[:, hdim:]
    v = r * h
    rh = bf16_round(v.astype(np.float32)).astype(dtype)
    c = np.tanh(xb @ wc[:i_l] + rh @ wc[i_l:] + bc)
    hn = u * h + (1.0 - u) * c
    near, allow = near_allow(v, h, u, np.abs(wc[i_l:].astype(np.float64)), dev_r)
    return dict(h_new=hn, r=r, u=u, c=c, v=v, near=near, allow=allow)


def logits_of(h_top, w, dtype=np.float64):
    """bf16(h_top) @ bf16(Wfc) + bfc."""
    hb = bf16_round(np.asarray(h_top, np.float32)).astype(dtype)
    return hb @ bf16_round(w["Wfc"]).astype(dtype) + w["bfc"].astype(dtype)


def check_call(w, mel_row, state_in, dev_state, dev_logits, seq_len=None, reset=None):
    """One one-frame call.  mel_row [B,I], state_in [L,B,H] (as given to the call), dev_state [L,B,H] and dev_logits [B,C] as the
    device returned them, seq_len [B] in {0, 1} or None, reset [B] or None.  Asserts
      live rows:  each layer's state_out within `bound` of the fp64 step evaluated on the DEVICE's lower-layer output,
                  the logits within the projection bound of logits_of(device top state);
      seq_len 0:  state equal to the (reset) input state and logits equal to bfc, bit for bit.
    -> dict for the report and for comparing two kernels on one input: ratio_plain / ratio_allow (worst err / bound on rows
    without / with allowance), rows, allow_rows, max_allow, ref [L,B,H], bound [L,B,H], ref_logits [B,C], bound_logits."""
    mel_row = np.asarray(mel_row, np.float32)
    state_in = np.array(state_in, np.float32)
    dev_state = np.asarray(dev_state, np.float32)
    dev_logits = np.asarray(dev_logits, np.float32)
    nb = mel_row.shape[0]
    if reset is not None:
        state_in[:, np.asarray(reset).astype(bool)] = 0.0
    live = np.ones(nb, bool) if seq_len is None else np.asarray(seq_len) > 0
    dead = ~live
    out = dict(ratio_plain=0.0, ratio_allow=0.0, rows=0, allow_rows=0, max_allow=0.0, ref=[], bound=[])
    x = mel_row
    for l, lay in enumerate(w["layers"]):
        h = state_in[l]
        s32 = cell_step(lay, x, h, np.float32)
        s64 = cell_step(lay, x, h, np.float64)
        dev_r = float(np.abs(s32["r"].astype(np.float64) - s64["r"]).max())
        i_l = x.shape[1]
        near, allow = near_allow(s64["v"], h, s64["u"], np.abs(bf16_round(lay["Wc"])[i_l:].astype(np.float64)), dev_r)
        tie_row = near.any(axis=1)
        dev_h = np.abs(s32["h_new"].astype(np.float64) - s64["h_new"])
        first = max(MARGIN * (dev_h[~tie_row].max() if (~tie_row).any() else 0.0),
                    FLOOR * max(1.0, float(np.abs(s64["h_new"]).max())))
        bound = first + MARGIN * ACT_ERR * (np.abs(h.astype(np.float64) - s64["c"]) + 1.0) + allow
        err = np.abs(dev_state[l].astype(np.float64) - s64["h_new"])
        ratio = (err / bound).max(axis=1)
        plain, withal = live & ~tie_row, live & tie_row
        if plain.any():
            out["ratio_plain"] = max(out["ratio_plain"], float(ratio[plain].max()))
        if withal.any():
            out["ratio_allow"] = max(out["ratio_allow"], float(ratio[withal].max()))
            out["max_allow"] = max(out["max_allow"], float(allow[withal].max()))
        out["rows"] += int(live.sum())
        out["allow_rows"] += int(withal.sum())
        out["ref"].append(s64["h_new"])
        out["bound"].append(bound)
        bad = live[:, None] & (err > bound)
        assert not bad.any(), "layer %d: %d of %d live values outside the bound, worst err/bound %.3f (err %.3e) at %s" % (
            l, int(bad.sum()), int(live.sum()) * h.shape[1], float((err / bound)[live].max()), float(err[bad].max()),
            np.argwhere(bad)[:4].tolist())
        assert np.array_equal(dev_state[l][dead].view(np.int32), h[dead].view(np.int32)), "layer %d: a row with seq_len 0 moved" % l
        x = dev_state[l]
    out["ref"], out["bound"] = np.stack(out["ref"]), np.stack(out["bound"])
    ref = logits_of(dev_state[-1], w, np.float64)
    dev32 = np.abs(logits_of(dev_state[-1], w, np.float32).astype(np.float64) - ref)
    lbound = max(MARGIN * float(dev32[live].max()), FLOOR * float(np.abs(ref[live]).max())) if live.any() else 0.0
    lerr = np.abs(dev_logits.astype(np.float64) - ref)
    out["ref_logits"], out["bound_logits"] = ref, lbound
    if live.any():
        out["ratio_logits"] = float(lerr[live].max() / lbound)
        assert lerr[live].max() <= lbound, "logits: err %.3e, bound %.3e" % (lerr[live].max(), lbound)
    bfc = np.broadcast_to(w["bfc"].astype(np.float32), dev_logits.shape)
    assert np.array_equal(dev_logits[dead].view(np.int32), np.ascontiguousarray(bfc[dead]).view(np.int32)), "a row with seq_len 0 emits other than bfc"
    return out


class Report(object):
    """The worst ratios and the allowance share over the calls of one case."""

    def __init__(self):
        self.plain = self.allow = self.max_allow = self.logits = 0.0
        self.rows = self.allow_rows = 0

    def add(self, r):
        self.plain, self.allow = max(self.plain, r["ratio_plain"]), max(self.allow, r["ratio_allow"])
        self.max_allow, self.logits = max(self.max_allow, r["max_allow"]), max(self.logits, r.get("ratio_logits", 0.0))
        self.rows += r["rows"]
        self.allow_rows += r["allow_rows"]

    @property
    def share(self):
        return self.allow_rows / max(self.rows, 1)

    def line(self, case, kernel):
        return "BF16-STEP %s %s: worst err/bound plain %.3f, with allowance %.3f, allowance rows %.1f %%" % (
            case, kernel, self.plain, self.allow, 100.0 * self.share)

    def check_condition(self):
        assert self.share <= MAX_ALLOW_SHARE, "allowance on %.1f %% of the rows" % (100.0 * self.share)
        assert self.max_allow <= MAX_ALLOW, "an allowance of %.2e" % self.max_allow
