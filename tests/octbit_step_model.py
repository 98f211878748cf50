"""Single-step restatement of the int8 ("octbit") GRU stack (csrc/gru_octbit.hip: gru_layer_octbit_kernel, octbit_top_range_kernel,
octbit_fc_kernel; pack_int8 in weight_pack.hip) for frame-by-frame checks -- a helper, numpy only, not a test.

The multi-frame int8 tolerances (0.1 on a logit, 2e-2 on the state) are wide because an activation that lands on the other side of
a rounding boundary of the u8 quantiser than it does in oracle.gru_oracle.gru_forward_octbit moves a pre-activation by
|W_q| * scale and the recurrence carries the difference on.  A ONE-FRAME call takes both out of the comparison: it returns the
fp32 h' of every layer, the input of layer l+1 is h'_l and the projection's input is h'_top -- numbers the call returns.  Fed the
device's own carried state and lower-layer output,
  * the GATE matmul of a quantised layer sees exactly the floats the device saw, and everything up to the sigmoid's argument is
    integer arithmetic plus separately rounded float32 operations (mul_rn / sub_rn / add_rn in the kernel, the same order as
    oracle.octbit_oracle.octbit_rows): that pre-activation is the device's bit for bit;
  * the CANDIDATE matmul quantises [x, v], v = r (.) h, and r comes from the device's sigmoid_f, which no CPU reproduces bit for
    bit.  The restatement knows which of the 256 quotients lie close enough to a rounding boundary n + 1/2 to flip (`near`) and
    what a flip can cost each unit (`allow`); a row without such a quotient is DECIDED: its integer accumulators are determined;
  * the PROJECTION quantises h'_top itself: no ties of its own, compared bit for bit (logits_of).

matmul      octbit_rows with the hooks the mutants of tests/test_octbit_step_host.py need and with what the report needs (the
            float quotients, the ranges, the pair sums that clipped).  Unmutated it IS octbit_rows, bit for bit.
cell_step   one quantised layer.  dtype=float32: gru_forward_octbit's own arithmetic (chained on its own values it equals it bit
            for bit); dtype=float64: the reference of the check -- the float32 gate pre-activation, the fp64 sigmoid of it,
            v = float32(r h), the candidate matmul on [x, v], the fp64 tanh, h' = u h + (1 - u) c in fp64.

  window[b, k] on the v half  = 4 * (3e-7 + dev_r) * |h_k| / bscale_b + |quo| * (rel_b + 4 * 2^-23)
               on the x half  = |quo| * (rel_b + 4 * 2^-23) where rel_b > 0, else 0 (x, the range and the float division are exact)
      3e-7: the absolute error csrc/gru_device.h states for sigmoid_f; dev_r: max |r32 - r64| of the two CPU runs of the call;
      4: the usual margin over a float32-CPU deviation (gru_step_model.py, bf16_step_model.py); 4 * 2^-23: the roundings of v
      and of the float quotient; rel_b: the relative error of bscale_b -- nonzero only where a v element is, or is within its
      window of, the extreme element of the call (then it is that element's window over the extreme).
  near[b, k]   = the float quotient lies within window[b, k] of n + 1/2
  allow[b, n]  = scale_c * bscale_b * sum_k near[b, k] |W_q[n, k]| * (1 - u[b, n])      (the int16 clamp and tanh are 1-Lipschitz)
                 + rel_b * |pre_c - bc|[b, n] * (1 - u[b, n])                            (the output scale's own error)
  bound[b, n]  = max(4 * 3e-7 * (|h - c| + 1)[b, n], 16 * 2^-23 * max(1, max |h'|)) + allow[b, n]
      3e-7 on u moves h' by |h - c|, on c by (1 - u) <= 1; the floor is the project's convention (gru_step_model.py).

Layer 0 runs on the fp32 kernels: gru_step_model.check_call's fp32 cell checks it, and its softmax bound checks the softmax.

CONDITIONS (asserted on the reference alone in tests/test_octbit_step_host.py, and on every GPU case):
  the (stream, layer, frame) rows that carry a near quotient are at most MAX_ALLOW_SHARE (bf16_step_model's 25 %) of a case,
  no single allowance exceeds MAX_ALLOW.
"""
import zlib
from collections import namedtuple

import numpy as np

import gru_step_model as S
from bf16_step_model import MAX_ALLOW_SHARE
from oracle import gru_oracle as G
from oracle import octbit_oracle as Q

F32 = np.float32
HID = 128
ACT_ERR, MARGIN, FLOOR = S.ACT_ERR, S.MARGIN, S.FLOOR
QUO_ERR = 4.0 * 2.0 ** -23
# The cap on one allowance.  One flip costs at most 127 * scale_w * bscale = max |W| * max |activation| / 127: 1.5e-3 for a glorot
# candidate matrix (max |W| = 0.125) at an activation range of 1.5, 1.0e-3 for the clip-heavy family's 0.125 at a range of 1.
# The CPU runs of the committed cases show at most 1.0e-3 (clip-heavy) and 6.2e-4 (glorot); 4e-3 leaves room for two flips of
# the largest kind on one row and is still 25 times below the multi-frame tolerance on a logit.
MAX_ALLOW = 4e-3
MAX_PRE = 30.0           # gru_device.h states the 3e-7 of sigmoid_f / tanh_f for arguments in [-30, 30]
CLIP_HEAVY_W = 0.125     # the clip-heavy family's constant |W|: pre-activations of a few units, far inside MAX_PRE

MUTANTS = ("no_clamp", "clamp_high_only", "half_even", "offset_128", "range_h_only", "swap_couple", "unsigned_corrected",
           "zero_k_eighth", "fc_range_per_frame", "fc_range_live_rows")
# the integer-side mutants are confined to ONE unit of the candidate of the top layer -- a fault of one lane --
MUT_UNIT, MUT_COUPLE, MUT_EIGHTH = 77, 37, 5


# ---------------------------------------------------------------------------------------------------------------------------
# the op
def matmul(x, wq, scale_w, bias, groups=None, mut=None, live_rows=None):
    """oracle.octbit_oracle.octbit_rows (the same float32 operation order) -> dict(out [R,N] float32, quo [R,K] the float
    quotients widened to fp64, bscale [R] float32, signed [R] bool, q [R,K], hi / lo [R]: the pair sums of each row that clipped high / low,
    pairs: the pair sums of one row).  mut: one of the activation- or clamp-side MUTANTS or None; live_rows [R] bool (fc_range_live_rows
    only): the rows the mutated range is taken over."""
    x = np.ascontiguousarray(x, F32)
    r_rows, k = x.shape
    assert scale_w > 0 and k % 64 == 0
    groups = np.arange(r_rows) if groups is None else np.asarray(groups)
    if mut == "fc_range_per_frame":
        groups = np.arange(r_rows)
    uniq, inv = np.unique(groups, return_inverse=True)
    ranged = x[:, k // 2:] if mut == "range_h_only" else x
    row_mn, row_mx = ranged.min(axis=1), ranged.max(axis=1)
    if mut == "fc_range_live_rows":
        row_mn, row_mx = np.where(live_rows, row_mn, F32(np.inf)), np.where(live_rows, row_mx, F32(-np.inf))
    mn = np.full(len(uniq), np.inf, F32)
    mx = np.full(len(uniq), -np.inf, F32)
    np.minimum.at(mn, inv, row_mn)
    np.maximum.at(mx, inv, row_mx)
    mn, mx = np.where(np.isfinite(mn), mn, F32(0)), np.where(np.isfinite(mx), mx, F32(0))      # a call without a live row
    signed_g = mn < 0
    bscale_g = np.where(signed_g, np.maximum(-mn, mx) / F32(127), mx / F32(254)).astype(F32)
    signed, bscale = signed_g[inv], bscale_g[inv]
    with np.errstate(divide="ignore", invalid="ignore"):
        quo = (x / bscale[:, None]).astype(np.float64)                       # the float quotient, widened for round()
    quo = np.where(bscale[:, None] == 0, 0.0, quo)
    rounded = np.rint(quo) if mut == "half_even" else np.sign(quo) * np.floor(np.abs(quo) + 0.5)
    q = rounded + np.where(signed, 128.0 if mut == "offset_128" else 127.0, 0.0)[:, None]
    q = q.astype(np.int64).astype(np.uint8).astype(np.int32)
    wt = np.ascontiguousarray(np.asarray(wq).T).astype(np.int32)             # [K, N]
    pair = q[:, 0::2, None] * wt[None, 0::2, :] + q[:, 1::2, None] * wt[None, 1::2, :]
    hi, lo = pair > 32767, pair < -32768
    acc = np.clip(pair, -32768, 32767).sum(axis=1)                           # [R, N], exact
    if mut in ("no_clamp", "clamp_high_only"):
        other = (pair if mut == "no_clamp" else np.minimum(pair, 32767)).sum(axis=1)
        acc[:, MUT_UNIT] = other[:, MUT_UNIT]
    corrected = np.ones_like(signed) if mut == "unsigned_corrected" else signed
    o = acc.astype(F32) - np.where(corrected[:, None], np.asarray(bias, F32)[None, :], F32(0))
    scale = (F32(scale_w) * bscale).astype(F32)
    out = (o.astype(F32) * scale[:, None]).astype(F32)
    return dict(out=out, quo=quo, bscale=bscale, signed=signed, q=q, hi=hi.sum(axis=(1, 2)), lo=lo.sum(axis=(1, 2)), pairs=pair[0].size)


_QUANTISED = {}


def quantised(w):
    """The quantised tables of a weight dict: ([per layer None | dict(g=(Wq, scale, b127), c=...)], fc=(Wq, scale, b127))."""
    hit = _QUANTISED.get(id(w))
    if hit is None or hit[0] is not w:
        layers = [dict(g=Q.octize_weight_int8_signed(lay["Wg"]), c=Q.octize_weight_int8_signed(lay["Wc"]))
                  if G.octbit_layer_is_quantised(l) else None for l, lay in enumerate(w["layers"])]
        hit = (w, layers, Q.octize_weight_int8_signed(w["Wfc"]))
        _QUANTISED[id(w)] = hit
    return hit[1], hit[2]


def _mutate_weights(cq, mut):
    """The weight-side mutants, on a copy of the candidate's Wq [N, K]."""
    if mut == "swap_couple":                 # couple j holds k = 4j .. 4j+3 as (even: 4j, 4j+2 | odd: 4j+1, 4j+3)
        cq = cq.copy()
        k0 = 4 * MUT_COUPLE
        cq[MUT_UNIT, [k0, k0 + 1, k0 + 2, k0 + 3]] = cq[MUT_UNIT, [k0 + 1, k0, k0 + 3, k0 + 2]]
    elif mut == "zero_k_eighth":
        cq = cq.copy()
        cq[MUT_UNIT, 32 * MUT_EIGHTH:32 * MUT_EIGHTH + 32] = 0
    return cq


def _frac_distance(quo):
    """Distance of each quotient from the nearest n + 1/2."""
    a = np.abs(quo)
    return np.abs(a - np.floor(a) - 0.5)


def cell_step(lay, tables, x, h, dtype=np.float64, mut=None):
    """One quantised layer on float32 x [B,H] (the lower layer's h' as the device returned it) and h [B,H] (the state the call was
    given).  -> dict(h_new, r, u, c, pre_g, pre_c: float32 pre-activations, dev_r, near [B,2H], near_row [B], allow [B,H],
    signed: (gates [B], candidate [B]), hi, lo [B], pairs (per stream), ties [B]: gate quotients exactly on n + 1/2)."""
    (gq, gs, gb), (cq, cs, cb) = tables["g"], tables["c"]
    x, h = np.asarray(x, F32), np.asarray(h, F32)
    act_mut = mut if mut in ("half_even", "offset_128", "range_h_only", "unsigned_corrected") else None
    mg = matmul(np.concatenate([x, h], 1), gq, gs, gb, mut=act_mut)
    pre_g = (mg["out"] + lay["bg"].astype(F32)).astype(F32)
    g32 = (F32(1) / (F32(1) + np.exp(-pre_g))).astype(F32)
    g64 = 1.0 / (1.0 + np.exp(-pre_g.astype(np.float64)))
    dev_r = float(np.abs(g32[:, :HID].astype(np.float64) - g64[:, :HID]).max())
    g = g32 if dtype == F32 else g64
    r, u = g[:, :HID], g[:, HID:]
    v = (r * h).astype(F32)
    clamp_mut = mut if mut in ("no_clamp", "clamp_high_only") else None
    mc = matmul(np.concatenate([x, v], 1), _mutate_weights(cq, mut), cs, cb, mut=act_mut or clamp_mut)
    pre_c = (mc["out"] + lay["bc"].astype(F32)).astype(F32)
    c = np.tanh(pre_c) if dtype == F32 else np.tanh(pre_c.astype(np.float64))
    hn = (u * h + (F32(1) - u) * c).astype(F32) if dtype == F32 else u * h.astype(np.float64) + (1.0 - u) * c

    # which quotients of the candidate's call the device may round the other way
    bscale = mc["bscale"].astype(np.float64)
    safe = np.where(bscale > 0, bscale, 1.0)
    win_v = MARGIN * (ACT_ERR + dev_r) * np.abs(h.astype(np.float64))                      # [B,H], in units of v
    extreme = np.where(mc["signed"], 127.0, 254.0) * bscale                                # max(-mn, mx) | mx
    reach = np.where(mc["signed"][:, None], np.abs(v.astype(np.float64)), v.astype(np.float64)) + win_v >= extreme[:, None]
    rel_b = np.where(bscale > 0, (win_v * reach).max(axis=1) / np.where(extreme > 0, extreme, 1.0), 0.0)
    rel_b = np.where(rel_b > 0, rel_b + 2.0 ** -23, 0.0)                                   # bscale's own rounding
    aq = np.abs(mc["quo"])
    window = aq * np.where(rel_b > 0, rel_b + QUO_ERR, 0.0)[:, None]
    window[:, HID:] = win_v / safe[:, None] + aq[:, HID:] * (rel_b[:, None] + QUO_ERR)
    near = (_frac_distance(mc["quo"]) <= window) & (bscale > 0)[:, None]
    one_minus_u = 1.0 - g64[:, HID:]
    wabs = np.abs(np.asarray(cq, np.float64))                                              # [N, K]
    allow = (float(cs) * bscale)[:, None] * (near.astype(np.float64) @ wabs.T) * one_minus_u
    allow = allow + rel_b[:, None] * np.abs(mc["out"].astype(np.float64)) * one_minus_u
    return dict(h_new=hn, r=r, u=u, c=c, pre_g=pre_g, pre_c=pre_c, dev_r=dev_r, near=near, near_row=near.any(axis=1), allow=allow,
                signed=(mg["signed"], mc["signed"]), hi=mg["hi"] + mc["hi"], lo=mg["lo"] + mc["lo"], pairs=mg["pairs"] + mc["pairs"],
                ties=(_frac_distance(mg["quo"]) == 0.0).sum(axis=1))


def logits_of(top_rows, w, use_relu=False, value_clip=-1.0, mut=None, live_rows=None, detail=False):
    """top_rows [B,T,H] float32: the rows the top layer emitted in ONE call, zero rows past seq_len included -> logits [B,T,C]:
    one op call per stream on its [T,H] block (one range over all T frames), + bfc, relu / clip as head_row applies them."""
    top_rows = np.asarray(top_rows, F32)
    b, t_len, _ = top_rows.shape
    fq, fs, fb = quantised(w)[1]
    m = matmul(top_rows.reshape(b * t_len, HID), fq, fs, fb, groups=np.repeat(np.arange(b), t_len), mut=mut,
               live_rows=None if live_rows is None else np.asarray(live_rows).reshape(b * t_len))
    logits = S.head((m["out"] + w["bfc"].astype(F32)).astype(F32), use_relu, value_clip).reshape(b, t_len, -1)
    return (logits, m) if detail else logits


def check_projection(w, top_rows, seq_len, dev_logits, use_relu=False, value_clip=-1.0):
    """A call of T frames: top_rows [B,T,H] the top layer's h' of every frame (as a chain of one-frame calls returned them),
    seq_len [B] or None, dev_logits [B,T,C].  The rows past seq_len are the zero rows the call emits; the logits must equal
    logits_of those rows BIT FOR BIT.  -> the op's detail (signed [B*T], bscale [B*T], ...)."""
    top_rows = np.array(top_rows, F32)
    b, t_len, _ = top_rows.shape
    if seq_len is not None:
        top_rows[np.arange(t_len)[None, :] >= np.asarray(seq_len)[:, None]] = 0.0
    want, m = logits_of(top_rows, w, use_relu, value_clip, detail=True)
    got = np.ascontiguousarray(dev_logits, F32)
    diff = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert len(diff) == 0, "projection: %d of %d logits differ, first at (stream, frame, class) %s: %r != %r" % (
        len(diff), got.size, diff[0].tolist(), float(got[tuple(diff[0])]), float(want[tuple(diff[0])]))
    return m


def emulate_call(w, mel_row, state_in, seq_len=None, reset=None, use_relu=False, value_clip=-1.0, mut=None):
    """What a one-frame call of a kernel that computes exactly gru_forward_octbit's float32 arithmetic (with `mut`) returns:
    (state [L,B,H], logits [B,C], softmax [B,C]).  The cell mutants apply to the TOP layer."""
    layers, _ = quantised(w)
    state_in = np.array(state_in, F32)
    if reset is not None:
        state_in[:, np.asarray(reset).astype(bool)] = 0.0
    nb = state_in.shape[1]
    live = np.ones(nb, bool) if seq_len is None else np.asarray(seq_len) > 0
    x, new = np.asarray(mel_row, F32), []
    nl = len(w["layers"])
    for l, lay in enumerate(w["layers"]):
        if layers[l] is None:
            hn = G.gru_cell(x, state_in[l], lay, F32)
        else:
            hn = cell_step(lay, layers[l], x, state_in[l], F32, mut if l == nl - 1 else None)["h_new"]
        new.append(np.where(live[:, None], hn, state_in[l]))
        x = hn
    top = np.where(live[:, None], x, F32(0))[:, None, :]
    fc_mut = mut if mut in ("fc_range_per_frame", "fc_range_live_rows") else None
    logits = logits_of(top, w, use_relu, value_clip, fc_mut, live[:, None])[:, 0]
    return np.stack(new), logits, S.softmax32(logits)


def check_call(w, mel_row, state_in, dev_state, dev_logits, dev_softmax=None, seq_len=None, reset=None, use_relu=False,
               value_clip=-1.0, enforce=True):
    """One one-frame call.  mel_row [B,I], state_in [L,B,H] (as given to the call), dev_state [L,B,H], dev_logits [B,C] and
    dev_softmax [B,C] (or None) as the device returned them, seq_len [B] in {0, 1} or None, reset [B] or None.  Asserts
      layer 0     gru_step_model.check_call's fp32 cell;
      live rows   each quantised layer within `bound` of the fp64 step on the DEVICE's lower-layer output;
      logits      equal to logits_of(device top state), bit for bit;
      softmax     within gru_step_model's softmax bound of the fp64 softmax of the device's own logits;
      seq_len 0   the state equals the (reset) input state and the logits equal bfc (relu / clip of bfc) bit for bit.
    enforce=False: the bounded checks are measured, not asserted.
    -> dict(layer0, decided, allowed: worst err / bound; softmax; rows, allow_rows, max_allow; hi, lo, pairs; max_pre; signed:
    every quantised call's branch as a flat bool array over (matmul, live stream); ties; err_state; logits_equal)."""
    layers, _ = quantised(w)
    mel_row = np.asarray(mel_row, F32)
    state_in = np.array(state_in, F32)
    dev_state, dev_logits = np.asarray(dev_state, F32), np.asarray(dev_logits, F32)
    nb = mel_row.shape[0]
    if reset is not None:
        state_in[:, np.asarray(reset).astype(bool)] = 0.0
    live = np.ones(nb, bool) if seq_len is None else np.asarray(seq_len) > 0
    dead = ~live
    out = dict(layer0=0.0, decided=0.0, allowed=0.0, softmax=0.0, rows=0, allow_rows=0, max_allow=0.0, hi=0, lo=0, pairs=0,
               max_pre=0.0, ties=0, err_state=0.0, signed=[])
    # layer 0 (and the softmax of the device's own logits): the fp32 model; its logits figure does not apply here
    first = dict(layers=w["layers"][:1], Wfc=w["Wfc"], bfc=w["bfc"])
    r0 = S.check_call(first, mel_row, state_in[:1], dev_state[:1], np.ascontiguousarray(np.broadcast_to(w["bfc"].astype(F32), dev_logits.shape)),
                      None, seq_len, None, precision="fp32", enforce=False)
    out["layer0"] = r0["state"]
    assert not enforce or r0["state"] <= 1.0, "layer 0 (fp32): worst err/bound %.3f (err %.3e)" % (r0["state"], r0["err_state"])
    x = dev_state[0]
    for l in range(1, len(w["layers"])):
        lay, h = w["layers"][l], state_in[l]
        s = cell_step(lay, layers[l], x, h, np.float64)
        ref = s["h_new"]
        bound = np.maximum(MARGIN * ACT_ERR * (np.abs(h.astype(np.float64) - s["c"]) + 1.0),
                           FLOOR * max(1.0, float(np.abs(ref).max()))) + s["allow"]
        err = np.abs(dev_state[l].astype(np.float64) - ref)
        ratio = (err / bound).max(axis=1)
        plain, withal = live & ~s["near_row"], live & s["near_row"]
        if plain.any():
            out["decided"] = max(out["decided"], float(ratio[plain].max()))
        if withal.any():
            out["allowed"] = max(out["allowed"], float(ratio[withal].max()))
            out["max_allow"] = max(out["max_allow"], float(s["allow"][withal].max()))
        if live.any():
            out["err_state"] = max(out["err_state"], float(err[live].max()))
            out["max_pre"] = max(out["max_pre"], float(np.abs(s["pre_g"][live]).max()), float(np.abs(s["pre_c"][live]).max()))
        out["rows"] += int(live.sum())
        out["allow_rows"] += int(withal.sum())
        for k in ("hi", "lo", "ties"):
            out[k] += int(s[k][live].sum())
        out["pairs"] += s["pairs"] * int(live.sum())
        out["signed"] += [s["signed"][0][live], s["signed"][1][live]]
        bad = live[:, None] & (err > bound)
        assert not (enforce and bad.any()), "layer %d: %d of %d live values outside the bound, worst err/bound %.3f (err %.3e) at %s" % (
            l, int(bad.sum()), int(live.sum()) * HID, float((err / bound)[live].max()), float(err[bad].max()),
            np.argwhere(bad)[:4].tolist())
        assert np.array_equal(dev_state[l][dead].view(np.int32), h[dead].view(np.int32)), "layer %d: a row with seq_len 0 moved" % l
        x = dev_state[l]
    top = np.where(live[:, None], dev_state[-1], F32(0))[:, None, :]
    want, m = logits_of(top, w, use_relu, value_clip, detail=True)
    out["signed"].append(m["signed"][live])
    out["signed"] = np.concatenate(out["signed"]) if out["signed"] else np.zeros(0, bool)
    out["logits_equal"] = bool(np.array_equal(dev_logits.view(np.int32), want[:, 0].view(np.int32)))
    if not out["logits_equal"]:
        diff = np.argwhere(dev_logits.view(np.int32) != want[:, 0].view(np.int32))
        raise AssertionError("logits: %d of %d differ from the projection of the device's own top state, first at %s: %r != %r" % (
            len(diff), dev_logits.size, diff[0].tolist(), float(dev_logits[tuple(diff[0])]), float(want[:, 0][tuple(diff[0])])))
    bfc = np.ascontiguousarray(np.broadcast_to(S.head(w["bfc"].astype(F32), use_relu, value_clip), dev_logits.shape))
    assert np.array_equal(dev_logits[dead].view(np.int32), bfc[dead].view(np.int32)), "a row with seq_len 0 emits other than bfc"
    assert np.array_equal(dev_state[0][dead].view(np.int32), state_in[0][dead].view(np.int32)), "layer 0: a row with seq_len 0 moved"
    if dev_softmax is not None:
        out["softmax"] = softmax_ratio(dev_logits, dev_softmax)
        assert not enforce or out["softmax"] <= 1.0, "softmax: worst err/bound %.3f" % out["softmax"]
    return out


def softmax_ratio(dev_logits, dev_softmax):
    """Worst err / bound of a softmax [..., C] against the fp64 softmax of the same logits, under the bound gru_step_model.py
    states for head_row: max(4 * max |float32 softmax - fp64|, 16 * 2^-23) + 4 * 1e-7 * (1 + C p_c) / S."""
    lg32 = np.asarray(dev_logits, F32).reshape(-1, np.shape(dev_logits)[-1])
    sm32 = np.asarray(dev_softmax, F32).reshape(lg32.shape)
    lg = lg32.astype(np.float64)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    s = e.sum(axis=1, keepdims=True)
    ref = e / s
    first = max(MARGIN * float(np.abs(S.softmax32(lg32).astype(np.float64) - ref).max()), FLOOR)
    sbound = first + MARGIN * S.EXP_ERR * (1.0 + lg.shape[1] * ref) / s
    return float((np.abs(sm32.astype(np.float64) - ref) / sbound).max())


class Report(object):
    """The worst ratios, the allowance share and the clip shares over the calls of one case."""

    def __init__(self):
        self.layer0 = self.decided = self.allowed = self.softmax = self.max_allow = self.max_pre = 0.0
        self.rows = self.allow_rows = self.hi = self.lo = self.pairs = self.ties = self.calls = 0
        self.signed = []

    def add(self, r):
        for k in ("layer0", "decided", "allowed", "softmax", "max_allow", "max_pre"):
            setattr(self, k, max(getattr(self, k), r[k]))
        for k in ("rows", "allow_rows", "hi", "lo", "pairs", "ties"):
            setattr(self, k, getattr(self, k) + r[k])
        self.signed.append(r["signed"])
        self.calls += 1

    @property
    def share(self):
        return self.allow_rows / max(self.rows, 1)

    @property
    def clip_hi(self):
        return self.hi / max(self.pairs, 1)

    @property
    def clip_lo(self):
        return self.lo / max(self.pairs, 1)

    @property
    def any_signed(self):
        return bool(np.concatenate(self.signed).any()) if self.signed else False

    def line(self, case, family):
        return ("OCTBIT-STEP %s %s: worst err/bound decided %.3f, allowed %.3f, layer 0 %.3f, softmax %.3f, allowance rows %.1f %%, "
                "largest allowance %.1e, clipped %.1f %% high %.1f %% low" % (
                    case, family, self.decided, self.allowed, self.layer0, self.softmax, 100.0 * self.share, self.max_allow,
                    100.0 * self.clip_hi, 100.0 * self.clip_lo))

    def check_condition(self, family, plain=True):
        """plain: a chain without masks -- a reset stream's zero state halves its row, so only there does the clip-heavy family
        promise its clip shares."""
        assert self.share <= MAX_ALLOW_SHARE, "allowance on %.1f %% of the rows" % (100.0 * self.share)
        assert self.max_allow <= MAX_ALLOW, "an allowance of %.2e" % self.max_allow
        assert self.max_pre <= MAX_PRE, "a pre-activation of %.1f" % self.max_pre
        if family == "clip" and plain and self.pairs:
            assert self.clip_hi + self.clip_lo >= 0.15 and min(self.clip_hi, self.clip_lo) >= 0.05, (self.clip_hi, self.clip_lo)
        if family == "nonneg":
            assert not self.any_signed, "a quantised call of the nonnegative family took the signed branch"


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
Case = namedtuple("Case", "family n_mel layers classes batch frames relu clip")


def _c(family, n_mel, layers, classes, batch, frames, relu=0, clip=-1.0):
    return Case(family, n_mel, layers, classes, batch, frames, relu, clip)


# batch 1 / 16 / 17 / 37: a lone stream, a full group, ragged last groups -- both halves tid >> 8 of the gate finalize, all four
# tid >> 7 quarters of the candidate finalize, all 16 slots of the exchange buffer; layers 1 (the projection range from
# octbit_top_range_kernel) / 2 / 3 (an octbit layer fed by an octbit layer, both ping-pong seams); n_mel 40 (resident layer 0)
# / 13 (generic); 3 / 8 classes (kMaxClasses)
CASES = [
    _c("glorot", 40, 2, 3, 1, 6), _c("glorot", 40, 2, 8, 16, 6), _c("glorot", 13, 3, 8, 17, 8), _c("glorot", 40, 1, 3, 17, 6),
    _c("glorot", 13, 1, 8, 16, 6), _c("glorot", 13, 2, 3, 37, 6), _c("glorot", 40, 2, 8, 17, 6, relu=1, clip=20.0),
    _c("clip", 40, 2, 3, 17, 6), _c("clip", 13, 3, 8, 37, 6),
    _c("nonneg", 40, 2, 3, 17, 6), _c("nonneg", 13, 3, 8, 16, 6), _c("nonneg", 40, 1, 8, 17, 6),
    _c("allzero", 40, 2, 3, 1, 6), _c("allzero", 13, 3, 8, 17, 6), _c("allzero", 40, 1, 3, 17, 6),
    _c("ties", 40, 2, 3, 17, 6),
]
PERSISTENT = _c("glorot", 40, 2, 3, 16 * 3 + 5, 2)


def case_id(c):
    return "%s_n%d_L%d_C%d_B%d_T%d%s" % (c.family, c.n_mel, c.layers, c.classes, c.batch, c.frames, "_relu" if c.relu else "")


def seed_of(c):
    return zlib.crc32(case_id(c).encode()) & 0x3FFFFFFF


def zero_streams(c):
    """allzero family: the streams whose every quantised call is all-zero (zero mel row, zero state, reset at every masked frame)
    -- every stream of a batch of one, else streams 0, 5 and the last inside an otherwise ordinary batch."""
    if c.family != "allzero":
        return np.zeros(c.batch, bool)
    z = np.zeros(c.batch, bool)
    z[[0, min(5, c.batch - 1), c.batch - 1]] = True
    return z


def case_inputs(c):
    """(weights, mel [B,T,I], state [L,B,H]) of a case; the seeds depend on the case alone.
      glorot   G.random_weights, a random state: the baseline
      clip     the quantised layers' Wg, Wc of constant magnitude CLIP_HEAVY_W and random sign: |W_q| = 127 everywhere
      nonneg   layer-0 weights zero, bc_0 > 0, state >= 0: x >= 0; upper layers' bc >= 3: h' >= 0 -- every quantised call unsigned
      allzero  bc_0 = 0 and, on zero_streams(c), a zero mel row and a zero state: x == 0, h == 0, bscale == 0, the op output 0
      ties     glorot with an upper-layer state whose gate quotients sit exactly on n + 1/2 (range 127/128, values (n + 1/2)/128)"""
    seed = seed_of(c)
    rng = np.random.default_rng(seed + 7)
    w = G.random_weights(c.n_mel, HID, c.layers, c.classes, seed=seed)
    if c.relu:
        w["Wfc"] = (w["Wfc"] * F32(20)).astype(F32)          # logits cross the clip at 20, as the relu rows of config_space_grid.py
    mel = G.synthetic_mel(c.batch, c.frames, c.n_mel, seed=seed + 1)
    st0 = (0.5 * np.random.default_rng(seed + 2).standard_normal((c.layers, c.batch, HID))).astype(F32)
    if c.family == "clip":
        for lay in w["layers"][1:]:
            for k in ("Wg", "Wc"):
                lay[k] = (F32(CLIP_HEAVY_W) * np.where(rng.random(lay[k].shape) < 0.5, -1.0, 1.0)).astype(F32)
    elif c.family == "nonneg":
        w["layers"][0]["Wg"][:] = 0
        w["layers"][0]["Wc"][:] = 0
        w["layers"][0]["bc"] = (2.5 + np.abs(w["layers"][0]["bc"])).astype(F32)      # x -> tanh(bc_0) > r h: the range is mostly x's
        for lay in w["layers"][1:]:
            lay["bc"] = (3.0 + np.abs(lay["bc"])).astype(F32)
        st0 = np.abs(st0)
    elif c.family == "allzero":
        w["layers"][0]["bc"][:] = 0
        z = zero_streams(c)
        mel[z] = 0
        st0[:, z] = 0
    elif c.family == "ties":
        st0 = np.clip(st0, -0.9, 0.9)
        st0[1:, :, 0] = 127.0 / 128.0
        for j in range(1, 13):
            st0[1:, :, j] = (-1.0) ** j * (2 * j + 0.5) / 128.0
    return w, mel, st0
