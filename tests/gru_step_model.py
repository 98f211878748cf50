"""Single-step restatement of the fp32 and f16x3 GRU stacks (csrc/gru_kernels.hip, gru_resident.hip, gru_f16x3.hip,
gru_f16x3_generic.hip) for frame-by-frame checks at a measured bound -- a helper, numpy only, not a test.

The multi-frame tests hold one flat 1e-4 on logits and state.  A ONE-FRAME call returns the fp32 h' of every layer, and the
input of layer l+1 is an exact function of numbers the call returns (h'_l itself; under the residual wrapper the float32
0.7071 (h'_l + x_l), which the kernel forms with one add and one multiply and which is formed the same way here).  Fed the
device's own carried state and the device's own lower-layer output, each layer is ONE cell against the fp64 cell, and what
may separate the two is the rounding of that one cell.

cell_step(lay, x, h, mode) -> h', r, u, c
  "f64"    oracle.gru_oracle.gru_cell in float64: the reference.
  "f32"    every value float32; a dot product starts from the bias and accumulates SEQUENTIALLY in k-chunks of 4 (the K of
           v_mfma_f32_16x16x4_f32), x rows first, then the hidden rows: acc = f32(acc + x[:, k:k+4] @ W[k:k+4]) -- a chained
           accumulation as in the kernels, no BLAS summation tree.  sigmoid = 1 / (1 + exp(-a)), tanh = 1 - 2 / (1 + exp(2a)),
           h' = u h + (1 - u) c (gru_device.h, gru_kernels.hip).
  "f16x3"  operands as two fp16 pieces, three products per chunk of 32 (the K of v_mfma_f32_16x16x32_f16), fp32 accumulation,
           as csrc/f16x3_device.h, the header of csrc/gru_f16x3.hip and weight_pack.hip state it.  The activations' exponent
           scales ride in the weights and biases (gates: -log2 e, candidate: 2 log2 e, one float32 multiply each), so a
           pre-activation is the argument of exp2: sigmoid = 1 / (1 + exp2(p)), tanh = fma(1 / (1 + exp2(p)), -2, 1),
           h' = fma(u, h - c, c).
           hidden 128 (gru_f16x3.hip): ONE accumulator; the lo piece of hidden values (h, r*h, an upper layer's input) and of
             their weights is UNSCALED, fp16(v - hi), and goes into the accumulator of hi.  The first layer's x-part is the
             exception: mel * 2^-8 (clamped to +-65504) against weights * 2^8, both lo pieces scaled by 2^11, the two cross
             products in a lo accumulator that is folded in with one fma (lo * 2^-11 + main) in front of the activation.
           any other hidden size (gru_f16x3_generic.hip): lo pieces scaled by 2^11 THROUGHOUT, a main and a lo accumulator
             per gate, folded with one fma.
  zero_lo_chunk=k, sigmoid_eps=, tanh_eps= MUTATE the restatement (the lo pieces of the 32 recurrent rows [32k, 32k+32) of
  the gate weights zeroed -- f16x3 only; a constant added to both sigmoids / to the tanh).  Only tests/test_gru_step_host.py
  uses them: they are the numeric slips the bound has to see.

Wrapped stacks (kws_create_wrapped; fp32 only): the cell reads layer_norm(x) (tests/wrapped_cell_model.py; the float32 runs
normalise in float32 as wrap_frame in gru_kernels.hip does: mean, then the variance around it, one rsqrt), layer 0 reads
layer_norm(mel); the residual output 0.7071 (h' + x) of a layer above the first is what the next layer and the projection see.

check_call, per layer, on the DEVICE's own lower-layer state:
  yardstick   = the f32 run for fp32 kernels, the f16x3 run for f16x3 kernels
  bound[b,i]  = max(4 * max |h'_yardstick - h'_f64|, 16 * 2^-23 * max(1, max |h'_f64|))
                + 4 * 3e-7 * (|h - c| + 1)[b,i]
      4x the deviation of a float32-CPU run, floored at 16 ulp: the project's convention (test_gpu_enroll.py, test_gpu_beam.py,
      bf16_step_model.py);  3e-7: the absolute error csrc/gru_device.h states for sigmoid_f / tanh_f -- on u it moves h' by
      |h - c|, on c by (1 - u) <= 1.
  No further term: the residual output is reproduced in float32 exactly as the kernel forms it (one add, one multiply by the
  float32 constant -- no product-sum for the compiler to contract), so it needs no allowance of its own.
  logits      within max(4 * max |yardstick - fp64|, 16 * 2^-23 * max |fp64|) of top . Wfc + bfc on the device's top output;
              the yardstick adds each wave's quarter of the units in chunks (fp32: of 4, f16x3: of 32), wave 0 starting from
              bfc, and then the four partials ((p0 + p1) + p2) + p3 (epilogue_fold).  relu / clip are applied to reference and
              yardstick alike: both are 1-Lipschitz, the bound stays.
  softmax     against the fp64 softmax of the device's OWN logits: max(4 * max |float32 softmax - fp64|, 16 * 2^-23)
              + 4 * 1e-7 * (1 + C p_c) / S.  1e-7: the error gru_device.h (head_row) states for __expf at arguments <= 0; with
              p_c = e_c / S and every e_k off by at most eps, |dp_c| <= eps (1 + C p_c) / S (S = sum_k e_k >= 1).
  seq_len 0   the state equals the (reset) input state and the logits equal bfc (under relu: relu / clip of bfc) bit for bit.
"""
import numpy as np

from oracle import gru_oracle as G
from wrapped_cell_model import LN_EPSILON, RESIDUAL_SCALE, layer_norm

F32 = np.float32
ACT_ERR = 3e-7          # csrc/gru_device.h: sigmoid_f / tanh_f, absolute
EXP_ERR = 1e-7          # csrc/gru_device.h, head_row: __expf at arguments <= 0
MARGIN = 4.0
FLOOR = 16.0 * 2.0 ** -23
LOG2E = F32(1.4426950408889634)
LO_SCALE, LO_INV = F32(2048.0), F32(1.0 / 2048.0)
MEL_SCALE = F32(1.0 / 256.0)
HALF_MAX = F32(65504.0)
RES32 = F32(RESIDUAL_SCALE)
YARDSTICK = {"fp32": "f32", "f16x3": "f16x3"}


def _f16(v):
    return np.asarray(v, F32).astype(np.float16).astype(F32)


def split(v, scaled):
    """v (float32) -> (hi, lo): hi = fp16(v), lo = fp16((v - hi) * 2^11) if scaled else fp16(v - hi)."""
    v = np.asarray(v, F32)
    hi = _f16(v)
    return hi, _f16((v - hi) * LO_SCALE if scaled else v - hi)


def _chain(acc, x, w, step):
    """acc = f32(acc + x[:, k:k+step] @ w[k:k+step]) chunk after chunk, all float32."""
    for k in range(0, x.shape[1], step):
        acc = acc + x[:, k:k + step] @ w[k:k + step]
    return acc


def _chain3(am, al, x, w, scaled, zero_lo_rows=None):
    """One f16x3 product, chunk by chunk of 32 rows: Wh Xh into the main accumulator, then Wl Xh and Wh Xl into the lo
    accumulator (scaled lo pieces) or into the main one (unscaled).  -> (am, al)"""
    xh, xl = split(x, scaled)
    wh, wl = split(w, scaled)
    if zero_lo_rows is not None:
        wl = wl.copy()
        wl[zero_lo_rows] = 0.0
    for k in range(0, x.shape[1], 32):
        s = slice(k, k + 32)
        am = am + xh[:, s] @ wh[s]
        if scaled:
            al = (al + xh[:, s] @ wl[s]) + xl[:, s] @ wh[s]
        else:
            am = (am + xh[:, s] @ wl[s]) + xl[:, s] @ wh[s]
    return am, al


def _fma(a, b, c):
    """float32 fma: the float64 product of two float32 values is exact."""
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, np.float64)).astype(F32)


def _cell_f64(lay, x, h):
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    hdim = h.shape[1]
    g = 1.0 / (1.0 + np.exp(-(np.concatenate([x, h], 1) @ lay["Wg"].astype(np.float64) + lay["bg"].astype(np.float64))))
    r, u = g[:, :hdim], g[:, hdim:]
    c = np.tanh(np.concatenate([x, r * h], 1) @ lay["Wc"].astype(np.float64) + lay["bc"].astype(np.float64))
    return G.gru_cell(x, h, lay, np.float64), r, u, c


def _cell_f32(lay, x, h, sigmoid_eps, tanh_eps):
    x, h = np.asarray(x, F32), np.asarray(h, F32)
    i_l, hdim = x.shape[1], h.shape[1]
    wg, wc = lay["Wg"].astype(F32), lay["Wc"].astype(F32)
    one, two = F32(1.0), F32(2.0)
    acc = np.broadcast_to(lay["bg"].astype(F32), (x.shape[0], 2 * hdim))
    acc = _chain(_chain(acc, x, wg[:i_l], 4), h, wg[i_l:], 4)
    g = one / (one + np.exp(-acc)) + F32(sigmoid_eps)
    r, u = g[:, :hdim], g[:, hdim:]
    acc = np.broadcast_to(lay["bc"].astype(F32), (x.shape[0], hdim))
    acc = _chain(_chain(acc, x, wc[:i_l], 4), r * h, wc[i_l:], 4)
    c = one - two / (one + np.exp(two * acc)) + F32(tanh_eps)
    hn = u * h + (one - u) * c
    assert hn.dtype == F32
    return hn, r, u, c


def _cell_f16x3(lay, x, h, first, zero_lo_chunk, sigmoid_eps, tanh_eps):
    x, h = np.asarray(x, F32), np.asarray(h, F32)
    nb, i_l, hdim = x.shape[0], x.shape[1], h.shape[1]
    resident = hdim == 128                 # gru_f16x3.hip; otherwise gru_f16x3_generic.hip
    one = F32(1.0)
    # weight_pack.hip: v = (first layer's x-part: 256) * (act * v)
    wg, wc = (-LOG2E) * lay["Wg"].astype(F32), (F32(2.0) * LOG2E) * lay["Wc"].astype(F32)
    bg, bc = lay["bg"].astype(F32) * (-LOG2E), lay["bc"].astype(F32) * (F32(2.0) * LOG2E)
    if first:
        xs = np.clip(x * MEL_SCALE, -HALF_MAX, HALF_MAX)
        x_scaled, x_w = True, F32(256.0)
    else:
        xs, x_scaled, x_w = x, not resident, one
    h_scaled = not resident
    zero = None if zero_lo_chunk is None else slice(32 * zero_lo_chunk, 32 * zero_lo_chunk + 32)

    def pre(w, bias, hvec, cols, zero_rows=None):
        am = np.broadcast_to(bias, (nb, cols))
        al = np.zeros((nb, cols), F32)
        am, al = _chain3(am, al, xs, x_w * w[:i_l], x_scaled)
        am, al = _chain3(am, al, hvec, w[i_l:], h_scaled, zero_rows)
        return _fma(al, LO_INV, am)        # al is zero where every lo piece went into the main accumulator

    with np.errstate(over="ignore"):
        g = one / (one + np.exp2(pre(wg, bg, h, 2 * hdim, zero))) + F32(sigmoid_eps)
        r, u = g[:, :hdim], g[:, hdim:]
        c = _fma(one / (one + np.exp2(pre(wc, bc, r * h, hdim))), -2.0, one) + F32(tanh_eps)
    hn = _fma(u, h - c, c)
    assert hn.dtype == F32 and g.dtype == F32
    return hn, r, u, c


def cell_step(lay, x, h, mode="f64", first=True, zero_lo_chunk=None, sigmoid_eps=0.0, tanh_eps=0.0):
    """One GRU cell.  x [B,I]: the layer's input (first: the mel row -- only the f16x3 run tells the two apart), h [B,H]: the
    state the call was given.  -> (h_new, r, u, c) in the mode's precision."""
    with np.errstate(over="ignore"):
        if mode == "f64":
            assert zero_lo_chunk is None and sigmoid_eps == 0.0 and tanh_eps == 0.0, "the reference has no mutants"
            return _cell_f64(lay, x, h)
        if mode == "f32":
            assert zero_lo_chunk is None, "zero_lo_chunk mutates the f16x3 run"
            return _cell_f32(lay, x, h, sigmoid_eps, tanh_eps)
        assert mode == "f16x3", mode
        return _cell_f16x3(lay, x, h, first, zero_lo_chunk, sigmoid_eps, tanh_eps)


def layer_norm32(x, ibeta, igamma):
    """wrap_frame (gru_kernels.hip) in float32: the mean, the variance around it, (x - mu) * (ibeta * rsqrt(var + 1e-5)) + igamma."""
    x = np.asarray(x, F32)
    n = F32(x.shape[1])
    d = x - (x.sum(axis=1, dtype=F32, keepdims=True) / n)
    var = (d * d).sum(axis=1, dtype=F32, keepdims=True) / n
    return d * (F32(ibeta) * (F32(1.0) / np.sqrt(var + F32(LN_EPSILON)))) + np.asarray(igamma, F32)


def _cell_input(lay, x_raw, mode, use_ln):
    if not use_ln:
        return x_raw
    if mode == "f64":
        return layer_norm(np.asarray(x_raw, np.float64), lay["ibeta"], lay["igamma"])
    return layer_norm32(x_raw, lay["ibeta"], lay["igamma"])


def _layer_output(hn, x_raw, layer, mode, use_res):
    """What the layer hands upward: h', or above the first layer under the residual wrapper 0.7071 (h' + x)."""
    if not use_res or layer == 0:
        return hn
    if mode == "f64":
        return RESIDUAL_SCALE * (np.asarray(hn, np.float64) + np.asarray(x_raw, np.float64))
    return RES32 * (np.asarray(hn, F32) + np.asarray(x_raw, F32))          # gru_kernels.hip: kResidualScale * (hn + xr[e])


def stack_step(w, x, state, mode="f64", wrap=(False, False), **mutant):
    """One frame of the whole stack on its OWN values: (x [B,I], state [L,B,H]) -> (state' [L,B,H], top output [B,H]).
    A zero_lo_chunk mutant applies to layer 0."""
    dtype = np.float64 if mode == "f64" else F32
    x_raw = np.asarray(x, dtype)
    new = []
    for l, lay in enumerate(w["layers"]):
        mut = dict(mutant) if l == 0 else {k: v for k, v in mutant.items() if k != "zero_lo_chunk"}
        hn = cell_step(lay, _cell_input(lay, x_raw, mode, wrap[0]), np.asarray(state[l], dtype), mode, first=l == 0, **mut)[0]
        x_raw = _layer_output(hn, x_raw, l, mode, wrap[1])
        new.append(hn)
    return np.stack(new), x_raw


def project(top, w, mode="f64"):
    """top [B,H] -> top . Wfc + bfc [B,C]."""
    if mode == "f64":
        return np.asarray(top, np.float64) @ w["Wfc"].astype(np.float64) + w["bfc"].astype(np.float64)
    top, wfc = np.asarray(top, F32), w["Wfc"].astype(F32)
    hdim, c = wfc.shape
    q = hdim // 4
    parts = []
    for wave in range(4):
        rows = slice(q * wave, q * wave + q)
        am = np.broadcast_to(w["bfc"].astype(F32), (top.shape[0], c)) if wave == 0 else np.zeros((top.shape[0], c), F32)
        if mode == "f32":
            parts.append(_chain(am, top[:, rows], wfc[rows], 4))
        else:
            scaled = hdim != 128
            am, al = _chain3(am, np.zeros((top.shape[0], c), F32), top[:, rows], wfc[rows], scaled)
            parts.append(_fma(al, LO_INV, am) if scaled else am)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def head(logits, use_relu=False, value_clip=-1.0):
    """models/rnn_ctc.py:280-283 in the dtype of `logits`."""
    if use_relu:
        logits = np.maximum(logits, logits.dtype.type(0))
        if value_clip > 0:
            logits = np.minimum(logits, logits.dtype.type(20))
    return logits


def softmax32(logits):
    """head_row (gru_device.h) in float32: exp(l - max), the sum class by class, one reciprocal."""
    lg = np.asarray(logits, F32)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    s = np.zeros((lg.shape[0], 1), F32)
    for k in range(lg.shape[1]):
        s = s + e[:, k:k + 1]
    return e * (F32(1.0) / s)


def emulate_call(w, mel_row, state_in, precision="fp32", wrap=(False, False), use_relu=False, value_clip=-1.0, seq_len=None,
                 reset=None, **mutant):
    """What a one-frame call of a kernel that computes exactly the yardstick run (with `mutant`) would return:
    (state [L,B,H], logits [B,C], softmax [B,C]), float32."""
    mode = YARDSTICK[precision]
    state_in = np.array(state_in, F32)
    if reset is not None:
        state_in[:, np.asarray(reset).astype(bool)] = 0.0
    live = np.ones(state_in.shape[1], bool) if seq_len is None else np.asarray(seq_len) > 0
    new, top = stack_step(w, np.asarray(mel_row, F32), state_in, mode, wrap, **mutant)
    new = np.where(live[None, :, None], new, state_in)
    logits = head(project(np.where(live[:, None], top, F32(0.0)), w, mode), use_relu, value_clip)
    return new, logits, softmax32(logits)


def check_call(w, mel_row, state_in, dev_state, dev_logits, dev_softmax=None, seq_len=None, reset=None, precision="fp32",
               wrap=(False, False), use_relu=False, value_clip=-1.0, enforce=True):
    """One one-frame call.  mel_row [B,I], state_in [L,B,H] (as given to the call), dev_state [L,B,H], dev_logits [B,C] and
    dev_softmax [B,C] (or None) as the device returned them, seq_len [B] in {0, 1} or None, reset [B] or None.  Asserts what
    the module's header lists (enforce=False: the bit-for-bit checks only, the ratios are returned).
    -> dict(state, logits, softmax: worst err / bound over the live rows; err_state, err_logits: worst absolute errors)."""
    mode = YARDSTICK[precision]
    mel_row = np.asarray(mel_row, F32)
    state_in = np.array(state_in, F32)
    dev_state = np.asarray(dev_state, F32)
    dev_logits = np.asarray(dev_logits, F32)
    nb = mel_row.shape[0]
    if reset is not None:
        state_in[:, np.asarray(reset).astype(bool)] = 0.0
    live = np.ones(nb, bool) if seq_len is None else np.asarray(seq_len) > 0
    dead = ~live
    out = dict(state=0.0, logits=0.0, softmax=0.0, err_state=0.0, err_logits=0.0)
    x_raw = mel_row
    for l, lay in enumerate(w["layers"]):
        h = state_in[l]
        yard = cell_step(lay, _cell_input(lay, x_raw, mode, wrap[0]), h, mode, first=l == 0)[0]
        ref, _, _, c = cell_step(lay, _cell_input(lay, x_raw, "f64", wrap[0]), h, "f64")
        first = max(MARGIN * float(np.abs(yard.astype(np.float64) - ref).max()), FLOOR * max(1.0, float(np.abs(ref).max())))
        bound = first + MARGIN * ACT_ERR * (np.abs(h.astype(np.float64) - c) + 1.0)
        err = np.abs(dev_state[l].astype(np.float64) - ref)
        if live.any():
            out["state"] = max(out["state"], float((err / bound)[live].max()))
            out["err_state"] = max(out["err_state"], float(err[live].max()))
        bad = live[:, None] & (err > bound)
        assert not (enforce and bad.any()), "layer %d: %d of %d live values outside the bound, worst err/bound %.3f (err %.3e) at %s" % (
            l, int(bad.sum()), int(live.sum()) * h.shape[1], float((err / bound)[live].max()), float(err[bad].max()),
            np.argwhere(bad)[:4].tolist())
        assert np.array_equal(dev_state[l][dead].view(np.int32), h[dead].view(np.int32)), "layer %d: a row with seq_len 0 moved" % l
        x_raw = _layer_output(dev_state[l], x_raw, l, mode, wrap[1])
    if live.any():
        top = x_raw[live]
        ref = head(project(top, w, "f64"), use_relu, value_clip)
        yard = head(project(top, w, mode), use_relu, value_clip)
        lbound = max(MARGIN * float(np.abs(yard.astype(np.float64) - ref).max()), FLOOR * float(np.abs(ref).max()))
        lerr = float(np.abs(dev_logits[live].astype(np.float64) - ref).max())
        out["logits"], out["err_logits"] = lerr / lbound, lerr
        assert not enforce or lerr <= lbound, "logits: err %.3e, bound %.3e" % (lerr, lbound)
    bfc = np.ascontiguousarray(np.broadcast_to(head(w["bfc"].astype(F32), use_relu, value_clip), dev_logits.shape))
    assert np.array_equal(dev_logits[dead].view(np.int32), bfc[dead].view(np.int32)), "a row with seq_len 0 emits other than bfc"
    if dev_softmax is not None:
        lg = dev_logits.astype(np.float64)
        e = np.exp(lg - lg.max(axis=1, keepdims=True))
        s = e.sum(axis=1, keepdims=True)
        ref = e / s
        first = max(MARGIN * float(np.abs(softmax32(dev_logits).astype(np.float64) - ref).max()), FLOOR)
        sbound = first + MARGIN * EXP_ERR * (1.0 + lg.shape[1] * ref) / s
        ratio = float((np.abs(np.asarray(dev_softmax, F32).astype(np.float64) - ref) / sbound).max())
        out["softmax"] = ratio
        assert not enforce or ratio <= 1.0, "softmax: worst err/bound %.3f" % ratio
    return out


class Report(object):
    """The worst ratios over the calls of one case."""

    def __init__(self):
        self.state = self.logits = self.softmax = 0.0
        self.calls = 0

    def add(self, r):
        self.state, self.logits, self.softmax = max(self.state, r["state"]), max(self.logits, r["logits"]), max(self.softmax, r["softmax"])
        self.calls += 1

    def line(self, case, names):
        return "GRU-STEP %s %s: worst err/bound state %.3f, logits %.3f, softmax %.3f" % (
            case, " | ".join(n for n in names if n), self.state, self.logits, self.softmax)
