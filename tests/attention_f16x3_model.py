"""Rounding model of the f16x3 attention path (csrc/attention_f16x3.hip) in numpy -- a helper, not a test.

float32 `@` throughout: fp32 accumulation and exact fp16 x fp16 products, as the matrix pipe gives them.  A split GEMM takes
both operands as fp16 pieces, hi = fp16(v) and lo = fp16((v - hi) * s) (round-to-nearest-even; s = 2^11, or 1 for unscaled lo
pieces, which fall into fp16's subnormal range for weights of O(0.1)), and sums Xh.Wh + (Xh.Wl + Xl.Wh) / s; `pieces=1` drops
the two lo products (one fp16 piece per operand).  The embedding sees mel * 2^-8 against W_in * 2^8 (both exact); activations are
clamped to +-65504 before the conversion.  The attention core, layer norm, output projection and softmax are never split.

    forward(cfg, w, mel, split=("embed", "qkv", "ffn"), scaled_lo=True, pieces=2) -> (logits, softmax) float32 [T', C]
"""
import numpy as np

import attention_model as AM

F32 = np.float32
HALF_MAX = F32(65504.0)
GEMMS = ("embed", "qkv", "ffn")


def _f16(v):
    return np.asarray(v, F32).astype(np.float16).astype(F32)


def split(v, scaled_lo=True):
    """v (float32, |v| clamped to fp16's range) -> (hi, lo, s) with v ~ hi + lo / s."""
    v = np.clip(np.asarray(v, F32), -HALF_MAX, HALF_MAX)
    s = F32(2048.0 if scaled_lo else 1.0)
    hi = _f16(v)
    return hi, _f16((v - hi) * s), s


def gemm(x, w, on, scaled_lo=True, pieces=2):
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    if not on:
        return x @ w
    xh, xl, s = split(x, scaled_lo)
    wh, wl, _ = split(w, scaled_lo)
    main = xh @ wh
    if pieces == 1:
        return main
    return main + (xh @ wl + xl @ wh) / s


def layer_norm(x, gamma, beta):
    mu = x.mean(dtype=F32)
    var = ((x - mu) ** 2).mean(dtype=F32)
    return (x - mu) / np.sqrt(var + F32(AM.LN_EPS)) * gamma + beta


def attention(qkv, H, heads):
    d = H // heads
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    out = np.empty((qkv.shape[0], H), F32)
    for h in range(heads):
        s = slice(h * d, (h + 1) * d)
        a = (q[:, s] * F32(1.0 / np.sqrt(d))) @ k[:, s].T
        a = np.exp(a - a.max(1, keepdims=True))
        out[:, s] = (a @ v[:, s]) / a.sum(1, keepdims=True)
    return out


def forward(cfg, w, mel, split=GEMMS, scaled_lo=True, pieces=2):
    kw = dict(scaled_lo=scaled_lo, pieces=pieces)
    f32 = lambda a: np.asarray(a, F32)
    H = cfg.hidden_size
    x = AM.stack_frames(mel, cfg.combine_frame).astype(F32)
    if "embed" in split:
        x = gemm(x * F32(2.0 ** -8), f32(w["W_in"]) * F32(2.0 ** 8), True, **kw)
    else:
        x = x @ f32(w["W_in"])
    x = (x + f32(w["b_in"])) + AM.pe_table(x.shape[0], H)
    for lay in w["layers"]:
        qkv = gemm(x, lay["W_qkv"], "qkv" in split, **kw) + f32(lay["b_qkv"])
        y = layer_norm(attention(qkv, H, cfg.multi_head_num) + x, f32(lay["ln_a_gamma"]), f32(lay["ln_a_beta"]))
        inner = np.maximum(gemm(y, lay["W1"], "ffn" in split, **kw) + f32(lay["b1"]), F32(0.0))
        z = (gemm(inner, lay["W2"], "ffn" in split, **kw) + f32(lay["b2"])) + y
        x = layer_norm(z, f32(lay["ln_b_gamma"]), f32(lay["ln_b_beta"]))
    logits = x @ f32(w["W_out"]) + f32(w["b_out"])
    if cfg.use_relu:
        logits = np.maximum(logits, F32(0.0))
    if not logits.size:
        return logits, logits.copy()
    e = np.exp(logits - logits.max(1, keepdims=True))
    return logits, e / e.sum(1, keepdims=True)
