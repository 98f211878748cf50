"""Weights of the self-attention CTC model (models/attention_ctc.py): the canonical dict, the flat fp32 blob
kws_attention_create takes, and the TF variable names of the reference graph.

dict layout (one entry per variable the reference graph creates, all under `model/`, main.py:54):
  W_in  [c*F, H]  input_linear_trans/kernel                (a 1x1 conv2d: stored [1, 1, c*F, H] in a checkpoint; F = config.freq_size)
  b_in  [H]       input_linear_trans/bias
  layers[j] = {W_qkv [H, 3H]   layer_j/self_attention/qkv_transform/kernel    (q, k, v = columns [0,H), [H,2H), [2H,3H))
               b_qkv [3H]      .../qkv_transform/bias
               ln_a_beta, ln_a_gamma [H]   layer_j/LayerNorm/{beta,gamma}     (after the attention)
               W1 [H, Fi], b1 [Fi]         layer_j/feed_forward/conv1/{kernel,bias}
               W2 [Fi, H], b2 [H]          layer_j/feed_forward/conv2/{kernel,bias}
               ln_b_beta, ln_b_gamma [H]   layer_j/LayerNorm_1/{beta,gamma}   (after the feed-forward)}
  W_out [H, C]    output_linear_trans/kernel
  b_out [C]       output_linear_trans/bias
The blob (kws_attention_weights_nbytes) is this order, row-major: W_in, b_in, per layer W_qkv, b_qkv, ln_a_beta, ln_a_gamma,
W1, b1, W2, b2, ln_b_beta, ln_b_gamma, then W_out, b_out.
"""
import re

import numpy as np

LAYER_KEYS = ("W_qkv", "b_qkv", "ln_a_beta", "ln_a_gamma", "W1", "b1", "W2", "b2", "ln_b_beta", "ln_b_gamma")
TOP_KEYS = ("W_in", "b_in", "W_out", "b_out")
_TF_TOP = {"W_in": "input_linear_trans/kernel", "b_in": "input_linear_trans/bias",
           "W_out": "output_linear_trans/kernel", "b_out": "output_linear_trans/bias"}
_TF_LAYER = {"W_qkv": "self_attention/qkv_transform/kernel", "b_qkv": "self_attention/qkv_transform/bias",
             "ln_a_beta": "LayerNorm/beta", "ln_a_gamma": "LayerNorm/gamma",
             "W1": "feed_forward/conv1/kernel", "b1": "feed_forward/conv1/bias",
             "W2": "feed_forward/conv2/kernel", "b2": "feed_forward/conv2/bias",
             "ln_b_beta": "LayerNorm_1/beta", "ln_b_gamma": "LayerNorm_1/gamma"}
_KEY_OF_TOP = {v: k for k, v in _TF_TOP.items()}
_KEY_OF_LAYER = {v: k for k, v in _TF_LAYER.items()}


def shapes(config):
    """({top key: shape}, {layer key: shape}) for `config` (an AttentionConfig)."""
    h, fi, c = config.hidden_size, config.feed_forward_inner_size, config.num_classes
    k = config.freq_size * config.combine_frame          # F = n_mel, or 3 * n_mfcc with config.mfcc (config/attention_config.py:97-99)
    top = {"W_in": (k, h), "b_in": (h,), "W_out": (h, c), "b_out": (c,)}
    layer = {"W_qkv": (h, 3 * h), "b_qkv": (3 * h,), "ln_a_beta": (h,), "ln_a_gamma": (h,), "W1": (h, fi), "b1": (fi,),
             "W2": (fi, h), "b2": (h,), "ln_b_beta": (h,), "ln_b_gamma": (h,)}
    return top, layer


def init(config, seed=0):
    """Random weights of the reference architecture (no checkpoint exists offline): uniform kernels scaled by 1/sqrt(fan_in),
    and -- unlike TF's initial values -- nonzero biases and betas and gammas away from 1, so that a swapped or dropped table
    changes the result."""
    rng = np.random.default_rng(seed)
    top, layer = shapes(config)

    def draw(key, shape):
        if key.startswith("W"):
            return rng.uniform(-1.0, 1.0, shape) * np.sqrt(3.0 / shape[0])
        if key.endswith("gamma"):
            return 1.0 + rng.uniform(-0.3, 0.3, shape)
        return rng.uniform(-0.2, 0.2, shape)

    w = {k: draw(k, s).astype(np.float32) for k, s in top.items()}
    w["layers"] = [{k: draw(k, s).astype(np.float32) for k, s in layer.items()} for _ in range(config.num_layers)]
    return w


def check_shapes(config, w):
    top, layer = shapes(config)
    if len(w["layers"]) != config.num_layers:
        raise ValueError("expected %d layers, got %d" % (config.num_layers, len(w["layers"])))
    for k, s in top.items():
        if k not in w:
            raise ValueError("no %s (%s)" % (k, _TF_TOP[k]))
        if tuple(np.shape(w[k])) != s:
            raise ValueError("%s has shape %s, expected %s" % (k, tuple(np.shape(w[k])), s))
    for j, lay in enumerate(w["layers"]):
        for k, s in layer.items():
            if k not in lay:
                raise ValueError("layer %d has no %s (layer_%d/%s)" % (j, k, j, _TF_LAYER[k]))
            if tuple(np.shape(lay[k])) != s:
                raise ValueError("layer %d %s has shape %s, expected %s" % (j, k, tuple(np.shape(lay[k])), s))


def to_blob(config, w):
    check_shapes(config, w)
    parts = [w["W_in"], w["b_in"]]
    for lay in w["layers"]:
        parts += [lay[k] for k in LAYER_KEYS]
    parts += [w["W_out"], w["b_out"]]
    return np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).ravel() for p in parts]))


def from_blob(config, blob):
    blob = np.asarray(blob, np.float32).ravel()
    top, layer = shapes(config)
    pos = 0

    def take(shape):
        nonlocal pos
        n = int(np.prod(shape))
        out = blob[pos:pos + n].reshape(shape).copy()
        pos += n
        return out

    w = {"W_in": take(top["W_in"]), "b_in": take(top["b_in"])}
    w["layers"] = [{k: take(layer[k]) for k in LAYER_KEYS} for _ in range(config.num_layers)]
    w["W_out"], w["b_out"] = take(top["W_out"]), take(top["b_out"])
    if pos != blob.size:
        raise ValueError("blob has %d floats, config needs %d" % (blob.size, pos))
    return w


def tf_names(config, prefix="model/"):
    """Every variable name of the reference graph for `config`, in blob order."""
    names = [prefix + _TF_TOP["W_in"], prefix + _TF_TOP["b_in"]]
    for j in range(config.num_layers):
        names += ["%slayer_%d/%s" % (prefix, j, _TF_LAYER[k]) for k in LAYER_KEYS]
    return names + [prefix + _TF_TOP["W_out"], prefix + _TF_TOP["b_out"]]


def from_tf_variables(config, variables):
    """Canonical dict from a {TF variable name: array} mapping (e.g. tf.trainable_variables() of a checkpoint dumped to .npz).
    Names may carry the `model/` scope and a `:0` suffix; kernels may be [1, 1, in, out] (tf.layers.conv2d) or [in, out].
    A missing, unknown, duplicated or mis-shaped variable raises ValueError naming it."""
    top, layer = shapes(config)
    w = {"layers": [dict() for _ in range(config.num_layers)]}
    for name, arr in variables.items():
        base = name[:-2] if name.endswith(":0") else name
        base = base[len("model/"):] if base.startswith("model/") else base
        m = re.match(r"layer_(\d+)/(.+)$", base)
        if m and m.group(2) in _KEY_OF_LAYER:
            j = int(m.group(1))
            if j >= config.num_layers:
                raise ValueError("variable %s belongs to layer %d, config has %d layers" % (name, j, config.num_layers))
            key, dst, want = _KEY_OF_LAYER[m.group(2)], w["layers"][j], layer[_KEY_OF_LAYER[m.group(2)]]
        elif base in _KEY_OF_TOP:
            key, dst, want = _KEY_OF_TOP[base], w, top[_KEY_OF_TOP[base]]
        else:
            raise ValueError("variable %s is not a variable of the attention model" % name)
        a = np.asarray(arr, np.float32)
        if a.ndim == 4 and len(want) == 2 and a.shape[:2] == (1, 1):
            a = a.reshape(a.shape[2:])
        if tuple(a.shape) != want:
            raise ValueError("variable %s has shape %s, config needs %s" % (name, tuple(np.shape(arr)), want))
        if key in dst:
            raise ValueError("two variables map to %s (second: %s)" % (base, name))
        dst[key] = a
    for k in TOP_KEYS:
        if k not in w:
            raise ValueError("missing variable model/%s" % _TF_TOP[k])
    for j, lay in enumerate(w["layers"]):
        for k in LAYER_KEYS:
            if k not in lay:
                raise ValueError("missing variable model/layer_%d/%s" % (j, _TF_LAYER[k]))
    return w


def to_tf_variables(config, w, prefix="model/", conv4d=True):
    """Inverse of from_tf_variables (round-trip tests, exporting back); conv4d: kernels as [1, 1, in, out]."""
    def k4(a):
        a = np.asarray(a, np.float32)
        return a.reshape((1, 1) + a.shape) if conv4d and a.ndim == 2 else a
    out = {prefix + _TF_TOP[k]: k4(w[k]) for k in TOP_KEYS}
    for j, lay in enumerate(w["layers"]):
        for k in LAYER_KEYS:
            out["%slayer_%d/%s" % (prefix, j, _TF_LAYER[k])] = k4(lay[k])
    return out
