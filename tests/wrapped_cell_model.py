"""fp64 numpy restatement of the reference's wrapped cell stack: MultiRNNCell of ResidualWrapper(LayerNormalizer(GRUCell))
under dynamic_rnn -- the model get_cell builds with config.use_layer_norm / config.use_residual (models/rnn_ctc.py:179-199).

  LayerNormalizer.__call__ (utils/custom_wrapper.py:145-158): the cell's input x [B, I_l] is replaced by
      _ln(x, ibeta, igamma) = (x - m) / sqrt(v + 1e-5) * ibeta + igamma          (:126-130)
  with m, v = tf.nn.moments(x, [1]) (the mean, then the population variance around it).  _ln's signature is (input, s, b):
  ibeta (shape [], initialised to 0) is the scale and igamma (shape [I_l], initialised to 1) the shift.
  ResidualWrapper.__call__ (:112-116): output = 0.7071067811865475 * (cell output + inputs), inputs being what the wrapper
  received, i.e. x BEFORE the layer norm; the new state is the cell's.  get_cell applies it for layer > 0 only (:196-197).
  dynamic_rnn: for t >= seq_len[b] every layer keeps its state and the emitted (top) row is zero -- logits = bfc.

The inner cell is oracle.gru_oracle.gru_cell (the TF-1.x GRUCell restatement the plain path is tested against)."""
import numpy as np

from oracle.gru_oracle import gru_cell

RESIDUAL_SCALE = 0.7071067811865475       # utils/custom_wrapper.py:116
LN_EPSILON = 1e-5                         # utils/custom_wrapper.py:126


def layer_norm(x, ibeta, igamma, eps=LN_EPSILON):
    """LayerNormalizer._ln(x, s=ibeta, b=igamma) over the feature axis of x [B, I]."""
    m = x.mean(axis=1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=1, keepdims=True)
    return (x - m) / np.sqrt(v + eps) * np.float64(ibeta) + np.asarray(igamma, np.float64)


def wrapped_cell(x, h, lay, layer, use_layer_norm, use_residual):
    """One step of layer `layer`: (output, new state)."""
    xin = layer_norm(x, lay["ibeta"], lay["igamma"]) if use_layer_norm else x
    hn = gru_cell(xin, h, lay, np.float64)
    out = RESIDUAL_SCALE * (hn + x) if use_residual and layer > 0 else hn
    return out, hn


def wrapped_forward(w, mel, use_layer_norm, use_residual, state=None, seq_len=None, use_relu=False, value_clip=-1.0):
    """(mel [B,T,I], state [L,B,H]) -> (logits [B,T,C], state' [L,B,H]), float64."""
    mel = np.asarray(mel, np.float64)
    b, t_len, _ = mel.shape
    nl = len(w["layers"])
    hdim = w["Wfc"].shape[0]
    h = [np.zeros((b, hdim)) if state is None else np.array(state[l], np.float64) for l in range(nl)]
    seq_len = np.full(b, t_len) if seq_len is None else np.asarray(seq_len)
    top = np.zeros((b, t_len, hdim))
    for t in range(t_len):
        live = (t < seq_len)[:, None]
        x = mel[:, t, :]
        new_h = []
        for l in range(nl):
            x, hn = wrapped_cell(x, h[l], w["layers"][l], l, use_layer_norm, use_residual)
            new_h.append(hn)
        for l in range(nl):
            h[l] = np.where(live, new_h[l], h[l])
        top[:, t, :] = np.where(live, x, 0.0)
    logits = (top.reshape(-1, hdim) @ w["Wfc"].astype(np.float64) + w["bfc"].astype(np.float64)).reshape(b, t_len, -1)
    if use_relu:
        logits = np.maximum(logits, 0.0)
        if value_clip > 0:
            logits = np.clip(logits, 0.0, 20.0)
    return logits, np.stack(h)


def random_ln(w, n_mel, seed):
    """Random layer-norm tables for a weights dict (in place): ibeta from +-[0.5, 2], igamma ~ N(0, 0.5).  With the TF initial
    values (ibeta = 0) the normalised input is igamma whatever x is, and a wrong mean or variance would go unseen."""
    rng = np.random.default_rng(seed)
    hdim = w["Wfc"].shape[0]
    for l, lay in enumerate(w["layers"]):
        i_l = n_mel if l == 0 else hdim
        lay["ibeta"] = np.float32(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)).reshape(())
        lay["igamma"] = (0.5 * rng.standard_normal(i_l)).astype(np.float32)
    return w
