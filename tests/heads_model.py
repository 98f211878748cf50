"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of a customised-keyword deploy graph: the GRU stack of models/rnn_ctc.py:228-243
stepped with oracle.gru_oracle.gru_cell under dynamic_rnn's copy-through rule, the top layer's rows kept as
oracle.gru_oracle._forward keeps `top` (zero past seq_len), and TWO dense layers on those rows (the reference README's
"Customize keyword": [H, C1] and [H, C2], softmax and decode respectively), each followed by inference2's relu / clip.

The weights are the canonical dict plus Wfc2 [H, C2] / bfc2 [C2].
"""
import numpy as np

from oracle import decode_oracle as D
from oracle import gru_oracle as G


def random_heads_weights(n_mel, hidden, num_layers, c1, c2, seed, scale=1.0):
    """oracle.random_weights plus a second head drawn the same way (truncated normal at 2 sigma, bias 0.5 N(0,1)); `scale`
    multiplies both heads' matrices (larger: more peaked softmaxes, so that words are emitted)."""
    w = G.random_weights(n_mel, hidden, num_layers, c1, seed)
    rng = np.random.default_rng(seed + 7919)
    wfc2 = np.clip(rng.standard_normal((hidden, c2)), -2.0, 2.0)
    w["Wfc"] = (w["Wfc"] * scale).astype(np.float32)
    w["Wfc2"] = (wfc2 * scale).astype(np.float32)
    w["bfc2"] = (0.5 * rng.standard_normal(c2)).astype(np.float32)
    return w


def heads_forward(w, mel, state=None, seq_len=None, use_relu=False, value_clip=-1.0):
    """(mel [B,T,I], state [L,B,H]) -> dict(top [B,T,H], logits1, softmax1, logits2, softmax2, state [L,B,H]); float64."""
    dt = np.float64
    mel = np.asarray(mel, dt)
    b, t_len, _ = mel.shape
    nl, hdim = len(w["layers"]), w["Wfc"].shape[0]
    h = [np.zeros((b, hdim), dt) if state is None else np.array(state[l], dt) for l in range(nl)]
    seq_len = np.full(b, t_len, np.int64) if seq_len is None else np.asarray(seq_len)
    top = np.zeros((b, t_len, hdim), dt)
    for t in range(t_len):
        live = (t < seq_len)[:, None]
        x = mel[:, t, :]
        new_h = []
        for l in range(nl):
            x = G.gru_cell(x, h[l], w["layers"][l], dt)
            new_h.append(x)
        for l in range(nl):                   # dynamic_rnn copy-through: finished rows keep every layer's state
            h[l] = np.where(live, new_h[l], h[l])
        top[:, t, :] = np.where(live, new_h[-1], 0.0)          # ... and emit the zero row
    out = dict(top=top, state=np.stack(h))
    for i, (wk, bk) in enumerate((("Wfc", "bfc"), ("Wfc2", "bfc2")), 1):
        lg = top @ w[wk].astype(dt) + w[bk].astype(dt)
        if use_relu:                          # models/rnn_ctc.py:280-283, one function for both heads
            lg = np.maximum(lg, 0.0)
            if value_clip > 0:
                lg = np.clip(lg, 0.0, 20.0)
        out["logits%d" % i], out["softmax%d" % i] = lg, G.softmax(lg)
    return out


def frame_tokens(softmax, classnum, thres, prev_word=-1, length=None):
    """ctc_decode2's frame rule (utils/prediction.py:67,74-80) as per-frame events: softmax [T,C] -> (tokens [T] int8: 0 or the word
    1..C-2 emitted at frame t, the last frame's word).  Frames t >= length have no word."""
    w = D.frame_words(softmax, 1, classnum - 1, thres)
    if length is not None:
        w = np.where(np.arange(len(w)) < length, w, -1)
    prev = np.concatenate([[prev_word], w[:-1]]) if len(w) else w
    tok = np.where((w >= 0) & (w != prev), w + 1, 0).astype(np.int8)
    return tok, (int(w[-1]) if len(w) else prev_word)
