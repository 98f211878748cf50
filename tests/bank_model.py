"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of a bank of enrolled heads (kws_bank): tests/heads_model.heads_forward's stack and
head 1, with head 2 spliced PER STREAM from the columns of that stream's bank slot (weights.extend_head's order: head 1's classes
0..C-2, the slot's n_new new classes, head 1's blank), and tests/heads_stream_model.policy_loop's two-head policy over it.

A stream whose user lies outside [0, capacity) has no second head: zero logits2 / softmax2 rows, which decode to nothing.
Not imported by the product.
"""
import numpy as np

import heads_model as HM
from heads_stream_model import _margin_ok
from oracle import decode_oracle as D
from oracle import gru_oracle as G


def random_bank(hidden, n_new, capacity, seed, scale=1.0):
    """`capacity` slots drawn as heads_model.random_heads_weights draws head 2: columns truncated normal at 2 sigma (times `scale`),
    bias 0.5 N(0,1).  -> (columns [capacity,H,n_new], bias [capacity,n_new]) float32."""
    rng = np.random.default_rng(seed + 104729)
    cols = np.clip(rng.standard_normal((capacity, hidden, n_new)), -2.0, 2.0) * scale
    return cols.astype(np.float32), (0.5 * rng.standard_normal((capacity, n_new))).astype(np.float32)


def bank_forward(w, cols, bias, users, mel, state=None, seq_len=None, use_relu=False, value_clip=-1.0):
    """(one-head weights w, bank, users [B]) -> heads_forward's dict; logits2 / softmax2 [B,T,C + n_new], zeros where the stream has
    no slot.  float64."""
    dt = np.float64
    one = dict(w, Wfc2=w["Wfc"], bfc2=w["bfc"])              # (head 2 of heads_forward is not used)
    r = HM.heads_forward(one, mel, state, seq_len)           # raw logits: relu / clip are applied below, to both heads alike
    users = np.asarray(users)
    capacity, _, n_new = cols.shape
    c = w["Wfc"].shape[1]
    top, l1 = r["top"], r["logits1"]
    l2 = np.zeros(l1.shape[:2] + (c + n_new,), dt)
    sm2 = np.zeros_like(l2)

    def act(lg):
        if use_relu:
            lg = np.maximum(lg, 0.0)
            if value_clip > 0:
                lg = np.clip(lg, 0.0, 20.0)
        return lg
    for b, u in enumerate(users):
        if not 0 <= u < capacity:
            continue
        new = top[b] @ cols[u].astype(dt) + bias[u].astype(dt)
        l2[b] = act(np.concatenate([l1[b][:, :c - 1], new, l1[b][:, c - 1:]], 1))
        sm2[b] = G.softmax(l2[b])
    l1 = act(l1)
    return dict(top=top, state=r["state"], logits1=l1, softmax1=G.softmax(l1), logits2=l2, softmax2=sm2)


def policy_loop(w, cols, bias, users, mel, chunks, speech, labels, thres, window_chunks=15):
    """heads_stream_model.policy_loop over bank_forward: silence clears both queues and resets the state, head k's rows go into queue
    k, each window is decoded at its own threshold against its own label, fired = hit_1 | hit_2 clears both and restarts.
    -> dict(mask [chunks, B] hit_1 | hit_2 << 1, margin_ok [chunks, B])."""
    b = mel.shape[0]
    users = np.asarray(users)
    capacity, _, n_new = cols.shape
    c = (w["Wfc"].shape[1], w["Wfc"].shape[1] + n_new)
    nl, hdim = len(w["layers"]), w["Wfc"].shape[0]
    state = np.zeros((nl, b, hdim), np.float64)
    queues = [[D.SimpleQueue(window_chunks) for _ in range(b)] for _ in range(2)]
    mask = np.zeros((len(chunks), b), np.int32)
    margin = np.ones((len(chunks), b), bool)
    restart = np.zeros(b, bool)
    pos = 0
    for ci, n in enumerate(chunks):
        silent = ~np.asarray(speech[ci], bool)
        state[:, silent | restart] = 0
        restart[:] = False
        for s in np.nonzero(silent)[0]:
            queues[0][s].clear()
            queues[1][s].clear()
        r = bank_forward(w, cols, bias, users, mel[:, pos:pos + n], state)
        state = r["state"]
        for s in range(b):
            hit = [0, 0]
            for k in range(2):
                sm = r["softmax%d" % (k + 1)][s]
                if k == 0 or 0 <= users[s] < capacity:
                    margin[ci, s] &= _margin_ok(sm, c[k], thres[k])
                queues[k][s].add(sm)
                hit[k] = int(bool(D.ctc_predict(D.ctc_decode2(np.concatenate(queues[k][s].get_all(), 0), c[k], thres[k]), labels[k])))
            mask[ci, s] = hit[0] | (hit[1] << 1)
            if mask[ci, s]:
                queues[0][s].clear()
                queues[1][s].clear()
                restart[s] = True
        pos += n
    return dict(mask=mask, margin_ok=margin)
