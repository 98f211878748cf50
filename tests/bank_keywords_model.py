"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of a bank whose slots carry keywords of their own (kws_bank_set_keyword): tests/bank_model.py
with a label and a width PER STREAM.  Slot u has (label_u or None, n_used_u); a stream on it has the C + n_used_u class head the user
enrolled:

    row = concat(l1[:C-1], new[:n_used], blank), activated and softmaxed over C + n_used, zero-padded to C + n_new

and its window 2 is decoded over those C + n_used classes against label_u.  A slot without a keyword (None, n_new) and a stream without a
slot are bank_model's: the manager's label2 over the full width / zero rows.  Not imported by the product.
"""
import numpy as np

import bank_model as BM
import heads_model as HM
from heads_stream_model import _margin_ok
from oracle import decode_oracle as D
from oracle import gru_oracle as G


def stream_keywords(keywords, users, n_new, label2):
    """keywords: per slot (label or None, n_used) -> per stream (label, n_used): the slot's own, or (label2, n_new)."""
    out = []
    for u in np.asarray(users):
        label, n_used = keywords[u] if 0 <= u < len(keywords) else (None, n_new)
        out.append((label2 if label is None else label, n_used))
    return out


def bank_forward(w, cols, bias, users, n_used, mel, state=None, seq_len=None, use_relu=False, value_clip=-1.0):
    """bank_model.bank_forward with n_used [B]: the width of each stream's head 2 (ignored where the stream has no slot)."""
    dt = np.float64
    one = dict(w, Wfc2=w["Wfc"], bfc2=w["bfc"])
    r = HM.heads_forward(one, mel, state, seq_len)
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
        k = int(n_used[b])
        new = top[b] @ cols[u][:, :k].astype(dt) + bias[u][:k].astype(dt)
        row = act(np.concatenate([l1[b][:, :c - 1], new, l1[b][:, c - 1:]], 1))
        l2[b, :, :c + k] = row
        sm2[b, :, :c + k] = G.softmax(row)
    l1 = act(l1)
    return dict(top=top, state=r["state"], logits1=l1, softmax1=G.softmax(l1), logits2=l2, softmax2=sm2)


def policy_loop(w, cols, bias, users, n_used, mel, chunks, speech, label1, labels2, thres, window_chunks=15):
    """bank_model.policy_loop with labels2 [B] and n_used [B]: window 2 of stream s is decoded over C + n_used[s] classes against
    labels2[s].  -> dict(mask [chunks, B] hit_1 | hit_2 << 1, margin_ok [chunks, B])."""
    b = mel.shape[0]
    users = np.asarray(users)
    capacity = cols.shape[0]
    c1 = w["Wfc"].shape[1]
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
        r = bank_forward(w, cols, bias, users, n_used, mel[:, pos:pos + n], state)
        state = r["state"]
        for s in range(b):
            hit = [0, 0]
            for k in range(2):
                classes = c1 if k == 0 else c1 + int(n_used[s])
                sm = r["softmax%d" % (k + 1)][s][:, :classes]
                if k == 0 or 0 <= users[s] < capacity:
                    margin[ci, s] &= _margin_ok(sm, classes, thres[k])
                queues[k][s].add(sm)
                label = label1 if k == 0 else labels2[s]
                hit[k] = int(bool(D.ctc_predict(D.ctc_decode2(np.concatenate(queues[k][s].get_all(), 0), classes, thres[k]), label)))
            mask[ci, s] = hit[0] | (hit[1] << 1)
            if mask[ci, s]:
                queues[0][s].clear()
                queues[1][s].clear()
                restart[s] = True
        pos += n
    return dict(mask=mask, margin_ok=margin)
