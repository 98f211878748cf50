"""Writes tests/golden/heads_golden.npz: hand-built 8-class softmaxes of a customised-keyword model's second head (columns: space,
three words, garbage, two new words, ctc blank) for tests/test_heads_host.py.  Each case spells the words 1, 2, 3, 3 as peaks of
probability 0.9, `gap` frames apart, over a blank background: server_demo.py passes the head's class count (8) where ctc_decode
takes its lockout, so peaks closer than 8 frames are swallowed.

    python tests/golden/make_heads_golden.py
"""
import os

import numpy as np


def spell(words, gap, lead=2, classes=8):
    t = lead + gap * len(words) + 2
    sm = np.full((t, classes), 0.02 / (classes - 1), np.float32)
    sm[:, classes - 1] = 0.98
    for k, w in enumerate(words):
        row = np.full(classes, 0.1 / (classes - 1), np.float32)
        row[w] = 0.9
        sm[lead + gap * k] = row
    return (sm / sm.sum(1, keepdims=True)).astype(np.float32)


out = {"h0_softmax": spell([1, 2, 3, 3], 9), "h1_softmax": spell([1, 2, 3, 3], 4), "h2_softmax": spell([1, 3, 2, 3], 9),
       "h3_softmax": spell([1, 2, 3, 3], 12, lead=5)}
np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "heads_golden.npz"), **out)
