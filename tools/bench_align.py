#!/usr/bin/env python3
"""CTC forced alignment (kws_ctc_align: one wave per utterance; Viterbi, backtrack, and for the loss and the posteriors alpha + beta, in one
launch) at B = 4096 utterances x T = 300 frames, C = 6, the keyword label 0 1 0 2 0 3 0 3 0 (S = 9), with kws_ctc_loss WITH its gradient
on the same inputs in the same process alongside: the sibling that runs alpha + beta.  Three forms of the call: everything (states, spans,
score, loss, post), the path alone (states, spans, score: no alpha, no beta), and the score alone.  Logits: N(0,1) plus 4.0 on one random
class that holds for 10 frames.  Device time from HIP events around one call, median of the rounds.  No pass/fail figure.
usage: bench_align.py [--batch 4096] [--frames 300] [--rounds 5] [--out profiles/align_bench.json]"""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from keyword_spotting_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
B, T, C, HOLD = a.batch, a.frames, 6, 10
LABEL = [0, 1, 0, 2, 0, 3, 0, 3, 0]
S = len(LABEL)
lib, st = _lib.load(), _lib.current_stream_ptr()


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


g = torch.Generator(device="cuda").manual_seed(C * 100 + S)
x = torch.randn(B, T, C, device="cuda", generator=g)
cls = torch.randint(0, C, (B, (T + HOLD - 1) // HOLD, 1), device="cuda", generator=g).repeat_interleave(HOLD, 1)[:, :T]
x.scatter_add_(2, cls, torch.full((B, T, 1), 4.0, device="cuda"))
states = torch.empty(B, T, dtype=torch.int32, device="cuda")
spans = torch.empty(B, S, 2, dtype=torch.int32, device="cuda")
score, loss, loss2 = torch.empty(B, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
post = torch.empty(B, T, S, device="cuda")
grad = torch.empty_like(x)
seq = np.full(B, T, np.int32)
lab = np.tile(np.array(LABEL, np.int32), (B, 1))
lab_len = np.full(B, S, np.int32)
host = [v.ctypes.data_as(ctypes.c_void_p) for v in (seq, lab, lab_len)]


def align(st_, sp_, lo_, po_):
    return lambda: _lib.check(lib.kws_ctc_align(_lib.ptr(x), host[0], host[1], host[2], B, T, C, S, _lib.ptr(st_), _lib.ptr(sp_), _lib.ptr(score),
                                                 _lib.ptr(lo_), _lib.ptr(po_), st))


def ctc():
    _lib.check(lib.kws_ctc_loss(_lib.ptr(x), host[0], host[1], host[2], B, T, C, S, _lib.ptr(loss2), _lib.ptr(grad), st))


forms = {"all": align(states, spans, loss, post), "path": align(states, spans, None, None), "score": align(None, None, None, None)}
times = {k: [] for k in list(forms) + ["ctc_loss_grad"]}
for _ in range(a.rounds):
    for k, fn in forms.items():
        times[k].append(timed(fn))
    times["ctc_loss_grad"].append(timed(ctc))
forms["all"]()
ctc()
torch.cuda.synchronize()
assert torch.equal(loss, loss2)
row = {"batch": B, "frames": T, "classes": C, "labels": S, "hold": HOLD,
       "ms_kws_ctc_align": float(np.median(times["all"])), "ms_kws_ctc_align_path_only": float(np.median(times["path"])),
       "ms_kws_ctc_align_score_only": float(np.median(times["score"])), "ms_kws_ctc_loss_with_gradient": float(np.median(times["ctc_loss_grad"])),
       "spread_ms": {k: [min(v), max(v)] for k, v in times.items()},
       "mean_score": float(score.mean()), "mean_loss": float(loss.mean()),
       "mean_span_frames": float((spans[:, :, 1] - spans[:, :, 0] + 1).float().mean())}
row["align_over_ctc_loss_with_gradient"] = row["ms_kws_ctc_align"] / row["ms_kws_ctc_loss_with_gradient"]
row["ns_per_utterance_frame"] = 1e6 * row["ms_kws_ctc_align"] / (B * T)
print("B=%d T=%d C=%d S=%d: align %.3f ms (path only %.3f, score only %.3f), ctc_loss with gradient %.3f ms (x%.2f); score %.2f, loss %.2f, "
      "%.1f frames per label" % (B, T, C, S, row["ms_kws_ctc_align"], row["ms_kws_ctc_align_path_only"], row["ms_kws_ctc_align_score_only"],
                                 row["ms_kws_ctc_loss_with_gradient"], row["align_over_ctc_loss_with_gradient"], row["mean_score"],
                                 row["mean_loss"], row["mean_span_frames"]))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": [row]}, f, indent=1)
