#!/usr/bin/env python3
"""The enrolment fit on frame-wise targets (kws_enroll_fit_frames) next to the plain fit (kws_enroll_fit) at one shape: E = 64 enrolments
x K = 3 utterances x T = 300 frames x 300 steps, hidden 128, C = 6 trained classes + 2 new ones, label [0,5,0,6,0], random nn_outputs /
logits1 and random frame-wise targets with runs of -1.  Three fits per round, alternating -- kws_enroll_fit, kws_enroll_fit_frames with
the frame loss alone (ctc_weight 0) and mixed 1 / 1 --, device time from HIP events around one whole fit (kws_enroll_set included),
median (min, max) of the rounds.  No pass/fail figure.
usage: bench_enroll_frames.py [--enrolments 64] [--slots 3] [--frames 300] [--steps 300] [--rounds 5] [--out profiles/enroll_frames_bench.json]"""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from keyword_spotting_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--enrolments", type=int, default=64)
ap.add_argument("--slots", type=int, default=3)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--lr", type=float, default=0.03)
ap.add_argument("--out", default=None)
a = ap.parse_args()
H, C, N, E, K, T = 128, 6, 2, a.enrolments, a.slots, a.frames
LABEL = [0, 5, 0, 6, 0]
lib, st = _lib.load(), _lib.current_stream_ptr()
B = E * K
g = torch.Generator(device="cuda").manual_seed(E)
nn = torch.randn(B, T, H, device="cuda", generator=g) * 0.5
logits1 = torch.randn(B, T, C, device="cuda", generator=g) * 2
w0 = torch.randn(E, H, N, device="cuda", generator=g).clamp(-2, 2)
b0 = torch.zeros(E, N, device="cuda")
rng = np.random.default_rng(E)
tg = rng.integers(0, C + N, size=(B, T)).astype(np.int32)
for b in range(B):          # runs of -1, two to four frames long, over about a third of the frames
    for t in rng.integers(0, T, size=T // 9):
        tg[b, t:t + int(rng.integers(2, 5))] = -1
targets = torch.from_numpy(tg).cuda()
seq = np.full(B, T, np.int32)
lab = np.tile(np.array(LABEL, np.int32), (B, 1))
lab_len = np.full(B, len(LABEL), np.int32)
trace = torch.empty(a.steps, B, device="cuda")
h = ctypes.c_void_p()
_lib.check(lib.kws_enroll_create(H, C, N, E, K, ctypes.byref(h)))
ptrs = (_lib.ptr(nn), _lib.ptr(logits1), seq.ctypes.data_as(ctypes.c_void_p), lab.ctypes.data_as(ctypes.c_void_p), lab_len.ctypes.data_as(ctypes.c_void_p))


def fit(ft):
    def run():
        _lib.check(lib.kws_enroll_set(h, _lib.ptr(w0), _lib.ptr(b0), st))
        if ft is None:
            _lib.check(lib.kws_enroll_fit(h, *ptrs, T, len(LABEL), a.lr, a.steps, _lib.ptr(trace), st))
        else:
            _lib.check(lib.kws_enroll_fit_frames(h, *ptrs, T, len(LABEL), ctypes.byref(ft), a.lr, a.steps, _lib.ptr(trace), st))
    return run


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


runs = {"kws_enroll_fit": fit(None),
        "kws_enroll_fit_frames ctc_weight 0": fit(_lib.KwsFrameTargets(targets.data_ptr(), None, 0.0, 1.0, None)),
        "kws_enroll_fit_frames 1 / 1": fit(_lib.KwsFrameTargets(targets.data_ptr(), None, 1.0, 1.0, None))}
times, first_last = {k: [] for k in runs}, {}
for fn in runs.values():          # warm-up: the first call at a shape allocates the upload block and grants the LDS
    fn()
torch.cuda.synchronize()
for _ in range(a.rounds):
    for name, fn in runs.items():
        times[name].append(timed(fn))
        first_last[name] = [float(trace[0].sum()), float(trace[-1].sum())]
lib.kws_enroll_destroy(h)
rows = []
for name, t in times.items():
    rows.append({"fit": name, "ms_median": float(np.median(t)), "ms_min": min(t), "ms_max": max(t), "loss_sum_first_last": first_last[name]})
    print("E=%d K=%d T=%d x %d steps  %-36s %.3f ms (%.3f, %.3f); loss %.1f -> %.1f"
          % (E, K, T, a.steps, name, rows[-1]["ms_median"], min(t), max(t), first_last[name][0], first_last[name][1]))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "hidden": H, "classes": C, "new_classes": N, "enrolments": E, "slots": K, "frames": T,
                   "steps": a.steps, "rounds": a.rounds, "rows": rows}, f, indent=1)
