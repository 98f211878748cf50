#!/usr/bin/env python3
"""CTC prefix beam search (kws_ctc_beam_search: one wave per utterance, the whole frame loop in one launch) at the headline shape --
B = 4096 utterances x T = 300 frames, C = 6, beam_width = config.beam_size = 5, top_paths = 1 -- and at the widest beam the kernel
takes (W = 32, K = 32, C = 8), with kws_ctc_loss (loss only, the keyword label 0 1 0 2 0 3 0 3 0) at the same B, T, C alongside: the
yardstick of one wave walking T frames.  Logits: N(0,1) plus 4.0 on one random class that holds for `hold` frames -- 10: an utterance of
some thirty labels, the shape speech has; 1: a new class every frame, the paths run into L_max = 64 and every comparison is long.
Device time from HIP events around one call, median of the rounds.  No pass/fail figure.
usage: bench_beam.py [--batch 4096] [--frames 300] [--rounds 5] [--out profiles/beam_bench.json]"""
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
B, T = a.batch, a.frames
LABEL = [0, 1, 0, 2, 0, 3, 0, 3, 0]
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


rows = []
for C, W, K in ((6, 5, 1), (8, 32, 32)):
    for hold in (10, 1):
        g = torch.Generator(device="cuda").manual_seed(C * 100 + W)
        x = torch.randn(B, T, C, device="cuda", generator=g)
        cls = torch.randint(0, C, (B, (T + hold - 1) // hold, 1), device="cuda", generator=g).repeat_interleave(hold, 1)[:, :T]
        x.scatter_add_(2, cls, torch.full((B, T, 1), 4.0, device="cuda"))
        paths = torch.empty(B, K, 64, dtype=torch.int32, device="cuda")
        lens = torch.empty(B, K, dtype=torch.int32, device="cuda")
        lp = torch.empty(B, K, device="cuda")
        loss = torch.empty(B, device="cuda")
        seq = np.full(B, T, np.int32)
        lab = np.tile(np.array(LABEL, np.int32), (B, 1))
        lab_len = np.full(B, len(LABEL), np.int32)

        def beam():
            _lib.check(lib.kws_ctc_beam_search(_lib.ptr(x), None, B, T, C, W, K, 64, 1, _lib.ptr(paths), _lib.ptr(lens), _lib.ptr(lp), st))

        def ctc():
            _lib.check(lib.kws_ctc_loss(_lib.ptr(x), seq.ctypes.data_as(ctypes.c_void_p), lab.ctypes.data_as(ctypes.c_void_p),
                                        lab_len.ctypes.data_as(ctypes.c_void_p), B, T, C, len(LABEL), _lib.ptr(loss), None, st))

        t_beam, t_ctc = [], []
        for _ in range(a.rounds):
            t_beam.append(timed(beam))
            t_ctc.append(timed(ctc))
        row = {"batch": B, "frames": T, "classes": C, "beam_width": W, "top_paths": K, "hold": hold, "ms_kws_ctc_beam_search": float(np.median(t_beam)),
               "ms_kws_ctc_loss": float(np.median(t_ctc)), "spread_ms": {"beam": [min(t_beam), max(t_beam)], "ctc_loss": [min(t_ctc), max(t_ctc)]},
               "mean_top_path_length": float(lens[:, 0].float().mean()), "mean_top_log_prob": float(lp[:, 0].mean())}
        row["beam_over_ctc_loss"] = row["ms_kws_ctc_beam_search"] / row["ms_kws_ctc_loss"]
        row["ns_per_utterance_frame"] = 1e6 * row["ms_kws_ctc_beam_search"] / (B * T)
        rows.append(row)
        print("B=%d T=%d C=%d W=%d K=%d hold %d: beam search %.3f ms, ctc_loss %.3f ms (x%.1f); top path %.1f labels, log P %.2f"
              % (B, T, C, W, K, hold, row["ms_kws_ctc_beam_search"], row["ms_kws_ctc_loss"], row["beam_over_ctc_loss"],
                 row["mean_top_path_length"], row["mean_top_log_prob"]))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
