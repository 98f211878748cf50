#!/usr/bin/env python3
"""Front-end alone: B streams x one 3600+240-sample chunk -> mel; prints ms per call (HIP events).
usage: bench_fe.py [B] [samples] [buffers] [--lengths | --dataset [--pre C]]
buffers > 1 rotates the input over that many PCM buffers: the same buffer again and again is served by the 256 MB Infinity Cache, a
streaming loop's fresh chunk comes from HBM.
--lengths   the whole-utterance mel launch instead (kws_frontend_run_lengths on a magnitude-mel handle: Utterances<float, 0>)
--dataset   the dataset's framing of it (kws_frontend_create_dataset: centred, reflected, Hann-windowed frames), --pre C with
            pre-emphasis C (0: none)"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from keyword_spotting_amd import get_config
from keyword_spotting_amd.frontend import DatasetFrontend, MelFrontend
ap = argparse.ArgumentParser()
ap.add_argument("B", type=int, nargs="?", default=4096)
ap.add_argument("N", type=int, nargs="?", default=3840)
ap.add_argument("NB", type=int, nargs="?", default=1)
ap.add_argument("--lengths", action="store_true")
ap.add_argument("--dataset", action="store_true")
ap.add_argument("--pre", type=float, default=0.0)
a = ap.parse_args()
B, N, NB = a.B, a.N, a.NB
if a.dataset:
    fe, what = DatasetFrontend(get_config(), pre_emphasis=a.pre), "dataset front-end (pre-emphasis %g)" % a.pre
    run = fe.forward
elif a.lengths:
    fe, what = MelFrontend(get_config()), "whole-utterance front-end"
    run = lambda x: fe._run_lengths(x, None, fe.config.n_mel)
else:
    fe, what = MelFrontend(get_config()), "front-end"
    run = fe.forward
pcms = [torch.randn(B, N, device="cuda") * 0.1 for _ in range(NB)]
for i in range(5): mel = run(pcms[i % NB])
torch.cuda.synchronize()
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for i in range(50): mel = run(pcms[i % NB])
b.record(); torch.cuda.synchronize()
ms = a.elapsed_time(b) / 50
print("%s B=%d samples=%d buffers=%d -> T=%d: %.4f ms per call, %.1f M frames/s" % (what, B, N, NB, mel.shape[1], ms, B * mel.shape[1] / ms / 1e3))
