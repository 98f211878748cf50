#!/usr/bin/env python3
"""MFCC front-end (kws_frontend_run_lengths on an MFCC handle: the coefficient kernel + the delta pass) against the magnitude-mel
launch of the same library and a torch-eager fp32 MFCC on the same GPU, at 4096 x 300-frame and 4096 x 22-frame utterances
(n_mel 60, n_mfcc 20: config/attention_config.py).  The library calls go straight to the C entry points with preallocated outputs
(no allocation, no Python wrapper per call); the figure is device time per call from HIP events around back-to-back calls on an
idle stream, so it still holds the gaps between launches.  Exclusive per-kernel times (and the split of the MFCC pair into its two
kernels) come from running this script under `rocprofv3 --kernel-trace --stats`.  The eager baseline allocates its temporaries
through torch's caching allocator, as an eager user would.
usage: bench_mfcc.py [--batch 4096] [--frames 300,22] [--reps 30] [--out file.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from keyword_spotting_amd import _lib
from keyword_spotting_amd.config import get_attention_config
from keyword_spotting_amd.frontend import MelFrontend, MfccFrontend

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--frames", default="300,22")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--out", default=None)
a = ap.parse_args()
cfg = get_attention_config(mfcc=True)
mfcc, mel = MfccFrontend(cfg), MelFrontend(cfg)
basis = torch.from_numpy(mel.mel_basis()).cuda().T.contiguous()
dct = torch.from_numpy(mfcc.dct_basis()).cuda()


def eager(pcm):
    """utils/mfcc.py in torch-eager fp32 (whole rows: no per-utterance lengths)"""
    fr = pcm.unfold(1, 400, 160)
    z = torch.fft.rfft(fr, 400, dim=-1)
    S = 10.0 * torch.log10(torch.clamp((z.real * z.real + z.imag * z.imag) @ basis, min=1e-10))
    c = S @ dct
    d = torch.cat([c[:, 1:], c[:, -1:]], 1) - torch.cat([c[:, :1], c[:, :-1]], 1)
    return torch.cat([c, d / 2, 0.3 * d], 2)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


rows = []
for T in (int(t) for t in a.frames.split(",")):
    n = 400 + 160 * (T - 1)
    pcm = torch.randn(a.batch, n, device="cuda") * 0.1
    lens = torch.randint(400, n + 1, (a.batch,), dtype=torch.int32, device="cuda")
    err = float((mfcc.forward(pcm) - eager(pcm)).abs().max())
    lib, st = _lib.load(), _lib.current_stream_ptr()
    out_c, out_m = torch.empty(a.batch, T, 3 * cfg.n_mfcc, device="cuda"), torch.empty(a.batch, T, cfg.n_mel, device="cuda")
    run_mfcc = lambda: lib.kws_frontend_run_lengths(mfcc._handle, _lib.ptr(pcm), None, a.batch, n, _lib.ptr(out_c), st)
    run_ragged = lambda: lib.kws_frontend_run_lengths(mfcc._handle, _lib.ptr(pcm), _lib.ptr(lens), a.batch, n, _lib.ptr(out_c), st)
    run_mel = lambda: lib.kws_frontend_run(mel._handle, _lib.ptr(pcm), a.batch, n, _lib.ptr(out_m), st)
    assert run_mfcc() == 0 and run_ragged() == 0 and run_mel() == 0
    # alternate the three so that clock and cache state are shared
    t = {"mfcc": [], "mfcc_ragged": [], "mel": [], "eager": []}
    for _ in range(3):
        t["mfcc"].append(timed(run_mfcc, a.reps))
        t["mfcc_ragged"].append(timed(run_ragged, a.reps))
        t["mel"].append(timed(run_mel, a.reps))
        t["eager"].append(timed(lambda: eager(pcm), max(2, a.reps // 10)))
    r = {k: float(np.median(v)) for k, v in t.items()}
    row = {"batch": a.batch, "frames": T, "ms_mfcc_pair": r["mfcc"], "ms_mfcc_pair_ragged_lengths": r["mfcc_ragged"], "ms_mel_power1": r["mel"],
           "ms_torch_eager_fp32": r["eager"], "mfcc_over_mel": r["mfcc"] / r["mel"], "eager_over_mfcc": r["eager"] / r["mfcc"],
           "mframes_per_s_mfcc": a.batch * T / r["mfcc"] / 1e3, "max_abs_diff_vs_eager": err, "spread_ms": {k: [min(v), max(v)] for k, v in t.items()}}
    rows.append(row)
    print("B=%d T=%d: MFCC pair %.4f ms (ragged lengths %.4f), mel %.4f ms, torch-eager fp32 %.3f ms; MFCC/mel %.2f, eager/MFCC %.1f; %.1f M frames/s; "
          "|kernel - eager| %.2e" % (a.batch, T, r["mfcc"], r["mfcc_ragged"], r["mel"], r["eager"], row["mfcc_over_mel"], row["eager_over_mfcc"],
                                      row["mframes_per_s_mfcc"], err))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
