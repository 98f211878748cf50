#!/usr/bin/env python3
"""The heads step (kws_step_heads: every layer through a seam, then dense_heads_kernel) against the plain step (kws_step: head 1 fused
into the last layer's launch) on ONE heads handle, at 4096 x 300 and 4096 x 22 frames, fp32, the reference shape (n_mel 40, hidden
128, 2 layers, C = 6 and 8).  The C entry points are called directly on preallocated outputs; the figure is device time per call
from HIP events around back-to-back calls, the variants alternated so that clock and cache state are shared, median of the rounds.
  (a) --parent-lib <libkws_amd.so of the parent commit>: kws_step of that library on a plain handle against kws_step of this one on
      the heads handle, alternated in the same process -- the same kernels, so a difference is host-side.
  (b) kws_step_heads - kws_step, and the heads launch alone as (full heads step) - (the same step with no head and no nn_outputs
      wanted: the stack with its seams and nothing behind it), with the bytes it moves per second: per stream and frame 4H in,
      4H out (nn_outputs), 8 C_i + 1 per head (logits, softmax, token).
usage: bench_heads.py [--batch 4096] [--frames 300,22] [--reps 20] [--rounds 5] [--parent-lib path] [--out file.json]"""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from keyword_spotting_amd import _lib, get_config, weights
from keyword_spotting_amd.rnn_ctc import DeployModel

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--frames", default="300,22")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()

cfg = get_config()
H, L, C1, C2 = cfg.hidden_size, cfg.num_layers, cfg.num_classes, 8
w = weights.init_weights(cfg, seed=0)
rng = np.random.default_rng(1)
w["Wfc2"], w["bfc2"] = weights.extend_head(w["Wfc"], w["bfc"], rng.standard_normal((H, 2)).astype(np.float32), np.zeros(2, np.float32))
plain_blob = weights.to_blob(cfg, {k: v for k, v in w.items() if k not in ("Wfc2", "bfc2")})
cfg.num_classes2 = C2
model = DeployModel(cfg, w)
lib, st = _lib.load(), _lib.current_stream_ptr()

parent, parent_handle = None, ctypes.c_void_p()
if a.parent_lib:
    parent = ctypes.CDLL(a.parent_lib)
    parent.kws_create.argtypes = [ctypes.POINTER(_lib.KwsConfig), ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    parent.kws_step.argtypes = lib.kws_step.argtypes
    parent.kws_destroy.argtypes = [ctypes.c_void_p]
    assert parent.kws_create(ctypes.byref(model._cfg), plain_blob.ctypes.data_as(ctypes.c_void_p), plain_blob.nbytes, ctypes.byref(parent_handle)) == 0


def timed(fn, reps):
    for _ in range(2):
        assert fn() == 0
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
    B = a.batch
    model.reserve(B, T)
    mel = torch.rand(B, T, cfg.n_mel, device="cuda") * 2
    s_in, s_out = torch.zeros(L, B, H, device="cuda"), torch.empty(L, B, H, device="cuda")
    lg = [torch.empty(B, T, c, device="cuda") for c in (C1, C2)]
    sm = [torch.empty(B, T, c, device="cuda") for c in (C1, C2)]
    tok = [torch.empty(B, T, dtype=torch.int8, device="cuda") for _ in range(2)]
    pw = [torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    nn = torch.empty(B, T, H, device="cuda")
    io = [_lib.KwsHeadIo(lg[i].data_ptr(), sm[i].data_ptr(), tok[i].data_ptr(), pw[i].data_ptr(), 0.4) for i in range(2)]
    step_args = (_lib.ptr(mel), _lib.ptr(s_in), _lib.ptr(lg[0]), _lib.ptr(sm[0]), _lib.ptr(s_out), None, None, _lib.ptr(tok[0]), _lib.ptr(pw[0]), 0.4, B, T, st)
    runs = {
        "step": lambda: lib.kws_step(model._handle, *step_args),
        "heads": lambda: lib.kws_step_heads(model._handle, _lib.ptr(mel), _lib.ptr(s_in), _lib.ptr(s_out), None, None, _lib.ptr(nn),
                                            ctypes.byref(io[0]), ctypes.byref(io[1]), B, T, st),
        "stack_only": lambda: lib.kws_step_heads(model._handle, _lib.ptr(mel), _lib.ptr(s_in), _lib.ptr(s_out), None, None, None, None, None, B, T, st),
    }
    if parent:
        runs["parent_step"] = lambda: parent.kws_step(parent_handle, *step_args)
    t = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(timed(fn, a.reps))
    r = {k: float(np.median(v)) for k, v in t.items()}
    heads_ms = r["heads"] - r["stack_only"]
    nbytes = B * T * (4 * H + 4 * H + (8 * C1 + 1) + (8 * C2 + 1))
    row = {"batch": B, "frames": T, "ms_kws_step": r["step"], "ms_kws_step_heads": r["heads"], "ms_heads_step_without_heads_launch": r["stack_only"],
           "ms_heads_minus_step": r["heads"] - r["step"], "ms_heads_launch": heads_ms, "heads_launch_bytes": nbytes,
           "heads_launch_TB_per_s": nbytes / heads_ms / 1e9, "spread_ms": {k: [min(v), max(v)] for k, v in t.items()}, "kernels": model.kernel_names()}
    if parent:
        row.update(ms_parent_kws_step=r["parent_step"], step_over_parent_step=r["step"] / r["parent_step"])
    rows.append(row)
    print("B=%d T=%d: kws_step %.4f ms%s, kws_step_heads %.4f ms (+%.4f), heads launch %.4f ms = %.2f TB/s over %.0f MB"
          % (B, T, r["step"], (" (parent %.4f)" % r["parent_step"]) if parent else "", r["heads"], row["ms_heads_minus_step"], heads_ms,
             row["heads_launch_TB_per_s"], nbytes / 1e6))
if parent:
    parent.kws_destroy(parent_handle)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
