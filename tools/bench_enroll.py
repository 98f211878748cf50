#!/usr/bin/env python3
"""Enrolment fit (kws_enroll_fit: every optimiser step of E enrolments inside one launch) against the same fit written with
torch.nn.functional.ctc_loss, autograd and torch.optim.Adam on the same GPU, the E enrolments batched with bmm.  E in {1, 256, 4096}
enrolments x K = 3 utterances x T = 100 frames x 100 steps, hidden 128, C = 6 trained classes + 2 new ones, label [0,5,0,6,0];
random nn_outputs / logits1 (the stack run that produces them is the same for both and is not timed).  Device time from HIP events
around one whole fit, median of the rounds.  torch's Adam places epsilon differently (tests/enroll_model.py): same cost, other bits.
No pass/fail figure.
usage: bench_enroll.py [--enrolments 1,256,4096] [--slots 3] [--frames 100] [--steps 100] [--rounds 5] [--out profiles/enroll_bench.json]"""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from keyword_spotting_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--enrolments", default="1,256,4096")
ap.add_argument("--slots", type=int, default=3)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--lr", type=float, default=0.03)
ap.add_argument("--out", default=None)
a = ap.parse_args()
H, C, N, K, T = 128, 6, 2, a.slots, a.frames
LABEL = [0, 5, 0, 6, 0]
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
for E in (int(e) for e in a.enrolments.split(",")):
    B = E * K
    g = torch.Generator(device="cuda").manual_seed(E)
    nn = torch.randn(B, T, H, device="cuda", generator=g) * 0.5
    logits1 = torch.randn(B, T, C, device="cuda", generator=g) * 2
    w0 = torch.randn(E, H, N, device="cuda", generator=g).clamp(-2, 2)
    b0 = torch.zeros(E, N, device="cuda")
    seq = np.full(B, T, np.int32)
    lab = np.tile(np.array(LABEL, np.int32), (B, 1))
    lab_len = np.full(B, len(LABEL), np.int32)
    trace = torch.empty(a.steps, B, device="cuda")
    h = ctypes.c_void_p()
    _lib.check(lib.kws_enroll_create(H, C, N, E, K, ctypes.byref(h)))

    def ours():
        _lib.check(lib.kws_enroll_set(h, _lib.ptr(w0), _lib.ptr(b0), st))
        _lib.check(lib.kws_enroll_fit(h, _lib.ptr(nn), _lib.ptr(logits1), seq.ctypes.data_as(ctypes.c_void_p), lab.ctypes.data_as(ctypes.c_void_p),
                                      lab_len.ctypes.data_as(ctypes.c_void_p), T, len(LABEL), a.lr, a.steps, _lib.ptr(trace), st))

    targets = torch.from_numpy(lab.astype(np.int64)).cuda()
    in_len, tg_len = torch.full((B,), T, dtype=torch.long, device="cuda"), torch.full((B,), len(LABEL), dtype=torch.long, device="cuda")
    torch_trace = torch.empty(a.steps, B, device="cuda")

    def theirs():
        w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        opt = torch.optim.Adam([w, b], lr=a.lr)
        for s in range(a.steps):
            opt.zero_grad(set_to_none=True)
            z = (torch.bmm(nn.view(E, K * T, H), w) + b[:, None, :]).view(B, T, N)
            lp = F.log_softmax(torch.cat([logits1[..., :-1], z, logits1[..., -1:]], dim=-1), dim=-1)
            loss = F.ctc_loss(lp.transpose(0, 1), targets, in_len, tg_len, blank=C + N - 1, reduction="none", zero_infinity=True)
            torch_trace[s] = loss.detach()
            (loss.sum() / K).backward()
            opt.step()

    t_ours, t_torch = [], []
    for _ in range(a.rounds):
        t_ours.append(timed(ours))
        t_torch.append(timed(theirs))
    lib.kws_enroll_destroy(h)
    row = {"enrolments": E, "slots": K, "frames": T, "steps": a.steps, "ms_kws_enroll_fit": float(np.median(t_ours)),
           "ms_torch_ctc_autograd_adam": float(np.median(t_torch)), "spread_ms": {"kws_enroll_fit": [min(t_ours), max(t_ours)],
                                                                                   "torch": [min(t_torch), max(t_torch)]},
           "first_step_loss_max_abs_diff": float((trace[0] - torch_trace[0]).abs().max()),
           "loss_sum_first_last": [float(trace[0].sum()), float(trace[-1].sum())]}
    row["torch_over_ours"] = row["ms_torch_ctc_autograd_adam"] / row["ms_kws_enroll_fit"]
    rows.append(row)
    print("E=%d K=%d T=%d x %d steps: kws_enroll_fit %.3f ms, torch ctc_loss + autograd + Adam %.3f ms (x%.1f); loss %.1f -> %.1f"
          % (E, K, T, a.steps, row["ms_kws_enroll_fit"], row["ms_torch_ctc_autograd_adam"], row["torch_over_ours"],
             row["loss_sum_first_last"][0], row["loss_sum_first_last"][1]))
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "hidden": H, "classes": C, "new_classes": N, "rows": rows}, f, indent=1)
