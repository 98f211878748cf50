#!/usr/bin/env python3
"""One training step of the GRU stack (kws_train_step: taped forward, CTC loss, BPTT, weight gradients, Adam) against the same graph in
torch eager float32 on the same GPU -- the ops of tests/train_model.py's torch_reference, F.ctc_loss, autograd and torch.optim.Adam.
L = 2, H = 128, n_mel in {40, 60}, C = 6, (B, T) in {(32, 300), (32, 2000), (1024, 300)}, full-length utterances, label [1,2,3,3] (four
states more would put T = 2000 past the CTC kernel's 160 KiB of LDS).
Device time from HIP events around one whole step after warm-up, ours and torch alternating within one process, median and spread
of the rounds.  torch's Adam places epsilon differently: same cost, other bits.  No pass/fail figure.
--ours-only: for a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_train.py --ours-only ...).
--wrapped: the stack with use_layer_norm and use_residual (kws_train_create_wrapped; random layer-norm tables), ours only: the eager
graph here is the plain cell's.
usage: bench_train.py [--shapes 32x300,32x2000,1024x300] [--mels 40,60] [--rounds 5] [--steps 3] [--ours-only] [--wrapped]
                      [--out profiles/train_bench.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from keyword_spotting_amd import get_config, weights
from keyword_spotting_amd.training import Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="32x300,32x2000,1024x300")
ap.add_argument("--mels", default="40,60")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=3, help="steps per timed call")
ap.add_argument("--ours-only", action="store_true")
ap.add_argument("--wrapped", action="store_true", help="layer norm + residual; implies --ours-only")
ap.add_argument("--out", default=None)
a = ap.parse_args()
LABEL = [1, 2, 3, 3]
LR = 1.5e-3


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


def torch_step_fn(cfg, w, x, B, T):
    """The eager graph: returns a function that runs forward, loss, backward and one Adam step."""
    dev = x.device
    params = []
    layers = []
    for lay in w["layers"]:
        t = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in lay.items()}
        layers.append(t)
        params += list(t.values())
    wfc, bfc = torch.tensor(w["Wfc"], device=dev, requires_grad=True), torch.tensor(w["bfc"], device=dev, requires_grad=True)
    params += [wfc, bfc]
    opt = torch.optim.Adam(params, lr=LR)
    targets = torch.tensor([LABEL] * B, dtype=torch.long, device=dev)
    in_len = torch.full((B,), T, dtype=torch.long, device=dev)
    tg_len = torch.full((B,), len(LABEL), dtype=torch.long, device=dev)
    hid = cfg.hidden_size

    def step():
        opt.zero_grad(set_to_none=True)
        inp = x
        for lay in layers:
            h = torch.zeros(B, hid, device=dev)
            ys = []
            for t in range(T):
                g = torch.sigmoid(torch.cat([inp[:, t], h], dim=1) @ lay["Wg"] + lay["bg"])
                r, u = g[:, :hid], g[:, hid:]
                c = torch.tanh(torch.cat([inp[:, t], r * h], dim=1) @ lay["Wc"] + lay["bc"])
                h = u * h + (1.0 - u) * c
                ys.append(h)
            inp = torch.stack(ys, dim=1)
        lp = F.log_softmax(inp @ wfc + bfc, dim=-1).transpose(0, 1)
        loss = F.ctc_loss(lp, targets, in_len, tg_len, blank=cfg.num_classes - 1, reduction="none", zero_infinity=True)
        (loss.sum() / B).backward()
        opt.step()
    return step


rows = []
for n_mel in (int(v) for v in a.mels.split(",")):
    cfg = get_config(n_mel=n_mel, use_layer_norm=a.wrapped, use_residual=a.wrapped)
    w = weights.init_weights(cfg, seed=0)
    if a.wrapped:          # TF's initial ibeta = 0 would feed the cells a constant
        rng = np.random.default_rng(0)
        for lay in w["layers"]:
            lay["ibeta"] = np.float32(rng.uniform(0.5, 2.0)).reshape(())
            lay["igamma"] = (0.5 * rng.standard_normal(lay["igamma"].shape)).astype(np.float32)
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(B + T)
        x = torch.randn(B, T, n_mel, device="cuda", generator=g)
        seq = np.full(B, T, np.int32)
        tr = Trainer(cfg, w, learning_rate=LR, lr_decay=1.0)
        ours = lambda: tr.step_raw(x, seq, [LABEL] * B, LR)      # noqa: E731
        theirs = None if a.ours_only or a.wrapped else torch_step_fn(cfg, w, x, B, T)
        ours()                                                   # warm-up: the tape is sized here
        if theirs:
            theirs()
        t_ours, t_torch = [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours))
            if theirs:
                t_torch.append(timed(theirs))
        st = tr.stats()
        tr.close()
        row = {"wrapped": bool(a.wrapped), "n_mel": n_mel, "B": B, "T": T, "layers": cfg.num_layers, "hidden": cfg.hidden_size, "ms_kws_train_step": float(np.median(t_ours)),
               "spread_ms_kws_train_step": [min(t_ours), max(t_ours)], "launches_per_step": st["launches"], "device_bytes": st["device_bytes"],
               "frame_loop_workgroups": (B + 15) // 16}
        if theirs:
            row.update(ms_torch_eager=float(np.median(t_torch)), spread_ms_torch_eager=[min(t_torch), max(t_torch)],
                       torch_over_ours=float(np.median(t_torch)) / float(np.median(t_ours)))
        rows.append(row)
        print("%sn_mel=%d B=%d T=%d: kws_train_step %.3f ms [%.3f, %.3f], %d launches, %.1f MB%s"
              % ("layer norm + residual, " if a.wrapped else "", n_mel, B, T, row["ms_kws_train_step"], min(t_ours), max(t_ours), st["launches"], st["device_bytes"] / 2.0 ** 20,
                 "; torch eager %.1f ms [%.1f, %.1f] (x%.1f)" % (row["ms_torch_eager"], min(t_torch), max(t_torch), row["torch_over_ours"]) if theirs else ""))
        del theirs, x
        torch.cuda.empty_cache()
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "steps_per_timed_call": a.steps, "rounds": a.rounds, "rows": rows}, f, indent=1)
