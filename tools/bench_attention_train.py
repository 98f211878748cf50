#!/usr/bin/env python3
"""One training step of the self-attention CTC model (kws_attention_train_step: taped forward, CTC loss, backward, weight gradients,
Adam) against the same graph in torch eager float32 on the same GPU -- the ops of tests/attention_train_model.py's torch graph batched
over full-length utterances (then the per-utterance block layer norm is a mean over dims (1, 2)), F.dropout at the three sites,
F.ctc_loss, autograd and torch.optim.Adam (eager_logits; tests/test_attention_train_host.py holds it equal to that graph at
keep_prob 1).  The reference shape (H 128, 8 heads, Fi 512, L 3, c 2, n_mel 60, C 6), keep_prob 0.9,
(B, T) in {(16, 300), (16, 2000), (256, 300)}, label [1,2,3,3].
Device time from HIP events around whole steps after warm-up, ours and torch alternating within one process, median and spread of
the rounds.  torch draws its masks from its own generator and places Adam's epsilon differently: same cost, other bits.  No pass/fail
figure.
--ours-only: for a kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_attention_train.py --ours-only ...).
usage: bench_attention_train.py [--shapes 16x300,16x2000,256x300] [--rounds 5] [--steps 3] [--keep-prob 0.9] [--ours-only]
                                [--out profiles/attention_train_bench.json]"""
import argparse, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from keyword_spotting_amd import attention_weights
from keyword_spotting_amd.attention_training import AttentionTrainer
from keyword_spotting_amd.config import get_attention_config

LABEL = [1, 2, 3, 3]
LR = 1e-3


def timed(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def pe_table(rows, H, dev):
    p = np.arange(rows, dtype=np.float64)[:, None]
    i = np.arange(H // 2, dtype=np.float64)[None, :]
    ang = p / np.power(10000.0, 2.0 * i / H)
    pe = np.empty((rows, H))
    pe[:, 0::2], pe[:, 1::2] = np.sin(ang), np.cos(ang)
    return torch.tensor(pe, dtype=torch.float32, device=dev)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x300,16x2000,256x300")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="steps per timed call")
    ap.add_argument("--keep-prob", type=float, default=0.9)
    ap.add_argument("--ours-only", action="store_true")
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def eager_logits(cfg, tw, layers, x, pe, drop):
    """The restatement's torch graph (tests/attention_train_model.py, torch_forward) batched over B full-length utterances:
    x [B, T, F] -> (logits [B, T', C], T').  tests/test_attention_train_host.py holds the two graphs equal at drop 0."""
    H, heads, c = cfg.hidden_size, cfg.multi_head_num, cfg.combine_frame
    d = H // heads
    B, T = x.shape[:2]
    pad = c - T % c if c > 1 else 0
    t1 = (T + pad) // c

    def ln(u, gamma, beta):
        mu = u.mean(dim=(1, 2), keepdim=True)
        var = ((u - mu) ** 2).mean(dim=(1, 2), keepdim=True)
        return (u - mu) / torch.sqrt(var + 1e-12) * gamma + beta

    xs = F.pad(x, (0, 0, 0, pad)).reshape(B, t1, -1)
    h = xs @ tw["W_in"] + tw["b_in"] + pe[:t1]
    for lay in layers:
        qkv = h @ lay["W_qkv"] + lay["b_qkv"]
        q, k, v = (t.reshape(B, t1, heads, d).transpose(1, 2) for t in qkv.split(H, dim=2))
        p = F.dropout(torch.softmax(q @ k.transpose(2, 3) / math.sqrt(d), dim=-1), drop)
        att = (p @ v).transpose(1, 2).reshape(B, t1, H)
        y = ln(F.dropout(att, drop) + h, lay["ln_a_gamma"], lay["ln_a_beta"])
        z = torch.relu(y @ lay["W1"] + lay["b1"]) @ lay["W2"] + lay["b2"]
        h = ln(F.dropout(z, drop) + y, lay["ln_b_gamma"], lay["ln_b_beta"])
    logits = h @ tw["W_out"] + tw["b_out"]
    return (torch.relu(logits) if cfg.use_relu else logits), t1


def torch_step_fn(cfg, w, x, B, T, keep_prob):
    """The eager graph: returns a function that runs forward, loss, backward and one Adam step."""
    dev = x.device
    tw = {k: torch.tensor(w[k], device=dev, requires_grad=True) for k in attention_weights.TOP_KEYS}
    layers = [{k: torch.tensor(v, device=dev, requires_grad=True) for k, v in lay.items()} for lay in w["layers"]]
    params = list(tw.values()) + [v for lay in layers for v in lay.values()]
    opt = torch.optim.Adam(params, lr=LR)
    t1 = T // cfg.combine_frame + 1 if cfg.combine_frame > 1 else T
    pe = pe_table(t1, cfg.hidden_size, dev)
    targets = torch.tensor([LABEL] * B, dtype=torch.long, device=dev)
    in_len = torch.full((B,), t1, dtype=torch.long, device=dev)
    tg_len = torch.full((B,), len(LABEL), dtype=torch.long, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        logits, _ = eager_logits(cfg, tw, layers, x, pe, 1.0 - keep_prob)
        lp = F.log_softmax(logits, dim=-1).transpose(0, 1)
        loss = F.ctc_loss(lp, targets, in_len, tg_len, blank=cfg.num_classes - 1, reduction="none", zero_infinity=True)
        (loss.sum() / B).backward()
        opt.step()
    return step


def main():
    a = parse_args()
    rows = []
    cfg = get_attention_config()
    w = attention_weights.init(cfg, seed=0)
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(B + T)
        x = torch.randn(B, T, cfg.freq_size, device="cuda", generator=g)
        seq = np.full(B, T, np.int32)
        tr = AttentionTrainer(cfg, w, learning_rate=LR, keep_prob=a.keep_prob)
        seed = [0]

        def ours():
            seed[0] += 1
            tr.step_raw(x, seq, [LABEL] * B, LR, seed=seed[0])

        theirs = None if a.ours_only else torch_step_fn(cfg, w, x, B, T, a.keep_prob)
        ours()                                                   # warm-up: the tape is sized here
        if theirs:
            theirs()
        t_ours, t_torch = [], []
        for _ in range(a.rounds):
            t_ours.append(timed(ours, a.steps))
            if theirs:
                t_torch.append(timed(theirs, a.steps))
        st = tr.stats()
        tr.close()
        row = {"B": B, "T": T, "rows_per_utterance": tr.frames_out(T), "layers": cfg.num_layers, "hidden": cfg.hidden_size, "keep_prob": a.keep_prob,
               "ms_kws_attention_train_step": float(np.median(t_ours)), "spread_ms_kws_attention_train_step": [min(t_ours), max(t_ours)],
               "launches_per_step": st["launches"], "device_bytes": st["device_bytes"]}
        if theirs:
            row.update(ms_torch_eager=float(np.median(t_torch)), spread_ms_torch_eager=[min(t_torch), max(t_torch)],
                       torch_over_ours=float(np.median(t_torch)) / float(np.median(t_ours)))
        rows.append(row)
        print("B=%d T=%d: kws_attention_train_step %.3f ms [%.3f, %.3f], %d launches, %.1f MB%s"
              % (B, T, row["ms_kws_attention_train_step"], min(t_ours), max(t_ours), st["launches"], st["device_bytes"] / 2.0 ** 20,
                 "; torch eager %.2f ms [%.2f, %.2f] (x%.2f)" % (row["ms_torch_eager"], min(t_torch), max(t_torch), row["torch_over_ours"]) if theirs else ""))
        del theirs, x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps_per_timed_call": a.steps, "rounds": a.rounds, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
