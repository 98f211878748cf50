#!/usr/bin/env python3
"""A two-head stream manager against what the parent offers, on one device and in one process: 4096 and 16384 streams x 3600-sample
int16 chunks, the reference shape (n_mel 40, hidden 128, 2 layers, C = 6 and 8), fp32.
  (a) two_head   StreamManager(label2=...) on a heads handle: front-end + 2 layers + heads_window_kernel
  (b) plain      StreamManager without label2 on the same heads handle: head 1 only, three launches (the parent's path)
  (c) two_plain  both heads the parent's way: two plain managers on two handles, the second handle's single head is Wfc2
The figure is device time per chunk from HIP events around back-to-back feeds of one case; the cases are alternated inside every
round so that clock and cache state are shared; median of the rounds, spread alongside.  The managers keep their own state, so
every feed is a real iteration (windows fill and evict; the labels are ones the random weights do not spell).
usage: bench_heads_stream.py [--streams 4096,16384] [--reps 30] [--rounds 7] [--out profiles/heads_stream_bench.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from keyword_spotting_amd import get_config, weights
from keyword_spotting_amd.detector import StreamManager
from keyword_spotting_amd.frontend import MelFrontend
from keyword_spotting_amd.rnn_ctc import DeployModel

ap = argparse.ArgumentParser()
ap.add_argument("--streams", default="4096,16384")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()

cfg = get_config()
H, C2 = cfg.hidden_size, 8
w = weights.init_weights(cfg, seed=0)
rng = np.random.default_rng(1)
w["Wfc2"], w["bfc2"] = weights.extend_head(w["Wfc"], w["bfc"], rng.standard_normal((H, 2)).astype(np.float32), np.zeros(2, np.float32))
first = {k: v for k, v in w.items() if k not in ("Wfc2", "bfc2")}
second = dict(first, Wfc=w["Wfc2"], bfc=w["bfc2"])
cfg2 = get_config()
cfg2.num_classes2 = C2
cfg_second = get_config(label_dict={"w%d" % i: i for i in range(1, C2 - 2)})      # num_classes = C2: the second head as a model of its own
fe = MelFrontend(cfg)
m_heads, m_first, m_second = DeployModel(cfg2, w), DeployModel(cfg, first), DeployModel(cfg_second, second)


def timed(fn, reps):
    for _ in range(2):
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
for B in (int(s) for s in a.streams.split(",")):
    pcm = torch.from_numpy(rng.integers(-6000, 6000, (B, 3600)).astype(np.int16)).cuda()
    two = StreamManager(m_heads, B, label="1233", label2="1233")
    plain = StreamManager(m_heads, B, label="1233")
    p1, p2 = StreamManager(m_first, B, label="1233"), StreamManager(m_second, B, label="1233")
    cases = {"two_head": lambda: two.feed_pcm(pcm, fe), "plain": lambda: plain.feed_pcm(pcm, fe),
             "two_plain": lambda: (p1.feed_pcm(pcm, fe), p2.feed_pcm(pcm, fe))}
    names = {}
    t = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            t[k].append(timed(fn, a.reps))
            names[k] = (m_second if k == "two_plain" else m_heads).kernel_names()
    r = {k: float(np.median(v)) for k, v in t.items()}
    rows.append({"streams": B, "chunk_samples": 3600, "ms_two_head": r["two_head"], "ms_plain_head1_only": r["plain"], "ms_two_plain_managers": r["two_plain"],
                 "two_head_minus_plain": r["two_head"] - r["plain"], "two_plain_minus_two_head": r["two_plain"] - r["two_head"],
                 "spread_ms": {k: [min(v), max(v)] for k, v in t.items()}, "kernels": names})
    print("B=%d: two-head %.4f ms, plain (head 1 only) %.4f ms, two plain managers %.4f ms per chunk; (a)-(b) %+.4f, (c)-(a) %+.4f"
          % (B, r["two_head"], r["plain"], r["two_plain"], r["two_head"] - r["plain"], r["two_plain"] - r["two_head"]), flush=True)
    for m in (two, plain, p1, p2):
        m.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "rows": rows}, f, indent=1)
