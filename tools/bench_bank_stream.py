#!/usr/bin/env python3
"""A bank stream manager (every stream its own enrolled keyword) against the two-head manager (one keyword shared by all), on one
device and in one process: 4096 and 16384 streams x 3600-sample int16 chunks, the reference shape (n_mel 40, hidden 128, 2 layers),
C = min(6, 8 - n_new) trained classes and n_new new ones, fp32.
  (a) bank       StreamManager(bank=, users=, label2=): every stream on its OWN slot -- front-end + 2 layers + bank_heads_window_kernel
  (b) two_head   StreamManager(label2=...) on a heads handle: front-end + 2 layers + heads_window_kernel (one shared keyword)
  (c) plain      StreamManager without label2 on the same heads handle: head 1 only, three launches
The figure is device time per chunk from HIP events around back-to-back feeds of one case; the cases are alternated inside every
round so that clock and cache state are shared; median of the rounds, spread alongside.  What is reported is (a) - (b) against (b).
usage: bench_bank_stream.py [--streams 4096,16384] [--n-new 2] [--reps 30] [--rounds 7] [--out profiles/bank_stream_bench.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from keyword_spotting_amd import get_config, weights
from keyword_spotting_amd.custom_keyword import KeywordBank
from keyword_spotting_amd.detector import StreamManager
from keyword_spotting_amd.frontend import MelFrontend
from keyword_spotting_amd.rnn_ctc import DeployModel

ap = argparse.ArgumentParser()
ap.add_argument("--streams", default="4096,16384")
ap.add_argument("--n-new", default="2")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()

rng = np.random.default_rng(1)
fe = MelFrontend(get_config())


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
for n_new in (int(s) for s in a.n_new.split(",")):
    labels = {"w%d" % i: i for i in range(1, min(6, 8 - n_new) - 2)}      # num_classes = len + 3
    cfg, cfg2 = get_config(label_dict=labels), get_config(label_dict=labels)
    H = cfg.hidden_size
    w = weights.init_weights(cfg, seed=0)
    m_one = DeployModel(cfg, w)
    cfg2.num_classes2 = cfg.num_classes + n_new
    w2 = dict(w)
    w2["Wfc2"], w2["bfc2"] = weights.extend_head(w["Wfc"], w["bfc"], rng.standard_normal((H, n_new)).astype(np.float32), np.zeros(n_new, np.float32))
    m_heads = DeployModel(cfg2, w2)
    for B in (int(s) for s in a.streams.split(",")):
        pcm = torch.from_numpy(rng.integers(-6000, 6000, (B, 3600)).astype(np.int16)).cuda()
        bank = KeywordBank(m_one, n_new, B)
        bank.set(0, torch.randn(B, H, n_new, device="cuda"), torch.zeros(B, n_new, device="cuda"))
        mgr = StreamManager(m_one, B, label="1233", bank=bank, users=torch.randperm(B), label2="1233")      # every stream its own slot
        two = StreamManager(m_heads, B, label="1233", label2="1233")
        plain = StreamManager(m_heads, B, label="1233")
        cases = {"bank": lambda: mgr.feed_pcm(pcm, fe), "two_head": lambda: two.feed_pcm(pcm, fe), "plain": lambda: plain.feed_pcm(pcm, fe)}
        names, t = {}, {k: [] for k in cases}
        for _ in range(a.rounds):
            for k, fn in cases.items():
                t[k].append(timed(fn, a.reps))
                names[k] = (bank.stack if k == "bank" else m_heads).kernel_names()
        r = {k: float(np.median(v)) for k, v in t.items()}
        rows.append({"streams": B, "n_new": n_new, "chunk_samples": 3600, "ms_bank": r["bank"], "ms_two_head": r["two_head"], "ms_plain": r["plain"],
                     "bank_minus_two_head": r["bank"] - r["two_head"], "bank_minus_two_head_relative": (r["bank"] - r["two_head"]) / r["two_head"],
                     "spread_ms": {k: [min(v), max(v)] for k, v in t.items()}, "kernels": names})
        print("B=%d n_new=%d: bank %.4f ms, two-head %.4f ms, plain %.4f ms per chunk; (a)-(b) %+.4f ms = %+.1f %% of (b)"
              % (B, n_new, r["bank"], r["two_head"], r["plain"], r["bank"] - r["two_head"], 100 * (r["bank"] - r["two_head"]) / r["two_head"]), flush=True)
        for m in (mgr, two, plain):
            m.close()
        bank.close()
    m_heads.close()
    m_one.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "rows": rows}, f, indent=1)
