#!/usr/bin/env python3
"""A bank stream manager whose slots carry keywords of their own against the same manager on a bank without keywords, on one device and
in one process: 4096 and 16384 streams x 3600-sample int16 chunks, the reference shape (n_mel 40, hidden 128, 2 layers), C = 6 trained
classes and n_new = 2 new ones, fp32, every stream on its OWN slot.
  (a) bank           no keyword on any slot: front-end + 2 layers + bank_heads_window_kernel (case (a) of tools/bench_bank_stream.py)
  (d) bank_keywords  a keyword on every slot, labels cycling through "5" (n_used 1), "56", "55" (n_used 1), "566", "1256":
                     front-end + 2 layers + bank_keyword_window_kernel
Device time per chunk from HIP events around back-to-back feeds of one case; the cases are alternated inside every round so that clock
and cache state are shared; median of the rounds, min-max alongside.  What is reported is (d) - (a) against (a).
usage: bench_bank_keywords.py [--streams 4096,16384] [--reps 30] [--rounds 7] [--out profiles/bank_keywords_bench.json]"""
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
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()

N_NEW = 2
PATTERNS = [("5", 1), ("56", 2), ("55", 1), ("566", 2), ("1256", 2)]
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


cfg = get_config()
H = cfg.hidden_size
m_one = DeployModel(cfg, weights.init_weights(cfg, seed=0))
rows = []
for B in (int(s) for s in a.streams.split(",")):
    pcm = torch.from_numpy(rng.integers(-6000, 6000, (B, 3600)).astype(np.int16)).cuda()
    cols, bias, users = torch.randn(B, H, N_NEW, device="cuda"), torch.zeros(B, N_NEW, device="cuda"), torch.randperm(B)
    banks = {"bank": KeywordBank(m_one, N_NEW, B).set(0, cols, bias), "bank_keywords": KeywordBank(m_one, N_NEW, B).set(0, cols, bias)}
    for slot in range(B):
        banks["bank_keywords"].set_keyword(slot, *PATTERNS[slot % len(PATTERNS)])
    mgrs = {k: StreamManager(m_one, B, label="1233", bank=bank, users=users, label2="1233") for k, bank in banks.items()}
    names, t = {}, {k: [] for k in mgrs}
    for _ in range(a.rounds):
        for k, mgr in mgrs.items():
            t[k].append(timed(lambda: mgr.feed_pcm(pcm, fe), a.reps))
            names[k] = banks[k].stack.kernel_names()
    r = {k: float(np.median(v)) for k, v in t.items()}
    d = r["bank_keywords"] - r["bank"]
    rows.append({"streams": B, "n_new": N_NEW, "chunk_samples": 3600, "ms_bank": r["bank"], "ms_bank_keywords": r["bank_keywords"],
                 "keywords_minus_bank": d, "keywords_minus_bank_relative": d / r["bank"],
                 "spread_ms": {k: [min(v), max(v)] for k, v in t.items()}, "kernels": names})
    print("B=%d: bank %.4f ms [%.4f, %.4f], with keywords %.4f ms [%.4f, %.4f] per chunk; (d)-(a) %+.4f ms = %+.1f %% of (a)"
          % (B, r["bank"], min(t["bank"]), max(t["bank"]), r["bank_keywords"], min(t["bank_keywords"]), max(t["bank_keywords"]), d, 100 * d / r["bank"]),
          flush=True)
    for k in mgrs:
        mgrs[k].close()
        banks[k].close()
m_one.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "patterns": PATTERNS, "rows": rows}, f, indent=1)
