#!/usr/bin/env python3
"""The self-attention model on live streams (attention_stream.AttentionStreamManager, kws_attention_stream_feed) at the reference shape:
hidden 128, 8 heads, 3 layers, combine_frame 2, n_mel 60, a window of 15 chunks of 3600 samples (225 ms), fp32 and f16x3 handles.

Per precision and batch: ms per chunk with FULL windows (HIP events around each feed; the median and range of the rounds' medians),
real-time streams = B x 225 ms / time, the bytes the manager owns, and -- at the first batch -- the host mirror
(AttentionHotwordDetector) doing the same chunks on the same GPU, wall clock around a synchronised feed.  The batches are 256 and
the largest the manager is given (--max-batch, halved while the device refuses the memory).

The share of the two new kernels comes from a kernel trace in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- python tools/bench_attention_stream.py --trace-only
    python tools/bench_attention_stream.py --kernel-stats DIR --out profiles/attention_stream_bench.json
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keyword_spotting_amd import _lib, attention_weights as AW                                          # noqa: E402
from keyword_spotting_amd.attention_ctc import DeployModel                                              # noqa: E402
from keyword_spotting_amd.attention_stream import AttentionHotwordDetector, AttentionStreamManager     # noqa: E402
from keyword_spotting_amd.config import get_attention_config                                            # noqa: E402

CHUNK, WINDOW, CHUNK_MS = 3600, 15, 225.0


def chunks(batch, n, seed):
    """n loud chunks [batch, CHUNK] on the device (noise at speech level: the VAD never clears, random weights never say 1233)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(batch, CHUNK, device="cuda", generator=g) * 0.1 for _ in range(n)]


def time_manager(model, batch, rounds, steps):
    mgr = AttentionStreamManager(model, batch, window_chunks=WINDOW, max_chunk_samples=CHUNK)
    data = chunks(batch, WINDOW + steps, batch)
    for x in data[:WINDOW]:                       # fill the windows: every timed chunk evicts a slot and runs over 15 chunks
        mgr.feed_pcm(x)
    medians = []
    for _ in range(rounds):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for (a, b), x in zip(ev, data[WINDOW:]):
            a.record()
            mgr.feed_pcm(x)
            b.record()
        torch.cuda.synchronize()
        medians.append(float(np.median([a.elapsed_time(b) for a, b in ev])))
    frames = int(mgr.window(want_mel=False)[1].min())
    stats = mgr.stats()
    hits = int(mgr.hit.sum())
    mgr.close()
    return medians, frames, stats, hits


def time_mirror(model, batch, rounds, steps):
    mir = AttentionHotwordDetector(model, batch, window_chunks=WINDOW, max_chunk_samples=CHUNK)
    data = chunks(batch, WINDOW + steps, batch)
    for x in data[:WINDOW]:
        mir.feed_pcm(x)
    medians = []
    for _ in range(rounds):
        ts = []
        for x in data[WINDOW:]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mir.feed_pcm(x)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        medians.append(float(np.median(ts)))
    return medians


def summary(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def kernel_shares(directory):
    """rocprofv3 --kernel-trace --stats: the share of a feed's kernel time per kernel family (the run's own input generation aside)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % directory)
    groups = {"attn_stream_window_kernel": 0.0, "attn_stream_decide_kernel": 0.0, "mel_fft400_kernel": 0.0, "model (attn_*)": 0.0}
    for row in csv.DictReader(open(files[0])):
        name, ns = row["Name"], float(row["TotalDurationNs"])
        key = next((k for k in list(groups)[:3] if k in name), "model (attn_*)" if "kws::attn_" in name else None)
        if key:
            groups[key] += ns
    total = sum(groups.values())
    return {k: v / total for k, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32,f16x3")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max-batch", type=int, default=65535)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--trace-only", action="store_true", help="feed full windows at --batch and exit (the run rocprofv3 traces)")
    ap.add_argument("--kernel-stats", help="directory of a rocprofv3 --kernel-trace --stats run of --trace-only")
    ap.add_argument("--out")
    args = ap.parse_args()
    cfg = get_attention_config()
    w = AW.init(cfg, 0)
    if args.trace_only:
        model = DeployModel(cfg, w)
        mgr = AttentionStreamManager(model, args.batch, window_chunks=WINDOW, max_chunk_samples=CHUNK)
        for x in chunks(args.batch, WINDOW + 20, args.batch):
            mgr.feed_pcm(x)
        torch.cuda.synchronize()
        return
    rows = []
    for precision in args.precision.split(","):
        model = DeployModel(cfg, w, precision=precision)
        runs, big = {}, args.max_batch
        while big > args.batch:
            try:
                runs[big] = time_manager(model, big, args.rounds, args.steps)
                break
            except (_lib.KwsError, RuntimeError) as e:         # the device refuses the memory: halve
                print("B=%d refused (%s)" % (big, str(e)[:120]), flush=True)
                torch.cuda.empty_cache()
                big //= 2
        runs[args.batch] = time_manager(model, args.batch, args.rounds, args.steps)
        for batch in sorted(runs):
            medians, frames, stats, hits = runs[batch]
            ms = summary(medians)
            row = {"precision": precision, "batch": batch, "window_frames": frames, "ms_per_chunk": ms,
                   "realtime_streams": batch * CHUNK_MS / ms["median"], "owned_bytes_per_stream": stats["device_bytes"] / batch,
                   "launches_per_feed": stats["launches_last_feed"], "hits": hits}
            if batch == args.batch:
                mirror = summary(time_mirror(model, batch, args.rounds, args.steps))
                row["host_mirror_ms_per_chunk"] = mirror
                row["speedup_over_host_mirror"] = mirror["median"] / ms["median"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        model.close()
    result = {"shape": {"hidden": cfg.hidden_size, "heads": cfg.multi_head_num, "layers": cfg.num_layers, "combine_frame": cfg.combine_frame,
                        "n_mel": cfg.n_mel, "window_chunks": WINDOW, "chunk_samples": CHUNK}, "rounds": args.rounds, "steps": args.steps,
              "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.kernel_stats:
        result["kernel_time_share_fp32_B%d" % args.batch] = kernel_shares(args.kernel_stats)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
