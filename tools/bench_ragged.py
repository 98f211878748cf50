#!/usr/bin/env python3
"""Cost of per-stream arrival in the stream manager (kws_stream_feed_ragged) against the lock-step feed (kws_stream_feed).

Per precision and streams per call, ms per chunk by device events (warm-up, then the variants alternated round by round):
  (a) lock-step kws_stream_feed, n = 3600
  (b) ragged, every n_b = 3600
  (c) ragged mixed: 10 % of the streams 0, the rest uniform in 3200..4000 (rows of 4000)
and (d) a paced run (serving.run_paced, 225 ms periods) with the mixed lengths of (c) at a fixed population: the managers
bench_serve sustains lock-step (--paced-managers, per precision) and 0.95 x that -- misses and p50 / p99 / max.

  python tools/bench_ragged.py [--precisions fp32,f16x3,bf16] [--batches 4096,16384] [--rounds 5] [--steps 20]
                               [--variants a,b,c] [--paced-managers fp32=186,f16x3=410,bf16=592] [--paced-periods 40]
                               [--no-paced] [--json]
Every variant is handed whole contiguous rows, as a capture buffer hands them over (no copy inside the timed loop).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CHUNK = 3600


def mixed_lengths(B, gen, device):
    import torch
    lens = torch.randint(3200, 4001, (B,), generator=gen, device=device, dtype=torch.int32)
    lens[torch.rand(B, generator=gen, device=device) < 0.10] = 0
    return lens


def per_chunk_ms(precision, B, rounds, steps, warmup=5, which="abc"):
    import torch
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.detector import StreamManager
    from keyword_spotting_amd.frontend import MelFrontend
    from keyword_spotting_amd.rnn_ctc import DeployModel
    dev = torch.device("cuda:0")
    cfg = get_config(precision=precision)
    model = DeployModel(cfg, weights.init_weights(cfg, seed=0), device=dev)
    fe = MelFrontend(cfg, device=dev)
    gen = torch.Generator(device=dev).manual_seed(4242)
    pcm = torch.randint(-3000, 3000, (B, 4000), dtype=torch.int16, device=dev, generator=gen)
    pcm_lock = pcm[:, :CHUNK].contiguous()          # [B, 3600] rows of their own: feed_pcm then copies nothing
    full = torch.full((B,), CHUNK, dtype=torch.int32, device=dev)
    mixed = mixed_lengths(B, gen, dev)
    lock, rag, mix = (StreamManager(model, B) for _ in range(3))
    variants = {
        "a_lockstep": lambda: lock.feed_pcm(pcm_lock, fe),
        "b_ragged_equal": lambda: rag.feed_pcm(pcm_lock, fe, lengths=full),
        "c_ragged_mixed": lambda: mix.feed_pcm(pcm, fe, lengths=mixed),
    }
    variants = {k: f for k, f in variants.items() if k[0] in which}
    out = {k: [] for k in variants}
    for k, f in variants.items():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    order = list(variants)
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                variants[k]()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / steps)
    if "c" in which:
        mix.feed_pcm(pcm, fe, lengths=mixed)
    names = [nm for nm in model.kernel_names() if nm]
    for m in (lock, rag, mix):
        m.close()
    fe.close()
    model.close()
    res = {k: {"ms_min": min(v), "ms_median": sorted(v)[len(v) // 2]} for k, v in out.items()}
    for k in ("b_ragged_equal", "c_ragged_mixed"):
        if k in res and "a_lockstep" in res:
            res[k[0] + "_over_a"] = res[k]["ms_median"] / res["a_lockstep"]["ms_median"]
    res["ragged_gru_kernels"] = names
    return res


def paced(precision, managers, periods, S=16384):
    import torch
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.serving import StreamServer, run_paced
    dev = torch.device("cuda:0")
    cfg = get_config(precision=precision)
    server = StreamServer(cfg, device=dev, streams_per_manager=S, handles=2)
    gen = torch.Generator(device=dev).manual_seed(777)
    out = {}
    try:
        for m in (managers, int(round(0.95 * managers))):
            server.resize(m)
            pcm = [torch.randint(-3000, 3000, (S, 4000), dtype=torch.int16, device=dev, generator=gen) for _ in range(m)]
            lens = [[mixed_lengths(S, gen, dev) for _ in range(m)] for _ in range(2)]
            torch.cuda.synchronize()
            r = run_paced(server, lambda p, k: pcm[k], periods=periods, lengths_of=lambda p, k: lens[p % 2][k])
            out["%d_managers" % m] = {"streams": m * S, "deadline_misses": r["deadline_misses"], "compute_ms_p50": r["compute_ms_p50"],
                                      "compute_ms_p99": r["compute_ms_p99"], "compute_ms_max": r["compute_ms_max"]}
            del pcm, lens
    finally:
        server.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--precisions", default="fp32,f16x3,bf16")
    ap.add_argument("--batches", default="4096,16384")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--variants", default="a,b,c", help="subset of a,b,c (e.g. b alone under a profiler)")
    ap.add_argument("--paced-managers", default="fp32=186,f16x3=410,bf16=592")
    ap.add_argument("--paced-periods", type=int, default=40)
    ap.add_argument("--no-paced", action="store_true")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    paced_m = dict((k, int(v)) for k, v in (kv.split("=") for kv in args.paced_managers.split(",")))
    result = {}
    for prec in args.precisions.split(","):
        result[prec] = {}
        for B in (int(b) for b in args.batches.split(",")):
            r = per_chunk_ms(prec, B, args.rounds, args.steps, which=args.variants.replace(",", ""))
            result[prec]["B%d" % B] = r
            if not args.json:
                cols = ["(%s) %.4f" % (k[0], v["ms_median"]) for k, v in r.items() if isinstance(v, dict)]
                cols += ["%s %.3f" % (k.replace("_over_", "/"), v) for k, v in r.items() if k.endswith("_over_a")]
                print("%-6s B=%-6d %s ms/chunk   %s" % (prec, B, "  ".join(cols), r["ragged_gru_kernels"]), flush=True)
        if not args.no_paced and prec in paced_m:
            result[prec]["paced"] = paced(prec, paced_m[prec], args.paced_periods)
            if not args.json:
                print(prec, "paced", json.dumps(result[prec]["paced"]), flush=True)
    if args.json:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
