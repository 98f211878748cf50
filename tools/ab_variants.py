#!/usr/bin/env python3
"""A/B of library builds on one GPU box: runs bench.py once per library (interleaved, `--rounds` times) and prints the
per-layer kernel times.  usage: tools/ab_variants.py [--rounds 2] [--steps 10 --warmup 3] [--args "--precision int8"] [--out FILE]
name=path.so ...  (`base` = the in-tree library).  With two or more libraries the summary judges every later one against the FIRST
and against the one listed before it, by the project's rule for a gain: every run faster than every run of the first, and the median ratio above
1 + 2 x (first's max - min) / (first's median)."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--args", default="")
ap.add_argument("--out", help="also append the report to this file")
ap.add_argument("libs", nargs="+")
a = ap.parse_args()
libs = []
for spec in a.libs:
    name, _, path = spec.partition("=")
    libs.append((name, os.path.abspath(path) if path else None))
res = {n: [] for n, _ in libs}
for r in range(a.rounds):
    for name, path in libs:
        env = dict(os.environ)
        if path:
            env["KWS_AMD_LIB"] = path
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(a.steps), "--warmup", str(a.warmup), "--no-cpu-baseline"] + a.args.split(),
                             env=env, capture_output=True, text=True, timeout=300)
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if out.returncode != 0 or not lines:      # nothing more is started on a GPU that a run has just failed on
            print(name, "FAILED rc=%d" % out.returncode, out.stderr[-500:])
            sys.exit(1)
        d = json.loads(lines[-1])
        clock = (d.get("per_rank") or [{}])[0].get("clock_mhz_if_readable")      # a lower clock on a denser stream is a finding
        res[name].append((d["value"], d["roofline"]["per_layer_ms"], clock))
        print("round %d %s done" % (r + 1, name), file=sys.stderr, flush=True)
lines = ["bench.py --steps %d --warmup %d %s, %d interleaved rounds" % (a.steps, a.warmup, a.args, a.rounds)]
for name, _ in libs:
    for v, pl, clock in res[name]:
        lines.append("%-16s %8.2f M frames/s   per-layer ms %s   shader clock %s" % (name, v / 1e6, " ".join("%.4f" % x for x in pl), "unreadable" if clock is None else "%s MHz" % clock))
median = lambda xs: sorted(xs)[len(xs) // 2] if len(xs) % 2 else sum(sorted(xs)[len(xs) // 2 - 1:len(xs) // 2 + 1]) / 2
pairs = [(libs[0][0], n) for n, _ in libs[1:]] + [(libs[i][0], libs[i + 1][0]) for i in range(1, len(libs) - 1)]
for ref, name in pairs:                    # every library against the first, and against the one listed before it
    base, new = [r[0] for r in res[ref]], [r[0] for r in res[name]]
    if not base or not new:
        continue
    bar = 1 + 2 * (max(base) - min(base)) / median(base)
    ratio = median(new) / median(base)
    lines.append("%s vs %s: median ratio %.4f (bar %.4f), slowest %s run %.2f vs fastest %s run %.2f M frames/s -> %s"
                 % (name, ref, ratio, bar, name, min(new) / 1e6, ref, max(base) / 1e6,
                    "GAIN" if min(new) > max(base) and ratio > bar else "no gain under the rule"))
    for l in range(len(res[ref][0][1])):   # the same rule per layer, on kernel ms (lower is better): median lower by more than the reference's max - min
        b_ms, n_ms = [r[1][l] for r in res[ref]], [r[1][l] for r in res[name]]
        diff, spread = median(n_ms) - median(b_ms), max(b_ms) - min(b_ms)
        lines.append("    layer %d kernel ms: %s median %.4f (min %.4f max %.4f), %s median %.4f (min %.4f max %.4f): %+.4f ms against a spread of %.4f -> %s"
                     % (l, ref, median(b_ms), min(b_ms), max(b_ms), name, median(n_ms), min(n_ms), max(n_ms), diff, spread,
                        "lower" if diff < -spread else "higher" if diff > spread else "within the spread"))
print("\n".join(lines))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
