"""A plain bench.py run does what its headline needs and no more; what takes runs of its own (sustained run, secondary lines,
CPU baseline) comes only with --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("sustained", "value_sustained_10s", "secondary", "realtime_streams_sustained_distinct", "cpu_baseline",
          "speedup_vs_cpu_baseline")


def test_full_is_an_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_without_the_extras():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["unit"] == "mel-frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["roofline"]["launches"] == 3 and line["value"] > 1e8
    assert abs(line["value"] - 4096 * 300 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not [k for k in EXTRAS if k in line], sorted(line)
