"""bench.py --dump-outputs DIR: what the last timed step returned, as float .npy files of at most 64 MB in all.  On CPU through
bench.py's own main() with the model stubbed (tests/bench_stub_main.py: every call fills what it returns with its call
number); on the GPU against the library run in this process on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("logits", "softmax", "tokens", "state", "prev_word", "stream_index")


def _run(script, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + list(args), cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    assert sorted(os.listdir(str(d))) == sorted(n + ".npy" for n in NAMES)
    got = {n: np.load(str(d / (n + ".npy"))) for n in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    return got


def test_dump_holds_the_last_timed_step(tmp_path):
    line = _run(os.path.join("tests", "bench_stub_main.py"), "--steps", "5", "--warmup", "2", "--batch", "16", "--frames", "7",
                "--dist-backend", "gloo", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 5 and line["roofline"]["launches"] == 5          # --steps is the number of timed calls
    assert line["ms_per_step"] >= 10.0                                         # the stub sleeps 10 ms per call
    got = _load(tmp_path)
    assert got["logits"].shape == got["softmax"].shape == (16, 7, 6) and got["tokens"].shape == (16, 7)
    assert got["state"].shape == (2, 16, 128) and got["prev_word"].shape == (16,)
    for n in NAMES[:-1]:
        assert (got[n] == 7).all(), n                                          # call 7 = warm-up 2 + timed 5
    np.testing.assert_array_equal(got["stream_index"], np.arange(16))


def test_dump_of_a_large_step_is_a_fixed_sample_within_64_mb(tmp_path):
    args = ["--steps", "1", "--warmup", "0", "--dist-backend", "gloo"]       # 4096 x 300: ~68 MB of outputs in all
    stub = os.path.join("tests", "bench_stub_main.py")
    _run(stub, *(args + ["--dump-outputs", str(tmp_path / "a")]))
    _run(stub, *(args + ["--dump-outputs", str(tmp_path / "b")]))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) for n in NAMES) <= 64 * 10 ** 6
    idx = a["stream_index"]
    assert 2048 < len(idx) < 4096 and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 4096
    assert a["logits"].shape == (len(idx), 300, 6) and a["state"].shape == (2, len(idx), 128)
    for n in NAMES:
        np.testing.assert_array_equal(a[n], b[n])


@pytest.mark.gpu
def test_dump_is_reproducible_and_is_what_the_library_returns(tmp_path):
    import torch
    from keyword_spotting_amd import get_config, sharding, weights
    from keyword_spotting_amd.rnn_ctc import DeployModel
    B, T, warmup, steps = 64, 30, 1, 2
    args = ["--steps", str(steps), "--warmup", str(warmup), "--batch", str(B), "--frames", str(T), "--no-cpu-baseline"]
    _run("bench.py", *(args + ["--dump-outputs", str(tmp_path / "a")]))
    _run("bench.py", *(args + ["--dump-outputs", str(tmp_path / "b")]))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in NAMES:
        np.testing.assert_array_equal(a[n], b[n])
    # bench.py's inputs, rebuilt here: seeded weights, seeded mel on the device, the state carried over every call
    cfg = get_config()
    model = DeployModel(cfg, weights.init_weights(cfg, seed=0), device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(sharding.shard_seed(1, 0))
    mel = (torch.randn(B, T, cfg.n_mel, generator=gen, device="cuda:0").abs() * 2).contiguous()
    state, prev_word = model.zero_state(B), model.fresh_prev_word(B)
    for _ in range(warmup + steps):
        r = model.forward(mel, state, prev_word=prev_word, state_out=state)
    model.close()
    want = {"logits": r["logits"], "softmax": r["softmax"], "tokens": r["tokens"], "state": state, "prev_word": prev_word}
    for n, t in want.items():
        np.testing.assert_array_equal(a[n], t.cpu().numpy().astype(a[n].dtype), err_msg=n)
    np.testing.assert_array_equal(a["stream_index"], np.arange(B))
