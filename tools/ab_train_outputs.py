#!/usr/bin/env python3
"""Do two builds of the library's training host code (api_train*.hip, api_attention_train.hip, api_enroll.hip) produce the same bytes?
  ab_train_outputs.py --out DIR      runs the cases below on the library KWS_AMD_LIB names (default: the built one) and writes every
                                     output array to DIR/train_outputs.npz
  ab_train_outputs.py --compare A B  exits non-zero unless both files hold the same arrays: dtype, shape and bytes
One process per library: run --out once under each KWS_AMD_LIB, then --compare.  The tool asserts nothing about the numbers.

Cases (every one: the per-utterance loss, the gradient blob and the logits of a loss_and_grad, then per optimiser three step_raw calls
and the weights, both moments and stats() -- device_bytes, allocs, steps, launches, chunk_rows -- as an int array):
  * Trainer on every name of tests/train_model.FIRST_CASES at train_model.TRAJECTORY_LR;
  * Trainer on every entry of tests/train_wrapped_model.CASES with its switches, one case under per-frame masks and one under
    variational masks at keep 0.6 (drop_masks);
  * one row of tests/train_state_model.TABLE with all four state fields: state_out / dstate_in too, then apply() of that gradient;
  * AttentionTrainer on every name of tests/attention_train_model.CASES at keep 1, one at keep 0.9 with drop_seed_for's seed;
  * per trainer one handle through a small, a large and the small shape again (one growth of the arena, then its reuse);
  * one kws_enroll_set / fit / get / moments round at the smallest shape of tests/test_gpu_enroll.py."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--compare", nargs=2, default=None)
a = ap.parse_args()

if a.compare:
    x, y = (np.load(f) for f in a.compare)
    bad = sorted(set(x.files) ^ set(y.files)) + [k for k in x.files if k in y.files and
                                                  (x[k].dtype != y[k].dtype or x[k].shape != y[k].shape or x[k].tobytes() != y[k].tobytes())]
    print("%d arrays, %d bytes: %s" % (len(x.files), sum(x[k].nbytes for k in x.files), "all byte-equal" if not bad else "DIFFERENT: %s" % bad[:20]))
    sys.exit(1 if bad else 0)
if not a.out:
    ap.error("--out DIR or --compare A B")

import torch
import attention_train_model as AM
import enroll_model as EM
import train_model as M
import train_state_model as SM
import train_wrapped_model as WM
from tests.test_gpu_enroll import Handle as EnrollHandle
from keyword_spotting_amd import _lib
from keyword_spotting_amd.attention_training import AttentionTrainer
from keyword_spotting_amd.training import Trainer

out = {}
f32_blob = lambda flat: lambda w: np.concatenate([np.asarray(v, np.float32).ravel() for _, v in flat(w)])      # noqa: E731
M_BLOB, WM_BLOB, AM_BLOB = f32_blob(M.flat), f32_blob(WM.flat), f32_blob(AM.flat)
STATS = ("device_bytes", "allocs", "steps", "launches", "chunk_rows")


def keep_state(name, t, blob_of):
    m, v = t.moments()
    out[name + "/weights"], out[name + "/m"], out[name + "/v"] = t.weights_blob(), blob_of(m), blob_of(v)
    out[name + "/stats"] = np.array([t.stats()[k] for k in STATS], np.int64)


def keep_grad(name, r, blob_of):
    """r: what a loss_and_grad with want_logits returned."""
    out[name + "/loss"], out[name + "/grad"], out[name + "/logits"] = r[2], blob_of(r[1]), r[3].cpu().numpy()


def run(name, make, blob_of, p, lrs, **call):
    """make(optimizer=) -> a trainer on p; call: what loss_and_grad and step_raw take besides the batch (drop=, seed=)."""
    for kind in ("adam", "nesterov"):
        t = make(optimizer=kind)
        if kind == "adam":
            keep_grad(name, t.loss_and_grad(p["x"], p["seq_len"], p["labels"], want_logits=True, **call), blob_of)
        for s in range(3):
            out["%s/%s/step%d" % (name, kind, s)] = t.step_raw(p["x"], p["seq_len"], p["labels"], lrs[kind], **call).cpu().numpy()
        keep_state("%s/%s" % (name, kind), t, blob_of)
        t.close()


def gru(p, keep_prob=1.0):
    return lambda **kw: Trainer(p["config"], p["w"], keep_prob=keep_prob, **kw)


for name in M.FIRST_CASES:
    p = M.make_problem(name)
    run("gru/" + name, gru(p), M_BLOB, p, M.TRAJECTORY_LR)
for name in sorted(WM.CASES):
    p = WM.make_problem(name)
    run("wrapped/" + name, gru(p), WM_BLOB, p, M.TRAJECTORY_LR)
p = WM.make_problem("both_ref_shape")
run("wrapped/both_ref_shape/frame_masks", gru(p, 0.6), WM_BLOB, p, M.TRAJECTORY_LR, drop=WM.drop_masks(p, 0.6))
p = WM.make_problem("res_l2", var=True)
run("wrapped/res_l2/variational", gru(p, 0.6), WM_BLOB, p, M.TRAJECTORY_LR, drop=WM.drop_masks(p, 0.6, variational=True))

p = SM.make_problem("both_ref_shape")
t = Trainer(p["config"], p["w"])
r = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], want_logits=True, state=p["state_in"], dstate_out=p["dstate_out"], want_state=True)
keep_grad("state/both_ref_shape", r, WM_BLOB)
out["state/both_ref_shape/state_out"], out["state/both_ref_shape/dstate_in"] = r[4][0].cpu().numpy(), r[4][1].cpu().numpy()
out["state/both_ref_shape/apply_norm"] = t.apply(r[1], lr=0.01).cpu().numpy()
keep_state("state/both_ref_shape/applied", t, WM_BLOB)
t.close()


def attention(p, keep_prob=1.0):
    return lambda **kw: AttentionTrainer(p["config"], p["w"], keep_prob=keep_prob, **kw)


for name in sorted(AM.CASES):
    p = AM.make_problem(name)
    run("attention/" + name, attention(p), AM_BLOB, p, AM.TRAJECTORY_LR)
p = AM.make_problem("c2")
run("attention/c2/keep0.9", attention(p, 0.9), AM_BLOB, p, AM.TRAJECTORY_LR, seed=AM.drop_seed_for("c2", 0.9)[0])

# one handle per trainer through small, large, small: the arena grows once and is carved three times
rng = np.random.default_rng(5)
p = M.make_problem("ref_shape")
t = Trainer(p["config"], p["w"])
for i, case in enumerate(("t2", "mel60_l3", "t2")):
    b, frames, seq_len, labels = M.CASES[case][4:]
    x = rng.standard_normal((b, frames, p["config"].n_mel)).astype(np.float32)
    keep_grad("arena/gru/%d" % i, t.loss_and_grad(x, np.array(seq_len, np.int32), labels, want_logits=True), M_BLOB)
    keep_state("arena/gru/%d" % i, t, M_BLOB)
t.close()
p = AM.make_problem("c2")
t = AttentionTrainer(p["config"], p["w"])
for i, (b, frames) in enumerate(((2, 6), (3, 12), (2, 6))):
    x = rng.standard_normal((b, frames, p["config"].freq_size)).astype(np.float32)
    keep_grad("arena/attention/%d" % i, t.loss_and_grad(x, None, p["labels"][:b], want_logits=True), AM_BLOB)
    keep_state("arena/attention/%d" % i, t, AM_BLOB)
t.close()

h = EnrollHandle([EM.make_problem("t1_empty_label")])
out["enroll/loss_trace"] = h.fit(3, 0.01)
out["enroll/W"], out["enroll/b"] = h.get()
m, v = (torch.empty(h.E * (h.H + 1) * h.n, device="cuda") for _ in range(2))
_lib.check(h.lib.kws_enroll_moments(h.h, _lib.ptr(m), _lib.ptr(v), None))
torch.cuda.synchronize()
out["enroll/m"], out["enroll/v"] = m.cpu().numpy(), v.cpu().numpy()
out["enroll/stats"] = np.array(h.stats(), np.int64)
h.close()

os.makedirs(a.out, exist_ok=True)
np.savez(os.path.join(a.out, "train_outputs.npz"), **out)
print("%d arrays written to %s (library: %s)" % (len(out), a.out, os.environ.get("KWS_AMD_LIB", "the built one")))
