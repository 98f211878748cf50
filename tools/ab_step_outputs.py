#!/usr/bin/env python3
"""Do two builds of the GRU kernels (gru_*.hip and the device headers they share) produce the same bytes?
  ab_step_outputs.py --out DIR      runs the cases below on the library KWS_AMD_LIB names (default: the built one) and writes every
                                    output array to DIR/step_outputs.npz
  ab_step_outputs.py --compare A B  exits non-zero unless both files hold the same arrays, byte for byte
One process per library: run --out once under each KWS_AMD_LIB, then --compare.  (The class-head kernels: tools/ab_heads_outputs.py.)

Cases:
  * every row of tests/config_space_grid.ROWS: one forward call with the row's masks, weights and inputs from
    tests/test_gpu_config_space.py (weights_of, inputs): logits, softmax, tokens, prev_word and state;
  * the wrapped generic stacks: layer norm, residual and both at hidden 64 / 128 / 256 with B = 19, T = 33, as one layer-pipelined
    launch and, with profiling on, as sequential launches;
  * a plain StreamManager per precision fp32 / f16x3 / bf16, fed chunks of {0, 1, 22, 33} frames with one silent chunk: hit, restart
    and state per chunk (the WINDOW = true instantiations of the last-layer kernels run nowhere else)."""
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
from oracle import gru_oracle as G
from tests import config_space_grid as S
from tests import test_gpu_config_space as CS
from wrapped_cell_model import random_ln
from keyword_spotting_amd import get_config
from keyword_spotting_amd.detector import StreamManager
from keyword_spotting_amd.rnn_ctc import DeployModel

out = {}
t_ = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v))


def keep(name, r, pw):
    for k, v in r.items():
        if torch.is_tensor(v):
            out["%s/%s" % (name, k)] = v.cpu().numpy()
    out["%s/prev_word" % name] = pw.cpu().numpy()


for row in S.ROWS:
    cfg = get_config(n_mel=row.n_mel, hidden_size=row.hidden, num_layers=row.layers, precision=row.prec, use_relu=bool(row.relu),
                     value_clip=row.clip)
    cfg.label_dict = {str(k): k for k in range(1, row.classes - 2)}
    m = DeployModel(cfg, CS.weights_of(row), kernel=row.kernel)
    mel, st0, lens, reset = CS.inputs(row)
    pw = m.fresh_prev_word(mel.shape[0])
    keep("row/" + row.name, m.forward(t_(mel), t_(st0), seq_len=t_(lens), reset_mask=t_(reset), prev_word=pw), pw)
    m.close()

B, T = 19, 33
for hidden, n_mel, layers in ((64, 13, 2), (128, 40, 2), (256, 60, 3)):
    for wrap, (ln, res) in {"ln": (True, False), "res": (False, True), "ln_res": (True, True)}.items():
        w = G.random_weights(n_mel, hidden, layers, 6, 7 + hidden)
        m = DeployModel(get_config(n_mel=n_mel, hidden_size=hidden, num_layers=layers, use_layer_norm=ln, use_residual=res),
                        random_ln(w, n_mel, 7 + hidden) if ln else w)
        rng = np.random.default_rng(hidden)
        mel = G.synthetic_mel(B, T, n_mel, seed=hidden + 1)
        st0 = (0.3 * rng.standard_normal((layers, B, hidden))).astype(np.float32)
        lens = rng.integers(0, T + 1, B).astype(np.int32)
        reset = (rng.random(B) < 0.3).astype(np.uint8)
        for launch in ("pipelined", "sequential"):
            m.set_profiling(launch == "sequential")
            pw = m.fresh_prev_word(B)
            keep("wrapped/h%d/%s/%s" % (hidden, wrap, launch), m.forward(t_(mel), t_(st0), seq_len=t_(lens), reset_mask=t_(reset), prev_word=pw), pw)
        m.set_profiling(False)
        m.close()

CHUNKS = [22, 0, 1, 33, 22, 22, 33, 1, 22, 0, 22, 33, 22, 22]
for prec in ("fp32", "f16x3", "bf16"):
    cfg = get_config(n_mel=40, hidden_size=128, num_layers=2, precision=prec)
    m = DeployModel(cfg, G.random_weights(40, 128, 2, cfg.num_classes, 11))
    rng = np.random.default_rng(12)
    mel = torch.from_numpy(G.synthetic_mel(B, sum(CHUNKS), 40, seed=13)).cuda()
    mgr = StreamManager(m, B, label="1", window_chunks=4, max_frames=40)
    pos = 0
    for ci, n in enumerate(CHUNKS):
        speech = rng.random(B) > (1.0 if ci == 5 else 0.1)
        hit = mgr.feed(mel[:, pos:pos + n].clone(), speech=torch.from_numpy(speech)).cpu().numpy()
        name = "manager/%s/chunk%d" % (prec, ci)
        out[name + "/hit"], out[name + "/restart"], out[name + "/state"] = hit.copy(), mgr.restart.cpu().numpy(), mgr.state.cpu().numpy()
        pos += n
    mgr.close()
    m.close()

os.makedirs(a.out, exist_ok=True)
np.savez(os.path.join(a.out, "step_outputs.npz"), **out)
print("%d arrays written to %s (library: %s)" % (len(out), a.out, os.environ.get("KWS_AMD_LIB", "the built one")))
