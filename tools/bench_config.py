#!/usr/bin/env python3
"""Times kws_step for an arbitrary model shape (informational; bench.py is the headline)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from keyword_spotting_amd import get_config, weights
from keyword_spotting_amd.rnn_ctc import DeployModel
ap = argparse.ArgumentParser()
ap.add_argument("--n-mel", type=int, default=60); ap.add_argument("--hidden", type=int, default=256)
ap.add_argument("--layers", type=int, default=4); ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--frames", type=int, default=300); ap.add_argument("--kernel", default="auto")
ap.add_argument("--precision", default="fp32")
ap.add_argument("--layer-norm", action="store_true", help="LayerNormalizer around every cell (kws_create_wrapped)")
ap.add_argument("--residual", action="store_true", help="ResidualWrapper on layers >= 1 (kws_create_wrapped)")
a = ap.parse_args()
cfg = get_config(n_mel=a.n_mel, hidden_size=a.hidden, num_layers=a.layers, precision=a.precision,
                 use_layer_norm=a.layer_norm, use_residual=a.residual)
w = weights.init_weights(cfg)
for lay in w["layers"]:
    if a.layer_norm:                 # not the TF initial ibeta = 0: a scale that lets the input through
        lay["ibeta"] = lay["ibeta"] + 1.0
m = DeployModel(cfg, w, kernel=a.kernel)
mel = torch.randn(a.batch, a.frames, a.n_mel, device="cuda").abs() * 2
st = m.zero_state(a.batch)
for _ in range(3): m.forward(mel, st, state_out=st)
torch.cuda.synchronize(); t0 = time.perf_counter()
n = 10
for _ in range(n): m.forward(mel, st, state_out=st)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / n
macs = sum(((a.n_mel if l == 0 else a.hidden) + a.hidden) * 3 * a.hidden for l in range(a.layers)) + a.hidden * 6
print("I=%d H=%d L=%d B=%d T=%d kernel=%s %s%s [%s]: %.3f ms/step  %.1f M frames/s  %.1f TFLOP/s (algorithmic)" % (a.n_mel, a.hidden, a.layers, a.batch, a.frames, a.kernel,
      a.precision, " ln" * a.layer_norm + " residual" * a.residual, m.kernel_names()[-1], dt * 1e3, a.batch * a.frames / dt / 1e6, 2 * macs * a.batch * a.frames / dt / 1e12))
