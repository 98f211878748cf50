#!/usr/bin/env python3
"""Weight converter: an .npz of TF variables of the reference graph (either naming generation) or this
package's own .npz  ->  the flat fp32 blob `kws_create` takes (+ the canonical .npz).  No TensorFlow
needed; dump a checkpoint with `np.savez(path, **{v.name: sess.run(v) for v in tf.global_variables()})`
on a machine that has it.  (Replaces the freeze/export half of main.py:316-371 for this path.)

    python tools/convert_weights.py vars.npz --n-mel 40 --out model          # model.blob + model.npz

--layer-norm / --residual: the model was trained with config.use_layer_norm / use_residual (models/rnn_ctc.py:186-197).  The
layer norm's LayerNormalizer/{ibeta,igamma} variables are then required (and refused without the flag); the blob is the one
kws_create_wrapped takes.  The residual has no variables: say so with the flag, nothing in the file can tell.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from keyword_spotting_amd import get_config, weights

ap = argparse.ArgumentParser()
ap.add_argument("src")
ap.add_argument("--out", required=True)
ap.add_argument("--n-mel", type=int, default=40)
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--layer-norm", action="store_true", help="LayerNormalizer around every cell (config.use_layer_norm)")
ap.add_argument("--residual", action="store_true", help="ResidualWrapper on layers >= 1 (config.use_residual)")
a = ap.parse_args()
cfg = get_config(n_mel=a.n_mel, hidden_size=a.hidden, num_layers=a.layers, use_layer_norm=a.layer_norm, use_residual=a.residual)
z = np.load(a.src)
if any("gru_cell" in k for k in z.files):
    w = weights.from_tf_variables(cfg, {k: z[k] for k in z.files})
else:
    w = weights.load_npz(a.src)
    weights.check_shapes(cfg, w)
blob = weights.to_blob(cfg, w)
blob.tofile(a.out + ".blob")
weights.save_npz(a.out + ".npz", w)
print("%s: %d floats (%d bytes) -> %s.blob, %s.npz%s" % (a.src, blob.size, blob.nbytes, a.out, a.out,
      " (cell wrappers: layer_norm=%d residual=%d -- kws_create_wrapped)" % (a.layer_norm, a.residual) if a.layer_norm or a.residual else ""))
