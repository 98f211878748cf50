#!/usr/bin/env python3
"""Weight converter: an .npz of TF variables of the reference graph (either naming generation) or this
package's own .npz  ->  the flat fp32 blob `kws_create` takes (+ the canonical .npz).  No TensorFlow
needed; dump a checkpoint with `np.savez(path, **{v.name: sess.run(v) for v in tf.global_variables()})`
on a machine that has it.  (Replaces the freeze/export half of main.py:316-371 for this path.)

    python tools/convert_weights.py vars.npz --n-mel 40 --out model          # model.blob + model.npz

--layer-norm / --residual: the model was trained with config.use_layer_norm / use_residual (models/rnn_ctc.py:186-197).  The
layer norm's LayerNormalizer/{ibeta,igamma} variables are then required (and refused without the flag); the blob is the one
kws_create_wrapped takes.  The residual has no variables: say so with the flag, nothing in the file can tell.

--model attention: the self-attention CTC model (models/attention_ctc.py, main.py --model attention) -> the blob
kws_attention_create takes (model.blob only).  Dump tf.trainable_variables() there: every variable must be one of the model's
(keyword_spotting_amd/attention_weights.py), none may be missing.  Shape flags default to config/attention_config.py.
--mfcc [--n-mfcc 20]: the checkpoint was trained on MFCC features (config.mfcc: input_linear_trans takes 3 * n_mfcc per frame).
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from keyword_spotting_amd import get_config, weights

ap = argparse.ArgumentParser()
ap.add_argument("src")
ap.add_argument("--out", required=True)
ap.add_argument("--model", choices=("rnn", "attention"), default="rnn")
ap.add_argument("--n-mel", type=int, default=None, help="default 40 (rnn) / 60 (attention)")
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--layers", type=int, default=None, help="default 2 (rnn) / 3 (attention)")
ap.add_argument("--layer-norm", action="store_true", help="LayerNormalizer around every cell (config.use_layer_norm)")
ap.add_argument("--residual", action="store_true", help="ResidualWrapper on layers >= 1 (config.use_residual)")
ap.add_argument("--combine-frame", type=int, default=2, help="attention: frames stacked per row")
ap.add_argument("--heads", type=int, default=8, help="attention: multi_head_num")
ap.add_argument("--ffn-inner", type=int, default=512, help="attention: feed_forward_inner_size")
ap.add_argument("--mfcc", action="store_true", help="attention: trained with config.mfcc (input width 3 * n_mfcc instead of n_mel)")
ap.add_argument("--n-mfcc", type=int, default=20, help="attention with --mfcc: config.n_mfcc")
a = ap.parse_args()
if a.model == "attention":
    from keyword_spotting_amd import attention_weights
    from keyword_spotting_amd.config import get_attention_config
    cfg = get_attention_config(n_mel=a.n_mel or 60, hidden_size=a.hidden, num_layers=a.layers or 3, combine_frame=a.combine_frame,
                               multi_head_num=a.heads, feed_forward_inner_size=a.ffn_inner, mfcc=a.mfcc, n_mfcc=a.n_mfcc)
    z = np.load(a.src)
    try:
        blob = attention_weights.to_blob(cfg, attention_weights.from_tf_variables(cfg, {k: z[k] for k in z.files}))
    except ValueError as e:
        sys.exit("%s: %s" % (a.src, e))
    blob.tofile(a.out + ".blob")
    print("%s: %d floats (%d bytes) -> %s.blob (kws_attention_create)" % (a.src, blob.size, blob.nbytes, a.out))
    sys.exit(0)
cfg = get_config(n_mel=a.n_mel or 40, hidden_size=a.hidden, num_layers=a.layers or 2, use_layer_norm=a.layer_norm, use_residual=a.residual)
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
