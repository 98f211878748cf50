"""Training of the self-attention CTC model on the device (main.py --model attention over models/attention_ctc.py:131-202): taped
forward, backward, tf.nn.ctc_loss, tf.clip_by_global_norm and tf.train.AdamOptimizer / MomentumOptimizer(0.9, use_nesterov=True)
behind kws_attention_train_* (include/kws_amd.h).  An AttentionTrainer owns the parameters on the device; weights() / save() /
deploy() hand them to the serving side (attention_ctc.DeployModel).

What is trained is what is served: every utterance over its own T'_b rows (its own keys, its own layer-norm block).  That is the
reference's graph whenever all utterances of a batch have the same length; on padded batches the reference lets the padded rows
take part as keys and in the layer-norm moments, and this trainer does not.  The dropout masks of the three sites are a counter
hash of a per-call seed (drop_keep below restates it through the library's host entry)."""
import ctypes

import numpy as np

from . import _lib
from . import attention_weights as _weights
from ._trainer import _TrainerBase, exponential_decay
from .custom_keyword import _ints, _pack_labels
from .training import OPTIMIZERS

SITE_PROB, SITE_ATT, SITE_FFN = 0, 1, 2


def polynomial_decay(learning_rate, step, decay_steps, end_learning_rate, power):
    """tf.train.polynomial_decay, cycle=False: the step is clamped to decay_steps."""
    s = min(float(step), float(decay_steps))
    return (float(learning_rate) - float(end_learning_rate)) * (1.0 - s / float(decay_steps)) ** float(power) + float(end_learning_rate)


def learning_rate_at(step, learning_rate=1e-3, lr_decay=0.9, decay_step=40000, warmup=False):
    """models/attention_ctc.py:171-181: the exponential decay of the configured rate; with warmup the smaller of
    polynomial_decay(5e-3, step, 40000, 1.35e-3, power 0.5) and exponential_decay(1.5e-3, step, decay_step, lr_decay)."""
    if warmup:
        return min(polynomial_decay(5e-3, step, 40000, 1.35e-3, 0.5), exponential_decay(1.5e-3, step, decay_step, lr_decay))
    return exponential_decay(learning_rate, step, decay_step, lr_decay)


def attention_config_struct(config):
    return _lib.KwsAttentionConfig(int(config.freq_size), int(config.combine_frame), int(config.hidden_size), int(config.multi_head_num),
                                   int(config.feed_forward_inner_size), int(config.num_layers), int(config.num_classes),
                                   int(bool(config.use_relu)), int(config.max_frames))


def train_config(config, optimizer="adam", max_grad_norm=-1.0, keep_prob=1.0):
    if optimizer not in OPTIMIZERS:
        raise _lib.InvalidArgumentError(-1, "optimizer %r: 'adam' or 'nesterov' (models/attention_ctc.py:183-190)" % (optimizer,))
    return _lib.KwsAttentionTrainConfig(attention_config_struct(config), OPTIMIZERS[optimizer], float(max_grad_norm), float(keep_prob))


def drop_keep(seed, keep_prob, site, layer, b, head, rows, cols):
    """kws_attention_drop_keep: the keep decisions (uint8, the shape of rows / cols) of one site at the given coordinates.  Host code."""
    rows, cols = np.broadcast_arrays(np.asarray(rows, np.int32), np.asarray(cols, np.int32))
    r, c = np.ascontiguousarray(rows).ravel(), np.ascontiguousarray(cols).ravel()
    out = np.empty(r.size, np.uint8)
    _lib.check(_lib.load().kws_attention_drop_keep(ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), float(keep_prob), int(site), int(layer), int(b),
                                                   int(head), r.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p), int(r.size),
                                                   out.ctypes.data_as(ctypes.c_void_p)))
    return out.reshape(rows.shape)


def check_call(config, x_shape, lengths, labels, optimizer="adam", max_grad_norm=-1.0, keep_prob=1.0):
    """kws_attention_train_check on host memory alone (no device): raises what a create / grad / step of these arguments would."""
    cfg = train_config(config, optimizer, max_grad_norm, keep_prob)
    b, t = int(x_shape[0]), int(x_shape[1])
    lab, lab_len = _pack_labels(labels, b)
    sl, sl_p = _ints(np.full(b, t) if lengths is None else lengths)
    lab, lab_p = _ints(lab)
    lab_len, ll_p = _ints(lab_len)
    dummy = np.zeros(4, np.float32)      # x and loss are only checked for null and alignment
    p = dummy.ctypes.data_as(ctypes.c_void_p)
    _lib.check(_lib.load().kws_attention_train_check(ctypes.byref(cfg), p, sl_p, lab_p, ll_p, b, t, int(lab.shape[1]), p))


class AttentionTrainer(_TrainerBase):
    """The reference's attention training graph on one device.  Defaults: config/attention_config.py:49-56,81 (learning_rate 1e-3,
    lr_decay 0.9, decay_step 40000, adam, no clipping, no warm-up); keep_prob defaults to 1 (the reference file ships 0.9, :83).
    weights: a dict (attention_weights.init's form), a blob, or None for attention_weights.init(config, seed).
    frame_weight, ctc_weight, class_weight: the objective of loss_and_grad_frames, step_frames and step_raw's targets= ([B,T'], a class
    per row of the logits, -1 for none): loss[b] = ctc_weight ctc_b + frame_weight ce_b, as training.Trainer's."""

    _prefix, _weights_mod, _feature = "kws_attention_train", _weights, "freq_size"

    def __init__(self, config, weights=None, optimizer="adam", learning_rate=1e-3, lr_decay=0.9, decay_step=40000, warmup=False,
                 max_grad_norm=-1, keep_prob=1.0, seed=0, device="cuda:0", frame_weight=0.0, ctc_weight=1.0, class_weight=None):
        self.config = config
        self._set_objective(frame_weight, ctc_weight, class_weight)
        self.optimizer, self.learning_rate, self.lr_decay, self.decay_step = optimizer, float(learning_rate), float(lr_decay), int(decay_step)
        self.warmup, self.max_grad_norm, self.keep_prob = bool(warmup), float(max_grad_norm), float(keep_prob)
        self._cfg = train_config(config, optimizer, max_grad_norm, keep_prob)
        self._open(device, "kws_attention_train_create")
        self._rng = np.random.default_rng(int(seed))          # the seeds of step()
        self.global_step = 0
        if weights is None:
            weights = _weights.init(config, seed=seed)
        self.set_weights(weights)

    def _floats(self):
        return self._lib.kws_attention_weights_nbytes(ctypes.byref(self._cfg.model)) // 4

    def frames_out(self, frames):
        c = int(self.config.combine_frame)
        return frames // c + 1 if c > 1 else frames

    # -- parameters --------------------------------------------------------------------------
    def save(self, path):
        w = self.weights()
        flat = {k: w[k] for k in _weights.TOP_KEYS}
        for j, lay in enumerate(w["layers"]):
            for k in _weights.LAYER_KEYS:
                flat["layer_%d/%s" % (j, k)] = lay[k]
        np.savez(path, **flat)

    def deploy(self, precision="fp32"):
        """attention_ctc.DeployModel on the current parameters."""
        from .attention_ctc import DeployModel
        return DeployModel(self.config, self.weights_blob(), device=str(self.device), precision=precision)

    # -- compute -----------------------------------------------------------------------------
    def learning_rate_at(self, step):
        return learning_rate_at(step, self.learning_rate, self.lr_decay, self.decay_step, self.warmup)

    def loss_and_grad(self, x, lengths, labels, seed=0, want_logits=False):
        """-> (loss = sum_b ctc_b / B, gradients in the dict form, per-utterance losses [B]) [, logits [B,T',C]]; the parameters stay.
        labels: B sequences over classes 0..C-2, or one for all; seed: the dropout seed of the call (ignored at keep_prob 1)."""
        return self.loss_and_grad_frames(x, lengths, labels, None, seed=seed, want_logits=want_logits)

    def loss_and_grad_frames(self, x, lengths, labels, targets, seed=0, want_logits=False, want_frame_loss=False):
        """loss_and_grad on frame-wise targets [B,T'] (kws_attention_train_grad_frames): the per-utterance losses are ctc_weight ctc_b +
        frame_weight ce_b; with want_frame_loss ce [B] (device) is appended.  labels may be None at ctc_weight 0; targets None is
        loss_and_grad."""
        import torch
        x, b, t, (sl, sl_p), (lab, lab_p), (ll, ll_p) = self._inputs(x, lengths, labels, targets)
        ft, keep_ft, ce = self._frames(targets, b, self.frames_out(t), want_frame_loss)
        loss = torch.empty(b, dtype=torch.float32, device=self.device)
        grad = torch.empty(self._floats(), dtype=torch.float32, device=self.device)
        logits = torch.empty(b, self.frames_out(t), self.config.num_classes, dtype=torch.float32, device=self.device) if want_logits else None
        with torch.cuda.device(self.device):
            if ft is not None:
                _lib.check(self._lib.kws_attention_train_grad_frames(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]),
                                                                     ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _lib.ptr(loss), _lib.ptr(grad),
                                                                     _lib.ptr(logits), ctypes.byref(ft), self._stream()))
            else:
                _lib.check(self._lib.kws_attention_train_grad(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]),
                                                              ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _lib.ptr(loss), _lib.ptr(grad),
                                                              _lib.ptr(logits), self._stream()))
        per = loss.cpu().numpy()
        out = (float(per.astype(np.float64).sum() / b), _weights.from_blob(self.config, grad.cpu().numpy()), per)
        if want_logits:
            out += (logits,)
        return out + (ce,) if want_frame_loss else out

    def step_raw(self, x, lengths, labels, lr, seed=0, want_norm=False, targets=None):
        """One kws_attention_train_step at learning rate lr with the masks of `seed` -> per-utterance losses [B] (device) [, global norm].
        targets [B,T']: the step of the trainer's mixed objective (kws_attention_train_step_frames)."""
        import torch
        x, b, t, (sl, sl_p), (lab, lab_p), (ll, ll_p) = self._inputs(x, lengths, labels, targets)
        ft, keep_ft, _ = self._frames(targets, b, self.frames_out(t))
        loss = torch.empty(b, dtype=torch.float32, device=self.device)
        norm = torch.empty(1, dtype=torch.float32, device=self.device) if want_norm else None
        with torch.cuda.device(self.device):
            if ft is not None:
                _lib.check(self._lib.kws_attention_train_step_frames(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]),
                                                                     ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), float(lr), _lib.ptr(loss),
                                                                     _lib.ptr(norm), ctypes.byref(ft), self._stream()))
            else:
                _lib.check(self._lib.kws_attention_train_step(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]),
                                                              ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), float(lr), _lib.ptr(loss), _lib.ptr(norm),
                                                              self._stream()))
        return (loss, norm) if want_norm else loss

    def step(self, x, lengths, labels):
        """One training step as main.py runs it: a fresh dropout seed from the trainer's own generator, the scheduled learning rate, the
        update -> loss = sum_b ctc_b / B."""
        return self.step_frames(x, lengths, labels, None)

    def step_frames(self, x, lengths, labels, targets):
        """step() on frame-wise targets [B,T']: the update of the trainer's mixed objective -> sum_b (ctc_weight ctc_b + frame_weight ce_b) / B."""
        seed = int(self._rng.integers(0, 2 ** 63))
        loss = self.step_raw(x, lengths, labels, self.learning_rate_at(self.global_step), seed=seed, targets=targets)
        self.global_step += 1
        return float(loss.cpu().numpy().astype(np.float64).sum() / loss.shape[0])
