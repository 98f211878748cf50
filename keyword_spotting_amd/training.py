"""Training of the GRU stack on the device (main.py's loop over models/rnn_ctc.py:34-101): taped forward, back-propagation through
time, tf.nn.ctc_loss, tf.clip_by_global_norm and tf.train.AdamOptimizer / MomentumOptimizer(0.9, use_nesterov=True) behind
kws_train_* (include/kws_amd.h).  A Trainer owns the parameters on the device; weights() / save() / deploy() hand them to the
serving side.  config.use_layer_norm / use_residual / variational_recurrent (get_cell's wrappers, models/rnn_ctc.py:179-199) take the
handle of kws_train_create_wrapped: the layer norm's ibeta / igamma are then parameters like the others.

Carried states (kws_train_grad_state / kws_train_step_state): loss_and_grad, step_raw and step take state= [L,B,H] (what DeployModel
calls the state) and hand out the state after each stream's last frame; dstate_out= is the gradient a later segment returned for that
state, so that a recording cut into segments is trained with the exact gradient (see Trainer.loss_and_grad).  apply() takes the
optimiser step from a gradient the caller supplies: a chain's sum, accumulated batches, the sum over several devices."""
import ctypes

import numpy as np

from . import _lib
from . import weights as _weights
from ._trainer import _TrainerBase, exponential_decay

OPTIMIZERS = {"adam": _lib.OPT_ADAM, "nesterov": _lib.OPT_NESTEROV}


def learning_rate_at(step, learning_rate=1.5e-3, lr_decay=0.8, decay_step=20000):
    """tf.train.exponential_decay(learning_rate, global_step, decay_step, lr_decay), staircase=False (models/rnn_ctc.py:76-78)."""
    return exponential_decay(learning_rate, step, decay_step, lr_decay)


def segment_lengths(lengths, start, frames):
    """The per-stream seq_len of the segment [start, start + frames) of utterances `lengths` frames long: clip(lengths - start, 0, frames).
    A stream that ended before the segment runs it at seq_len 0: its state and its state's gradient pass through."""
    return np.clip(np.asarray(lengths, np.int64) - int(start), 0, int(frames)).astype(np.int32)


def train_config(config, optimizer="adam", max_grad_norm=-1.0, keep_prob=1.0):
    """The kws_train_config of a model config: every option a train handle refuses travels with its own field, so the refusal names it.
    The three switches of kws_train_create_wrapped are read from the config (use_layer_norm, use_residual, variational_recurrent)."""
    if optimizer not in OPTIMIZERS:
        raise _lib.InvalidArgumentError(-1, "optimizer %r: 'adam' or 'nesterov' (models/rnn_ctc.py:80-87)" % (optimizer,))
    model = _lib.KwsConfig(config.n_mel, config.hidden_size, config.num_layers, config.num_classes, int(bool(config.use_relu)),
                           float(config.value_clip),
                           {"fp32": _lib.FP32, "bf16": _lib.BF16, "int8": _lib.INT8, "f16x3": _lib.F16X3}[getattr(config, "precision", "fp32")])
    wrap = _lib.KwsCellWrappers(int(bool(getattr(config, "use_layer_norm", False))), int(bool(getattr(config, "use_residual", False))))
    return _lib.KwsTrainConfig(model, wrap, int(bool(getattr(config, "variational_recurrent", False))), OPTIMIZERS[optimizer],
                               float(max_grad_norm), float(keep_prob))


class Trainer(_TrainerBase):
    """The reference's training graph on one device.  Defaults: config/rnn_config.py:44-55,77 (learning_rate 1.5e-3, lr_decay 0.8,
    decay_step 20000, adam, max_grad_norm -1 = no clipping); keep_prob defaults to 1 (the reference file ships 0.6, :81).

    weights: a dict (weights.init_weights' form), a blob, or None for init_weights(config, seed).  With config.use_layer_norm the dict
    carries each layer's ibeta / igamma and the blob is kws_weights_nbytes_wrapped's; with config.variational_recurrent the output masks
    are [L,B,H], one per stream and layer held for all frames.
    wrapped: None takes kws_train_create_wrapped exactly when one of the three switches is set; True takes it always (with every switch
    off it gives kws_train_create's handle: the same launches, the same bits).
    state_noise: > 0 starts every step() that is given no state from state_noise * randn([L,B,H]) (the reference README's "noisy
    states": a model served with carried state never sees the zero state after its first chunk).
    frame_weight, ctc_weight, class_weight: the objective of the calls that are given targets= (frame-wise targets [B,T], the form of
    custom_keyword.frame_labels: a class per frame, the blank included, -1 for none) -- loss_and_grad_frames, step_frames and step_raw's
    targets=: loss[b] = ctc_weight ctc_b + frame_weight ce_b (kws_train_grad_frames / kws_train_step_frames); with ctc_weight 0 labels
    may be None.  A call without targets is the CTC loss alone."""

    _prefix, _weights_mod, _feature = "kws_train", _weights, "n_mel"

    def __init__(self, config, weights=None, optimizer="adam", learning_rate=1.5e-3, lr_decay=0.8, decay_step=20000, max_grad_norm=-1,
                 keep_prob=1.0, seed=0, device="cuda:0", wrapped=None, state_noise=0.0, frame_weight=0.0, ctc_weight=1.0, class_weight=None):
        import torch
        self.config = config
        self._set_objective(frame_weight, ctc_weight, class_weight)
        self.optimizer, self.learning_rate, self.lr_decay, self.decay_step = optimizer, float(learning_rate), float(lr_decay), int(decay_step)
        self.max_grad_norm, self.keep_prob, self.state_noise = float(max_grad_norm), float(keep_prob), float(state_noise)
        self._cfg = train_config(config, optimizer, max_grad_norm, keep_prob)
        self.variational = bool(self._cfg.variational_recurrent)
        if wrapped is None:
            wrapped = self.variational or bool(self._cfg.wrappers.use_layer_norm) or bool(self._cfg.wrappers.use_residual)
        self._open(device, "kws_train_create_wrapped" if wrapped else "kws_train_create")
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        self.global_step = 0
        if weights is None:
            weights = _weights.init_weights(config, seed=seed)
        self.set_weights(weights)

    def _floats(self):
        """Floats of the handle's blobs: the canonical blob and, with the layer norm, every layer's ibeta and igamma behind it."""
        return self._lib.kws_weights_nbytes_wrapped(ctypes.byref(self._cfg.model), ctypes.byref(self._cfg.wrappers)) // 4

    def _drop_shape(self, b, t):
        cfg = self.config
        return (cfg.num_layers, b, cfg.hidden_size) if self.variational else (cfg.num_layers, b, t, cfg.hidden_size)

    # -- parameters --------------------------------------------------------------------------
    def save(self, path):
        _weights.save_npz(path, self.weights())

    def deploy(self, **kw):
        """rnn_ctc.DeployModel on the current parameters; kw: config overrides (precision="f16x3") and DeployModel's kernel=."""
        import copy
        from .rnn_ctc import DeployModel
        cfg = copy.copy(self.config)
        kernel = kw.pop("kernel", "auto")
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise AttributeError("unknown config key %r" % k)
            setattr(cfg, k, v)
        return DeployModel(cfg, self.weights_blob(), device=str(self.device), kernel=kernel)

    # -- compute -----------------------------------------------------------------------------
    def learning_rate_at(self, step):
        return learning_rate_at(step, self.learning_rate, self.lr_decay, self.decay_step)

    def _inputs(self, x, lengths, labels, drop, targets=None):
        import torch
        x, b, t, sl, lab, lab_len = super(Trainer, self)._inputs(x, lengths, labels, targets)
        if drop is not None:
            drop = torch.as_tensor(drop).to(device=self.device, dtype=torch.uint8).contiguous()
            if tuple(drop.shape) != self._drop_shape(b, t):
                raise _lib.InvalidArgumentError(-1, "drop must be [%s]%s, got %s" % (",".join(map(str, self._drop_shape(b, t))),
                                                    " (variational_recurrent: one mask per stream and layer)" if self.variational else "",
                                                    tuple(drop.shape)))
        return x, b, t, sl, lab, lab_len, drop

    def zero_state(self, batch):
        """[L,B,H] zeros on the trainer's device: the state every call without state= starts from."""
        import torch
        return torch.zeros(self.config.num_layers, int(batch), self.config.hidden_size, dtype=torch.float32, device=self.device)

    def _state_io(self, b, state, dstate_out, want_state):
        """-> (kws_train_state_io or None, the tensors it points to, (state_out, dstate_in) or None).  None: the plain call."""
        import torch
        if state is None and dstate_out is None and not want_state:
            return None, (), None
        shape = (self.config.num_layers, b, self.config.hidden_size)

        def given(v, name):
            if v is None:
                return None
            v = torch.as_tensor(v).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(v.shape) != shape:
                raise _lib.InvalidArgumentError(-1, "%s must be [%d,%d,%d], got %s" % ((name,) + shape + (tuple(v.shape),)))
            return v
        state, dstate_out = given(state, "state"), given(dstate_out, "dstate_out")
        outs = (torch.empty(shape, dtype=torch.float32, device=self.device), torch.empty(shape, dtype=torch.float32, device=self.device)) if want_state else None
        io = _lib.KwsTrainStateIo(state.data_ptr() if state is not None else None, outs[0].data_ptr() if outs else None,
                                  dstate_out.data_ptr() if dstate_out is not None else None, outs[1].data_ptr() if outs else None)
        return io, (state, dstate_out), outs

    def loss_and_grad(self, x, lengths, labels, drop=None, want_logits=False, state=None, dstate_out=None, want_state=False):
        """-> (loss = sum_b ctc_b / B, gradients in the dict form, per-utterance losses [B]) [, logits [B,T,C]] [, (state_out, dstate_in)];
        the parameters stay.  labels: B sequences over classes 0..C-2 (prediction.ctc_label's form), or one for all.
        state [L,B,H]: where every layer starts (None: zeros); state_out: every layer's state after frame lengths[b] - 1.  The gradients
        are those of sum_b ctc_b / B + <dstate_out, state_out> (dstate_out None: zeros) and dstate_in is that objective's gradient with
        respect to state.  A recording in two segments: (.., (sa, _)) = f(A, want_state=True); (.., gb, .., (sb, da)) = f(B, state=sa,
        want_state=True); (.., ga, .., (_, d0)) = f(A, dstate_out=da, want_state=True): ga + gb is the gradient of both losses."""
        return self._grad(x, lengths, labels, None, drop, want_logits, state, dstate_out, want_state, False)

    def loss_and_grad_frames(self, x, lengths, labels, targets, drop=None, want_logits=False, state=None, dstate_out=None, want_state=False,
                             want_frame_loss=False):
        """loss_and_grad on frame-wise targets [B,T] (kws_train_grad_frames): the per-utterance losses are ctc_weight ctc_b + frame_weight
        ce_b, the gradients those of their sum / B (+ <dstate_out, state_out>); with want_frame_loss ce [B] (device) is appended to what
        loss_and_grad returns.  labels may be None at ctc_weight 0; targets None is loss_and_grad."""
        return self._grad(x, lengths, labels, targets, drop, want_logits, state, dstate_out, want_state, want_frame_loss)

    def _grad(self, x, lengths, labels, targets, drop, want_logits, state, dstate_out, want_state, want_frame_loss):
        import torch
        x, b, t, (sl, sl_p), (lab, lab_p), (ll, ll_p), drop = self._inputs(x, lengths, labels, drop, targets)
        io, keep, outs = self._state_io(b, state, dstate_out, want_state)
        ft, keep_ft, ce = self._frames(targets, b, t, want_frame_loss)
        loss = torch.empty(b, dtype=torch.float32, device=self.device)
        grad = torch.empty(self._floats(), dtype=torch.float32, device=self.device)
        logits = torch.empty(b, t, self.config.num_classes, dtype=torch.float32, device=self.device) if want_logits else None
        with torch.cuda.device(self.device):
            if ft is not None:
                _lib.check(self._lib.kws_train_grad_frames(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]), _lib.ptr(drop),
                                                           _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(logits),
                                                           None if io is None else ctypes.byref(io), ctypes.byref(ft), self._stream()))
            elif io is None:
                _lib.check(self._lib.kws_train_grad(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]), _lib.ptr(drop),
                                                    _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(logits), self._stream()))
            else:
                _lib.check(self._lib.kws_train_grad_state(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]), _lib.ptr(drop),
                                                          _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(logits), ctypes.byref(io), self._stream()))
        per = loss.cpu().numpy()
        out = (float(per.astype(np.float64).sum() / b), _weights.from_blob(self.config, grad.cpu().numpy()), per)
        if want_logits:
            out += (logits,)
        if want_state:
            out += (outs,)
        return out + (ce,) if want_frame_loss else out

    def step_raw(self, x, lengths, labels, lr, drop=None, want_norm=False, state=None, dstate_out=None, want_state=False, targets=None):
        """One kws_train_step at learning rate lr with the given masks -> per-utterance losses [B] (device) [, global norm (device)]
        [, (state_out, dstate_in)]; state / dstate_out as loss_and_grad's: the step applies the gradient of the whole objective.
        targets [B,T]: the step of the trainer's mixed objective (kws_train_step_frames)."""
        import torch
        x, b, t, (sl, sl_p), (lab, lab_p), (ll, ll_p), drop = self._inputs(x, lengths, labels, drop, targets)
        io, keep, outs = self._state_io(b, state, dstate_out, want_state)
        ft, keep_ft, _ = self._frames(targets, b, t)
        loss = torch.empty(b, dtype=torch.float32, device=self.device)
        norm = torch.empty(1, dtype=torch.float32, device=self.device) if want_norm else None
        with torch.cuda.device(self.device):
            if ft is not None:
                _lib.check(self._lib.kws_train_step_frames(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]), _lib.ptr(drop),
                                                           float(lr), _lib.ptr(loss), _lib.ptr(norm),
                                                           None if io is None else ctypes.byref(io), ctypes.byref(ft), self._stream()))
            elif io is None:
                _lib.check(self._lib.kws_train_step(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]), _lib.ptr(drop),
                                                    float(lr), _lib.ptr(loss), _lib.ptr(norm), self._stream()))
            else:
                _lib.check(self._lib.kws_train_step_state(self._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, t, int(lab.shape[1]), _lib.ptr(drop),
                                                          float(lr), _lib.ptr(loss), _lib.ptr(norm), ctypes.byref(io), self._stream()))
        out = (loss, norm) if want_norm else (loss,)
        if want_state:
            out += (outs,)
        return out if len(out) > 1 else loss

    def apply(self, grads, lr=None):
        """One optimiser step from a gradient the caller supplies (kws_train_apply): the dict form, or a blob (numpy, or a tensor on the
        device) -- clip over it, Adam / Nesterov with the trainer's moments, the packed weights.  lr None: the scheduled rate, and
        global_step advances as in step().  -> the gradient's global norm before clipping (device, one float)."""
        import torch
        if isinstance(grads, dict):
            grads = _weights.to_blob(self.config, grads)
        g = torch.as_tensor(grads).to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        if g.numel() != self._floats():
            raise _lib.InvalidArgumentError(-1, "the gradient has %d floats, the parameters %d" % (g.numel(), self._floats()))
        scheduled = lr is None
        norm = torch.empty(1, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_train_apply(self._handle, _lib.ptr(g), float(self.learning_rate_at(self.global_step) if scheduled else lr),
                                                 _lib.ptr(norm), self._stream()))
        if scheduled:
            self.global_step += 1
        return norm

    def step(self, x, lengths, labels, state=None, want_state=False):
        """One training step as main.py runs it: input dropout on x and one output mask per layer ([L,B,T,H]; variational: [L,B,H]), both
        floor(keep_prob + U) from the trainer's own generator (keep_prob < 1 only), the scheduled learning rate, then the update
        -> loss = sum_b ctc_b / B [, state_out with want_state].  state [L,B,H]: where the layers start, e.g. the state_out of the
        step on the recording's previous chunk; without one and with state_noise > 0 it is state_noise * randn([L,B,H]), drawn from
        the same generator after the dropout draws."""
        return self.step_frames(x, lengths, labels, None, state=state, want_state=want_state)

    def step_frames(self, x, lengths, labels, targets, state=None, want_state=False):
        """step() on frame-wise targets [B,T]: the same draws, the schedule and the update of the trainer's mixed objective
        (kws_train_step_frames) -> loss = sum_b (ctc_weight ctc_b + frame_weight ce_b) / B [, state_out].  targets None is step()."""
        import torch
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32)
        drop = None
        if self.keep_prob < 1.0:
            keep = torch.floor(self.keep_prob + torch.rand(x.shape, generator=self._gen, device=self.device))
            x = x / self.keep_prob * keep           # tf.nn.dropout(inputX, keep_prob) (models/rnn_ctc.py:41-42)
            drop = torch.floor(self.keep_prob + torch.rand(self._drop_shape(x.shape[0], x.shape[1]), generator=self._gen,
                                                           device=self.device)).to(torch.uint8)
        if state is None and self.state_noise > 0.0:
            state = self.state_noise * torch.randn((self.config.num_layers, x.shape[0], self.config.hidden_size), generator=self._gen,
                                                   device=self.device)
        out = self.step_raw(x, lengths, labels, self.learning_rate_at(self.global_step), drop=drop, state=state, want_state=want_state,
                            targets=targets)
        loss = out[0] if want_state else out
        self.global_step += 1
        total = float(loss.cpu().numpy().astype(np.float64).sum() / loss.shape[0])
        return (total, out[1][0]) if want_state else total
