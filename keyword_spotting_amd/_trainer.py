"""What training.Trainer and attention_training.AttentionTrainer share: the life of a train handle, its parameters, moments and
counters, and the packing of a batch.  A trainer names its C entry points (_prefix), the module of its blob (_weights_mod) and the
config field that holds its feature dimension (_feature), and supplies _floats()."""
import ctypes

import numpy as np

from . import _lib
from .custom_keyword import _class_weight, _frame_targets, _ints, _pack_labels


def exponential_decay(learning_rate, step, decay_step, lr_decay):
    """tf.train.exponential_decay, staircase=False."""
    return float(learning_rate) * float(lr_decay) ** (float(step) / float(decay_step))


class _TrainerBase(object):
    _prefix = None            # "kws_train" / "kws_attention_train"
    _weights_mod = None       # to_blob / from_blob of the trainer's parameters
    _feature = None           # "n_mel" / "freq_size"

    def _open(self, device, create):
        """The handle that the entry point `create` makes of self._cfg on `device`."""
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.InvalidArgumentError(-1, "%s needs a CUDA/HIP device, got %s" % (type(self).__name__, device))
        self._lib = _lib.load()
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, create)(ctypes.byref(self._cfg), ctypes.byref(self._handle)))

    def _call(self, name, *args):
        """kws_[attention_]train_<name>(handle, args...) on the trainer's device."""
        import torch
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, "%s_%s" % (self._prefix, name))(self._handle, *args))

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            getattr(self._lib, self._prefix + "_destroy")(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return _lib.current_stream_ptr()

    # -- parameters --------------------------------------------------------------------------
    def set_weights(self, weights):
        """Loads parameters; zeroes the optimiser's moments and the step count of its bias corrections."""
        blob = weights if isinstance(weights, np.ndarray) else self._weights_mod.to_blob(self.config, weights)
        blob = np.ascontiguousarray(blob, np.float32)
        self._call("set_weights", blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, self._stream())

    def weights_blob(self):
        blob = np.empty(self._floats(), np.float32)
        self._call("get_weights", blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, self._stream())
        return blob

    def weights(self):
        """The current parameters in the canonical dict form (from_blob of the trainer's weights module)."""
        return self._weights_mod.from_blob(self.config, self.weights_blob())

    def moments(self):
        """(m, v) in the dict form: Adam's moments; Nesterov's accumulator and zeros."""
        n = self._floats()
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        self._call("moments", m.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p), self._stream())
        return self._weights_mod.from_blob(self.config, m), self._weights_mod.from_blob(self.config, v)

    def reserve(self, batch, frames, max_label=31):
        _lib.check(getattr(self._lib, self._prefix + "_reserve")(self._handle, int(batch), int(frames), int(max_label)))

    def stats(self):
        """dict(device_bytes, allocs, steps, launches of the last call, chunk_rows of the weight-gradient reduction)."""
        nbytes = ctypes.c_size_t()
        a, s, l, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(getattr(self._lib, self._prefix + "_stats")(self._handle, ctypes.byref(nbytes), ctypes.byref(a), ctypes.byref(s), ctypes.byref(l),
                                                                 ctypes.byref(c)))
        return dict(device_bytes=int(nbytes.value), allocs=a.value, steps=s.value, launches=l.value, chunk_rows=c.value)

    # -- frame-wise targets (kws_*_frames) ---------------------------------------------------
    def _set_objective(self, frame_weight, ctc_weight, class_weight):
        """The objective of the calls that are given targets=: loss[b] = ctc_weight ctc_b + frame_weight ce_b, ce_b the cross-entropy of
        the utterance's labelled frames under class_weight ([C] or None).  Calls without targets stay the CTC loss alone."""
        self.frame_weight, self.ctc_weight = float(frame_weight), float(ctc_weight)
        self.class_weight = _class_weight(class_weight, int(self.config.num_classes))[0]

    def _frames(self, targets, b, rows, want_frame_loss=False):
        """-> (kws_frame_targets or None for targets None, the tensors it points to, the frame_loss tensor or None).  rows: the frames
        per utterance of the logits (the attention trainer's T')."""
        import torch
        if targets is None:
            if want_frame_loss:
                raise _lib.InvalidArgumentError(-1, "want_frame_loss needs targets")
            return None, (), None
        tg = _frame_targets(targets, (b, rows), int(self.config.num_classes), self.device)
        ce = torch.empty(b, dtype=torch.float32, device=self.device) if want_frame_loss else None
        w = self.class_weight
        ft = _lib.KwsFrameTargets(tg.data_ptr(), None if w is None else w.ctypes.data, self.ctc_weight, self.frame_weight,
                                  None if ce is None else ce.data_ptr())
        return ft, (tg, w), ce

    # -- compute -----------------------------------------------------------------------------
    def _inputs(self, x, lengths, labels, targets=None):
        """-> x [B,T,F] (float32, on the device), B, T, and lengths, labels and label lengths as _ints gives them.  labels may be None
        in a call with targets whose objective has no CTC term (ctc_weight 0)."""
        import torch
        feature = getattr(self.config, self._feature)
        x = torch.as_tensor(x)
        if x.dim() != 3 or x.shape[2] != feature:
            raise _lib.InvalidArgumentError(-1, "x must be [B,T,%d], got %s" % (feature, tuple(x.shape)))
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        b, t = int(x.shape[0]), int(x.shape[1])
        if labels is None:
            if targets is None or self.ctc_weight != 0.0:
                raise _lib.InvalidArgumentError(-1, "labels may be None only with targets and ctc_weight 0")
            lab, lab_len = np.zeros((b, 1), np.int32), np.zeros(b, np.int32)
        else:
            lab, lab_len = _pack_labels(labels, b)
        sl = np.full(b, t) if lengths is None else np.asarray(lengths)
        if sl.shape != (b,):
            raise _lib.InvalidArgumentError(-1, "lengths: %s for %d utterances" % (sl.shape, b))
        return x, b, t, _ints(sl), _ints(lab), _ints(lab_len)
