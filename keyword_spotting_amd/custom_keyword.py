"""Customised-keyword serving -- the decision of the reference's demo server (server_demo.py:104-130) on a model with two
dense layers (README "Customize keyword": the trained [H, C] head and a second [H, C2] head on the same frozen GRU stack,
"do softmax and decode respectively").

    model = DeployModel(config, weights)          # config.num_classes2 set, weights with Wfc2 / bfc2
    hit, text = predict_ctc(model, pcm, config.label_seqs)

That is the whole-utterance form.  The streaming form -- both heads decoded per chunk in the detector loop, one stack run, a
window per head -- is detector.StreamManager(model, batch, label=..., label2=...) (device) and its host mirror
detector.HotwordDetector(model, label=..., label2=...).

Producing the second head is the README's training step -- freeze the stack and the trained head, train n new columns on about
three utterances with the CTC loss and Adam (models/rnn_ctc.py:59-101):

    weights2 = enroll(model, [mel1, mel2, mel3], ctc_label([5, 6]), n_new=2)    # one user
    enroller = Enroller(model, n_new=2, enrolments=4096, utterances_per_enrolment=3)   # thousands of users, one launch
    new_columns, new_bias, loss_trace = enroller.fit(mel, lengths, labels, steps=100)

The stack runs once (kws_step_heads: nn_outputs and head 1's logits); every optimiser step is inside kws_enroll_fit.

Whether the new words were found in those recordings, and where, before the columns go anywhere (kws_ctc_align: the best path through
the transcript, a first and last frame per label, the posterior of every label at every frame):

    found = enroller.align(mel, lengths, labels, new_columns, new_bias)     # Alignment(states, spans, score, loss, post)
    targets = frame_labels(ctc_align(logits, lengths, labels).states, labels, blank)      # frame-wise targets of any CTC model

Serving thousands of users who each enrolled their own keyword takes ONE bank of those columns on one frozen model, not a model handle
per user:

    bank = KeywordBank(model, n_new=2, capacity=4096)
    bank.set(0, new_columns, new_bias)            # device tensors straight from Enroller.fit: no host copy
    r = bank.forward(mel, state, users)           # users [B] int32: the slot of each stream (-1: no second head)
    manager = detector.StreamManager(model, batch, label="12", bank=bank, users=users, label2="56")

Users whose keyword has another word pattern, or fewer new words than the bank is wide, share that bank and that manager: a slot can
carry a keyword of its own -- a label and how many of its columns are in use --, and label2 is the pattern of the slots that have none:

    bank.set(7, columns_of_a_one_word_enroller, bias, labels=["5"])      # [count, H, 1]: padded to n_new, keyword ("5", n_used 1)
    bank.set_keyword(8, "1256")                                          # a trained word followed by the two new ones

Three clean utterances seen at every step are a narrow training set.  The reference's reader mixes a slice of background noise into
the linear spectrogram on every training step (reader.py:207-280); Enroller.fit_augmented does the same on the device, with fresh
noise per batch of optimiser steps:

    frontend = DatasetFrontend(config)                                   # a mel front-end of |X| (config.power 1)
    clean, noise = frontend.linear(utterances, n_samples), frontend.linear(noise_clips, noise_samples)
    new_columns, new_bias, loss_trace = enroller.fit_augmented(frontend, clean, noise, NoiseAugmenter(seed=1), labels, steps=100)

The CTC loss of three positive recordings never says "do not fire here".  A frame-wise target does: on every frame labelled with a
trained class or the blank the frame cross-entropy pushes the new columns' mass down (kws_enroll_fit_frames: the frame loss inside the
fit, alone or mixed with the CTC loss), in the user's own recordings and in a recording without the keyword that sits in a spare slot:

    targets = enroller.frame_targets(mel, lengths, labels, new_columns, new_bias)       # align, then frame_labels: [E*K, T]
    new_columns, new_bias, loss_trace = enroller.fit_frames(mel, lengths, labels, targets, steps=100, init=(new_columns, new_bias))
    weights2 = enroll_frames(model, [mel1, mel2, mel3], ctc_label([5, 6]), n_new=2, negatives=[mel4], negative_labels=[0, 4, 0])
"""
import collections
import copy
import ctypes

import numpy as np

from . import _lib
from . import prediction as _prediction
from . import weights as _weights
from .rnn_ctc import FEED_INPUT, FEED_STATE, FETCH_NN_OUTPUTS, FETCH_SOFTMAX1, FETCH_SOFTMAX2


def predict_ctc(model, inputX, label_seqs, decoders=_prediction):
    """server_demo.py:104-130.  One utterance `inputX` (what model/inputX:0 takes: 1-D PCM or [T, n_mel] mel) from the zero
    state -> (result, output1, output2): the two decoded [0, w, 0, ...] sequences and result = ctc_predict(output1) |
    ctc_predict(output2).  Head 1 goes through ctc_decode_strict and head 2 through ctc_decode, each called with its own class
    count, positionally as the server does -- which makes it ctc_decode's `lockout` (utils/prediction.py:18), the server's
    behaviour and kept.  `decoders`: the module the three functions come from (keyword_spotting_amd.prediction)."""
    classes1, classes2 = model.config.num_classes, model.num_classes2
    softmax1, softmax2, _ = model.run([FETCH_SOFTMAX1, FETCH_SOFTMAX2, FETCH_NN_OUTPUTS],
                                      {FEED_INPUT: inputX, FEED_STATE: model.zero_state(1)})
    output1 = decoders.ctc_decode_strict(softmax1, classes1)
    output2 = decoders.ctc_decode(softmax2, classes2)
    result = decoders.ctc_predict(output1, label_seqs) | decoders.ctc_predict(output2, label_seqs)
    return result, output1, output2


MAX_LABEL = 31        # states of the extended label: one lane of a wave each


def _pack_labels(labels, batch, what="labels"):
    """A list of `batch` label sequences (or one sequence for all) -> (labels [batch, S_max] int32, label_len [batch] int32)."""
    if len(labels) and np.ndim(labels[0]) == 0:
        labels = [labels] * batch
    if len(labels) != batch:
        raise _lib.InvalidArgumentError(-1, "%s: %d sequences for %d utterances" % (what, len(labels), batch))
    rows = [np.asarray(l, np.int64).ravel() for l in labels]
    s_max = max([len(r) for r in rows] + [1])
    out, lens = np.zeros((batch, s_max), np.int32), np.zeros(batch, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
        lens[i] = len(r)
    return out, lens


def _ints(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def ctc_loss(logits, seq_len, labels, want_grad=True):
    """kws_ctc_loss: logits [B,T,C] (device tensor or array; the blank is class C-1), seq_len [B], labels: B sequences over
    0..C-2 -> (loss [B], grad_logits [B,T,C] or None), device tensors.  torch's F.ctc_loss(log_softmax(logits), blank=C-1,
    reduction='none', zero_infinity=True) with its gradient, except that an utterance without a valid path reports loss +inf."""
    import torch
    lib = _lib.load()
    lg = torch.as_tensor(logits)
    if lg.dim() != 3:
        raise _lib.InvalidArgumentError(-1, "logits must be [B,T,C], got %s" % (tuple(lg.shape),))
    if not lg.is_cuda:
        lg = lg.to("cuda:0")
    lg = lg.to(torch.float32).contiguous()
    b, t, c = (int(v) for v in lg.shape)
    lab, lab_len = _pack_labels(labels, b)
    sl, sl_p = _ints(np.full(b, t) if seq_len is None else seq_len)
    lab, lab_p = _ints(lab)
    lab_len, lab_len_p = _ints(lab_len)
    loss = torch.empty(b, dtype=torch.float32, device=lg.device)
    grad = torch.empty_like(lg) if want_grad else None
    with torch.cuda.device(lg.device):
        _lib.check(lib.kws_ctc_loss(_lib.ptr(lg), sl_p, lab_p, lab_len_p, b, t, c, int(lab.shape[1]), _lib.ptr(loss), _lib.ptr(grad),
                                    _lib.current_stream_ptr()))
    return loss, grad


def _class_weight(class_weight, classes):
    """None, or the [classes] float32 host array of a frame loss's class weights with its pointer."""
    if class_weight is None:
        return None, None
    w = np.ascontiguousarray(class_weight, np.float32)
    if w.shape != (classes,):
        raise _lib.InvalidArgumentError(-1, "class_weight: %s for %d classes" % (w.shape, classes))
    return w, w.ctypes.data_as(ctypes.c_void_p)


def _frame_targets(targets, shape, classes, device):
    """targets [B,T] -> an int32 tensor on `device`.  A host array is range-checked here (-1: no target, else 0..classes-1) before
    it is uploaded; a device tensor is passed through unsynchronised (the kernel reports a value out of range as a NaN loss)."""
    import torch
    if isinstance(targets, torch.Tensor) and targets.is_cuda:
        t = targets.to(device=device, dtype=torch.int32).contiguous()
    else:
        a = targets.numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
        if a.shape == tuple(shape) and ((a < -1).any() or (a >= classes).any()):
            raise _lib.InvalidArgumentError(-1, "targets outside [-1,%d] (-1: no target; the blank is class %d)" % (classes - 1, classes - 1))
        t = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(device)
    if tuple(t.shape) != tuple(shape):
        raise _lib.InvalidArgumentError(-1, "targets must be [%d,%d], got %s" % (shape[0], shape[1], tuple(t.shape)))
    return t


def frame_loss(logits, seq_len, targets, class_weight=None, want_grad=True):
    """kws_frame_loss: logits [B,T,C] (device tensor or array), seq_len [B] or None, targets [B,T] (frame_labels' form: the class of
    every frame, the blank C-1 included, -1 for none; array or device tensor), class_weight [C] or None -> (loss [B], grad_logits
    [B,T,C] or None), device tensors.  Per utterance torch's F.cross_entropy(logits[:n], targets[:n], weight=class_weight,
    ignore_index=-1, reduction='mean') with its gradient, except that an utterance without a labelled frame of positive weight
    has loss 0 and gradient 0.  A target outside [-1, C) in a device tensor makes its utterance's loss NaN."""
    import torch
    lib = _lib.load()
    lg = torch.as_tensor(logits)
    if lg.dim() != 3:
        raise _lib.InvalidArgumentError(-1, "logits must be [B,T,C], got %s" % (tuple(lg.shape),))
    if not lg.is_cuda:
        lg = lg.to("cuda:0")
    lg = lg.to(torch.float32).contiguous()
    b, t, c = (int(v) for v in lg.shape)
    tg = _frame_targets(targets, (b, t), c, lg.device)
    sl, sl_p = _ints(np.full(b, t) if seq_len is None else seq_len)
    if sl.shape != (b,):
        raise _lib.InvalidArgumentError(-1, "seq_len: %s for %d utterances" % (sl.shape, b))
    w, w_p = _class_weight(class_weight, c)
    loss = torch.empty(b, dtype=torch.float32, device=lg.device)
    grad = torch.empty_like(lg) if want_grad else None
    with torch.cuda.device(lg.device):
        _lib.check(lib.kws_frame_loss(_lib.ptr(lg), sl_p, _lib.ptr(tg), w_p, b, t, c, _lib.ptr(loss), _lib.ptr(grad), _lib.current_stream_ptr()))
    return loss, grad


Alignment = collections.namedtuple("Alignment", ["states", "spans", "score", "loss", "post"])


def ctc_align(logits, seq_len, labels, want_post=False):
    """kws_ctc_align: where in each utterance the labels of its transcript lie.  logits [B,T,C] (device tensor or array; the blank is
    class C-1), seq_len [B] or None, labels: B sequences over 0..C-2 (or one for all), as ctc_loss takes them -> Alignment of device
    tensors: states [B,T] int32, the best path's state of the extended label per frame (2k+1: label k, even: a blank, -1 past
    seq_len); spans [B,S_max,2] int32, first and last frame (inclusive) of label k, -1 past the utterance's labels; score [B], the best
    path's log-probability; loss [B], ctc_loss's value bit for bit; post [B,T,S_max], the posterior of label k at frame t (None unless
    want_post).  An empty slot (seq_len 0) has score 0, loss 0; an utterance without a valid path score -inf, loss +inf; both have
    states and spans of -1 and zero posteriors."""
    import torch
    lib = _lib.load()
    lg = torch.as_tensor(logits)
    if lg.dim() != 3:
        raise _lib.InvalidArgumentError(-1, "logits must be [B,T,C], got %s" % (tuple(lg.shape),))
    if not lg.is_cuda:
        lg = lg.to("cuda:0")
    lg = lg.to(torch.float32).contiguous()
    b, t, c = (int(v) for v in lg.shape)
    lab, lab_len = _pack_labels(labels, b)
    sl, sl_p = _ints(np.full(b, t) if seq_len is None else seq_len)
    lab, lab_p = _ints(lab)
    lab_len, lab_len_p = _ints(lab_len)
    s_max = int(lab.shape[1])
    states = torch.empty(b, t, dtype=torch.int32, device=lg.device)
    spans = torch.empty(b, s_max, 2, dtype=torch.int32, device=lg.device)
    score = torch.empty(b, dtype=torch.float32, device=lg.device)
    loss = torch.empty(b, dtype=torch.float32, device=lg.device)
    post = torch.empty(b, t, s_max, dtype=torch.float32, device=lg.device) if want_post else None
    with torch.cuda.device(lg.device):
        _lib.check(lib.kws_ctc_align(_lib.ptr(lg), sl_p, lab_p, lab_len_p, b, t, c, s_max, _lib.ptr(states), _lib.ptr(spans), _lib.ptr(score),
                                     _lib.ptr(loss), _lib.ptr(post), _lib.current_stream_ptr()))
    return Alignment(states, spans, score, loss, post)


def frame_labels(states, labels, blank):
    """The frame-wise targets of an alignment (the reference README's "frame-wise label with alignment for word"): states [B,T]
    (Alignment.states, tensor or array) and the B label sequences it was made with (or one for all) -> [B,T] int32 array, the class of
    every frame: an odd state 2k+1 its label k, an even state `blank`, -1 stays -1.  Host code."""
    st = states.cpu().numpy() if hasattr(states, "cpu") else np.asarray(states)
    if st.ndim != 2:
        raise _lib.InvalidArgumentError(-1, "states must be [B,T], got %s" % (tuple(st.shape),))
    lab, lab_len = _pack_labels(labels, st.shape[0])
    if (st < -1).any() or (st > 2 * lab_len[:, None]).any():
        raise _lib.InvalidArgumentError(-1, "states outside -1..2S of their utterance's label")
    k = np.minimum(np.maximum(st, 0) // 2, lab.shape[1] - 1)
    out = np.where(st % 2 == 1, np.take_along_axis(lab, k, axis=1), np.int32(blank))
    return np.where(st < 0, -1, out).astype(np.int32)


def extend_targets(targets, C, n_new):
    """Frame-wise targets in the numbering of the trained head (C classes, blank C-1) -> the extended head's (C + n_new classes): the
    blank C-1 becomes C+n_new-1, classes 0..C-2 and -1 stay.  What a recording WITHOUT the new keyword needs before Enroller.fit_frames
    takes it in a spare slot: its transcript is aligned on head 1's own logits (ctc_align, frame_labels with blank C-1).  Host code."""
    a = targets.cpu().numpy() if hasattr(targets, "cpu") else np.asarray(targets)
    c, n = int(C), int(n_new)
    if c < 3 or n < 1 or c + n > 8:
        raise _lib.InvalidArgumentError(-1, "C=%d n_new=%d: the trained head has 3..7 classes and the extended one C + n_new <= 8" % (c, n))
    if a.dtype.kind not in "iu" or (a < -1).any() or (a >= c).any():
        raise _lib.InvalidArgumentError(-1, "targets outside [-1,%d] (-1: no target; the blank is class %d)" % (c - 1, c - 1))
    return np.where(a == c - 1, c + n - 1, a).astype(np.int32)


def truncated_normal(shape, seed=0):
    """tf.truncated_normal's distribution (models/rnn_ctc.py:266): standard normal, redrawn outside two sigma."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    bad = np.abs(x) > 2.0
    while bad.any():
        x[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(x) > 2.0
    return x.astype(np.float32)


class NoiseAugmenter(object):
    """The random variables of the reader's background-noise augmentation (reader.py:229-253) with the shipped config's values as
    defaults (config/rnn_config.py:60,69-73): per BATCH one decay ~ U[bg_decay_min_db, bg_decay_max_db) dB, one start ~ uniform integer
    in [0, max_sequence_length - T) and one Bernoulli(bg_noise_prob) that decides whether the whole batch gets noise -- drawn in that
    order, as the reader's graph lists them.  Row i is paired with noise clip i % n_noise (the reader pairs row i of the utterance
    batch with row i of the noise batch).  per_row=True draws all three per row instead: more variety from a handful of utterances.

    The draws come from a numpy.random.Generator seeded with `seed`.  TensorFlow's random stream cannot be reproduced (its kernels'
    Philox streams are keyed by graph-level and op-level seeds and by the op's position in the graph): only the distributions are the
    reader's, not the numbers."""

    def __init__(self, bg_noise_prob=0.5, bg_decay_min_db=-15, bg_decay_max_db=-5, max_sequence_length=2000, seed=0, per_row=False):
        if not 0.0 <= float(bg_noise_prob) <= 1.0:
            raise _lib.InvalidArgumentError(-1, "bg_noise_prob=%r is no probability" % (bg_noise_prob,))
        if not float(bg_decay_min_db) <= float(bg_decay_max_db):
            raise _lib.InvalidArgumentError(-1, "bg_decay_min_db=%r above bg_decay_max_db=%r" % (bg_decay_min_db, bg_decay_max_db))
        self.bg_noise_prob = float(bg_noise_prob)
        self.bg_decay_min_db, self.bg_decay_max_db = float(bg_decay_min_db), float(bg_decay_max_db)
        self.max_sequence_length, self.per_row = int(max_sequence_length), bool(per_row)
        self._rng = np.random.default_rng(seed)

    def draw(self, rows, n_noise, T):
        """-> (src, noise_index, start, gain_db), each [rows] (int32, int32, int32, float32): the row arrays of
        DatasetFrontend.augment for `rows` utterances of up to T frames and n_noise noise clips.  src is 0..rows-1; noise_index is
        i % n_noise, or -1 where the Bernoulli said no noise.  T >= max_sequence_length is refused, as tf.random_uniform refuses an
        empty range (reader.py:241-243)."""
        rows, n_noise, T = int(rows), int(n_noise), int(T)
        if rows < 1 or n_noise < 1:
            raise _lib.InvalidArgumentError(-1, "rows=%d n_noise=%d: at least one of each" % (rows, n_noise))
        if T >= self.max_sequence_length:
            raise _lib.InvalidArgumentError(-1, "T=%d frames leave no start in [0, max_sequence_length - T) with max_sequence_length=%d"
                                            % (T, self.max_sequence_length))
        n = rows if self.per_row else 1
        decay = self._rng.uniform(self.bg_decay_min_db, self.bg_decay_max_db, n)
        start = self._rng.integers(0, self.max_sequence_length - T, n)
        add = self._rng.random(n) < self.bg_noise_prob
        src = np.arange(rows, dtype=np.int32)
        noise_index = np.where(np.broadcast_to(add, (rows,)), src % n_noise, -1).astype(np.int32)
        return (src, noise_index, np.broadcast_to(start, (rows,)).astype(np.int32),
                np.broadcast_to(decay, (rows,)).astype(np.float32))


class Enroller(object):
    """E independent enrolments of K utterances each on one frozen one-head fp32 model: n_new columns [H, n_new] and their bias
    per enrolment, trained with the CTC loss and TensorFlow's Adam inside one kernel launch per fit (kws_enroll_fit).

    The frozen part comes from a heads handle of the enroller's own: the model's weights (DeployModel.weights_blob) with a
    second head whose new columns are zero -- kws_step_heads on it returns nn_outputs and head 1's logits in one stack run."""

    def __init__(self, model, n_new, enrolments=1, utterances_per_enrolment=3):
        cfg = model.config
        _frozen_model_check("Enroller", model)
        self.n_new, self.enrolments, self.slots = int(n_new), int(enrolments), int(utterances_per_enrolment)
        self.config, self.device = cfg, model.device
        self.num_classes2 = cfg.num_classes + self.n_new
        self._lib = _lib.load()
        self._handle = ctypes.c_void_p()
        import torch
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_enroll_create(cfg.hidden_size, cfg.num_classes, self.n_new, self.enrolments, self.slots,
                                                   ctypes.byref(self._handle)))
        from .rnn_ctc import DeployModel
        self.weights = _weights.from_blob(cfg, model.weights_blob)
        zeros = np.zeros((cfg.hidden_size, self.n_new), np.float32)
        self._stack = DeployModel(self.heads_config(), self.extended_weights(zeros, zeros[0]), device=str(self.device))

    def heads_config(self):
        """The model's config with num_classes2 = C + n_new: what the extended weights are served with."""
        cfg2 = copy.copy(self.config)
        cfg2.num_classes2 = self.num_classes2
        return cfg2

    def extended_weights(self, new_columns, new_bias):
        """The model's weights with the second head built from one enrolment's columns [H, n_new] and bias [n_new] (weights.extend_head)."""
        w = dict(self.weights)
        w["Wfc2"], w["bfc2"] = _weights.extend_head(w["Wfc"], w["bfc"], new_columns, new_bias)
        return w

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.kws_enroll_destroy(self._handle)
            self._handle = ctypes.c_void_p()
        if getattr(self, "_stack", None) is not None:
            self._stack.close()
            self._stack = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        """(device bytes the handle holds, device allocations since create, optimiser steps since the last fit began)."""
        nbytes, allocs, steps = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.kws_enroll_stats(self._handle, ctypes.byref(nbytes), ctypes.byref(allocs), ctypes.byref(steps)))
        return int(nbytes.value), int(allocs.value), int(steps.value)

    def features(self, inputs, lengths=None):
        """The frozen part of every step, computed once: mel [B,T,n_mel] from the zero state -> (nn_outputs [B,T,H], logits1 [B,T,C])."""
        r = self._stack.forward_heads(inputs, self._stack.zero_state(self.enrolments * self.slots), seq_len=lengths, heads=(1,),
                                      want_softmax=False)
        return r["nn_outputs"], r["head1"]["logits"]

    def fit(self, inputs, lengths, labels, steps, lr=1.5e-3, init=None, seed=0):
        """inputs: mel [E*K, T, n_mel] (enrolment e owns rows e*K .. e*K+K-1); lengths [E*K] frames (0: an empty slot) or None;
        labels: E*K sequences over the C + n_new classes of the new head (prediction.ctc_label form), or one for all; `steps` Adam
        steps at learning rate lr from `init` = (columns [E,H,n_new], bias [E,n_new]) or, None, the reference's truncated normal
        (models/rnn_ctc.py:266) with zero bias.  -> (new_columns [E,H,n_new], new_bias [E,n_new], loss_trace [steps, E*K]):
        device tensors; loss_trace[s] holds every slot's loss before step s's update."""
        return self._fit(inputs, lengths, labels, steps, lr, init, seed, None)

    def fit_frames(self, inputs, lengths, labels, targets, steps, frame_weight=1.0, ctc_weight=1.0, class_weight=None, lr=1.5e-3, init=None,
                   seed=0, want_frame_loss=False):
        """fit on frame-wise targets (kws_enroll_fit_frames): per step and slot loss = ctc_weight ctc + frame_weight ce, ce the frame
        cross-entropy (frame_loss's) of the extended head's rows.  targets [E*K, T] over the C + n_new classes of that head, -1 for no
        target -- frame_targets' form (array, range-checked here, or device tensor); class_weight [C + n_new] or None.  labels may be None
        at ctc_weight = 0, and then neither fit's limit on T nor the one on the labels applies.  inputs, lengths, steps, lr, init, seed
        and the result (new_columns, new_bias, loss_trace) are fit's; with want_frame_loss a fourth tensor [steps, E*K]: ce alone."""
        return self._fit(inputs, lengths, labels, steps, lr, init, seed, (targets, frame_weight, ctc_weight, class_weight, want_frame_loss))

    def _start(self, labels, init, seed, with_labels):
        """What both fits take from labels, init and seed: (labels [E*K,S_max], label_len [E*K]) or (None, None), and the start (columns,
        bias) on the device."""
        import torch
        e, k, h, n = self.enrolments, self.slots, self.config.hidden_size, self.n_new
        lab = lab_len = None
        if with_labels:
            lab, lab_len = _pack_labels(labels, e * k)
            if lab.shape[1] > MAX_LABEL:
                raise _lib.InvalidArgumentError(-1, "labels of up to %d entries, got %d" % (MAX_LABEL, lab.shape[1]))
        if init is None:
            init = (truncated_normal((e, h, n), seed), np.zeros((e, n), np.float32))
        wn = torch.as_tensor(init[0]).to(device=self.device, dtype=torch.float32).contiguous()
        bn = torch.as_tensor(init[1]).to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(wn.shape) != (e, h, n) or tuple(bn.shape) != (e, n):
            raise _lib.InvalidArgumentError(-1, "init must be ([%d,%d,%d], [%d,%d]), got %s %s" % (e, h, n, e, n, tuple(wn.shape), tuple(bn.shape)))
        return lab, lab_len, wn, bn

    def _frame_term(self, frames, t, steps):
        """fit_frames' (targets, frame_weight, ctc_weight, class_weight, want_frame_loss) for utterances of t frames -> (kws_frame_targets,
        what its pointers point to, the ce trace [steps, E*K] or None)."""
        import torch
        targets, frame_weight, ctc_weight, class_weight, want = frames
        b = self.enrolments * self.slots
        tg = _frame_targets(targets, (b, t), self.num_classes2, self.device)
        w, _ = _class_weight(class_weight, self.num_classes2)
        ce = torch.empty(int(steps), b, dtype=torch.float32, device=self.device) if want else None
        ft = _lib.KwsFrameTargets(tg.data_ptr(), None if w is None else w.ctypes.data, float(ctc_weight), float(frame_weight), None)
        return ft, (tg, w), ce

    def _steps(self, nn, logits1, sl_p, lab, lab_len, t, ft, ce, lr, s0, count, trace, stream):
        """`count` optimiser steps from step s0 of the fit on the handle's current state: kws_enroll_fit, or kws_enroll_fit_frames (ft)."""
        lab_p = None if lab is None else lab.ctypes.data_as(ctypes.c_void_p)
        lab_len_p = None if lab_len is None else lab_len.ctypes.data_as(ctypes.c_void_p)
        s_max = 0 if lab is None else int(lab.shape[1])
        if ft is None:
            _lib.check(self._lib.kws_enroll_fit(self._handle, _lib.ptr(nn), _lib.ptr(logits1), sl_p, lab_p, lab_len_p, t, s_max, float(lr),
                                                int(count), _lib.ptr(trace[s0:]), stream))
        else:
            ft.frame_loss = None if ce is None else ce[s0:].data_ptr()
            _lib.check(self._lib.kws_enroll_fit_frames(self._handle, _lib.ptr(nn), _lib.ptr(logits1), sl_p, lab_p, lab_len_p, t, s_max,
                                                       ctypes.byref(ft), float(lr), int(count), _lib.ptr(trace[s0:]), stream))

    def _fit(self, inputs, lengths, labels, steps, lr, init, seed, frames):
        import torch
        b = self.enrolments * self.slots
        lab, lab_len, wn, bn = self._start(labels, init, seed, frames is None or labels is not None)
        nn, logits1 = self.features(inputs, lengths)
        t = int(nn.shape[1])
        ft, keep, ce = self._frame_term(frames, t, steps) if frames is not None else (None, None, None)
        sl, sl_p = _ints(np.full(b, t) if lengths is None else torch.as_tensor(lengths).cpu().numpy())
        if lab is not None:
            lab, lab_len = np.ascontiguousarray(lab, np.int32), np.ascontiguousarray(lab_len, np.int32)
        trace = torch.empty(int(steps), b, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            stream = _lib.current_stream_ptr()
            _lib.check(self._lib.kws_enroll_set(self._handle, _lib.ptr(wn), _lib.ptr(bn), stream))
            self._steps(nn, logits1, sl_p, lab, lab_len, t, ft, ce, lr, 0, steps, trace, stream)
            out_w, out_b = torch.empty_like(wn), torch.empty_like(bn)
            _lib.check(self._lib.kws_enroll_get(self._handle, _lib.ptr(out_w), _lib.ptr(out_b), stream))
        return (out_w, out_b, trace) if ce is None else (out_w, out_b, trace, ce)

    def align(self, inputs, lengths, labels, new_columns, new_bias):
        """Where the enrolled words lie in the recordings they were enrolled from, and how sure the new head is of them: inputs,
        lengths and labels as fit takes them, new_columns [E,H,n_new] and new_bias [E,n_new] as fit returns them -> ctc_align's
        Alignment over the C + n_new classes of the new head.  The stack runs once (features); the head-2 logits are assembled as
        every fit step assembles them -- head 1's columns 0..C-2, nn_outputs . columns + bias of the row's enrolment, head 1's blank
        (a batched torch product of n_new columns: plumbing in front of the kernel) -- and aligned by kws_ctc_align."""
        import torch
        e, k, h, n = self.enrolments, self.slots, self.config.hidden_size, self.n_new
        wn = torch.as_tensor(new_columns).to(device=self.device, dtype=torch.float32)
        bn = torch.as_tensor(new_bias).to(device=self.device, dtype=torch.float32)
        if tuple(wn.shape) != (e, h, n) or tuple(bn.shape) != (e, n):
            raise _lib.InvalidArgumentError(-1, "new_columns / new_bias must be [%d,%d,%d] / [%d,%d], got %s %s"
                                            % (e, h, n, e, n, tuple(wn.shape), tuple(bn.shape)))
        nn, logits1 = self.features(inputs, lengths)
        t = int(nn.shape[1])
        new = torch.bmm(nn.reshape(e, k * t, h), wn).reshape(e * k, t, n) + bn.repeat_interleave(k, 0).unsqueeze(1)
        logits2 = torch.cat([logits1[..., :-1], new, logits1[..., -1:]], dim=-1)
        if lengths is not None:
            lengths = torch.as_tensor(lengths).cpu().numpy()
        return ctc_align(logits2, lengths, labels, want_post=True)

    def fit_augmented(self, frontend, clean, noise, augmenter, labels, steps, steps_per_batch=1, lr=1.5e-3, init=None, seed=0):
        """fit on noisy versions of the utterances, redrawn every steps_per_batch optimiser steps as the reference's training loop draws
        them per step (reader.py:207-280).  frontend: a front-end whose features are the model's mel input (DatasetFrontend /
        MelFrontend of n_mel filters); clean: frontend.linear of the E*K utterances (enrolment e owns rows e*K .. e*K+K-1; an utterance
        without frames is an empty slot); noise: frontend.linear of the noise clips; augmenter: a NoiseAugmenter.  Per batch:
        augmenter.draw -> frontend.augment -> features (the frozen stack) -> kws_enroll_fit for the batch's steps.  kws_enroll_set is
        called once, in front: Adam's moments and its step count run on across the batches.  labels, lr, init, seed and the result
        (new_columns, new_bias, loss_trace [steps, E*K]) are fit's."""
        return self._fit_augmented(frontend, clean, noise, augmenter, labels, steps, steps_per_batch, lr, init, seed, None)

    def fit_augmented_frames(self, frontend, clean, noise, augmenter, labels, targets, steps, steps_per_batch=1, frame_weight=1.0,
                             ctc_weight=1.0, class_weight=None, lr=1.5e-3, init=None, seed=0, want_frame_loss=False):
        """fit_augmented on frame-wise targets: the same loop with kws_enroll_fit_frames for every batch's steps and the SAME targets on
        every redraw -- additive noise moves no word boundary.  targets, frame_weight, ctc_weight, class_weight, want_frame_loss and the
        result are fit_frames'; everything else is fit_augmented's."""
        return self._fit_augmented(frontend, clean, noise, augmenter, labels, steps, steps_per_batch, lr, init, seed,
                                   (targets, frame_weight, ctc_weight, class_weight, want_frame_loss))

    def _fit_augmented(self, frontend, clean, noise, augmenter, labels, steps, steps_per_batch, lr, init, seed, frames):
        import torch
        e, k = self.enrolments, self.slots
        b = e * k
        steps, per = int(steps), int(steps_per_batch)
        if steps < 1 or per < 1:
            raise _lib.InvalidArgumentError(-1, "steps=%d steps_per_batch=%d: at least one of each" % (steps, per))
        if int(frontend._lib.kws_frontend_feature_size(frontend._handle)) != int(self.config.n_mel) or getattr(frontend.config, "mfcc", False):
            raise _lib.InvalidArgumentError(-1, "fit_augmented needs a front-end whose features are the model's %d mel filters" % self.config.n_mel)
        if int(clean.spec.shape[0]) != b:
            raise _lib.InvalidArgumentError(-1, "clean holds %d utterances for %d enrolments of %d slots" % (int(clean.spec.shape[0]), e, k))
        lab, lab_len, wn, bn = self._start(labels, init, seed, frames is None or labels is not None)
        t, n_noise = int(clean.spec.shape[1]), int(noise.spec.shape[0])
        ft, keep, ce = self._frame_term(frames, t, steps) if frames is not None else (None, None, None)
        frames_dev = torch.as_tensor(clean.frames).to(device=self.device, dtype=torch.int32).contiguous()
        lengths = frames_dev.cpu().numpy()          # the one host copy: kws_enroll_fit takes seq_len from host memory
        sl, sl_p = _ints(lengths)
        if lab is not None:
            lab, lab_len = np.ascontiguousarray(lab, np.int32), np.ascontiguousarray(lab_len, np.int32)
        trace = torch.empty(steps, b, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            stream = _lib.current_stream_ptr()
            _lib.check(self._lib.kws_enroll_set(self._handle, _lib.ptr(wn), _lib.ptr(bn), stream))
            for s0 in range(0, steps, per):
                src, noise_index, start, gain_db = augmenter.draw(b, n_noise, t)
                mel = frontend.augment(clean, noise, src, noise_index, start, gain_db)
                nn, logits1 = self.features(mel, frames_dev)
                self._steps(nn, logits1, sl_p, lab, lab_len, t, ft, ce, lr, s0, min(per, steps - s0), trace, stream)
            out_w, out_b = torch.empty_like(wn), torch.empty_like(bn)
            _lib.check(self._lib.kws_enroll_get(self._handle, _lib.ptr(out_w), _lib.ptr(out_b), stream))
        return (out_w, out_b, trace) if ce is None else (out_w, out_b, trace, ce)

    def frame_targets(self, inputs, lengths, labels, new_columns, new_bias):
        """The frame-wise targets of the enrolment recordings for fit_frames: align with the given columns, then frame_labels with the
        extended head's blank -> [E*K, T] int32 array over its C + n_new classes, -1 past an utterance's frames (and in a slot that is
        empty or has no valid path)."""
        found = self.align(inputs, lengths, labels, new_columns, new_bias)
        return frame_labels(found.states, labels, self.num_classes2 - 1)


def _frozen_model_check(who, model):
    """The refusals Enroller and KeywordBank share: the one-head fp32 model without relu / clip and without cell wrappers."""
    cfg = model.config
    if getattr(model, "num_classes2", 0):
        raise _lib.InvalidArgumentError(-1, "%s takes the one-head model the new head is derived from, not a model that has a second head" % who)
    if getattr(cfg, "precision", "fp32") != "fp32":
        raise _lib.UnsupportedError(_lib.KWS_ERR_UNSUPPORTED, "%s needs an fp32 model, got precision %r" % (who, cfg.precision))
    if cfg.use_relu:
        raise _lib.UnsupportedError(_lib.KWS_ERR_UNSUPPORTED, "%s: use_relu / value_clip models are out of scope (the gradient of "
                                    "TensorFlow's relu and clip at their ties is not pinned)" % who)
    if any(getattr(model, "wrappers", (False, False))):
        raise _lib.UnsupportedError(_lib.KWS_ERR_UNSUPPORTED, "%s: a second class head has no wrapped form (use_layer_norm / use_residual)" % who)


class KeywordBank(object):
    """`capacity` slots of enrolled columns [H, n_new] + bias [n_new] on the device for one frozen one-head fp32 model (kws_bank):
    stream b of a step or a stream manager projects its new classes with the columns of slot users[b].  Every slot is zero at creation.

    Like Enroller the bank builds a heads handle of its own from the model's weights (DeployModel.weights_blob) -- `stack`, whose plan
    and seams serve the bank step; its own second head (zero new columns) is never read by a bank call."""

    def __init__(self, model, n_new, capacity, kernel="auto"):
        _frozen_model_check("KeywordBank", model)
        cfg = model.config
        self.n_new, self.capacity = int(n_new), int(capacity)
        if self.n_new < 1 or cfg.num_classes + self.n_new > 8:
            raise _lib.InvalidArgumentError(-1, "n_new=%d: the extended head has num_classes + n_new <= 8 classes" % self.n_new)
        if self.capacity < 1:
            raise _lib.InvalidArgumentError(-1, "capacity=%d slots: at least one" % self.capacity)
        self.config, self.device = cfg, model.device
        self.model = model               # the one-head model the bank was built on (StreamManager / HotwordDetector check it)
        self.num_classes2 = cfg.num_classes + self.n_new
        self._lib = _lib.load()
        self._handle = ctypes.c_void_p()
        self._has_keywords = False
        import torch
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_bank_create(cfg.hidden_size, cfg.num_classes, self.n_new, self.capacity, ctypes.byref(self._handle)))
        from .rnn_ctc import DeployModel
        w = dict(_weights.from_blob(cfg, model.weights_blob))
        zeros = np.zeros((cfg.hidden_size, self.n_new), np.float32)
        w["Wfc2"], w["bfc2"] = _weights.extend_head(w["Wfc"], w["bfc"], zeros, zeros[0])
        cfg2 = copy.copy(cfg)
        cfg2.num_classes2 = self.num_classes2
        self.stack = DeployModel(cfg2, w, device=str(self.device), kernel=kernel)      # kernel: DeployModel's kernel family switch

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.kws_bank_destroy(self._handle)
            self._handle = ctypes.c_void_p()
        if getattr(self, "stack", None) is not None:
            self.stack.close()
            self.stack = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _slots(self, columns, bias):
        """-> (columns [count,H,n_new], bias [count,n_new], n_u): narrower columns [count,H,n_u] (an Enroller of fewer new words) are
        padded with zero columns."""
        import torch
        wn = torch.as_tensor(columns).to(device=self.device, dtype=torch.float32).contiguous()
        bn = torch.as_tensor(bias).to(device=self.device, dtype=torch.float32).contiguous()
        if wn.dim() == 2:
            wn, bn = wn.unsqueeze(0), bn.reshape(1, -1)
        h, n = self.config.hidden_size, self.n_new
        n_u = int(wn.shape[2]) if wn.dim() == 3 else -1
        if wn.dim() != 3 or int(wn.shape[1]) != h or not 1 <= n_u <= n or tuple(bn.shape) != (wn.shape[0], n_u):
            raise _lib.InvalidArgumentError(-1, "columns / bias must be [count,%d,%d] / [count,%d], got %s %s" % (h, n, n, tuple(wn.shape), tuple(bn.shape)))
        if n_u < n:
            wn = torch.nn.functional.pad(wn, (0, n - n_u)).contiguous()
            bn = torch.nn.functional.pad(bn, (0, n - n_u)).contiguous()
        return wn, bn, n_u

    def set(self, first, columns, bias, labels=None):
        """Slots first .. first+count-1 <- columns [count,H,n_new], bias [count,n_new] (device tensors or arrays, e.g. straight from
        Enroller.fit; one slot may come as [H,n_new], [n_new]).  Stream-ordered on the current stream (kws_bank_set).
        Columns [count,H,n_u] with n_u < n_new -- what Enroller(model, n_u).fit returns -- are padded with zero columns.  labels (count
        strings, or one for all): each slot's keyword becomes (labels[i], n_u) (set_keyword); narrower columns need them."""
        import torch
        wn, bn, n_u = self._slots(columns, bias)
        count = int(wn.shape[0])
        if labels is None and n_u != self.n_new:
            raise _lib.InvalidArgumentError(-1, "columns of %d new words in a bank of %d need labels (the slots' keywords)" % (n_u, self.n_new))
        if labels is not None:
            labels = [labels] * count if isinstance(labels, str) else [str(l) for l in labels]
            if len(labels) != count:
                raise _lib.InvalidArgumentError(-1, "labels: %d for %d slots" % (len(labels), count))
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_bank_set(self._handle, int(first), count, _lib.ptr(wn), _lib.ptr(bn), _lib.current_stream_ptr()))
        for i, label in enumerate(labels or ()):
            self.set_keyword(int(first) + i, label, n_u)
        return self

    def set_keyword(self, slot, label, n_used=None):
        """Slot `slot` gets a keyword of its own (kws_bank_set_keyword): head 2 of a stream on it has num_classes + n_used classes (n_used
        of the slot's columns, default all n_new) and its window 2 matches `label` instead of the manager's label2.  label None: back to
        no keyword of its own.  Stream-ordered.  Streams of a live manager on that slot are recycled by the caller before their next feed
        (their queued chunk summaries were built for the label before)."""
        import torch
        n_used = self.n_new if n_used is None else int(n_used)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_bank_set_keyword(self._handle, int(slot), n_used, None if label is None else str(label).encode(),
                                                      _lib.current_stream_ptr()))
        self._has_keywords = self._has_keywords or label is not None
        return self

    def keyword(self, slot):
        """-> (label or None, n_used) of the slot (kws_bank_get_keyword)."""
        n_used, own = ctypes.c_int(), ctypes.c_int()
        label = ctypes.create_string_buffer(16)
        _lib.check(self._lib.kws_bank_get_keyword(self._handle, int(slot), ctypes.byref(n_used), label, ctypes.byref(own)))
        return (label.value.decode() if own.value else None), int(n_used.value)

    def has_keywords(self):
        """A keyword was set on some slot: from then on the bank's launches take the keyword form of their kernels."""
        return self._has_keywords

    def get(self, first=0, count=None):
        """-> (columns [count,H,n_new], bias [count,n_new]) device tensors: the slots as the bank holds them (kws_bank_get)."""
        import torch
        count = self.capacity - int(first) if count is None else int(count)
        wn = torch.empty(max(count, 0), self.config.hidden_size, self.n_new, dtype=torch.float32, device=self.device)
        bn = torch.empty(max(count, 0), self.n_new, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_bank_get(self._handle, int(first), count, _lib.ptr(wn), _lib.ptr(bn), _lib.current_stream_ptr()))
        return wn, bn

    def zero_state(self, batch=1):
        return self.stack.zero_state(batch)

    def forward(self, inputs, state, users, seq_len=None, heads=(1, 2), **kw):
        """DeployModel.forward_heads with head 2 of stream b from slot users[b] (kws_step_bank): the same dict, head2 rows of
        num_classes + n_new classes.  users [B] int32, host or device; outside [0, capacity) (-1): no second head for that stream."""
        return self.stack.forward_heads(inputs, state, seq_len=seq_len, heads=heads, bank=self, users=users, **kw)


def enroll(model, utterances, label, n_new, steps=300, lr=1.5e-3, init=None, seed=0):
    """The README's single-user flow: up to four utterances (mel [T_i, n_mel] each) of the new keyword, `label` its
    prediction.ctc_label over the extended classes (the new words are classes C-1 .. C+n_new-2) -> the weights dict of the
    customised model, ready for DeployModel with config.num_classes2 = C + n_new."""
    import torch
    mels = [torch.as_tensor(u, dtype=torch.float32) for u in utterances]
    if not mels or any(m.dim() != 2 for m in mels):
        raise _lib.InvalidArgumentError(-1, "enroll takes a list of mel utterances [T, n_mel]")
    t = max(int(m.shape[0]) for m in mels)
    batch = torch.zeros(len(mels), t, int(mels[0].shape[1]))
    for i, m in enumerate(mels):
        batch[i, :m.shape[0]] = m
    enroller = Enroller(model, n_new, enrolments=1, utterances_per_enrolment=len(mels))
    try:
        wn, bn, _ = enroller.fit(batch, [int(m.shape[0]) for m in mels], list(label), steps, lr=lr, init=init, seed=seed)
        return enroller.extended_weights(wn[0].cpu().numpy(), bn[0].cpu().numpy())
    finally:
        enroller.close()


def _mel_batch(mels):
    import torch
    t = max(int(m.shape[0]) for m in mels)
    batch = torch.zeros(len(mels), t, int(mels[0].shape[1]))
    for i, m in enumerate(mels):
        batch[i, :m.shape[0]] = m
    return batch, [int(m.shape[0]) for m in mels]


def enroll_frames(model, utterances, label, n_new, negatives=(), negative_labels=(), steps=300, refit_steps=100, frame_weight=1.0,
                  ctc_weight=1.0, class_weight=None, lr=1.5e-3, init=None, seed=0):
    """enroll with a second fit on frame-wise targets, which can say "do not fire here" where the CTC loss cannot: on every frame labelled
    with a trained class or the blank -- the silence around the user's own words, and whole recordings without the keyword -- the frame
    loss pushes the new columns' softmax mass down.  utterances, label, n_new, steps, lr, init, seed: enroll's, and the first fit is
    enroll's (CTC, `steps` steps).  negatives: recordings (mel [T_i, n_mel]) that do NOT hold the keyword, negative_labels their
    transcripts over the TRAINED head's classes in prediction.ctc_label form (e.g. [0, 4, 0]; one for all, or one each); positives and
    negatives together fill at most four slots.  Then: Enroller.frame_targets for the positives (the CTC result's own alignment), ctc_align
    on head 1's logits + extend_targets for the negatives, and refit_steps steps of Enroller.fit_frames from the CTC result on all of
    them with ctc_weight / frame_weight / class_weight.  -> the weights dict of the customised model, as enroll."""
    import torch
    pos = [torch.as_tensor(u, dtype=torch.float32) for u in utterances]
    neg = [torch.as_tensor(u, dtype=torch.float32) for u in negatives]
    if not pos or any(m.dim() != 2 for m in pos + neg):
        raise _lib.InvalidArgumentError(-1, "enroll_frames takes lists of mel utterances [T, n_mel]")
    if len(pos) + len(neg) > 4:
        raise _lib.InvalidArgumentError(-1, "%d utterances and %d negatives: an enrolment has at most 4 slots" % (len(pos), len(neg)))
    neg_labels = []
    if neg:
        neg_labels = list(negative_labels)
        if neg_labels and np.ndim(neg_labels[0]) == 0:
            neg_labels = [neg_labels] * len(neg)
        if len(neg_labels) != len(neg):
            raise _lib.InvalidArgumentError(-1, "negative_labels: %d transcripts for %d negatives" % (len(neg_labels), len(neg)))
        neg_labels = [[int(v) for v in l] for l in neg_labels]
    c = model.config.num_classes
    first = Enroller(model, n_new, enrolments=1, utterances_per_enrolment=len(pos))
    both = first
    try:
        batch, lengths = _mel_batch(pos)
        labels = [[int(v) for v in label]] * len(pos)
        wn, bn, _ = first.fit(batch, lengths, labels, steps, lr=lr, init=init, seed=seed)
        targets = first.frame_targets(batch, lengths, labels, wn, bn)
        if neg:
            both = Enroller(model, n_new, enrolments=1, utterances_per_enrolment=len(pos) + len(neg))
            batch, lengths = _mel_batch(pos + neg)
            labels = labels + neg_labels
            _, logits1 = both.features(batch, lengths)
            states = ctc_align(logits1[len(pos):], lengths[len(pos):], neg_labels).states
            neg_targets = extend_targets(frame_labels(states, neg_labels, c - 1), c, n_new)
            full = np.full((len(pos) + len(neg), int(batch.shape[1])), -1, np.int32)
            full[:len(pos), :targets.shape[1]] = targets
            full[len(pos):] = neg_targets
            targets = full
        wn, bn, _ = both.fit_frames(batch, lengths, labels, targets, refit_steps, frame_weight=frame_weight, ctc_weight=ctc_weight,
                                    class_weight=class_weight, lr=lr, init=(wn, bn))
        return both.extended_weights(wn[0].cpu().numpy(), bn[0].cpu().numpy())
    finally:
        first.close()
        if both is not first:
            both.close()
