"""HotwordDetector -- the streaming state-carry loop of detector.py:104-316 without the audio I/O
(pyaudio capture, wav dumps and matplotlib plots are host I/O with no arithmetic and are out of scope).

What is reproduced, per sess.run-sized chunk and per stream:
  * zero-initialised recurrent state owned by the caller of the model (detector.py:123-124)
  * VAD gate: a silent chunk resets the state and clears the decode window BEFORE the chunk is run
    (detector.py:168-177; vad(data, 30))
  * model run with the carried state, state replaced by the returned one (detector.py:190-196)
  * 15-chunk sliding window of softmax chunks (SimpleQueue(15), detector.py:122,195,197)
  * ctc_decode2 over the whole concatenated window, ctc_predict(result, '1233') (detector.py:200-201)
  * on trigger: callback, window cleared, state reset (detector.py:202-209)
  * sample carry arithmetic between PCM chunks (detector.py:179-183) -- ChunkFramer
  * test2: chunked replay of a whole utterance, one ctc_decode at the end (detector.py:254-289)

A customised-keyword model (config.num_classes2: a second dense layer on the frozen stack, README "Customize keyword": "do
softmax and decode respectively") streams BOTH heads when label2 is given: the stack once per chunk, a window per head, each
decoded at its own threshold against its own label, the two decisions ORed (server_demo.py:122-129), and a detection of EITHER
head clears both windows and restarts the state (detector.py:202-208).  hit = hit_1 | hit_2 << 1 per stream.

B independent streams run in lock step (one kws_step per chunk for all of them); the window
bookkeeping is per stream.  feed() takes the mel variant of the graph (models/rnn_ctc.py:150-153); feed_pcm() is
the shipped graph's contract (PCM in, front-end on the device).
"""
import numpy as np
import torch

from . import _lib
from .basic_vad import vad as _vad
from .prediction import decode_batch
from .prediction import ctc_predict as _ctc_predict
from .queue import SimpleQueue


def buf_to_float(x, n_bytes=2, dtype=torch.float32):
    """detector.py:40-43 (RingBuffer.get, :74-79): little-endian signed PCM -> float in [-1, 1), scale 2^-(8n-1).
    Integer tensors stay on their device, so 16-bit PCM crosses PCIe at half the bytes and is widened there
    (exact: a power-of-two scale)."""
    x = torch.as_tensor(x)
    if x.dtype.is_floating_point:
        return x.to(dtype)
    want = {2: torch.int16, 4: torch.int32, 1: torch.int8}[n_bytes]
    if x.dtype != want:
        raise _lib.InvalidArgumentError(-1, "expected %s PCM for n_bytes=%d, got %s" % (want, n_bytes, x.dtype))
    return x.to(dtype) * (1.0 / float(1 << (8 * n_bytes - 1)))


class ChunkFramer(object):
    """Sample bookkeeping of detector.py:179-183: how many frames a PCM chunk yields once the carried
    tail of the previous chunk is prepended, and how many samples are carried forward."""

    def __init__(self, fft_size=400, hop_size=160):
        self.fft_size, self.hop_size = fft_size, hop_size
        self.carry = 0

    def push(self, n_samples):
        total = self.carry + n_samples
        frames = 0 if total < self.fft_size else (total - self.fft_size) // self.hop_size + 1
        self.carry = (total - self.fft_size) % self.hop_size + (self.fft_size - self.hop_size)
        return frames


def _second_head(model, label2, decode_thres2, decode_thres):
    """(label2, threshold 2) of a two-head detector / manager; label2 None: (None, None), the one-head loop as it always was."""
    if label2 is None:
        if decode_thres2 is not None:
            raise _lib.InvalidArgumentError(-1, "decode_thres2 needs label2")
        return None, None
    if not getattr(model, "num_classes2", 0):
        raise _lib.InvalidArgumentError(-1, "label2 needs a model with a second class head (config.num_classes2)")
    return str(label2), float(decode_thres if decode_thres2 is None else decode_thres2)


def _bank_model(model, bank, users, label2, batch):
    """(model to step, users [batch] int32 on its device) of a detector / manager whose head 2 comes from a custom_keyword.KeywordBank:
    the bank's own heads stack stands in for `model` (the same weights, a second head of num_classes + n_new classes).  `model` has to
    be the one-head model the bank was built on (bank.model), or None for "the bank's"; any other model is refused.  bank None:
    (model, None)."""
    if bank is None:
        if users is not None:
            raise _lib.InvalidArgumentError(-1, "users needs bank")
        return model, None
    if users is None or label2 is None:
        raise _lib.InvalidArgumentError(-1, "bank needs users (the slot of each stream) and label2 (the new words' pattern)")
    if model is not None and model is not getattr(bank, "model", None):
        raise _lib.InvalidArgumentError(-1, "model is not the model this bank was built on (pass bank.model, or None)")
    users = torch.as_tensor(users)
    if users.dtype.is_floating_point or tuple(users.shape) != (batch,):
        raise _lib.InvalidArgumentError(-1, "users must be [%d] integers, got %s %s" % (batch, users.dtype, list(users.shape)))
    return bank.stack, users.to(bank.device, torch.int32).contiguous()


class HotwordDetector(object):
    def __init__(self, model, batch=1, window_chunks=15, vad_thres=30, label=None, decode_thres=0.4,
                 detected_callback=None, label2=None, decode_thres2=None, bank=None, users=None):
        # head 2 per stream from a bank of enrolled columns: the host mirror of StreamManager(bank=..., users=...); a stream with
        # user -1 has all-zero softmax2 rows, which decode to nothing -- a plain detector
        model, self.users = _bank_model(model, bank, users, label2, int(batch))
        self.bank = bank
        self.model = model
        self.config = model.config
        self.batch = int(batch)
        self.vad_thres = vad_thres
        self.label = label or self.config.label_seqs
        self.decode_thres = decode_thres
        self.detected_callback = detected_callback
        self.prob_queue = [SimpleQueue(window_chunks) for _ in range(self.batch)]
        # the second head of a customised-keyword model: its own queue, label and threshold; the host mirror of StreamManager(label2=...)
        self.label2, self.decode_thres2 = _second_head(model, label2, decode_thres2, decode_thres)
        self.prob_queue2 = [SimpleQueue(window_chunks) for _ in range(self.batch)] if self.label2 is not None else None
        self.hit_mask = np.zeros(self.batch, np.int32)      # the last chunk's hit_1 | hit_2 << 1 per stream
        self.state = model.zero_state(self.batch)
        self.reset_next = torch.zeros(self.batch, dtype=torch.uint8, device=model.device)
        self.triggers = [0] * self.batch

    # detector.py:313-316 -- on the device the reset is a per-stream mask consumed by the next kws_step
    def clean_state(self, which=None):
        if which is None:
            self.reset_next.fill_(1)
        else:
            self.reset_next[which] = 1

    def feed(self, mel_chunk, pcm_chunk=None, speech=None):
        """One loop iteration of detector.py:158-209 for every stream.
        mel_chunk [B,T,n_mel] (or [T,n_mel] when batch == 1).  The VAD decision comes from `speech`
        ([B] bool) or is computed from `pcm_chunk` ([B,N]) with vad(data, vad_thres); neither -> speech.
        Returns the list of streams that triggered on this chunk."""
        mel = torch.as_tensor(mel_chunk)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        if mel.shape[0] != self.batch:
            raise _lib.InvalidArgumentError(-1, "expected %d streams, got %d" % (self.batch, mel.shape[0]))
        if speech is None and pcm_chunk is not None:
            pcm = torch.as_tensor(pcm_chunk)
            speech = _vad(pcm if pcm.dim() == 2 else pcm.unsqueeze(0), self.vad_thres).bool().cpu().numpy()
        if speech is not None:
            for b in np.nonzero(~np.asarray(speech, bool))[0]:       # :171-177
                self.clean_state(int(b))
                self.prob_queue[int(b)].clear()
                if self.prob_queue2 is not None:
                    self.prob_queue2[int(b)].clear()
        if self.label2 is not None:
            return self._feed_heads(mel)
        # (zero frames: dynamic_rnn hands the state back, clean_state() has zeroed it where the mask says so)
        r = self.model.forward(mel, self.state, reset_mask=self.reset_next, want_logits=False, want_softmax=True,
                               state_out=self.state)
        self.reset_next.zero_()
        softmax = r["softmax"]
        for b in range(self.batch):                                  # :195
            self.prob_queue[b].add(softmax[b])
        hits = self._window_hits(self.prob_queue, self.config.num_classes, self.decode_thres, self.label)
        self.hit_mask = hits.astype(np.int32)
        fired = []
        for b in np.nonzero(hits)[0]:
            b = int(b)
            fired.append(b)
            self.triggers[b] += 1
            if self.detected_callback is not None:
                self.detected_callback(b)
            self.prob_queue[b].clear()                               # :203
            self.clean_state(b)                                      # :208
        return fired

    def _window_hits(self, queues, num_classes, thres, label):
        """detector.py:197-201 for the streams of `queues`, one head: concatenate the window, ctc_decode2, ctc_predict -> [len(queues)]
        0 / 1.  Queued rows wider than num_classes are sliced to it (a bank slot's own width: the rows are zero-padded to the bank's)."""
        windows = [torch.cat(q.get_all(), 0)[:, :num_classes] for q in queues]            # :197
        lens = torch.tensor([w.shape[0] for w in windows], dtype=torch.int32)
        tmax = int(lens.max()) if len(queues) else 0
        padded = torch.zeros(len(queues), max(tmax, 1), num_classes, device=self.model.device)
        for b, w in enumerate(windows):
            padded[b, :w.shape[0]] = w
        words, counts = decode_batch(_lib.DECODE2, padded, lens, 3, thres, 0.0)   # :200
        return _ctc_predict((words, counts), label).cpu().numpy()                 # :201

    def _bank_window_hits(self):
        """Window 2 of a bank whose slots carry keywords of their own (KeywordBank.set_keyword): stream b is decoded against its slot's
        label over its slot's C + n_used classes -- at the bank's full width the slot's blank column would be read as a word class --,
        a stream on a slot without one (or without a slot) against label2 over the full width.  Streams that share both go together."""
        users = self.users.cpu().numpy()
        groups = {}
        for b in range(self.batch):
            label, n_used = self.bank.keyword(int(users[b])) if 0 <= users[b] < self.bank.capacity else (None, self.bank.n_new)
            groups.setdefault((self.label2 if label is None else label, self.config.num_classes + n_used), []).append(b)
        hits = np.zeros(self.batch, np.int64)
        for (label, classes), idx in groups.items():
            hits[idx] = self._window_hits([self.prob_queue2[b] for b in idx], classes, self.decode_thres2, label)
        return hits

    def _feed_heads(self, mel):
        """The loop body for both heads (the VAD part is done): the stack once, head k's softmax into queue k, each window decoded
        at its own threshold against its own label; a hit of either head clears both queues and restarts the state."""
        r = self.model.forward_heads(mel, self.state, reset_mask=self.reset_next, want_nn_outputs=False, want_logits=False,
                                     state_out=self.state, bank=self.bank, users=self.users)
        self.reset_next.zero_()
        sm1, sm2 = r["head1"]["softmax"], r["head2"]["softmax"]
        for b in range(self.batch):
            self.prob_queue[b].add(sm1[b])
            self.prob_queue2[b].add(sm2[b])
        hit1 = self._window_hits(self.prob_queue, self.config.num_classes, self.decode_thres, self.label)
        hit2 = self._bank_window_hits() if self.bank is not None and self.bank.has_keywords() else \
            self._window_hits(self.prob_queue2, self.model.num_classes2, self.decode_thres2, self.label2)
        self.hit_mask = (hit1 != 0).astype(np.int32) | ((hit2 != 0).astype(np.int32) << 1)
        fired = []
        for b in np.nonzero(self.hit_mask)[0]:
            b = int(b)
            fired.append(b)
            self.triggers[b] += 1
            if self.detected_callback is not None:
                self.detected_callback(b)
            self.prob_queue[b].clear()
            self.prob_queue2[b].clear()
            self.clean_state(b)
        return fired

    def feed_pcm(self, pcm_chunk, frontend):
        """The reference's real input contract (detector.py:162-193): raw PCM chunks [B,n].  Prepends the
        carried tail (:179), keeps the new tail (:181-183), runs the in-graph front-end
        (models/rnn_ctc.py:134-149, here `frontend` = keyword_spotting_amd.frontend.MelFrontend) and the
        loop body; VAD looks at the newly captured chunk only (:168)."""
        chunk = torch.as_tensor(pcm_chunk)
        if chunk.dim() == 1:
            chunk = chunk.unsqueeze(0)
        chunk = buf_to_float(chunk.to(self.model.device))             # int16 PCM -> [-1, 1) as RingBuffer.get does (:74-79)
        if not hasattr(self, "res"):
            self.res = chunk[:, :0]                                   # :125
        if chunk.shape[1] == 0:                                       # :164-166: an empty read is skipped
            self.hit_mask = np.zeros(self.batch, np.int32)
            return []
        data = torch.cat([self.res, chunk], 1)                        # :179
        fft, hop = self.config.fft_size, self.config.hop_size
        n = int(data.shape[1])
        if n < fft:
            # not a full frame yet: the reference still runs the whole iteration -- vad / clean_state / queue.clear (:168-177),
            # every sample carried (:181-183 keeps them all), sess.run over zero frames, an empty softmax into the queue (:195)
            self.res = data
            mel = torch.zeros(self.batch, 0, self.config.n_mel, device=self.model.device)
            return self.feed(mel, pcm_chunk=chunk)
        keep = (n - fft) % hop + (fft - hop)                          # :181-182
        self.res = data[:, n - keep:].contiguous()                    # :183
        mel = frontend.forward(data.contiguous())
        return self.feed(mel, pcm_chunk=chunk)

    def test(self, pcm, frontend, label=None):
        """detector.py:214-229 without the file and plot I/O: whole utterances [B,N] (or [N]) of PCM in ONE run from the
        detector's current state -- front-end, GRU stack -- then ctc_decode over the whole softmax and ctc_predict.
        Returns (hit [B] int32, (words, counts), softmax [B,T,C], logits [B,T,C]); the state is left untouched, as there."""
        x = torch.as_tensor(pcm)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        x = buf_to_float(x.to(self.model.device))
        mel = frontend.forward(x.contiguous())
        state = self.state if x.shape[0] == self.batch else self.model.zero_state(int(x.shape[0]))
        r = self.model.forward(mel, state, want_logits=True, want_softmax=True)
        decoded = decode_batch(_lib.DECODE, r["softmax"], None, 3, 0.5, 0.2)                     # :224
        return _ctc_predict(decoded, label or self.label), decoded, r["softmax"], r["logits"]    # :226

    def test2(self, mel, chunk_frames):
        """detector.py:254-289: replay whole utterances [B,T,n_mel] in chunks with the state threaded
        through, accumulate the softmax, decode once with ctc_decode.  Returns (words, counts)."""
        mel = torch.as_tensor(mel)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        mel = mel.to(self.model.device)
        state = self.model.zero_state(mel.shape[0])                  # :263
        parts, pos = [], 0
        for n in chunk_frames:
            r = self.model.forward(mel[:, pos:pos + n].contiguous(), state, want_logits=False, want_softmax=True)
            state = r["state"]                                       # :284
            parts.append(r["softmax"])                               # :285
            pos += n
        accu = torch.cat(parts, 1)
        return decode_batch(_lib.DECODE, accu, None, 3, 0.5, 0.2)    # :288


def _stream_lengths(lengths, batch):
    """feed_pcm's per-stream lengths -> a [batch] integer tensor (not yet on the device); rejects a wrong shape or dtype."""
    t = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths))
    if t.dtype == torch.bool or t.dtype.is_floating_point or t.dtype.is_complex:
        raise _lib.InvalidArgumentError(-1, "lengths must be integers, got %s" % t.dtype)
    if tuple(t.shape) != (batch,):
        raise _lib.InvalidArgumentError(-1, "lengths must have shape [%d], got %s" % (batch, list(t.shape)))
    return t


def _recycle_mask(slots, batch):
    """recycle's slots -> a [batch] uint8 mask: a bool / uint8 mask of that shape, or stream indices."""
    if isinstance(slots, torch.Tensor) and slots.dtype in (torch.bool, torch.uint8):
        if tuple(slots.shape) != (batch,):
            raise _lib.InvalidArgumentError(-1, "a slot mask must have shape [%d], got %s" % (batch, list(slots.shape)))
        return slots.to(torch.uint8)
    idx = slots.reshape(-1).cpu().tolist() if isinstance(slots, torch.Tensor) else [int(i) for i in slots]
    if any(i < 0 or i >= batch for i in idx):
        raise _lib.InvalidArgumentError(-1, "slot indices must lie in [0, %d)" % batch)
    mask = torch.zeros(batch, dtype=torch.uint8)
    mask[idx] = 1
    return mask


class StreamManager(object):
    """The same loop with every per-stream decision on the device.  feed_pcm is ONE native call
    per chunk (kws_stream_feed: VAD gate -> front-end with sample carry -> GRU stack -> 15-chunk window with windowed
    ctc_decode2 + ctc_predict, trigger -> clear + restart; the window step rides inside the last GRU layer's launch); feed
    takes mel chunks and chains kws_step and kws_window_step_incremental itself.  No per-stream host work; results are identical to HotwordDetector
    (tests/test_gpu_detector.py, tests/test_gpu_frontend.py).

    label2 (on a model with a second class head): both heads per chunk on one manager -- a second window (C = num_classes2,
    threshold decode_thres2, default decode_thres), the stack run once, ONE launch behind it for both projections, both windows
    and the coupled clear + restart (kws_stream_create_heads / kws_step_heads_window; front-end + L layers + 1 launches per chunk).
    hit carries hit_1 | hit_2 << 1: non-zero = detected.  Identical to HotwordDetector(label2=...) (tests/test_gpu_heads_stream.py).
    Without label2 the manager is what it always was, on a two-head model too: head 1 through the fused tail.

    bank (custom_keyword.KeywordBank) with users [B] and label2: per-user customised keywords on one manager -- head 2 of stream b is
    projected with the columns of bank slot users[b] (kws_stream_create_bank / kws_step_bank_window), everything else as with label2
    alone; `model` is the one-head model the bank was built on, the manager runs on the bank's own heads stack.  self.users is the
    device tensor the feeds read: rewrite users[b] in place when a slot is recycled for a new client (-1: no second head).  label2
    is the pattern of every slot without a keyword of its own: with a fixed n_new every user's new words are classes C-1 .. C+n_new-2
    over their own columns; a slot given its own label and width (KeywordBank.set_keyword) is matched against that -- the bank carries
    the keywords, the manager takes no further argument.  After set_keyword on a slot live streams use, or after moving users[b] to a
    slot with another keyword, recycle those streams before their next feed.
    Identical to HotwordDetector(bank=..., users=..., label2=...) (tests/test_gpu_bank_stream.py)."""

    def __init__(self, model, batch, window_chunks=15, max_frames=32, vad_thres=30, label=None, decode_thres=0.4, label2=None,
                 decode_thres2=None, bank=None, users=None):
        import ctypes
        model, self.users = _bank_model(model, bank, users, label2, int(batch))
        self.bank = bank
        self.model, self.config, self.batch = model, model.config, int(batch)
        self.vad_thres, self.decode_thres = vad_thres, decode_thres
        self.label = (label or self.config.label_seqs).encode()
        label2, self.decode_thres2 = _second_head(model, label2, decode_thres2, decode_thres)
        self.label2 = None if label2 is None else label2.encode()
        self._lib = _lib.load()
        # one decode window per head in use: (classes, threshold) -> handle
        heads = [(self.config.num_classes, decode_thres)] + ([(model.num_classes2, self.decode_thres2)] if self.label2 is not None else [])
        self._wins = []
        with torch.cuda.device(model.device):
            for classes, thres in heads:
                self._wins.append(ctypes.c_void_p())
                _lib.check(self._lib.kws_window_create(self.batch, int(window_chunks), int(max_frames), classes, float(thres),
                                                       ctypes.byref(self._wins[-1])))
        # the same handle objects by head, as callers outside the class name them (_win2: a null handle on a one-head manager)
        self._win, self._win2 = (self._wins + [ctypes.c_void_p()])[:2]
        dev = model.device
        self.state = model.zero_state(self.batch)
        self.restart = torch.zeros(self.batch, dtype=torch.uint8, device=dev)     # reset requested by a trigger
        self.hit = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self.max_frames = int(max_frames)
        self._stream, self._stream_frontend, self._stream_fe_handle = None, None, None

    def _close_stream(self):
        if getattr(self, "_stream", None) is not None and self._stream.value:
            self._lib.kws_stream_destroy(self._stream)
        self._stream, self._stream_frontend, self._stream_fe_handle = None, None, None

    def close(self):
        self._close_stream()
        for win in getattr(self, "_wins", None) or ():
            if win.value:
                self._lib.kws_window_destroy(win)
                win.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, mel_chunk, pcm_chunk=None, speech=None):
        """-> hit [B] int32 device tensor (1 = keyword detected on this chunk; with label2: hit_1 | hit_2 << 1)."""
        mel = torch.as_tensor(mel_chunk)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        dev = self.model.device
        if speech is None and pcm_chunk is not None:
            pcm = torch.as_tensor(pcm_chunk)
            speech = _vad(pcm if pcm.dim() == 2 else pcm.unsqueeze(0), self.vad_thres)
        if speech is None:
            silent = torch.zeros(self.batch, dtype=torch.uint8, device=dev)
        else:
            silent = (torch.as_tensor(speech).to(dev) == 0).to(torch.uint8)
        reset = torch.maximum(self.restart, silent)                       # detector.py:171-177 and :208
        if self.label2 is not None:
            return self._feed_heads(mel, reset, silent)
        r = self.model.forward(mel, self.state, reset_mask=reset, want_logits=False, want_softmax=True,
                               state_out=self.state)
        sm = r["softmax"]
        with torch.cuda.device(dev):
            # the incremental form of the window step: the state kws_stream_feed (feed_pcm) keeps, so mel-fed and PCM-fed
            # chunks may alternate on one manager
            _lib.check(self._lib.kws_window_step_incremental(self._wins[0], _lib.ptr(sm), int(sm.shape[1]), _lib.ptr(silent), self.label,
                                                             _lib.ptr(self.hit), _lib.ptr(self.restart), _lib.current_stream_ptr()))
        return self.hit

    def _feed_heads(self, mel, reset, silent):
        """One mel-fed iteration of the two-head manager (kws_step_heads_window): the stack as a heads step, then the one launch
        on both windows."""
        model, cfg = self.model, self.config
        mel = model._dev(mel, torch.float32, "mel")
        if mel.dim() != 3 or mel.shape[0] != self.batch or mel.shape[2] != cfg.n_mel:
            raise _lib.InvalidArgumentError(-1, "mel must be [%d,T,%d], got %s" % (self.batch, cfg.n_mel, tuple(mel.shape)))
        t = int(mel.shape[1])
        with torch.cuda.device(model.device):
            step = self._lib.kws_step_heads_window if self.bank is None else self._lib.kws_step_bank_window
            lead = (model._handle,) if self.bank is None else (model._handle, self.bank._handle, _lib.ptr(self.users))
            _lib.check(step(
                *lead, _lib.ptr(mel), _lib.ptr(self.state), _lib.ptr(self.state), _lib.ptr(reset), self.batch, t,
                self._wins[0], self._wins[1], self.label, self.label2, _lib.ptr(silent), None, None,
                _lib.ptr(self.hit), _lib.ptr(self.restart), _lib.current_stream_ptr()))
        return self.hit

    def feed_pcm(self, pcm_chunk, frontend, lengths=None):
        """pcm_chunk [B, n]: float samples, or int16 PCM as the sound card delivers it (widened on the device as
        buf_to_float does, detector.py:74-79).  One native call per chunk (kws_stream_feed): VAD + reset masks, the
        front-end on [carried samples | chunk] (detector.py:179-183, never concatenated), the GRU stack on the carried
        state, the window / decode / trigger step.  lengths: None (every stream reads all n samples), or a [B] integer tensor /
        sequence, host or device -- stream b reads the first lengths[b] samples of its row and skips its iteration when that is
        0 (kws_stream_feed_ragged; values outside [0, n] are clamped).  -> hit [B] int32 device tensor."""
        chunk = torch.as_tensor(pcm_chunk)
        if chunk.dim() == 1:
            chunk = chunk.unsqueeze(0)
        if chunk.shape[0] != self.batch:
            raise _lib.InvalidArgumentError(-1, "expected %d streams, got %d" % (self.batch, chunk.shape[0]))
        if chunk.dtype == torch.int16:
            is_i16 = 1
        elif chunk.dtype.is_floating_point:
            is_i16, chunk = 0, chunk.to(torch.float32)
        else:
            raise _lib.InvalidArgumentError(-1, "expected float or int16 PCM, got %s" % chunk.dtype)
        lens = None if lengths is None else _stream_lengths(lengths, self.batch)
        dev = self.model.device
        chunk = chunk.to(dev).contiguous()
        stream = self._stream_on(frontend)
        with torch.cuda.device(dev):
            if lens is None:
                _lib.check(self._lib.kws_stream_feed(stream, _lib.ptr(chunk), int(chunk.shape[1]), is_i16, _lib.ptr(self.hit),
                                                     _lib.current_stream_ptr()))
            else:
                lens = lens.to(dev, torch.int32).contiguous()         # queued on the current stream, as the feed is
                _lib.check(self._lib.kws_stream_feed_ragged(stream, _lib.ptr(chunk), int(chunk.shape[1]), _lib.ptr(lens), is_i16,
                                                            _lib.ptr(self.hit), _lib.current_stream_ptr()))
        return self.hit

    def recycle(self, slots, frontend=None):
        """A new client takes over the streams `slots` names ([B] bool / uint8 mask, or a sequence of stream indices): each
        becomes what a fresh manager's stream is -- no carried samples, zero state, empty window, no restart pending
        (kws_stream_recycle); the other streams are untouched.  The manager must have been fed PCM before, or `frontend` given."""
        mask = _recycle_mask(slots, self.batch)
        if frontend is not None:
            stream = self._stream_on(frontend)
        elif self._stream is not None:
            stream = self._stream
        else:
            raise _lib.InvalidArgumentError(-1, "recycle needs the manager's PCM stream handle: feed_pcm first, or pass frontend")
        dev = self.model.device
        mask = mask.to(dev).contiguous()
        with torch.cuda.device(dev):
            _lib.check(self._lib.kws_stream_recycle(stream, _lib.ptr(mask), _lib.current_stream_ptr()))
        return self

    def carry(self):
        """-> (samples [B, fft_size - 1] float32, lengths [B] int32) device tensors: each stream's carried samples, the first
        lengths[b] of its row (kws_stream_carry; the rest of a row is unspecified).  Needs a manager that was fed PCM."""
        if self._stream is None:
            raise _lib.InvalidArgumentError(-1, "no PCM has been fed to this manager: it carries nothing")
        dev = self.model.device
        samples = torch.empty(self.batch, self._stream_frontend.config.fft_size - 1, dtype=torch.float32, device=dev)
        lengths = torch.empty(self.batch, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.kws_stream_carry(self._stream, _lib.ptr(samples), _lib.ptr(lengths), _lib.current_stream_ptr()))
        return samples, lengths

    def _stream_on(self, frontend):
        """The native stream handle of this manager on `frontend` (created on first use, again after a front-end change)."""
        import ctypes
        dev = self.model.device
        if not self.model._handle.value or not frontend._handle.value:
            raise _lib.InvalidArgumentError(-1, "the model or the front-end has been closed")
        if self._stream is None or self._stream_frontend is not frontend or self._stream_fe_handle != frontend._handle.value:
            self._close_stream()
            self._stream = ctypes.c_void_p()
            with torch.cuda.device(dev):
                # (model, front-end, window per head, B, samples, vad, label per head, state, restart, out)
                create = self._lib.kws_stream_create if len(self._wins) == 1 else self._lib.kws_stream_create_heads
                labels = [self.label, self.label2][:len(self._wins)]
                bank = ()
                if self.bank is not None:
                    create, bank = self._lib.kws_stream_create_bank, (self.bank._handle, _lib.ptr(self.users))
                _lib.check(create(self.model._handle, frontend._handle, *self._wins, *bank, self.batch, self.max_frames * int(self.config.hop_size),
                                  float(self.vad_thres), *labels, _lib.ptr(self.state), _lib.ptr(self.restart), ctypes.byref(self._stream)))
            self._stream_frontend, self._stream_fe_handle = frontend, frontend._handle.value
        return self._stream
