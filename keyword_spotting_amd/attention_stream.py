"""The self-attention CTC model on live streams (kws_attention_stream_*, include/kws_amd.h).

The model carries no state, so streaming is what detector.py:158-209 does with its queue of softmax chunks, one stage earlier: per
stream a bounded FIFO of the last `window_chunks` chunks of mel frames, cleared by the VAD on silence and by a trigger; after every
chunk the model runs over the whole window (nothing can be cached: the positional table and the whole-block layer norm tie every row
to the window's start and content) and ctc_decode2 + ctc_predict run over all of its output rows.

    manager = AttentionStreamManager(model, batch=256)             # model: attention_ctc.DeployModel, either precision
    hit = manager.feed_pcm(pcm)                                    # [B, n] float or int16 -> hit [B] int32 on the device
    hit = manager.feed_pcm(pcm, lengths)                           # stream b reads its first lengths[b] samples; 0 skips it

AttentionStreamManager is one native call per chunk, with no host work per stream.  AttentionHotwordDetector is the same loop on the
host from the public pieces -- one SimpleQueue of mel chunks per stream, kws_vad, the front-end with carry, DeployModel.forward with
lengths, ctc_decode2's batched form and ctc_predict: the specification the manager is tested against (tests/test_gpu_attention_stream.py:
identical hits, windows and carries), and the fallback for shapes the manager refuses.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .basic_vad import vad as _vad
from .detector import _recycle_mask, _stream_lengths, buf_to_float
from .prediction import ctc_predict as _ctc_predict, decode_batch
from .queue import SimpleQueue

__all__ = ["AttentionStreamManager", "AttentionHotwordDetector"]


def _pcm_chunk(pcm, batch):
    """feed_pcm's chunk -> ([B, n] tensor, is_int16); float input as float32."""
    chunk = torch.as_tensor(pcm)
    if chunk.dim() == 1:
        chunk = chunk.unsqueeze(0)
    if chunk.dim() != 2 or chunk.shape[0] != batch:
        raise _lib.InvalidArgumentError(-1, "expected PCM of shape [%d, n], got %s" % (batch, list(chunk.shape)))
    if chunk.dtype == torch.int16:
        return chunk, 1
    if chunk.dtype.is_floating_point:
        return chunk.to(torch.float32), 0
    raise _lib.InvalidArgumentError(-1, "expected float or int16 PCM, got %s" % chunk.dtype)


class AttentionStreamManager(object):
    """B live streams on one attention DeployModel: per chunk ONE native call (kws_attention_stream_feed) -- the front-end with the
    per-stream VAD gate and sample carry, the window update, the model over every stream's window, the decision; 5 + 3 L launches.
    The manager borrows the model and its front-end (model.frontend) and owns per stream the carried samples and the mel window
    (stats()['device_bytes']).  Shapes it refuses (a window longer than config.max_frames, an MFCC front-end) raise; the host mirror
    below takes them."""

    def __init__(self, model, batch, window_chunks=15, max_chunk_samples=3600, vad_thres=30, label=None, decode_thres=0.4):
        self.model, self.config, self.batch = model, model.config, int(batch)
        self.window_chunks, self.max_chunk_samples = int(window_chunks), int(max_chunk_samples)
        self.vad_thres, self.decode_thres = vad_thres, decode_thres
        self.label = self.config.label_seqs if label is None else label
        self._lib = _lib.load()
        self._handle = ctypes.c_void_p()
        self._frontend = model.frontend
        dev = model.device
        with torch.cuda.device(dev):
            _lib.check(self._lib.kws_attention_stream_create(model._handle, self._frontend._handle, self.batch, self.max_chunk_samples,
                                                             self.window_chunks, float(vad_thres), float(decode_thres),
                                                             self.label.encode(), ctypes.byref(self._handle)))
        self.chunk_frames = self._frontend.num_frames(self.config.fft_size - 1 + self.max_chunk_samples)
        self.window_frames = self.window_chunks * self.chunk_frames                  # W
        self.rows_out = model.frames_out(self.window_frames)                         # T'_max
        self.hit = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self.softmax = None

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.kws_attention_stream_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed_pcm(self, pcm, lengths=None, want_softmax=False):
        """pcm [B, n] float samples or int16 PCM (scaled by 2^-15 on the device); lengths None (every stream reads all n samples) or
        [B] integers, host or device: stream b reads its first lengths[b] samples (clamped to [0, n]) and skips the iteration when
        that is 0.  -> hit [B] int32 device tensor (1 = the label occurs in this chunk's window), or (hit, softmax [B, T'_max, C]) with
        want_softmax: the rows the decision was taken on, zeros past each stream's T'_b."""
        chunk, is_i16 = _pcm_chunk(pcm, self.batch)
        lens = None if lengths is None else _stream_lengths(lengths, self.batch)
        dev = self.model.device
        chunk = chunk.to(dev).contiguous()
        softmax = None
        if want_softmax:
            if self.softmax is None:
                self.softmax = torch.zeros(self.batch, self.rows_out, self.config.num_classes, dtype=torch.float32, device=dev)
            softmax = self.softmax
        with torch.cuda.device(dev):
            if lens is not None:
                lens = lens.to(dev, torch.int32).contiguous()              # queued on the current stream, as the feed is
            _lib.check(self._lib.kws_attention_stream_feed(self._handle, _lib.ptr(chunk), int(chunk.shape[1]), _lib.ptr(lens), is_i16,
                                                           _lib.ptr(self.hit), _lib.ptr(softmax), _lib.current_stream_ptr()))
        return (self.hit, softmax) if want_softmax else self.hit

    def recycle(self, slots):
        """A new client takes over the streams `slots` names ([B] bool / uint8 mask, or stream indices): no carried samples and an
        empty window, as a fresh manager's stream; the other streams are untouched."""
        mask = _recycle_mask(slots, self.batch).to(self.model.device).contiguous()
        with torch.cuda.device(self.model.device):
            _lib.check(self._lib.kws_attention_stream_recycle(self._handle, _lib.ptr(mask), _lib.current_stream_ptr()))
        return self

    def carry(self):
        """-> (samples [B, fft_size - 1] float32, lengths [B] int32) device tensors: the first lengths[b] of row b are carried."""
        dev = self.model.device
        samples = torch.empty(self.batch, self.config.fft_size - 1, dtype=torch.float32, device=dev)
        lengths = torch.empty(self.batch, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.kws_attention_stream_carry(self._handle, _lib.ptr(samples), _lib.ptr(lengths), _lib.current_stream_ptr()))
        return samples, lengths

    def window(self, want_mel=True):
        """-> (mel [B, W, n_mel] float32 or None, frames [B] int32, chunks [B] int32) device tensors: the first frames[b] rows of
        stream b are its window, oldest first, in chunks[b] slots."""
        dev = self.model.device
        mel = torch.empty(self.batch, self.window_frames, self.config.n_mel, dtype=torch.float32, device=dev) if want_mel else None
        frames = torch.empty(self.batch, dtype=torch.int32, device=dev)
        chunks = torch.empty(self.batch, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self._lib.kws_attention_stream_window(self._handle, _lib.ptr(mel), _lib.ptr(frames), _lib.ptr(chunks),
                                                             _lib.current_stream_ptr()))
        return mel, frames, chunks

    def stats(self):
        nbytes, launches = ctypes.c_size_t(), ctypes.c_int32()
        _lib.check(self._lib.kws_attention_stream_stats(self._handle, ctypes.byref(nbytes), ctypes.byref(launches)))
        return {"device_bytes": int(nbytes.value), "launches_last_feed": int(launches.value)}


class AttentionHotwordDetector(object):
    """The same loop on the host, stream by stream (detector.py:158-209 with the queue in front of the model): the specification of
    AttentionStreamManager, from the public pieces only.  Streams that share a chunk length (and carry length) go through kws_vad and
    the front-end together; the model and the decoder take all streams at once with their window lengths."""

    def __init__(self, model, batch, window_chunks=15, max_chunk_samples=3600, vad_thres=30, label=None, decode_thres=0.4):
        self.model, self.config, self.batch = model, model.config, int(batch)
        self.window_chunks, self.max_chunk_samples = int(window_chunks), int(max_chunk_samples)
        self.vad_thres, self.decode_thres = vad_thres, decode_thres
        self.label = self.config.label_seqs if label is None else label
        self._frontend = model.frontend
        self.res = [torch.zeros(0, dtype=torch.float32, device=model.device) for _ in range(self.batch)]     # detector.py:125
        self.queue = [SimpleQueue(self.window_chunks) for _ in range(self.batch)]
        self.hit_mask = np.zeros(self.batch, np.int32)
        self.softmax, self.rows = None, np.zeros(self.batch, np.int32)
        self.triggers = [0] * self.batch
        self.silences = [0] * self.batch

    def recycle(self, slots):
        for b in np.nonzero(_recycle_mask(slots, self.batch).cpu().numpy())[0]:
            self.res[int(b)] = self.res[int(b)][:0]
            self.queue[int(b)].clear()
        return self

    def window_frames_of(self, b):
        return sum(int(m.shape[0]) for m in self.queue[b].get_all())

    def window_of(self, b):
        """The stream's window [len_b, n_mel], oldest first."""
        parts = self.queue[b].get_all()
        if not parts:
            return torch.zeros(0, self.config.n_mel, dtype=torch.float32, device=self.model.device)
        return torch.cat(parts, 0)

    def feed_pcm(self, pcm, lengths=None, want_softmax=False):
        """As AttentionStreamManager.feed_pcm; -> hit [B] numpy int32 (or (hit, softmax [B, T', C] device tensor of this call's
        longest window, None when no stream ran the model); self.rows has every stream's decoded rows T'_b)."""
        chunk, _ = _pcm_chunk(pcm, self.batch)
        dev = self.model.device
        chunk = buf_to_float(chunk.to(dev))                                  # int16 PCM -> [-1, 1) (detector.py:74-79)
        n = int(chunk.shape[1])
        if n > self.max_chunk_samples:
            raise _lib.InvalidArgumentError(-1, "chunk of %d samples outside [0,%d]" % (n, self.max_chunk_samples))
        if lengths is None:
            lens = np.full(self.batch, n, np.int64)
        else:
            lens = np.clip(_stream_lengths(lengths, self.batch).cpu().numpy().astype(np.int64), 0, n)
        cfg = self.config
        fft, hop = int(cfg.fft_size), int(cfg.hop_size)
        live = [b for b in range(self.batch) if lens[b] > 0]                 # :164-166: an empty read is skipped
        # vad over the new samples (:168): streams of one length together
        for nb in sorted(set(int(lens[b]) for b in live)):
            idx = [b for b in live if lens[b] == nb]
            speech = _vad(chunk[idx, :nb].contiguous(), self.vad_thres).cpu().numpy()
            for i, b in enumerate(idx):
                if not speech[i]:
                    self.queue[b].clear()                                    # :171-177
                    self.silences[b] += 1
        # front-end on [carried | chunk], the new carry (:179-183): streams of one (carry, chunk) length together
        groups = {}
        for b in live:
            groups.setdefault((int(self.res[b].shape[0]), int(lens[b])), []).append(b)
        for (nc, nb), idx in sorted(groups.items()):
            data = chunk[idx, :nb].contiguous()
            carry = torch.stack([self.res[b] for b in idx], 0) if nc else None
            total = nc + nb
            if total < fft:                                                  # no frame yet: every sample is carried, an empty slot
                nxt = data if carry is None else torch.cat([carry, data], 1)
                mel = torch.zeros(len(idx), 0, cfg.n_mel, dtype=torch.float32, device=dev)
            else:
                keep = (total - fft) % hop + (fft - hop)                     # :181-182
                mel, nxt = self._frontend.forward_carry(carry, data, keep)
            for i, b in enumerate(idx):
                self.res[b] = nxt[i].clone()
                self.queue[b].add(mel[i].clone())                            # SimpleQueue.add: the oldest slot goes when full
        # the model over every live stream's window, oldest first; a skipped stream enters with length 0
        wlen = np.array([self.window_frames_of(b) if lens[b] > 0 else 0 for b in range(self.batch)], np.int32)
        self.hit_mask = np.zeros(self.batch, np.int32)
        self.rows = np.where(wlen > 0, [self.model.frames_out(int(v)) for v in wlen], 0).astype(np.int32)
        self.softmax = None
        if wlen.max() > 0:
            padded = torch.zeros(self.batch, int(wlen.max()), cfg.n_mel, dtype=torch.float32, device=dev)
            for b in range(self.batch):
                if wlen[b] > 0:
                    padded[b, :wlen[b]] = self.window_of(b)
            r = self.model.forward(padded, torch.from_numpy(wlen), want_logits=False, want_softmax=True)
            self.softmax = r["softmax"]
            words, counts = decode_batch(_lib.DECODE2, self.softmax, torch.from_numpy(self.rows), 3, self.decode_thres, 0.0)
            hits = _ctc_predict((words, counts), self.label).cpu().numpy()
            self.hit_mask = np.where(wlen > 0, hits != 0, False).astype(np.int32)
            for b in np.nonzero(self.hit_mask)[0]:
                self.triggers[int(b)] += 1
                self.queue[int(b)].clear()                                   # :203
        return (self.hit_mask, self.softmax) if want_softmax else self.hit_mask
