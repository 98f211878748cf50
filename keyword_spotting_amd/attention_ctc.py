"""DeployModel of the self-attention CTC model (models/attention_ctc.py:215-274) batched over B independent utterances, on
the HIP kernels behind kws_attention_* (include/kws_amd.h, csrc/attention_kernels.hip).

    model = DeployModel(get_attention_config(), weights)                        # precision="f16x3": the GEMMs on the fp16 matrix pipe
    r = model.forward(mel, lengths)        # mel [B, T, n_mel] -> logits / softmax [B, T', C], lengths_out [B] (T'_b)
    softmax = model.run(['model/softmax:0'], {'model/inputX:0': pcm})[0]        # the reference's 1-D PCM feed: [1, T', C]
    seqs, hits = model.decode(r["softmax"], r["lengths_out"])                      # main.py:186-191 per utterance

Each utterance's results are what the reference's batch-1 graph gives for it, whatever the other utterances and the padding.
The post-relu logits are an extension: the reference's deploy graph exports the softmax only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import attention_weights as _weights

FEED_INPUT = "model/inputX:0"
FETCH_SOFTMAX = "model/softmax:0"
FETCH_LOGIT = "model/logit:0"              # extension: the post-relu logits
FETCH_LENGTHS = "model/seq_lengths:0"      # extension: T'_b of every utterance (inference's new seqLengths)


def frames_out(config, frames):
    """T' of an utterance of `frames` mel frames (models/attention_ctc.py:78-89)."""
    c = int(config.combine_frame)
    return frames // c + 1 if c > 1 else frames


PRECISIONS = {"fp32": _lib.FP32, "f16x3": _lib.F16X3}


class DeployModel(object):
    def __init__(self, config, weights, device="cuda:0", precision="fp32"):
        """precision "fp32" (exact fp32 products) or "f16x3" (the embedding, qkv and FFN products on the fp16 matrix pipe with split
        operands: same tolerance, not bit-identical; needs |w| < 64 in every matrix)."""
        if precision not in PRECISIONS:
            raise _lib.UnsupportedError(_lib.KWS_ERR_UNSUPPORTED, "precision %r unsupported for the attention model (%s)"
                                        % (precision, ", ".join(sorted(PRECISIONS))))
        self.precision = precision
        self.config = config
        self._frontend = None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.InvalidArgumentError(-1, "DeployModel needs a CUDA/HIP device, got %s" % device)
        self._lib = _lib.load()
        blob = weights if isinstance(weights, np.ndarray) else _weights.to_blob(config, weights)
        blob = np.ascontiguousarray(blob, np.float32)
        # kws_attention_config.n_mel is the model's input width F: the mel bins, or the 3 * n_mfcc MFCC features (config.mfcc)
        self._cfg = _lib.KwsAttentionConfig(int(config.freq_size), int(config.combine_frame), int(config.hidden_size),
                                            int(config.multi_head_num), int(config.feed_forward_inner_size),
                                            int(config.num_layers), int(config.num_classes), int(bool(config.use_relu)),
                                            int(config.max_frames))
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            # "fp32" through this entry is kws_attention_create itself
            _lib.check(self._lib.kws_attention_create_precision(ctypes.byref(self._cfg), PRECISIONS[precision],
                                                                blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes,
                                                                ctypes.byref(self._handle)))

    def close(self):
        if getattr(self, "_frontend", None) is not None:
            self._frontend.close()
            self._frontend = None
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.kws_attention_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def frontend(self):
        """The in-graph audio front-end (models/attention_ctc.py:241-261; :249-250 with config.mfcc), created on first use."""
        if self._frontend is None:
            from .frontend import MelFrontend, MfccFrontend
            self._frontend = (MfccFrontend if self.config.mfcc else MelFrontend)(self.config, device=self.device)
        return self._frontend

    def frames_out(self, frames):
        return frames_out(self.config, frames)

    def reserve(self, batch, frames):
        _lib.check(self._lib.kws_attention_reserve(self._handle, int(batch), int(frames)))

    def selftest(self):
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_attention_selftest(self._handle))

    def pe_table(self):
        """The fp32 positional table [max_frames // combine_frame + 1, hidden] the handle adds to the embedding."""
        out = np.empty((self.config.max_frames // self.config.combine_frame + 1, self.config.hidden_size), np.float32)
        _lib.check(self._lib.kws_attention_pe_table(self._handle, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def forward(self, mel, lengths=None, want_logits=True, want_softmax=True, out=None):
        """mel [B, T, freq_size] (device or host; the MFCC features with config.mfcc), lengths [B] frames or None (= T) -> dict with the
        requested 'logits' and 'softmax' [B, T', C] (rows past each utterance's T'_b are 0) and 'lengths_out' [B] int32 (T'_b)."""
        cfg = self.config
        mel = self._dev(mel, torch.float32, "mel")
        if mel.dim() != 3 or mel.shape[2] != cfg.freq_size:
            raise _lib.InvalidArgumentError(-1, "mel must be [B,T,%d], got %s" % (cfg.freq_size, tuple(mel.shape)))
        b, t = int(mel.shape[0]), int(mel.shape[1])
        if lengths is not None:
            lengths = self._dev(lengths, torch.int32, "lengths")
            if tuple(lengths.shape) != (b,):
                raise _lib.InvalidArgumentError(-1, "lengths must be [%d]" % b)
        t1, c = self.frames_out(t), cfg.num_classes
        out = out or {}
        logits = out.get("logits", torch.empty(b, t1, c, dtype=torch.float32, device=self.device)) if want_logits else None
        softmax = out.get("softmax", torch.empty(b, t1, c, dtype=torch.float32, device=self.device)) if want_softmax else None
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_attention_run(self._handle, _lib.ptr(mel) if mel.numel() else None, _lib.ptr(lengths), b, t,
                                                   _lib.ptr(logits), _lib.ptr(softmax), _lib.current_stream_ptr()))
        n = torch.full((b,), t, dtype=torch.int32, device=self.device) if lengths is None else lengths.clamp(0, t)
        res = {"lengths_out": (n // cfg.combine_frame + 1 if cfg.combine_frame > 1 else n).to(torch.int32)}
        if want_logits:
            res["logits"] = logits
        if want_softmax:
            res["softmax"] = softmax
        return res

    def run(self, fetches, feed_dict):
        """tf.Session.run on the deploy graph's names.  model/inputX:0 is the reference's 1-D float PCM (framed, |rfft|, mel
        on the device, then the model): the fetches are then [1, T', C] as the graph has them.  A list of 1-D PCM arrays is a
        batch of utterances of their own lengths: [B, T'_max, C], rows past each T'_b zero (model/seq_lengths:0 has T'_b)."""
        single = isinstance(fetches, str)
        names = [fetches] if single else list(fetches)
        known = (FETCH_SOFTMAX, FETCH_LOGIT, FETCH_LENGTHS)
        for n in names:
            if n not in known:
                raise _lib.InvalidArgumentError(-1, "unknown fetch %r (graph exports %s)" % (n, ", ".join(known)))
        for k in feed_dict:
            if k != FEED_INPUT:
                raise _lib.InvalidArgumentError(-1, "unknown feed %r" % k)
        if FEED_INPUT not in feed_dict:
            raise _lib.InvalidArgumentError(-1, "feed %s is required" % FEED_INPUT)
        feed = feed_dict[FEED_INPUT]
        pcms = [torch.as_tensor(p) for p in feed] if isinstance(feed, (list, tuple)) else [torch.as_tensor(feed)]
        for p in pcms:
            if p.dim() != 1 or not p.dtype.is_floating_point:
                raise _lib.InvalidArgumentError(-1, "model/inputX:0 is a 1-D float32 PCM placeholder, got %s %s"
                                                % (p.dtype, tuple(p.shape)))
        fe = self.frontend
        n_max = max(int(p.shape[0]) for p in pcms)
        pcm = torch.zeros(len(pcms), n_max, dtype=torch.float32)
        for i, p in enumerate(pcms):
            pcm[i, :p.shape[0]] = p.to(torch.float32).cpu()
        if self.config.mfcc:
            # every utterance's own sample count: the zero-padded tail must not enter its last delta (utils/mfcc.py:58-69)
            mel = fe.forward(pcm, torch.tensor([int(p.shape[0]) for p in pcms], dtype=torch.int32))
        else:
            mel = fe.forward(pcm)                                             # [B, T, n_mel]; padding frames masked below
        frames = torch.tensor([fe.num_frames(int(p.shape[0])) for p in pcms], dtype=torch.int32)
        r = self.forward(mel, frames, want_logits=FETCH_LOGIT in names, want_softmax=FETCH_SOFTMAX in names)
        table = {FETCH_SOFTMAX: r.get("softmax"), FETCH_LOGIT: r.get("logits"), FETCH_LENGTHS: r["lengths_out"]}
        outs = [table[n] for n in names]
        return outs[0] if single else outs

    def decode(self, softmax, lengths=None, lockout=3, thres=0.5, loose_thres=0.2, label=None):
        """main.py:186-191 / :290-291 for every utterance: ctc_decode over its T'_b rows (kws_ctc_decode, KWS_DECODE), then
        ctc_predict(seq, label) (kws_ctc_predict).  -> (list of the reference's [0, w, 0, ...] arrays, hits [B] numpy int32)."""
        from . import prediction
        label = self.config.label_seqs if label is None else label
        words, counts = prediction.decode_batch(_lib.DECODE, softmax, lengths, lockout, thres, loose_thres, device=self.device)
        hits = prediction.ctc_predict((words, counts), label)
        return prediction._format(words, counts, False), hits.cpu().numpy()

    def _dev(self, x, dtype, name):
        t = torch.as_tensor(x)
        if t.dtype != dtype:
            if dtype == torch.float32 and t.dtype in (torch.float64, torch.float16, torch.bfloat16):
                t = t.to(dtype)
            elif dtype == torch.int32 and not t.dtype.is_floating_point:
                t = t.to(dtype)
            else:
                raise _lib.InvalidArgumentError(-1, "%s must be %s, got %s" % (name, dtype, t.dtype))
        if t.device != self.device:
            t = t.to(self.device)
        return t.contiguous()
