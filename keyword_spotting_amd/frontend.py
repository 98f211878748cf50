"""MelFrontend -- the in-graph audio front-end of models/rnn_ctc.py:134-149 on the GPU (kws_frontend_*):
tf_frame(400, 160) -> |rfft(., 400)| -> matmul with librosa.filters.mel(...)^T, power 1, no window.
MfccFrontend -- the config.mfcc branch of models/attention_ctc.py:249-250 (utils/mfcc.py:72-99): the same frames -> |rfft|^2 -> mel
-> dB -> DCT -> [c | delta | delta-delta], a whole-utterance transform (kws_frontend_create_features / kws_frontend_run_lengths).
DatasetFrontend -- the features the models are trained and validated on (process_wav.py:38-44,69-78 -> reader.py:264-269;
server_demo.py:59-82): optional pre-emphasis -> |librosa.stft(y, 400, 160)| (centred, reflect-padded, Hann-windowed) -> mel of |X| or
|X|^2, or MFCC + deltas (kws_frontend_create_dataset / kws_frontend_run_lengths).
Every fft-400 front-end also hands out the linear spectrum and mixes background noise into it in front of its own features, as the
training reader does on every step (reader.py:207-280; kws_frontend_run_linear / kws_frontend_augment):

    clean, noise = frontend.linear(utterances, n_samples), frontend.linear(noise_clips, noise_samples)
    features = frontend.augment(clean, noise, src, noise_index, start, gain_db)        # one row per entry of src"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib


LinearSpec = collections.namedtuple("LinearSpec", ["spec", "frames", "energy"])
LinearSpec.__doc__ = """What _Frontend.linear returns, device tensors: spec [B, T_max, 201] float32 (|X|, rows past an utterance's own frame
count zero), frames [B] int32 (T_b), energy [B] float32 (the sum of spec ** 2 over the utterance: what reader.py's compute_db sums)."""


class _Frontend(object):
    """What the front-ends share: the handle and its lifetime, the mel basis, the PCM normalisation, the linear spectrum and the
    noise mix."""

    def __init__(self, config, device, create, features=None, dataset=None):
        self.config = config
        self.device = torch.device(device)
        self._lib = _lib.load()
        self._base = _lib.KwsFrontendConfig(int(config.samplerate), int(config.fft_size), int(config.hop_size),
                                            int(config.n_mel), float(config.fmin), float(config.fmax))
        self._cfg = self._base if features is None else _lib.KwsFeatureConfig(self._base, *features)
        if dataset is not None:
            self._cfg = _lib.KwsDatasetConfig(self._cfg, *dataset)
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, create)(ctypes.byref(self._cfg), ctypes.byref(self._handle)))

    def close(self):
        if getattr(self, "_handle", None) is not None and self._handle.value:
            self._lib.kws_frontend_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_frames(self, n_samples):
        return int(self._lib.kws_frontend_frames(ctypes.byref(self._base), int(n_samples)))

    def mel_basis(self):
        """[n_mel, fft/2+1] fp32 -- librosa.filters.mel layout (the graph uses its transpose)."""
        out = np.empty((self.config.n_mel, self.config.fft_size // 2 + 1), np.float32)
        _lib.check(self._lib.kws_frontend_mel_basis(self._handle, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def _pcm(self, pcm):
        """pcm [B,N] (or [N]) -> (contiguous float32 [B,N] on the device, B, N, whether it was [N])."""
        x = torch.as_tensor(pcm)
        if x.dtype != torch.float32:
            x = x.to(torch.float32)
        single = x.dim() == 1
        if single:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise _lib.InvalidArgumentError(-1, "expected signal to have rank 2 but was %d" % x.dim())
        return x.to(self.device).contiguous(), int(x.shape[0]), int(x.shape[1]), single


    def _run_lengths(self, pcm, n_samples, width):
        """kws_frontend_run_lengths: pcm [B,N] (or [N]), n_samples [B] or None -> [B,T,width] (or [T,width]), T = num_frames(N)."""
        x, b, n, single = self._pcm(pcm)
        if n_samples is not None:
            n_samples = torch.as_tensor(n_samples).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(n_samples.shape) != (b,):
                raise _lib.InvalidArgumentError(-1, "n_samples must be [%d]" % b)
        out = torch.empty(b, self.num_frames(n), width, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_frontend_run_lengths(self._handle, _lib.ptr(x), _lib.ptr(n_samples), b, n, _lib.ptr(out),
                                                          _lib.current_stream_ptr()))
        return out[0] if single else out

    def linear(self, pcm, n_samples=None):
        """kws_frontend_run_linear: pcm [B,N] (or [N]) float, n_samples [B] int32 or None (= N for all) -> LinearSpec of the B utterances
        (always batched: spec [B, num_frames(N), 201]).  Noise clips are utterances and take the same call."""
        x, b, n, _ = self._pcm(pcm)
        if n_samples is not None:
            n_samples = torch.as_tensor(n_samples).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(n_samples.shape) != (b,):
                raise _lib.InvalidArgumentError(-1, "n_samples must be [%d]" % b)
        with torch.cuda.device(self.device):
            bins = self._lib.kws_frontend_linear_size(self._handle)
            if bins < 0:
                _lib.check(bins)
            spec = torch.empty(b, max(self.num_frames(n), 0), bins, dtype=torch.float32, device=self.device)
            frames = torch.empty(b, dtype=torch.int32, device=self.device)
            energy = torch.empty(b, dtype=torch.float32, device=self.device)
            _lib.check(self._lib.kws_frontend_run_linear(self._handle, _lib.ptr(x), _lib.ptr(n_samples), b, n, _lib.ptr(spec),
                                                         _lib.ptr(frames), _lib.ptr(energy), _lib.current_stream_ptr()))
        return LinearSpec(spec, frames, energy)

    def augment(self, clean, noise, src, noise_index, start, gain_db):
        """kws_frontend_augment: clean, noise: LinearSpec (of this front-end's linear); src, noise_index, start [R] int32 and gain_db
        [R] float32 (arrays or tensors) -> this front-end's features [R, T_max, feature_size] of
            clean.spec[src[r]] + factor_r * noise.spec[noise_index[r], start[r]:start[r] + T_r]
        with factor_r the reader's 10 ** ((db(clean) - db(noise) + gain_db[r]) / 20) (reader.py:226-253).  noise_index -1: no noise for
        that row; the other edge cases are the kernel's (include/kws_amd.h)."""
        def triple(s, what):
            spec = torch.as_tensor(s.spec).to(device=self.device, dtype=torch.float32).contiguous()
            frames = torch.as_tensor(s.frames).to(device=self.device, dtype=torch.int32).contiguous()
            energy = torch.as_tensor(s.energy).to(device=self.device, dtype=torch.float32).contiguous()
            if spec.dim() != 3 or tuple(frames.shape) != (spec.shape[0],) or tuple(energy.shape) != (spec.shape[0],):
                raise _lib.InvalidArgumentError(-1, "%s must be (spec [B,T,bins], frames [B], energy [B]), got %s %s %s" %
                                                (what, tuple(spec.shape), tuple(frames.shape), tuple(energy.shape)))
            return spec, frames, energy

        with torch.cuda.device(self.device):
            bins = self._lib.kws_frontend_linear_size(self._handle)
            if bins < 0:
                _lib.check(bins)
        cs, cf, ce = triple(clean, "clean")
        ns, nf, ne = triple(noise, "noise")
        if int(cs.shape[2]) != bins or int(ns.shape[2]) != bins:
            raise _lib.InvalidArgumentError(-1, "spectra of %d bins, got %d and %d" % (bins, cs.shape[2], ns.shape[2]))
        rows = [torch.as_tensor(a).to(device=self.device, dtype=torch.int32).contiguous() for a in (src, noise_index, start)]
        rows.append(torch.as_tensor(gain_db).to(device=self.device, dtype=torch.float32).contiguous())
        r = int(rows[0].numel())
        if any(a.dim() != 1 or int(a.numel()) != r for a in rows):
            raise _lib.InvalidArgumentError(-1, "src, noise_index, start and gain_db must be [R], got %s" % ([tuple(a.shape) for a in rows],))
        with torch.cuda.device(self.device):
            width = int(self._lib.kws_frontend_feature_size(self._handle))
            out = torch.empty(r, int(cs.shape[1]), width, dtype=torch.float32, device=self.device)
            _lib.check(self._lib.kws_frontend_augment(self._handle, _lib.ptr(cs), _lib.ptr(cf), _lib.ptr(ce), int(cs.shape[0]), int(cs.shape[1]),
                                                      _lib.ptr(ns), _lib.ptr(nf), _lib.ptr(ne), int(ns.shape[0]), int(ns.shape[1]),
                                                      _lib.ptr(rows[0]), _lib.ptr(rows[1]), _lib.ptr(rows[2]), _lib.ptr(rows[3]), r,
                                                      _lib.ptr(out), _lib.current_stream_ptr()))
        return out


class MelFrontend(_Frontend):
    def __init__(self, config, device="cuda:0"):
        super(MelFrontend, self).__init__(config, device, "kws_frontend_create")

    def forward(self, pcm):
        """pcm [B,N] (or [N]) float -> mel [B,T,n_mel] (or [T,n_mel]) on the device."""
        x, b, n, single = self._pcm(pcm)
        t = self.num_frames(n)
        mel = torch.empty(b, t, self.config.n_mel, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_frontend_run(self._handle, _lib.ptr(x), b, n, _lib.ptr(mel),
                                                  _lib.current_stream_ptr()))
        return mel[0] if single else mel

    def forward_carry(self, carry, chunk, n_next):
        """Streaming form (detector.py:179-183): mel of [carry | chunk] without building the concatenation, and the
        next carry (its last n_next samples).  carry [B,n_c] or None, chunk [B,n] float32 device tensors."""
        chunk = chunk.contiguous()
        b, n = int(chunk.shape[0]), int(chunk.shape[1])
        nc = 0 if carry is None else int(carry.shape[1])
        if carry is not None:
            carry = carry.contiguous()
        t = self.num_frames(nc + n)
        mel = torch.empty(b, t, self.config.n_mel, dtype=torch.float32, device=self.device)
        nxt = torch.empty(b, int(n_next), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.kws_frontend_run_carry(self._handle, _lib.ptr(carry) if nc else None, nc, _lib.ptr(chunk), n, b,
                                                        _lib.ptr(mel), _lib.ptr(nxt), int(n_next), _lib.current_stream_ptr()))
        return mel, nxt


class MfccFrontend(_Frontend):
    """utils/mfcc.py:mfcc on B utterances of their own lengths: features [B, T_max, 3 * n_mfcc], rows past an utterance's own
    frame count zero, its delta edges at its own last frame."""

    def __init__(self, config, device="cuda:0"):
        super(MfccFrontend, self).__init__(config, device, "kws_frontend_create_features", (_lib.FEAT_MFCC, 2, int(config.n_mfcc)))

    @property
    def feature_size(self):
        return int(self._lib.kws_frontend_feature_size(self._handle))

    def dct_basis(self):
        """[n_mel, n_mfcc] fp32 -- utils/mfcc.py:dct(n_mfcc, n_mel) as the graph casts it (:93)."""
        out = np.empty((self.config.n_mel, self.config.n_mfcc), np.float32)
        _lib.check(self._lib.kws_frontend_dct_basis(self._handle, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def forward(self, pcm, n_samples=None):
        """pcm [B,N] (or [N]) float, n_samples [B] int32 or None (= N for all) -> features [B,T,3*n_mfcc] (or [T,3*n_mfcc]) on
        the device, T = num_frames(N)."""
        return self._run_lengths(pcm, n_samples, 3 * int(self.config.n_mfcc))


class DatasetFrontend(_Frontend):
    """The dataset's features of B utterances of their own lengths: [B, T_max, feature_size] with T = 1 + n // hop centred
    frames per utterance (none for n <= fft_size // 2), rows past an utterance's own frame count zero.  What the rows hold follows the
    config as reader.py:264-269 decides: config.mfcc -> MFCC + deltas (3 * n_mfcc), else mel of |X| ** config.power (n_mel).
    pre_emphasis: the coefficient, or None for config.pre_emphasis (True: 0.97, process_wav.py:38)."""

    def __init__(self, config, device="cuda:0", pre_emphasis=None):
        if pre_emphasis is None:
            pre_emphasis = getattr(config, "pre_emphasis", False)
        if pre_emphasis is True or pre_emphasis is False:
            pre_emphasis = 0.97 if pre_emphasis else 0.0
        self.pre_emphasis = float(pre_emphasis)
        if getattr(config, "mfcc", False):
            features = (_lib.FEAT_MFCC, 2, int(config.n_mfcc))
        else:
            features = (_lib.FEAT_MEL, int(getattr(config, "power", 1)), 0)
        super(DatasetFrontend, self).__init__(config, device, "kws_frontend_create_dataset", features,
                                              (_lib.FRAMES_DATASET, self.pre_emphasis))

    def num_frames(self, n_samples):
        return int(self._lib.kws_frontend_frames_of(self._handle, int(n_samples)))

    @property
    def feature_size(self):
        return int(self._lib.kws_frontend_feature_size(self._handle))

    def window(self):
        """[fft_size] fp32 -- the periodic Hann window the frames are multiplied by."""
        out = np.empty(int(self.config.fft_size), np.float32)
        _lib.check(self._lib.kws_frontend_window(self._handle, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def forward(self, pcm, n_samples=None):
        """pcm [B,N] (or [N]) float, n_samples [B] int32 or None (= N for all) -> features [B,T,feature_size] (or
        [T,feature_size]) on the device, T = num_frames(N)."""
        return self._run_lengths(pcm, n_samples, self.feature_size)
