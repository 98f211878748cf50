"""fp64 numpy restatement of the features the reference's models are trained and validated on, for ONE utterance -- the contract
kws_frontend_run_lengths is tested against on a dataset handle (kws_frontend_create_dataset, include/kws_amd.h):

    process_wav.py:38-44,72-73   y = pre_emphasis(x): np.append(x[0], x[1:] - 0.97 * x[:-1]) on float32 samples
    process_wav.py:74-78         |librosa.stft(y, 400, 160)|: center=True, reflect padding of 200 samples, periodic Hann window
    reader.py:264-269            mel of |X| (config.power 1) or |X|^2 (2), or utils/mfcc.py:mfcc (config.mfcc)

The pre-emphasis is float32 arithmetic as numpy does it (the multiply and the subtract each rounded); everything behind it is
float64, with the float32-rounded mel bank and DCT basis as in tests/mfcc_model.py.  librosa itself is not available offline:
tests/test_dataset_host.py pins the framing and the window to scipy.signal.stft and transformers.audio_utils.spectrogram, and the
index formula to np.pad(mode='reflect').  np.pad's repeated reflection of a signal shorter than the pad is deliberately not
restated: an utterance of n <= 200 samples has no frames."""
import numpy as np

import mfcc_model as M
from oracle import frontend_oracle as F

N_FFT, HOP = 400, 160
KINDS = ("mel", "power", "mfcc")


def pre_emphasis(x, c=0.97):
    """float32 in, float32 out: y[0] = x[0], y[i] = x[i] - fl32(c * x[i-1]); c == 0 returns x."""
    x = np.asarray(x, np.float32)
    if not c or x.size == 0:
        return x
    return np.append(x[0], x[1:] - np.float32(c) * x[:-1]).astype(np.float32)


def num_frames(n, n_fft=N_FFT, hop=HOP):
    return 1 + n // hop if n >= n_fft // 2 + 1 else 0


def source_index(n, n_fft=N_FFT, hop=HOP):
    """[T(n), n_fft] sample index of every tap: s = hop t + i - n_fft/2, reflected once at either end."""
    s = hop * np.arange(num_frames(n, n_fft, hop))[:, None] + np.arange(n_fft)[None] - n_fft // 2
    s = np.where(s < 0, -s, s)
    return np.where(s >= n, 2 * (n - 1) - s, s)


def window(n_fft=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def frames(y, n_fft=N_FFT, hop=HOP):
    """y [n] -> windowed frames [T(n), n_fft] in the dtype of y."""
    y = np.asarray(y)
    if num_frames(y.size, n_fft, hop) == 0:
        return np.zeros((0, n_fft), y.dtype)
    return y[source_index(y.size, n_fft, hop)] * window(n_fft).astype(y.dtype)[None]


def linearspec(pcm, pre=0.0):
    """pcm [n] float32 -> |X| [T(n), 201] in float64."""
    return np.abs(np.fft.rfft(frames(pre_emphasis(pcm, pre).astype(np.float64)), N_FFT, axis=-1))


def _basis(n_mel, sr=16000, fmin=300.0, fmax=8000.0):
    return F.mel_basis(sr, N_FFT, n_mel, fmin, fmax).astype(np.float32)


def features(pcm, kind, n_mel, n_mfcc=0, pre=0.0, with_db=False):
    """pcm [n] -> [T(n), n_mel] (kind 'mel': |X|, 'power': |X|^2) or [T(n), 3 n_mfcc] ('mfcc')."""
    lin = linearspec(pcm, pre)
    if kind == "mfcc":
        S, c = M.static_from_power(lin ** 2, n_mel, n_mfcc)
        out = M.features_from_static(c)
        return (out, S) if with_db else out
    return (lin if kind == "mel" else lin ** 2) @ _basis(n_mel).astype(np.float64).T


def features_float32(pcm, kind, n_mel, n_mfcc=0, pre=0.0):
    """The same formula in float32 on the CPU (float32 window multiply, torch.fft.rfft in float32, float32 matmuls and log), as
    mfcc_model.mfcc_float32: how far plain float32 arithmetic lands from the restatement -- the yardstick of the MFCC tolerance."""
    import torch
    fr = frames(pre_emphasis(pcm, pre))
    width = 3 * n_mfcc if kind == "mfcc" else n_mel
    if fr.shape[0] == 0:
        return np.zeros((0, width), np.float32)
    z = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr.astype(np.float32))), N_FFT, dim=-1)
    P = z.real * z.real + z.imag * z.imag
    basis = torch.from_numpy(_basis(n_mel))
    if kind != "mfcc":
        return ((torch.sqrt(P) if kind == "mel" else P) @ basis.T).numpy()
    S = 10.0 * torch.log(torch.clamp(P @ basis.T, min=1e-10)) / float(np.float32(np.log(10.0)))
    c = (S @ torch.from_numpy(M.dct(n_mfcc, n_mel).astype(np.float32))).numpy()
    T = c.shape[0]
    d = c[np.minimum(np.arange(T) + 1, T - 1)] - c[np.maximum(np.arange(T) - 1, 0)]
    return np.concatenate([c, d / np.float32(2), (d + np.float32(2) * d) / np.float32(10)], 1).astype(np.float32)


def tolerance(pcm, kind, n_mel, n_mfcc=0, pre=0.0):
    """Bound on |kernel - features()| for this signal, from the restatement alone, with the constants the project already uses for
    this transform: mel of |X|: 2e-5 of the largest value (tests/test_gpu_frontend.py); of |X|^2: twice that relative bound
    (tests/test_gpu_mfcc.py: d(x^2) / x^2 = 2 dx / x); MFCC: max(4 x float32-CPU deviation, DCT floor) as mfcc_model.tolerance."""
    if kind != "mfcc":
        want = features(pcm, kind, n_mel, n_mfcc, pre)
        return (2e-5 if kind == "mel" else 4e-5) * float(np.abs(want).max()) if want.size else 0.0
    want, S = features(pcm, kind, n_mel, n_mfcc, pre, with_db=True)
    if want.shape[0] == 0:
        return 0.0
    dev = float(np.abs(features_float32(pcm, kind, n_mel, n_mfcc, pre).astype(np.float64) - want).max())
    floor = n_mel * float(np.abs(S).max()) * 2.0 ** -23 * float(np.abs(M.dct(n_mfcc, n_mel)).max())
    return max(4.0 * dev, floor)
