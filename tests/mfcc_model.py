"""fp64 numpy restatement of the reference's MFCC feature path (utils/mfcc.py:20-99) for ONE utterance -- the contract
kws_frontend_run_lengths is tested against on an MFCC handle (include/kws_amd.h).

The graph holds two float32 constants: the mel bank (tf.constant(..., dtype=tf.float32), :84) and the DCT basis (tf.cast, :93).
Both are rounded to float32 here and everything else is float64.  The mel bank is oracle.frontend_oracle.mel_basis (librosa's
Slaney bank restated; pinned by tests/test_frontend_golden.py).  top_db is None on every call site of mfcc()
(models/attention_ctc.py:250, reader.py:265,290 pass batch_size as the third argument), so there is no per-utterance maximum."""
import numpy as np

from oracle import frontend_oracle as F


def dct(n_filters, n_input):
    """utils/mfcc.py:33-42 verbatim in meaning: orthonormal DCT-II basis, returned transposed: [n_input, n_filters]."""
    basis = np.empty((n_filters, n_input))
    basis[0, :] = 1.0 / np.sqrt(n_input)                                     # :35
    samples = np.arange(1, 2 * n_input, 2) * np.pi / (2.0 * n_input)          # :37
    for i in range(1, n_filters):
        basis[i, :] = np.cos(i * samples) * np.sqrt(2.0 / n_input)           # :40
    return basis.T                                                           # :42


def power_to_db(S, amin=1e-10):
    """:20-30 with ref_value = 1 (the second term is 0) and top_db = None."""
    return 10.0 * np.log(np.maximum(amin, S)) / np.log(10.0)                 # :23


def delta_order(feat, order):
    """_delta_order (:58-69): the shift is one frame whatever `order` is; `order` only scales.  feat [T, n]."""
    head, tail = feat[:1], feat[-1:]
    subtracted = np.concatenate([feat, tail, tail], 0)                       # :62-65 (the tail tiled twice)
    subtractor = np.concatenate([head, head, feat], 0)                       # :60-61,66
    return ((subtracted - subtractor) * order)[1:1 + feat.shape[0]]          # :67-69


def delta(feat, N):
    """:45-55"""
    den = 2 * sum(i ** 2 for i in range(1, N + 1))
    return sum(delta_order(feat, i) for i in range(1, N + 1)) / den


def static_from_power(P, n_mel, n_mfcc, sr=16000, n_fft=400, fmin=300.0, fmax=8000.0):
    """power spectrum [T, 201] -> (S [T, n_mel] in dB, c [T, n_mfcc]) (:78-95)."""
    basis = F.mel_basis(sr, n_fft, n_mel, fmin, fmax).astype(np.float32).astype(np.float64)
    S = power_to_db(P @ basis.T)                                             # :87-88
    D = dct(n_mfcc, n_mel).astype(np.float32).astype(np.float64)             # :90,93
    return S, S @ D                                                          # :95


def features_from_static(c):
    """[T, n] -> [T, 3n]: [c | delta(c, 1) | delta(c, 2)] (:96-99)."""
    if c.shape[0] == 0:
        return np.zeros((0, 3 * c.shape[1]))
    return np.concatenate([c, delta(c, 1), delta(c, 2)], 1)


def mfcc(pcm, n_mel=60, n_mfcc=20, sr=16000, n_fft=400, hop=160, fmin=300.0, fmax=8000.0, with_db=False):
    """pcm [N] -> features [T, 3 n_mfcc], T = 1 + (N - n_fft) // hop frames (tf_frame: no window, no padding)."""
    fr = F.frames(np.asarray(pcm, np.float64), n_fft, hop)
    P = np.abs(np.fft.rfft(fr, n_fft, axis=-1)) ** 2                         # :77 tf.square(linearspec)
    S, c = static_from_power(P, n_mel, n_mfcc, sr, n_fft, fmin, fmax)
    out = features_from_static(c)
    return (out, S) if with_db else out


def mfcc_float32(pcm, n_mel=60, n_mfcc=20, sr=16000, n_fft=400, hop=160, fmin=300.0, fmax=8000.0):
    """The same formula evaluated in float32 on the CPU (torch.fft.rfft in float32, float32 matmuls and log): how far plain
    float32 arithmetic lands from the float64 restatement on this signal -- the yardstick of the GPU tests' tolerance."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(F.frames(np.asarray(pcm, np.float32), n_fft, hop)))
    if x.shape[0] == 0:
        return np.zeros((0, 3 * n_mfcc), np.float32)
    z = torch.fft.rfft(x, n_fft, dim=-1)
    P = z.real * z.real + z.imag * z.imag
    basis = torch.from_numpy(F.mel_basis(sr, n_fft, n_mel, fmin, fmax).astype(np.float32))
    S = 10.0 * torch.log(torch.clamp(P @ basis.T, min=1e-10)) / float(np.float32(np.log(10.0)))
    c = (S @ torch.from_numpy(dct(n_mfcc, n_mel).astype(np.float32))).numpy()
    T = c.shape[0]
    nxt, prv = c[np.minimum(np.arange(T) + 1, T - 1)], c[np.maximum(np.arange(T) - 1, 0)]
    d = nxt - prv
    return np.concatenate([c, d / np.float32(2), (d + np.float32(2) * d) / np.float32(10)], 1).astype(np.float32)


def tolerance(pcm, n_mel, n_mfcc, **kw):
    """Bound on |kernel - mfcc()| for this signal, from the restatement alone: 4 x the deviation of the float32 CPU evaluation
    (the factor covers another FFT factorisation and the MFMA summation order), and never less than the rounding of the DCT's
    own sum, n_mel * max|S| * 2^-23 * max|D|."""
    want, S = mfcc(pcm, n_mel, n_mfcc, with_db=True, **kw)
    if want.shape[0] == 0:
        return 0.0, 0.0, 0.0
    dev = float(np.abs(mfcc_float32(pcm, n_mel, n_mfcc, **kw).astype(np.float64) - want).max())
    floor = n_mel * float(np.abs(S).max()) * 2.0 ** -23 * float(np.abs(dct(n_mfcc, n_mel)).max())
    return max(4.0 * dev, floor), dev, floor
