"""fp64 numpy restatement of the training reader's background-noise augmentation for ONE output row -- the contract
kws_frontend_run_linear / kws_frontend_augment are tested against (include/kws_amd.h):

    reader.py:325-332    compute_db: 10 log(sum(spectrum^2) / fft / fft / length) / log(10)
    reader.py:226-234    factor = 10 ** ((audio_db - noise_db + decay) / 20)
    reader.py:238-253    linearspec + (noise * factor)[start : start + T]     (the noise zero-padded to max_sequence_length)
    reader.py:264-269    mfcc(linearspec), or mel of linearspec (config.power 1) or of its square (2)

on top of tests/dataset_model.py's linearspec, mel bank and MFCC, in the reference's own log / 10 ** form.  Where the reference
would produce NaN (a noise clip without energy or without frames) the restatement follows the header's table: factor 0.  Beside it the
same formula in float32 on the CPU (augment_float32) -- the yardstick of the MFCC bound -- and tolerance()."""
import math

import numpy as np

import dataset_model as D
import mfcc_model as M

FFT = D.N_FFT


def compute_db(spectrum, length):
    """reader.py:325-332 for one utterance: spectrum [T, 201] (zero rows past `length` add nothing)."""
    energy = np.sum(np.square(np.asarray(spectrum, np.float64))) / FFT
    energy = energy / FFT / float(length)
    with np.errstate(divide="ignore"):
        return 10 * np.log(energy) / math.log(10)


def factor(clean, noise, gain_db):
    """reader.py:226-234 for one (utterance, clip) pair of spectra [T, 201], [Tn, 201], with the header's edge cases: a clip without
    frames or without energy adds no noise (the reference: NaN); an utterance without energy gives 10 ** -inf = 0."""
    if clean.shape[0] == 0 or noise.shape[0] == 0 or not np.square(noise).sum() > 0:
        return 0.0
    f = compute_db(clean, clean.shape[0]) - compute_db(noise, noise.shape[0]) + float(gain_db)
    return float(10 ** (f / 20))


def noise_slice(noise, start, T):
    """[T, 201]: rows start .. start + T of the clip, zero-padded past its end (reader.py:223-224: "already padded")."""
    start = max(int(start), 0)
    out = np.zeros((T, noise.shape[1]), np.float64)
    have = noise[start:start + T]
    out[:have.shape[0]] = have
    return out


def mix(clean, noise, start, fac):
    """reader.py:238-253: clean [T, 201] + fac * the noise slice."""
    return clean + fac * noise_slice(noise, start, clean.shape[0])


def features_of(lin, kind, n_mel, n_mfcc=0, with_db=False):
    """reader.py:264-269 on a linear spectrum [T, 201] (float64) -> [T, n_mel] or [T, 3 n_mfcc]."""
    if kind == "mfcc":
        S, c = M.static_from_power(lin ** 2, n_mel, n_mfcc)
        out = M.features_from_static(c)
        return (out, S) if with_db else out
    return (lin if kind == "mel" else lin ** 2) @ D._basis(n_mel).astype(np.float64).T


def augment(clean_pcm, noise_pcm, start, gain_db, kind, n_mel, n_mfcc=0, pre=0.0, with_db=False):
    """One row: the utterance and the clip as PCM -> (features [T, width] in float64, factor).  noise_pcm None: no noise."""
    clean = D.linearspec(clean_pcm, pre)
    if noise_pcm is None:
        fac, mixed = 0.0, clean
    else:
        noise = D.linearspec(noise_pcm, pre)
        fac = factor(clean, noise, gain_db)
        mixed = mix(clean, noise, start, fac)
    out = features_of(mixed, kind, n_mel, n_mfcc, with_db)
    return (out[0], out[1], fac) if with_db else (out, fac)


def _linearspec_float32(pcm, pre):
    import torch
    fr = D.frames(D.pre_emphasis(pcm, pre))
    if fr.shape[0] == 0:
        return torch.zeros(0, FFT // 2 + 1)
    z = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr.astype(np.float32))), FFT, dim=-1)
    return torch.sqrt(z.real * z.real + z.imag * z.imag)


def augment_float32(clean_pcm, noise_pcm, start, gain_db, kind, n_mel, n_mfcc=0, pre=0.0):
    """The same formula in float32 on the CPU (torch.fft.rfft in float32, float32 sums, log, power, mix, matmuls), as
    dataset_model.features_float32: how far plain float32 arithmetic lands from the restatement."""
    import torch
    clean = _linearspec_float32(clean_pcm, pre)
    T = clean.shape[0]
    width = 3 * n_mfcc if kind == "mfcc" else n_mel
    if T == 0:
        return np.zeros((0, width), np.float32)
    mixed = clean
    if noise_pcm is not None:
        noise = _linearspec_float32(noise_pcm, pre)
        e_n = (noise * noise).sum()
        if noise.shape[0] > 0 and float(e_n) > 0:
            ln10 = float(np.float32(math.log(10)))
            db = lambda e, n: 10 * torch.log(e / FFT / FFT / float(n)) / ln10        # noqa: E731
            f = db((clean * clean).sum(), T) - db(e_n, noise.shape[0]) + np.float32(gain_db)
            fac = torch.pow(torch.tensor(10.0), f / 20)
            sl = torch.zeros_like(clean)
            start = max(int(start), 0)
            have = noise[start:start + T]
            sl[:have.shape[0]] = have
            mixed = clean + sl * fac
    basis = torch.from_numpy(D._basis(n_mel))
    if kind != "mfcc":
        return ((mixed if kind == "mel" else mixed * mixed) @ basis.T).numpy()
    S = 10.0 * torch.log(torch.clamp((mixed * mixed) @ basis.T, min=1e-10)) / float(np.float32(np.log(10.0)))
    c = (S @ torch.from_numpy(M.dct(n_mfcc, n_mel).astype(np.float32))).numpy()
    d = c[np.minimum(np.arange(T) + 1, T - 1)] - c[np.maximum(np.arange(T) - 1, 0)]
    return np.concatenate([c, d / np.float32(2), (d + np.float32(2) * d) / np.float32(10)], 1).astype(np.float32)


SPEC_REL, ENERGY_REL = 2e-5, 4e-5        # the front-end's bound on |X| (dataset_model.tolerance, mel of |X|); on |X|^2: d(x^2)/x^2 = 2 dx/x


def tolerance(clean_pcm, noise_pcm, start, gain_db, kind, n_mel, n_mfcc=0, pre=0.0):
    """Bound on |kernel - augment()| for this row, from the restatement alone.
    mel:   2e-5 max|mel(clean)| + factor (2e-5 + 4e-5) max|mel(noise slice)| -- the two spectra's own bounds (each is linear in its
           spectrum) and the factor's relative error: factor = sqrt(E_a / E_n) ..., so half the sum of two 4e-5 energy bounds.
    power: the result is mel of mixed^2 and d(x^2) / x^2 = 2 dx / x: twice the mel bound's size RELATIVE to max|mel(mixed)|, times
           the largest value of the power result.
    mfcc:  max(4 x float32-CPU deviation, the DCT's own rounding floor), as mfcc_model.tolerance / dataset_model.tolerance."""
    if noise_pcm is None:
        return D.tolerance(clean_pcm, kind, n_mel, n_mfcc, pre)
    clean, noise = D.linearspec(clean_pcm, pre), D.linearspec(noise_pcm, pre)
    if clean.shape[0] == 0:
        return 0.0
    fac = factor(clean, noise, gain_db)
    if kind == "mfcc":
        want, S, _ = augment(clean_pcm, noise_pcm, start, gain_db, kind, n_mel, n_mfcc, pre, with_db=True)
        dev = float(np.abs(augment_float32(clean_pcm, noise_pcm, start, gain_db, kind, n_mel, n_mfcc, pre).astype(np.float64) - want).max())
        floor = n_mel * float(np.abs(S).max()) * 2.0 ** -23 * float(np.abs(M.dct(n_mfcc, n_mel)).max())
        return max(4.0 * dev, floor)
    basis = D._basis(n_mel).astype(np.float64)
    sl = noise_slice(noise, start, clean.shape[0])
    mel_tol = SPEC_REL * float(np.abs(clean @ basis.T).max()) + fac * (SPEC_REL + ENERGY_REL) * float(np.abs(sl @ basis.T).max())
    if kind == "mel":
        return mel_tol
    mixed = clean + fac * sl
    top = float(np.abs(mixed @ basis.T).max())
    return 2.0 * (mel_tol / top) * float(np.abs((mixed ** 2) @ basis.T).max()) if top > 0 else 0.0
