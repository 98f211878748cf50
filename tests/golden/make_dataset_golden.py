"""Generates tests/golden/dataset_golden.npz: a THIRD-PARTY pin of the dataset's linear spectrogram, |librosa.stft(y, 400, 160)|
of process_wav.py:74-78 (center=True, reflect padding, periodic Hann window) behind the optional pre-emphasis of :38-44, which
tests/dataset_model.py restates.  librosa cannot be installed offline; two other implementations of the same transform stand in:

    scipy.signal.stft(np.pad(y, 200, 'reflect'), window='hann', nperseg=400, noverlap=240, boundary=None, padded=False),
        rescaled by the window sum (scipy normalises by it) -- scipy.signal.get_window('hann', 400, fftbins=True) is the very
        function librosa.filters.get_window calls
    transformers.audio_utils.spectrogram(y, get_window('hann', 400), 400, 160, 400, power=1.0, center=True, pad_mode='reflect')
        -- WITHOUT its `preemphasis` argument, which works per frame (Kaldi style): the waveform is pre-emphasised first

Neither was written by the reference's author or this repository's.  The pre-emphasis itself is process_wav.py's one numpy
expression on float32 samples and is computed here the same way.

    python tests/golden/make_dataset_golden.py            (writes the .npz next to this file)
"""
import os

import numpy as np
import scipy
import scipy.signal
import transformers
from transformers import audio_utils as A

HERE = os.path.dirname(os.path.abspath(__file__))
NFFT, HOP = 400, 160
LENGTHS = (201, 360, 1234)        # two frames that reflect on both sides; a hop boundary; eight frames with interior ones
PRE = (0.0, 0.97)


def pre_emphasis(x, c):
    return np.append(x[0], x[1:] - np.float32(c) * x[:-1]).astype(np.float32) if c else x


def scipy_linearspec(y):
    win = scipy.signal.get_window("hann", NFFT, fftbins=True)
    _, _, Z = scipy.signal.stft(np.pad(y.astype(np.float64), NFFT // 2, mode="reflect"), window="hann", nperseg=NFFT, noverlap=NFFT - HOP,
                                nfft=NFFT, boundary=None, padded=False, return_onesided=True)
    return np.abs(Z.T) * win.sum()


def transformers_linearspec(y):
    win = scipy.signal.get_window("hann", NFFT, fftbins=True)
    return A.spectrogram(y.astype(np.float64), win, NFFT, HOP, NFFT, power=1.0, center=True, pad_mode="reflect", onesided=True).T.astype(np.float64)


def main():
    rng = np.random.default_rng(20)
    out = {"transformers_version": np.array(transformers.__version__), "scipy_version": np.array(scipy.__version__),
           "window": scipy.signal.get_window("hann", NFFT, fftbins=True)}
    for n in LENGTHS:
        pcm = (rng.standard_normal(n) * 0.1).astype(np.float32)
        out["pcm_%d" % n] = pcm
        for c in PRE:
            y = pre_emphasis(pcm, c)
            out["scipy_%d_pre%g" % (n, c)] = scipy_linearspec(y)
            out["transformers_%d_pre%g" % (n, c)] = transformers_linearspec(y)
    np.savez_compressed(os.path.join(HERE, "dataset_golden.npz"), **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", None))


if __name__ == "__main__":
    main()
