"""Generates tests/golden/mfcc_golden.npz: a THIRD-PARTY pin of the static MFCC coefficients of utils/mfcc.py:72-95
(|rfft|^2 -> Slaney mel -> 10 log10(max(1e-10, .)) -> orthonormal DCT-II, first n_mfcc columns).

    transformers.audio_utils.spectrogram(power=2.0, log_mel="dB", mel_floor=1e-10, min_value=1e-10, reference=1.0,
                                         db_range=None, center=False, window=ones(400))
    scipy.fft.dct(type=2, norm="ortho")[:, :n_mfcc]

Neither was written by the reference's author or this repository's.  The inputs are the seven pcm_* signals of
tests/golden/frontend_golden.npz (read here, not duplicated); the mel bank is that fixture's float32-rounded one, as the graph
holds it.  Not the reference run here (TensorFlow and librosa cannot be installed): the deltas are pinned by their definition in
tests/test_mfcc_host.py only.

    python tests/golden/make_mfcc_golden.py            (writes the .npz next to this file)
"""
import os

import numpy as np
import scipy
import scipy.fft
import transformers
from transformers import audio_utils as A

HERE = os.path.dirname(os.path.abspath(__file__))
NFFT, HOP = 400, 160
SHAPES = ((60, 20), (40, 13))          # config/attention_config.py:66-67; a common 13-coefficient front-end on the 40-filter bank


def static_mfcc(pcm, fb, n_mfcc):
    s = A.spectrogram(np.asarray(pcm, np.float64), window=np.ones(NFFT), frame_length=NFFT, hop_length=HOP, fft_length=NFFT,
                      power=2.0, center=False, mel_filters=fb, mel_floor=1e-10, log_mel="dB", reference=1.0, min_value=1e-10,
                      db_range=None, dtype=np.float64)
    return scipy.fft.dct(s.T, type=2, norm="ortho", axis=-1)[:, :n_mfcc]


def main():
    src = np.load(os.path.join(HERE, "frontend_golden.npz"))
    out = {"transformers_version": np.array(transformers.__version__), "scipy_version": np.array(scipy.__version__)}
    for name in sorted(k[4:] for k in src.files if k.startswith("pcm_")):
        for n_mel, n_mfcc in SHAPES:
            fb32 = src["basis_%d" % n_mel].astype(np.float32).astype(np.float64)
            out["mfcc%d_%d_%s" % (n_mel, n_mfcc, name)] = static_mfcc(src["pcm_" + name], fb32, n_mfcc)
    np.savez_compressed(os.path.join(HERE, "mfcc_golden.npz"), **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", None))


if __name__ == "__main__":
    main()
