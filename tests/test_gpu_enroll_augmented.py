"""Enroller.fit_augmented: enrolment on noisy versions of the utterances, redrawn per batch of optimiser steps as the reference's
training loop draws them (reader.py:207-280).  Nothing here has a tolerance: without noise it is Enroller.fit on the front-end's own
mel, and with noise it is the loop of the public pieces (NoiseAugmenter.draw, DatasetFrontend.augment, Enroller.features, kws_enroll_set /
_fit / _get) written out below -- bit for bit.  The mix itself is checked in tests/test_gpu_augment.py.

Model: hidden 128, 2 layers, 6 classes; 2 new words, E = 2 enrolments of K = 3 utterances, 20 steps."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, K, N_NEW, STEPS, LR = 2, 3, 2, 20, 0.03
N_MAX, LENS = 4000, (4000, 3200, 3520, 2880, 4000, 3360)
NOISE_MAX, NOISE_LENS = 8000, (8000, 2400)


@functools.lru_cache(maxsize=None)
def _signals():
    rng = np.random.default_rng(31)
    pcm, noise = np.zeros((E * K, N_MAX), np.float32), np.zeros((len(NOISE_LENS), NOISE_MAX), np.float32)
    for b, n in enumerate(LENS):
        pcm[b, :n] = rng.standard_normal(n) * 0.1 * np.sin(np.arange(n) * (0.002 + 0.001 * b))
    for k, n in enumerate(NOISE_LENS):
        noise[k, :n] = rng.standard_normal(n) * 0.05
    return pcm, noise


class Setup(object):
    def __init__(self):
        from keyword_spotting_amd import get_config, weights
        from keyword_spotting_amd.custom_keyword import Enroller
        from keyword_spotting_amd.frontend import DatasetFrontend
        from keyword_spotting_amd.prediction import ctc_label
        from keyword_spotting_amd.rnn_ctc import DeployModel
        cfg = get_config()
        assert (cfg.hidden_size, cfg.num_layers, cfg.num_classes) == (128, 2, 6)
        self.model = DeployModel(cfg, weights.init_weights(cfg, seed=0))
        self.frontend = DatasetFrontend(cfg, pre_emphasis=0.97)
        self.enroller = Enroller(self.model, N_NEW, enrolments=E, utterances_per_enrolment=K)
        pcm, noise = _signals()
        self.pcm, self.lens = torch.from_numpy(pcm), torch.tensor(LENS, dtype=torch.int32)
        self.clean = self.frontend.linear(self.pcm, self.lens)
        self.noise = self.frontend.linear(torch.from_numpy(noise), torch.tensor(NOISE_LENS, dtype=torch.int32))
        self.labels = list(ctc_label([5, 6]))

    def augmented(self, steps_per_batch=1, seed=0, **kw):
        from keyword_spotting_amd.custom_keyword import NoiseAugmenter
        return self.enroller.fit_augmented(self.frontend, self.clean, self.noise, NoiseAugmenter(seed=seed, **kw), self.labels, STEPS,
                                           steps_per_batch=steps_per_batch, lr=LR, seed=3)

    def close(self):
        self.enroller.close()
        self.frontend.close()
        self.model.close()


@pytest.fixture(scope="module")
def setup():
    s = Setup()
    yield s
    s.close()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_without_noise_it_is_fit_on_the_front_ends_mel(setup):
    mel = setup.frontend.forward(setup.pcm, setup.lens)
    frames = setup.clean.frames.cpu().numpy()
    assert frames.tolist() == [1 + n // 160 for n in LENS]
    want = setup.enroller.fit(mel, frames, setup.labels, STEPS, lr=LR, seed=3)
    assert want[2].shape == (STEPS, E * K) and torch.isfinite(want[2]).all()
    for per in (1, 5):
        got = setup.augmented(per, bg_noise_prob=0.0)
        assert _same(got, want), per                   # columns, bias and trace
    assert setup.enroller.stats()[2] == STEPS          # one kws_enroll_set in front, the step count ran on across the batches


def test_with_noise_it_is_the_loop_of_the_public_pieces(setup):
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.custom_keyword import NoiseAugmenter, _ints, _pack_labels, truncated_normal
    per, seed = 5, 17
    got = setup.augmented(per, seed=seed, bg_noise_prob=1.0, per_row=True)
    en, lib = setup.enroller, _lib.load()
    b, h = E * K, 128
    aug = NoiseAugmenter(seed=seed, bg_noise_prob=1.0, per_row=True)
    wn = torch.from_numpy(truncated_normal((E, h, N_NEW), 3)).cuda()
    bn = torch.zeros(E, N_NEW, device="cuda")
    lab, lab_len = _pack_labels(setup.labels, b)
    (sl, sl_p), (lab, lab_p), (lab_len, lab_len_p) = _ints(setup.clean.frames.cpu().numpy()), _ints(lab), _ints(lab_len)
    t = int(setup.clean.spec.shape[1])
    trace = torch.empty(STEPS, b, device="cuda")
    stream = _lib.current_stream_ptr()
    _lib.check(lib.kws_enroll_set(en._handle, _lib.ptr(wn), _lib.ptr(bn), stream))
    mixed_rows = 0
    for s0 in range(0, STEPS, per):
        src, noise_index, start, gain_db = aug.draw(b, 2, t)
        assert (noise_index == np.arange(b) % 2).all()
        mel = setup.frontend.augment(setup.clean, setup.noise, src, noise_index, start, gain_db)
        mixed_rows += int((mel != setup.frontend.forward(setup.pcm, setup.lens)).flatten(1).any(1).sum())
        nn, logits1 = en.features(mel, setup.clean.frames)
        _lib.check(lib.kws_enroll_fit(en._handle, _lib.ptr(nn), _lib.ptr(logits1), sl_p, lab_p, lab_len_p, t, int(lab.shape[1]), LR, per,
                                      _lib.ptr(trace[s0:]), stream))
    w, bias = torch.empty_like(wn), torch.empty_like(bn)
    _lib.check(lib.kws_enroll_get(en._handle, _lib.ptr(w), _lib.ptr(bias), stream))
    assert mixed_rows > 0                               # noise did reach the stack's input
    assert _same(got, (w, bias, trace))
    assert torch.isfinite(got[2]).all()


def test_same_seed_same_bits_another_seed_another_trace(setup):
    a = setup.augmented(2, seed=5, bg_noise_prob=1.0)
    b = setup.augmented(2, seed=5, bg_noise_prob=1.0)
    c = setup.augmented(2, seed=6, bg_noise_prob=1.0)
    plain = setup.augmented(2, seed=5, bg_noise_prob=0.0)
    assert _same(a, b)
    assert not torch.equal(a[2], c[2]) and not torch.equal(a[2], plain[2])
    for r in (a, c, plain):
        assert torch.isfinite(r[2]).all() and torch.isfinite(r[0]).all() and torch.isfinite(r[1]).all()


def test_refusals(setup):
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.custom_keyword import NoiseAugmenter
    from keyword_spotting_amd.frontend import DatasetFrontend
    from keyword_spotting_amd.config import get_attention_config
    with pytest.raises(_lib.InvalidArgumentError, match="max_sequence_length"):          # T = 26 frames >= 26
        setup.enroller.fit_augmented(setup.frontend, setup.clean, setup.noise, NoiseAugmenter(max_sequence_length=26), setup.labels, 2)
    wide = DatasetFrontend(get_attention_config(n_mel=60))
    with pytest.raises(_lib.InvalidArgumentError, match="40 mel filters"):
        setup.enroller.fit_augmented(wide, setup.clean, setup.noise, NoiseAugmenter(), setup.labels, 2)
    wide.close()
    with pytest.raises(_lib.InvalidArgumentError, match="steps"):
        setup.enroller.fit_augmented(setup.frontend, setup.clean, setup.noise, NoiseAugmenter(), setup.labels, 0)
