#!/usr/bin/env python3
"""Do two builds of the FFT front-end (csrc/fft_frontend.hip) produce the same bytes?
  ab_frontend_outputs.py --out DIR      runs the cases below on the library KWS_AMD_LIB names (default: the built one) and writes every
                                        output array to DIR/frontend_outputs.npz
  ab_frontend_outputs.py --compare A B  exits non-zero unless both files hold the same arrays, byte for byte
One process per library: run --out once under each KWS_AMD_LIB, then --compare.

Cases, the smallest at which each phase of mel_fft400_kernel can go wrong (fft 400, hop 160):
  plain     n_mel 13 / 20 / 40 / 60 (one to four mel tiles; 13: the scalar row store), float, no gate: B = 3 x 22 frames (five blocks, the
            last partial, streams straddling blocks) and B = 19 x 2 frames (several streams start in one block)
  carry     forward_carry with 240 carried samples and chunks of 160 (one frame), 3600, 3601 and 4320 samples
  manager   lock-step stream managers on float and int16 PCM, n_mel 40 (the resident stack) and 13 (the generic one): chunks of 0, 160,
            3600 and 3601 samples, one of them silent -- the gate's fast and slow path, the masks, the next carry -- and a ragged chunk
            at the end (the lock-step carry read by the ragged kernel).  Per chunk: hit, restart, state, and the carried samples
            (kws_stream_carry; past each row's length zeroed here).  The mel is not readable there; it shows in the state.
  ragged    B = 19, n_max 3600, lengths 0, 1, 159, 160, 399, 3599, 3600 ... rotating through the streams, so that a stream stays
            below 400 carried + new samples for several chunks running; float and int16
  lengths   kws_frontend_run_lengths on the deploy framing: B = 5, n_max 4000, lengths 0, 399, 400, 401, 4000 and none; power 1 and
            2, MFCC with 13 and 20 coefficients (one and two coefficient tiles)
  dataset   the centred framing: lengths 0, 200, 201, 202, 2001 and n_max, pre-emphasis 0 and 0.97; mel, power mel, MFCC and the linear
            spectrum with its frames and energies
  augment   both framings x mel / power / MFCC, T_max = 7 (a 16-frame block spans several rows) and 40; rows with src -1, src >= B,
            noise -1, a start past the clip's frames, a clip without energy, plain mixed rows
Input builders: tests/test_gpu_ragged.py (_pcm), tests/test_gpu_augment.py (_config), oracle/gru_oracle.py (weights)."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--compare", nargs=2, default=None)
a = ap.parse_args()

if a.compare:
    x, y = (np.load(f) for f in a.compare)
    bad = sorted(set(x.files) ^ set(y.files)) + [k for k in x.files if k in y.files and
                                                  (x[k].dtype != y[k].dtype or x[k].shape != y[k].shape or x[k].tobytes() != y[k].tobytes())]
    print("%d arrays, %d bytes: %s" % (len(x.files), sum(x[k].nbytes for k in x.files), "all byte-equal" if not bad else "DIFFERENT: %s" % bad[:20]))
    sys.exit(1 if bad else 0)
if not a.out:
    ap.error("--out DIR or --compare A B")

import torch
import test_gpu_augment as TA
import test_gpu_ragged as TR
from oracle import gru_oracle as G
from keyword_spotting_amd import _lib, get_config
from keyword_spotting_amd.detector import StreamManager
from keyword_spotting_amd.frontend import DatasetFrontend, MelFrontend, _Frontend
from keyword_spotting_amd.rnn_ctc import DeployModel

N_MFCC = TA.N_MFCC          # {40: 13, 60: 20}
KINDS = ("mel", "power", "mfcc")
out = {}


def keep(name, t):
    out[name] = t.detach().cpu().numpy().copy()


def floats(rng, *shape):
    return torch.from_numpy((rng.standard_normal(shape) * 0.2).astype(np.float32))


def deploy_features(kind, n_mel):
    """kws_frontend_create_features on the deploy framing: mel, power mel or MFCC of whole utterances"""
    cfg = TA._config(kind, n_mel, N_MFCC.get(n_mel, 13) if kind == "mfcc" else 0)
    feat = (_lib.FEAT_MFCC, 2, int(cfg.n_mfcc)) if kind == "mfcc" else (_lib.FEAT_MEL, 2 if kind == "power" else 1, 0)
    fe = _Frontend(cfg, "cuda:0", "kws_frontend_create_features", feat)
    fe.width = int(fe._lib.kws_frontend_feature_size(fe._handle))
    return fe


def plain_and_carry():
    rng = np.random.default_rng(1)
    for n_mel in (13, 20, 40, 60):
        fe = MelFrontend(get_config(n_mel=n_mel))
        keep("plain/mel%d/B3xT22" % n_mel, fe.forward(floats(rng, 3, 400 + 21 * 160)))
        keep("plain/mel%d/B19xT2" % n_mel, fe.forward(floats(rng, 19, 560)))
        carry = floats(rng, 5, 240).cuda()
        for n in (160, 3600, 3601, 4320):
            mel, nxt = fe.forward_carry(carry, floats(rng, 5, n).cuda(), 240)
            keep("carry/mel%d/n%d/mel" % (n_mel, n), mel)
            keep("carry/mel%d/n%d/next" % (n_mel, n), nxt)
        fe.close()


def snapshot(name, mgr, hit):
    keep(name + "/hit", hit)
    keep(name + "/restart", mgr.restart)
    keep(name + "/state", mgr.state)
    samples, lengths = mgr.carry()
    cols = torch.arange(samples.shape[1], device=samples.device)[None, :] < lengths[:, None]
    keep(name + "/carry", torch.where(cols, samples, torch.zeros_like(samples)))
    keep(name + "/carry_len", lengths)


RAGGED_LENS = np.array([0, 1, 159, 160, 399, 3599, 3600, 3600, 1800, 0, 3599, 400, 401, 3600, 160, 1, 159, 3200, 3600], np.int32)


def managers():
    B = 19
    for n_mel, hidden, kernel in ((40, 128, "auto"), (13, 64, "generic")):
        cfg = get_config(n_mel=n_mel, hidden_size=hidden)
        fe = MelFrontend(cfg)
        w = G.random_weights(n_mel, hidden, 2, 6, seed=7200 + n_mel)
        model = DeployModel(cfg, w, kernel=kernel)
        for dtype in ("float", "int16"):
            tag = "mel%d/%s" % (n_mel, dtype)
            pcm = lambda rng, lens, n: torch.from_numpy(TR._pcm(rng, B, lens)[:, :n] if dtype == "int16" else
                                                        (TR._pcm(rng, B, lens)[:, :n] / np.float32(32768.0)).astype(np.float32))
            rng = np.random.default_rng(31)
            mgr = StreamManager(model, B, label="1")
            for ci, n in enumerate((3600, 160, 0, 3601, 3600, 160, 3601, 3600)):
                chunk = pcm(rng, np.full(B, n, np.int32), n)
                if ci == 4:
                    chunk = chunk // 4096 if dtype == "int16" else chunk / 4096.0          # the silent chunk: below vad(data, 30)
                snapshot("manager/%s/chunk%d" % (tag, ci), mgr, mgr.feed_pcm(chunk, fe))
            lens = RAGGED_LENS.copy()
            snapshot("manager/%s/then_ragged" % tag, mgr, mgr.feed_pcm(pcm(rng, lens, 3600), fe, lengths=torch.from_numpy(lens)))
            mgr.close()
            mgr = StreamManager(model, B, label="1")
            for ci in range(6):
                lens = np.roll(RAGGED_LENS, -ci)
                snapshot("ragged/%s/chunk%d" % (tag, ci), mgr, mgr.feed_pcm(pcm(rng, lens, 3600), fe, lengths=torch.from_numpy(lens)))
            mgr.close()
        model.close()
        fe.close()


def utterances():
    rng = np.random.default_rng(3)
    pcm = floats(rng, 5, 4000)
    lens = torch.tensor([0, 399, 400, 401, 4000], dtype=torch.int32)
    for kind in KINDS:
        for n_mel in (13, 20, 40, 60):
            if kind == "mfcc" and n_mel not in N_MFCC:
                continue
            fe = deploy_features(kind, n_mel)
            keep("lengths/%s/mel%d/lens" % (kind, n_mel), fe._run_lengths(pcm, lens, fe.width))
            keep("lengths/%s/mel%d/full" % (kind, n_mel), fe._run_lengths(pcm, None, fe.width))
            fe.close()


def dataset():
    rng = np.random.default_rng(4)
    n_max = 2400
    pcm = floats(rng, 6, n_max)
    lens = torch.tensor([0, 200, 201, 202, 2001, n_max], dtype=torch.int32)
    for pre in (0.0, 0.97):
        for kind in KINDS:
            for n_mel in (40, 60):
                fe = TA._fe(kind, n_mel, pre)
                tag = "dataset/pre%g/%s/mel%d" % (pre, kind, n_mel)
                keep(tag + "/lens", fe.forward(pcm, lens))
                keep(tag + "/full", fe.forward(pcm))
                if kind == "mel" and n_mel == 40:
                    for form, n in (("lens", lens), ("full", None)):
                        lin = fe.linear(pcm, n)
                        for field in lin._fields:
                            keep("dataset/pre%g/linear/%s/%s" % (pre, form, field), getattr(lin, field))
                fe.close()
    fe = deploy_features("mel", 40)            # the linear spectrum on the deploy framing
    lin = fe.linear(pcm, lens)
    for field in lin._fields:
        keep("lengths/linear/%s" % field, getattr(lin, field))
    fe.close()


# (src, noise, start, gain_db) against B = 4 utterances (the last silent) and K = 3 clips (the last without energy)
AUG_ROWS = ((1, 1, 0, -5.0), (2, 0, 2, -15.0), (-1, 0, 0, -5.0), (7, 1, 0, -5.0), (0, -1, 0, 0.0), (1, 0, 500, -5.0), (1, 2, 0, -5.0),
            (3, 1, 4, -5.0), (2, 1, 3, 5.0), (0, 1, 1, -5.0), (1, 9, 0, -5.0))


def augment():
    rng = np.random.default_rng(5)
    src, k, start, gain = (np.array([r[i] for r in AUG_ROWS]) for i in range(4))
    for framing in ("deploy", "dataset"):
        for t_max in (7, 40):
            n_max = 400 + (t_max - 1) * 160 if framing == "deploy" else (t_max - 1) * 160 + 80
            pcm, noise = floats(rng, 4, n_max), floats(rng, 3, n_max + 800)
            pcm[3], noise[2] = 0.0, 0.0
            lens = torch.tensor([n_max, n_max - 170, n_max // 2, n_max], dtype=torch.int32)
            nlens = torch.tensor([700, n_max + 800, 700], dtype=torch.int32)
            for kind in KINDS:
                for n_mel in (40, 60):
                    fe = deploy_features(kind, n_mel) if framing == "deploy" else TA._fe(kind, n_mel, 0.0)
                    got = fe.augment(fe.linear(pcm, lens), fe.linear(noise, nlens), src.astype(np.int32), k.astype(np.int32),
                                     start.astype(np.int32), gain.astype(np.float32))
                    assert got.shape[1] == t_max, (framing, t_max, tuple(got.shape))
                    keep("augment/%s/T%d/%s/mel%d" % (framing, t_max, kind, n_mel), got)
                    fe.close()


plain_and_carry()
managers()
utterances()
dataset()
augment()
torch.cuda.synchronize()
os.makedirs(a.out, exist_ok=True)
np.savez(os.path.join(a.out, "frontend_outputs.npz"), **out)
print("%d arrays, %d bytes -> %s" % (len(out), sum(v.nbytes for v in out.values()), os.path.join(a.out, "frontend_outputs.npz")))
