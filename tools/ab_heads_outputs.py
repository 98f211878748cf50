#!/usr/bin/env python3
"""Do two builds of the class-head kernels (dense_heads.hip, heads_window.hip, bank_heads.hip) produce the same bytes?
  ab_heads_outputs.py --out DIR      runs the cases below on the library KWS_AMD_LIB names (default: the built one) and writes every
                                     output array to DIR/heads_outputs.npz
  ab_heads_outputs.py --compare A B  exits non-zero unless both files hold the same arrays, byte for byte
One process per library: run --out once under each KWS_AMD_LIB, then --compare.

Cases, the smallest at which each phase can go wrong: B = 19 (two groups, the second with three streams); hidden 64 / 128 / 256 on the
generic kernels and n_mel 40 x hidden 128 on AUTO; steps of T in {1, 31, 32, 33, 70} frames (32 per workgroup: no halo, an exact block,
a one-frame second block, three blocks) with ragged seq_len including 0 and T, a reset mask, relu and clip on and off, each head absent
in turn, C1 / C2 = 6 / 8 and 5 / 7 (the even and the odd row store); banks of n_new 2 and 1 with users -1, past the capacity and two
streams on one slot, then keywords on some slots only (one with n_used < n_new).  Managers (two-head, bank, bank with keywords): chunks
of {0, 1, 22, 33} frames with silent chunks, one-digit labels the inputs spell -- both heads must fire, so the cross-clear occurs --
and on the reference shape the ragged PCM feed with skipped streams.  Recorded per chunk: hit, restart and the state; the windows'
head / count are not readable through the API and show in the hits of the chunks that follow.
Input builders: tests/heads_model.py, tests/bank_model.py, oracle/."""
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
import bank_model as BM
import heads_model as HM
from oracle import decode_oracle as D
from oracle import gru_oracle as G
import keyword_spotting_amd.custom_keyword as CK
from keyword_spotting_amd import get_config
from keyword_spotting_amd.custom_keyword import KeywordBank
from keyword_spotting_amd.detector import StreamManager
from keyword_spotting_amd.frontend import MelFrontend
from keyword_spotting_amd.rnn_ctc import DeployModel

# KeywordBank refuses relu / clip models for the enrolment's sake (the gradient at the ties); the bank kernels apply both like the dense
# ones, and this comparison wants that path too
CK._frozen_model_check = lambda who, model: None
B, CAPACITY, THRES = 19, 4, (0.4, 0.3)
FRAMES = (1, 31, 32, 33, 70)
STACKS = [(13, 64, 2), (13, 128, 1), (13, 256, 1), (40, 128, 2)]          # (n_mel, hidden, layers)
# (C1, dense C2, bank n_new, relu, clip, the slots' keywords (label, n_used) or None)
HEADS = [(6, 8, 2, False, -1.0, [("5", 1), ("56", 2), None, None]), (5, 7, 1, True, 20.0, [None, ("4", 1), None, ("44", 1)])]
USERS = np.array([0, 1, 2, 3, -1, 9, 1, 0, 2, 3, 3, -1, 0, 1, 2, 0, 3, 4, 1], np.int32)          # 4 and 9: past the capacity
out = {}


def keep(name, r, pw=None):
    for k, v in r.items():
        for kk, vv in (v.items() if isinstance(v, dict) else [(None, v)]):
            out["%s/%s%s" % (name, k, "/" + kk if kk else "")] = vv.cpu().numpy()
    for i, p in enumerate(pw or ()):
        out["%s/prev_word%d" % (name, i + 1)] = p.cpu().numpy()


def config(stack, c1, c2, relu, clip):
    cfg = get_config(n_mel=stack[0], hidden_size=stack[1], num_layers=stack[2], label_dict={"w%d" % i: i for i in range(1, c1 - 2)})
    cfg.use_relu, cfg.value_clip = relu, clip
    if c2:
        cfg.num_classes2 = c2
    return cfg


def kernel(stack):
    return "auto" if stack[:2] == (40, 128) else "generic"


def steps(name, fwd, seed):
    """fwd(mel, state, **kw) at every T: ragged seq_len with 0 and T, a reset mask, carried words; at T = 33 also each head alone."""
    rng = np.random.default_rng(seed)
    for t in FRAMES:
        mel = torch.from_numpy(G.synthetic_mel(B, t, fwd.n_mel, seed=seed + t))
        st = torch.from_numpy((0.3 * rng.standard_normal(fwd.state_shape)).astype(np.float32))
        lens = rng.integers(0, t + 1, B).astype(np.int32)
        lens[:3] = (0, t, t)
        reset = torch.from_numpy((rng.random(B) < 0.3).astype(np.uint8))
        for heads in ((1, 2), (1,), (2,)) if t == 33 else ((1, 2),):
            pw = [torch.full((B,), 2, dtype=torch.int32, device="cuda"), torch.full((B,), 1, dtype=torch.int32, device="cuda")]
            r = fwd(mel, st, seq_len=torch.from_numpy(lens), reset_mask=reset, heads=heads, prev_words=pw, decode2_thres=THRES)
            keep("%s/T%d/heads%s" % (name, t, "".join(map(str, heads))), r, pw)
        keep("%s/T%d/full" % (name, t), fwd(mel, st, want_logits=False))


def wrap(f, stack, **fixed):
    g = lambda mel, st, **kw: f(mel, st, **fixed, **kw)
    g.n_mel, g.state_shape = stack[0], (stack[2], B, stack[1])
    return g


def set_keywords(bank, keywords):
    for slot, kw in enumerate(keywords):
        if kw:
            bank.set_keyword(slot, *kw)


def labels_of(r, c1, c2):
    """each head's most frequent word as its one-digit label (head 2's among the new words where there are any)"""
    got = []
    for i, c in ((1, c1), (2, c2)):
        sm = r["head%d" % i]["softmax"].cpu().numpy()
        words = np.concatenate([D.ctc_decode2(sm[k], c, THRES[i - 1])[1::2] for k in range(B) if sm[k].any()]).astype(np.int64)
        new = words[words >= c1 - 1] if i == 2 and (words >= c1 - 1).any() else words
        got.append(str(int(np.bincount(new).argmax())))
    return got


def manager(name, make, stack, seed, fe=None):
    """mel-fed chunks of {0, 1, 22, 33} frames with a silent chunk and silent streams; with fe the ragged PCM feed too"""
    rng = np.random.default_rng(seed)
    chunks = [22, 0, 1, 33, 22, 22, 33, 1, 22, 0, 22, 33, 22, 22]
    mel = torch.from_numpy(G.synthetic_mel(B, sum(chunks), stack[0], seed=seed)).cuda()
    mgr = make(mel)
    hits, pos = 0, 0
    for ci, n in enumerate(chunks):
        speech = rng.random(B) > (1.0 if ci == 5 else 0.1)
        hit = mgr.feed(mel[:, pos:pos + n].clone(), speech=torch.from_numpy(speech)).cpu().numpy()
        out["%s/chunk%d/hit" % (name, ci)], out["%s/chunk%d/restart" % (name, ci)] = hit.copy(), mgr.restart.cpu().numpy()
        out["%s/chunk%d/state" % (name, ci)] = mgr.state.cpu().numpy()
        hits, pos = hits | int(np.bitwise_or.reduce(hit)), pos + n
    print("%s: hit_1 | hit_2 over the run = %d%s" % (name, hits, "" if hits == 3 else "  (NOT both heads: the cross-clear is not covered)"))
    if fe is not None:
        for p in range(6):
            lens = rng.choice([0, 150, 1800, 3600, 5000], size=B, p=[0.15, 0.1, 0.2, 0.4, 0.15]).astype(np.int32)
            pcm = torch.from_numpy(rng.integers(-6000, 6000, (B, 5000)).astype(np.int16)).cuda()
            hit = mgr.feed_pcm(pcm, fe, lengths=torch.from_numpy(lens)).cpu().numpy()
            out["%s/pcm%d/hit" % (name, p)], out["%s/pcm%d/restart" % (name, p)] = hit.copy(), mgr.restart.cpu().numpy()
            out["%s/pcm%d/state" % (name, p)] = mgr.state.cpu().numpy()
    mgr.close()


for si, stack in enumerate(STACKS):
    for hi, (c1, c2, n_new, relu, clip, keywords) in enumerate(HEADS):
        tag, seed = "mel%d-h%d-l%d/c%d" % (stack + (c1,)), 100 * si + 10 * hi + 1
        w = HM.random_heads_weights(stack[0], stack[1], stack[2], c1, c2, seed, scale=3.0)
        one_w = {k: v for k, v in w.items() if k not in ("Wfc2", "bfc2")}
        cols, bias = BM.random_bank(stack[1], n_new, CAPACITY, seed, scale=3.0)
        model = DeployModel(config(stack, c1, c2, relu, clip), w, kernel=kernel(stack))
        steps(tag + "/dense", wrap(model.forward_heads, stack), seed)
        one = DeployModel(config(stack, c1, 0, relu, clip), one_w, kernel=kernel(stack))
        bank = KeywordBank(one, n_new, CAPACITY, kernel=kernel(stack)).set(0, cols, bias)
        steps(tag + "/bank", wrap(bank.forward, stack, users=USERS), seed)
        set_keywords(bank, keywords)
        steps(tag + "/bank_keywords", wrap(bank.forward, stack, users=USERS), seed)
        bank.close()
        if stack[1] in (64, 128) and stack[2] == 2 and hi == 0:          # the managers: one generic stack and the reference shape
            fe = MelFrontend(get_config()) if stack[0] == 40 else None
            st0 = model.zero_state(B)
            lab = lambda mel: labels_of(model.forward_heads(mel, st0), c1, c2)
            kw = dict(decode_thres=THRES[0], decode_thres2=THRES[1], max_frames=40)
            manager(tag + "/manager", lambda mel: StreamManager(model, B, **dict(zip(("label", "label2"), lab(mel))), **kw), stack, seed, fe)
            for form, kws in (("bank_manager", None), ("bank_keywords_manager", keywords)):
                bank = KeywordBank(one, n_new, CAPACITY, kernel=kernel(stack)).set(0, cols, bias)
                set_keywords(bank, kws or ())
                lab = lambda mel: labels_of(bank.forward(mel, st0, USERS), c1, c1 + n_new)
                manager(tag + "/" + form, lambda mel: StreamManager(None, B, bank=bank, users=USERS, **dict(zip(("label", "label2"), lab(mel))), **kw),
                        stack, seed, fe)
                bank.close()
        one.close()
        model.close()
torch.cuda.synchronize()
os.makedirs(a.out, exist_ok=True)
np.savez(os.path.join(a.out, "heads_outputs.npz"), **out)
print("%d arrays, %d bytes -> %s" % (len(out), sum(v.nbytes for v in out.values()), os.path.join(a.out, "heads_outputs.npz")))
