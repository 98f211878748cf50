"""The last-layer epilogue of the fp32 resident kernels (csrc/gru_resident.hip, epilogue_flush_partials in csrc/gru_device.h): every
wave leaves its partial logits of a frame in a 16-frame ring, and every 16 frames (and at the end of a call) wave w turns streams
4w..4w+3 x 16 frames into logits, softmax, words and tokens -- one lane per (stream, frame), the previous frame's word from the lane
below, the word before the block from a register -- without a fold pass and without a barrier of its own.
What can go wrong there is a block boundary (the carried word, a ring slot read before or after its frame), a partial block, a
partial group, and the store paths; a call cut into chunks at any frame must give the bytes of the single call.
Tolerances are the project's: logits and state within 1e-4 of the fp64 oracle, softmax within 2e-5."""
import functools

import numpy as np
import pytest
import torch

from oracle import decode_oracle as D
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu
TOL, TOL_SM = 1e-4, 2e-5
KEYS = ("logits", "softmax", "tokens", "state")
BATCHES, FRAMES = (1, 17, 37), (1, 15, 16, 17, 33)      # one lane row / a partial second group / a partial third; around one and two blocks
BMAX, TMAX = 37, 33
# two layers (the headline kernels), a layer that is first and last, and five classes (rows that are not 24 bytes)
SHAPES = {"mel40_L2": (40, 128, 2, 6), "mel32_L1": (32, 128, 1, 6), "mel40_L2_C5": (40, 128, 2, 5)}


def _model(shape, w):
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    i, h, l, c = shape
    cfg = get_config(n_mel=i, hidden_size=h, num_layers=l, label_dict={str(k): k for k in range(1, c - 2)})
    assert cfg.num_classes == c
    return DeployModel(cfg, w, kernel="resident")


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _assert_same(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bytes(a[k]), _bytes(b[k])), (what, k)


def _run(m, x, state, chunks, seq_len=None, reset=None):
    """forward() over x cut into `chunks`, state and prev_word carried; every output concatenated, prev_word beside them."""
    b = x.shape[0]
    pw = m.fresh_prev_word(b) + 3            # word 2 carried in: a stream under the reset mask must start from -1 all the same
    parts, pos = {k: [] for k in KEYS[:3]}, 0
    for n in chunks:
        sl = None if seq_len is None else torch.clamp(seq_len - pos, 0, n).to(torch.int32)
        r = m.forward(x[:, pos:pos + n].contiguous(), state, seq_len=sl, reset_mask=reset if pos == 0 else None, prev_word=pw)
        for k in parts:
            parts[k].append(r[k].clone())
        state, pos = r["state"].clone(), pos + n
    assert pos == x.shape[1]
    out = {k: torch.cat(v, 1) for k, v in parts.items()}
    out["state"], out["prev_word"] = state, pw.clone()
    return out


def _cut(t):
    """A chunk schedule with a one-frame call in the middle."""
    return (t,) if t == 1 else (t // 2, 1, t - t // 2 - 1) if t > 2 else (1, 1)


def test_chunked_equals_one_call_across_ring_boundaries():
    w = G.init_weights()
    b, t = 40, 120
    mel = G.synthetic_mel(b, t, 40, seed=61)
    want_l, _ = G.gru_forward(w, mel, dtype=np.float64)
    want_sm = G.softmax(want_l)
    m = _model((40, 128, 2, 6), w)
    x = torch.from_numpy(mel).cuda()
    runs = []
    for chunks in ((t,), (16, 16, 1, 15, 17, 32, 23), (21, 22, 23, 22, 1, 31)):
        pw = m.fresh_prev_word(b)
        state, pos, parts = m.zero_state(b), 0, {k: [] for k in KEYS[:3]}
        for n in chunks:
            r = m.forward(x[:, pos:pos + n].contiguous(), state, prev_word=pw)
            for k in parts:
                parts[k].append(r[k].clone())
            state, pos = r["state"].clone(), pos + n
        assert pos == t
        out = {k: torch.cat(v, 1) for k, v in parts.items()}
        out["state"], out["prev_word"] = state, pw.clone()
        runs.append(out)
    _assert_same(runs[0], runs[1], "chunks 16,16,1,15,17,32,23")
    _assert_same(runs[0], runs[2], "chunks 21,22,23,22,1,31")
    from keyword_spotting_amd.prediction import tokens_to_seq
    toks = runs[0]["tokens"].cpu().numpy()
    across = 0
    for k in range(b):
        p = np.sort(want_sm[k][:, 1:5], axis=1)
        assert (np.abs(p[:, -1] - 0.4) > 1e-4).all() and (p[:, -1] - p[:, -2] > 1e-4).all(), k     # no stream is skipped
        np.testing.assert_array_equal(tokens_to_seq(toks[k]), D.ctc_decode2(want_sm[k], 6), err_msg=str(k))
        words = D.frame_words(want_sm[k], 1, 5, 0.4)
        across += int(sum(words[f] >= 0 and words[f] != words[f - 1] for f in range(16, t, 16)))
    print("oracle token events in the first frame of a 16-frame block: %d; tokens %d" % (across, int((toks > 0).sum())))
    assert across >= 20            # the lane-to-lane predecessor ends at a block's first frame: the carried word decides these
    m.close()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    i, h, l, c = SHAPES[name]
    w = G.random_weights(i, h, l, c, seed=1601)
    mel = G.synthetic_mel(BMAX, TMAX, i, seed=1602)
    st0 = (0.5 * np.random.default_rng(1603).standard_normal((l, BMAX, h))).astype(np.float32)
    rng = np.random.default_rng(1604)
    lens = rng.integers(0, TMAX + 1, BMAX).astype(np.int32)
    lens[:6], lens[16:20] = [0, 1, 15, 16, 17, TMAX], [TMAX, 16, 0, 20]      # inside and across a 16-frame block, in full and partial groups
    reset = (rng.random(BMAX) < 0.4).astype(np.uint8)
    reset[:3], reset[16:19], reset[36] = [1, 0, 1], [0, 1, 0], 1
    for a in (mel, st0, lens, reset):
        a.setflags(write=False)
    return w, mel, st0, lens, reset


@functools.lru_cache(maxsize=None)
def _oracle(name, t, mode):
    """fp64 logits and state of all BMAX streams over the first t frames; streams are independent, so a batch is a slice."""
    w, mel, st0, lens, reset = _inputs(name)
    st = st0 * (1 - reset)[None, :, None] if mode == "ragged_reset" else st0
    sl = np.minimum(lens, t) if mode == "ragged_reset" else None
    return G.gru_forward(w, mel[:, :t], st, seq_len=sl, dtype=np.float64)


@pytest.mark.parametrize("mode", ["plain", "ragged_reset"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_flush_shapes_chunked_and_against_the_oracle(name, mode):
    """plain: the unmasked kernels.  ragged_reset: seq_len ragged inside and across a block (the masked kernels: copy-through state,
    bias-only rows past the length) and a reset mask on some streams (zero state, no carried word)."""
    w, mel, st0, lens, reset = _inputs(name)
    c = SHAPES[name][3]
    m = _model(SHAPES[name], w)
    for b in BATCHES:
        for t in FRAMES:
            x = torch.from_numpy(mel[:b, :t].copy()).cuda()
            s0 = torch.from_numpy(st0[:, :b].copy()).cuda()
            sl = torch.from_numpy(np.minimum(lens[:b], t)).cuda() if mode == "ragged_reset" else None
            rs = torch.from_numpy(reset[:b].copy()).cuda() if mode == "ragged_reset" else None
            whole = _run(m, x, s0, (t,), sl, rs)
            assert all("gru_layer_resident" in n for n in m.kernel_names())
            _assert_same(whole, _run(m, x, s0, _cut(t), sl, rs), (name, mode, b, t))
            want_l, want_s = _oracle(name, t, mode)
            got_l, got_s = whole["logits"].cpu().numpy(), whole["state"].cpu().numpy()
            el, es = np.abs(got_l - want_l[:b]).max(), np.abs(got_s - want_s[:, :b]).max()
            esm = np.abs(whole["softmax"].cpu().numpy() - G.softmax(want_l[:b])).max()
            assert el < TOL and es < TOL and esm < TOL_SM, (name, mode, b, t, el, es, esm)
            # tokens and the carried word, from the kernel's own softmax (the oracle's decides test 1): the frame rule and its predecessor
            sm, tok, pw = whole["softmax"].cpu().numpy(), whole["tokens"].cpu().numpy(), whole["prev_word"].cpu().numpy()
            for k in range(b):
                words = D.frame_words(sm[k], 1, c - 1, 0.4)
                first = -1 if (mode == "ragged_reset" and reset[k]) else 2
                prev = np.concatenate([[first], words[:-1]])
                np.testing.assert_array_equal(tok[k], np.where((words >= 0) & (words != prev), words + 1, 0), err_msg=str((name, mode, b, t, k)))
                assert pw[k] == words[-1], (name, mode, b, t, k)
            if mode == "ragged_reset":
                for k in range(b):              # past seq_len: the zero output of dynamic_rnn -> the bias row
                    n = min(int(lens[k]), t)
                    np.testing.assert_array_equal(got_l[k, n:], np.broadcast_to(w["bfc"], (t - n, c)))
    m.close()


def test_alternating_inputs_on_one_handle_equal_fresh_handles():
    """A ring slot that outlives its call would show here: two inputs alternated on one handle against a fresh handle each."""
    name, b, t = "mel40_L2", 37, 33
    w, mel, st0, _, _ = _inputs(name)
    xa, sa = torch.from_numpy(mel[:b, :t].copy()).cuda(), torch.from_numpy(st0[:, :b].copy()).cuda()
    xb = torch.from_numpy(G.synthetic_mel(b, 17, 40, seed=1605) * np.float32(3.0)).cuda()
    sb = torch.from_numpy(np.ascontiguousarray(-st0[:, :b])).cuda()
    fresh = []
    for x, s in ((xa, sa), (xb, sb)):
        m = _model(SHAPES[name], w)
        fresh.append(_run(m, x, s, (x.shape[1],)))
        m.close()
    m = _model(SHAPES[name], w)
    for rep in range(3):
        for (x, s), want in zip(((xa, sa), (xb, sb)), fresh):
            _assert_same(want, _run(m, x, s, (x.shape[1],)), ("rep", rep, x.shape[1]))
    m.close()
