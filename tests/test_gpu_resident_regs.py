"""The fp32 resident kernel (csrc/gru_resident.hip) with its gate x-part weights in the spare accumulator registers and
without the per-frame sequence-length mask.  A call without seq_len runs the unmasked kernels, one with seq_len the masked
ones; with seq_len == T everywhere both do the same arithmetic, so every output is the same bytes.  The first layer keeps its
whole x-part in registers at every instantiated width (KCX = 8, 10, 12, 15, 16), upper layers 16 of 32 k-chunks: each width is
held against the fp64 oracle, and the chunked call against the single one.  Tolerances are the project's: logits and state
within 1e-4 of the fp64 oracle, softmax within 2e-5.
The launch names are the library's tags, which are the same for the masked and the unmasked kernel: these tests hold the two bodies to the
same bytes, they do not tell which one ran.  That a call with seq_len runs the masked one is held by the suite's tests with seq_len < T (the
unmasked body has no copy-through); that a call without it runs the unmasked one shows in the kernel symbols of profiles/r15_kernel_stats.csv."""
import functools

import numpy as np
import pytest
import torch

from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu
TOL, TOL_SM = 1e-4, 2e-5
# the prologue-only call, one steady frame, a partial second and third group, a 16-frame flush plus a partial one; a middle
# layer (48, 3), a layer that is first and last (32, 1), the odd KCX = 15 (60)
MASK_SHAPES = [(40, 128, 2, 6), (48, 128, 3, 6), (32, 128, 1, 6), (60, 128, 2, 6)]
MASK_BATCHES, MASK_FRAMES = (1, 17, 33), (1, 2, 17, 35)
BMAX, TMAX = 33, 35


def _model(shape, w):
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    i, h, l, c = shape
    return DeployModel(get_config(n_mel=i, hidden_size=h, num_layers=l), w, kernel="resident")


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """Weights, mel and a non-zero start state of one shape at the largest batch and length; read-only afterwards."""
    i, h, l, c = shape
    w = G.random_weights(i, h, l, c, seed=1501)
    mel = G.synthetic_mel(BMAX, TMAX, i, seed=1502)
    st0 = (0.5 * np.random.default_rng(1503).standard_normal((l, BMAX, h))).astype(np.float32)
    for a in (mel, st0):
        a.setflags(write=False)
    return w, mel, st0


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "mel%d_L%d" % (s[0], s[2]))
def test_masked_equals_unmasked_bit_for_bit(shape):
    w, mel, st0 = _inputs(shape)
    m = _model(shape, w)
    for b in MASK_BATCHES:
        for t in MASK_FRAMES:
            x = torch.from_numpy(mel[:b, :t].copy()).cuda()
            s = torch.from_numpy(st0[:, :b].copy()).cuda()
            pw_u, pw_m = m.fresh_prev_word(b), m.fresh_prev_word(b)
            plain = m.forward(x, s, prev_word=pw_u)
            plain = {k: v.clone() for k, v in plain.items()}
            assert all("gru_layer_resident" in n for n in m.kernel_names())
            masked = m.forward(x, s, seq_len=torch.full((b,), t, dtype=torch.int32), prev_word=pw_m)
            assert all("gru_layer_resident" in n for n in m.kernel_names())
            for k in ("logits", "softmax", "tokens", "state"):
                assert _same_bytes(plain[k], masked[k]), (shape, b, t, k)
            assert _same_bytes(pw_u, pw_m), (shape, b, t)
    m.close()


@pytest.mark.parametrize("n_mel", [32, 40, 48, 60, 64])
def test_every_first_layer_width_against_the_oracle(n_mel):
    shape, b, t = (n_mel, 128, 2, 6), 17, 19
    w, mel, st0 = _inputs(shape)
    want_l, want_s = G.gru_forward(w, mel[:b, :t], st0[:, :b], dtype=np.float64)
    m = _model(shape, w)
    r = m.forward(torch.from_numpy(mel[:b, :t].copy()), torch.from_numpy(st0[:, :b].copy()))
    got_l, got_sm, got_s = r["logits"].cpu().numpy(), r["softmax"].cpu().numpy(), r["state"].cpu().numpy()
    el, es = np.abs(got_l - want_l).max(), np.abs(got_s - want_s).max()
    esm = np.abs(got_sm - G.softmax(want_l)).max()
    print("n_mel=%d  |dlogit| %.2e  |dstate| %.2e  |dsoftmax| %.2e  %s" % (n_mel, el, es, esm, m.kernel_names()))
    assert el < TOL and es < TOL and esm < TOL_SM
    assert all("gru_layer_resident" in n for n in m.kernel_names())
    m.close()


@pytest.mark.parametrize("shape", [(40, 128, 2, 6), (60, 128, 2, 6)], ids=lambda s: "mel%d_L%d" % (s[0], s[2]))
def test_chunks_16_1_18_equal_one_call_bitwise(shape):
    w, mel, st0 = _inputs(shape)
    m = _model(shape, w)
    x, s0 = torch.from_numpy(mel.copy()).cuda(), torch.from_numpy(st0.copy()).cuda()
    whole = {k: v.clone() for k, v in m.forward(x, s0).items()}
    state, pos, parts, sms = s0, 0, [], []
    for n in (16, 1, 18):
        r = m.forward(x[:, pos:pos + n].contiguous(), state)
        parts.append(r["logits"].clone()); sms.append(r["softmax"].clone()); state = r["state"].clone(); pos += n
    assert pos == TMAX
    assert _same_bytes(torch.cat(parts, 1), whole["logits"]) and _same_bytes(torch.cat(sms, 1), whole["softmax"])
    assert _same_bytes(state, whole["state"])
    m.close()
