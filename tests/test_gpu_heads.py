"""GPU checks of a customised-keyword model (kws_create_heads / kws_step_heads, DeployModel.forward_heads): both class heads and
nn_outputs against the fp64 restatement tests/heads_model.py, seq_len / reset, chunking and batch composition (bitwise), the
relation to kws_step on the same handle, the per-head token rule, optional outputs, reservation, and run() / predict_ctc.

Bounds (tests/test_gpu_parity.py): logits and nn_outputs <= 1e-4, softmax <= 2e-5, rows sum to 1 within 1e-6; against kws_step
2e-5 (test_resident_and_generic_kernels_agree: same math, another K order).  Shapes: B in {1, 17} (a partial group, a second
group), T in {1, 33, 65} (dense_heads_kernel takes 32 frames per workgroup: a block boundary and its halo)."""
import functools

import numpy as np
import pytest
import torch

import heads_model as HM
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu

C1 = 6
# (n_mel, hidden, layers): n_mel 40 at hidden 128 takes the resident kernels, everything else the generic ones
STACKS = [(40, 128, 1), (40, 128, 2), (40, 128, 3), (13, 128, 1), (13, 128, 2), (13, 128, 3), (13, 64, 2), (13, 256, 2)]
B_MAX, T_MAX = 17, 65


def _model(stack, c2, w, relu=False, clip=-1.0):
    """n_mel 40 at hidden 128: AUTO, the resident kernels on every layer; the other stacks: the generic kernels on every layer (AUTO
    would give the upper layers of a hidden-128 stack the resident kernel whatever n_mel is)."""
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    kernel = "auto" if stack[:2] == (40, 128) else "generic"
    cfg = get_config(n_mel=stack[0], hidden_size=stack[1], num_layers=stack[2], use_relu=relu, value_clip=clip)
    cfg.num_classes2 = c2
    return DeployModel(cfg, w, kernel=kernel)


@functools.lru_cache(maxsize=None)
def _case(stack, c2, seed=11, scale=1.0, relu=False, clip=-1.0):
    """Weights, inputs and the fp64 restatement of the largest shape; the GRU is causal and streams are independent, so every
    smaller (B, T) is a slice of it.  Computed once, never modified."""
    w = HM.random_heads_weights(stack[0], stack[1], stack[2], C1, c2, seed=seed, scale=scale)
    mel = G.synthetic_mel(B_MAX, T_MAX, stack[0], seed=seed + 1)
    st = (0.3 * np.random.default_rng(seed + 2).standard_normal((stack[2], B_MAX, stack[1]))).astype(np.float32)
    return w, mel, st, HM.heads_forward(w, mel, st, use_relu=relu, value_clip=clip)


def _np(x):
    return x.cpu().numpy()


def _check_against(r, ref, b, t, what):
    for i in (1, 2):
        lg, sm = _np(r["head%d" % i]["logits"]), _np(r["head%d" % i]["softmax"])
        el = np.abs(lg - ref["logits%d" % i][:b, :t]).max()
        es = np.abs(sm - ref["softmax%d" % i][:b, :t]).max()
        print("%s head%d: max|dlogit| %.2e max|dsoftmax| %.2e" % (what, i, el, es))
        assert el <= 1e-4 and es <= 2e-5, (what, i, el, es)
        assert np.abs(sm.astype(np.float64).sum(-1) - 1).max() <= 1e-6
    en = np.abs(_np(r["nn_outputs"]) - ref["top"][:b, :t]).max()
    print("%s max|dnn_outputs| %.2e" % (what, en))
    assert en <= 1e-4, (what, en)


@pytest.mark.parametrize("c2", [3, 8])
@pytest.mark.parametrize("stack", STACKS, ids=lambda s: "mel%d-h%d-l%d" % s)
def test_heads_match_the_restatement(stack, c2):
    w, mel, st, ref = _case(stack, c2)
    m = _model(stack, c2, w)
    for b in (1, B_MAX):
        for t in (1, 33, T_MAX):
            r = m.forward_heads(torch.from_numpy(mel[:b, :t].copy()), torch.from_numpy(st[:, :b].copy()))
            _check_against(r, ref, b, t, "B=%d T=%d" % (b, t))
            if t == T_MAX:
                assert np.abs(_np(r["state"]) - ref["state"][:, :b]).max() <= 1e-4
    names = m.kernel_names()
    family = "gru_layer_resident" if stack[:2] == (40, 128) else "gru_layer_generic"
    assert all(n.startswith(family) and ", false>" in n for n in names), names          # no layer is `last`
    assert names[-1].endswith(" + dense_heads_kernel<%d>" % (stack[1] // 16)) and "dense_heads" not in "".join(names[:-1]), names
    m.close()


def test_heads_with_relu_and_clip():
    """inference2's relu and clip [0, 20] apply to both heads; heads scaled so that both ends of the clip are reached."""
    stack = (40, 128, 2)
    w, mel, st, ref = _case(stack, 8, scale=6.0, relu=True, clip=20.0)
    assert (ref["logits1"] == 0).any() and (ref["logits1"] == 20).any() and (ref["logits2"] == 0).any() and (ref["logits2"] == 20).any()
    m = _model(stack, 8, w, relu=True, clip=20.0)
    r = m.forward_heads(torch.from_numpy(mel), torch.from_numpy(st))
    _check_against(r, ref, B_MAX, T_MAX, "relu+clip")
    for i in (1, 2):
        lg = _np(r["head%d" % i]["logits"])
        assert lg.min() == 0.0 and lg.max() == 20.0
    m.close()


@pytest.mark.parametrize("stack", [(40, 128, 2), (13, 128, 2)], ids=["resident", "generic"])
def test_seq_len_rows_and_reset(stack):
    w, mel, st, _ = _case(stack, 8)
    b, t = B_MAX, 33
    lens = np.array([0, 1, t - 1, t] * 5, np.int32)[:b]
    ref = HM.heads_forward(w, mel[:, :t], st, lens)
    m = _model(stack, 8, w)
    thres = (0.05, 0.05)          # below softmax(bfc)'s largest word: a row past the length WOULD carry a word
    pw = [torch.full((b,), 2, dtype=torch.int32, device="cuda"), torch.full((b,), 2, dtype=torch.int32, device="cuda")]
    r = m.forward_heads(torch.from_numpy(mel[:, :t].copy()), torch.from_numpy(st), seq_len=torch.from_numpy(lens), prev_words=pw,
                        decode2_thres=thres)
    _check_against(r, ref, b, t, "seq_len")
    nn, state = _np(r["nn_outputs"]), _np(r["state"])
    assert np.abs(state - ref["state"]).max() <= 1e-4
    for k, n in enumerate(lens):
        assert not nn[k, n:].any()                                          # exactly the zero row
        for i, bias in ((1, w["bfc"]), (2, w["bfc2"])):
            h = r["head%d" % i]
            assert np.array_equal(_np(h["logits"])[k, n:], np.broadcast_to(bias, (t - n, len(bias))))      # exactly bfc
            assert not _np(h["tokens"])[k, n:].any()                        # no token
            if n < t:
                assert int(pw[i - 1][k]) == -1                              # ... and no word to carry
            sm_bias = G.softmax(bias.astype(np.float64))
            assert sm_bias[1:len(bias) - 1].max() > thres[i - 1]            # the rule above was needed
        if n == 0:
            assert np.array_equal(state[:, k], st[:, k])                    # the state is carried
        else:
            assert np.array_equal(nn[k, n - 1], state[-1, k])               # the last live row IS the top layer's state
    # the token rule on the live part, from the device's own softmax
    for i, c in ((1, C1), (2, 8)):
        sm, tok = _np(r["head%d" % i]["softmax"]), _np(r["head%d" % i]["tokens"])
        for k, n in enumerate(lens):
            want, last = HM.frame_tokens(sm[k], c, np.float32(thres[i - 1]), prev_word=2, length=n)
            assert np.array_equal(tok[k], want), (i, k)
            assert int(pw[i - 1][k]) == last

    # reset_mask: zero state and both prev_word = -1, over T > 0 ...
    mask = np.array([1, 0] * 9, np.uint8)[:b]
    st0 = st.copy()
    st0[:, mask == 1] = 0
    ref0 = HM.heads_forward(w, mel[:, :t], st0)
    pw = [torch.full((b,), 2, dtype=torch.int32, device="cuda"), torch.full((b,), 1, dtype=torch.int32, device="cuda")]
    r = m.forward_heads(torch.from_numpy(mel[:, :t].copy()), torch.from_numpy(st), reset_mask=torch.from_numpy(mask), prev_words=pw,
                        decode2_thres=thres)
    _check_against(r, ref0, b, t, "reset")
    for i, c, before in ((1, C1, 2), (2, 8, 1)):
        sm, tok = _np(r["head%d" % i]["softmax"]), _np(r["head%d" % i]["tokens"])
        for k in range(b):
            want, _ = HM.frame_tokens(sm[k], c, np.float32(thres[i - 1]), prev_word=-1 if mask[k] else before)
            assert np.array_equal(tok[k], want), (i, k)
    # ... and over zero frames
    pw = [torch.full((b,), 2, dtype=torch.int32, device="cuda"), torch.full((b,), 1, dtype=torch.int32, device="cuda")]
    r = m.forward_heads(torch.from_numpy(mel[:, :0].copy()), torch.from_numpy(st), reset_mask=torch.from_numpy(mask), prev_words=pw)
    assert np.array_equal(_np(r["state"]), st0)
    assert np.array_equal(_np(pw[0]), np.where(mask, -1, 2)) and np.array_equal(_np(pw[1]), np.where(mask, -1, 1))
    assert r["nn_outputs"].shape == (b, 0, stack[1]) and r["head2"]["softmax"].shape == (b, 0, 8)
    m.close()


def _all_outputs(r):
    out = {"state": r["state"], "nn_outputs": r["nn_outputs"]}
    for i in (1, 2):
        for k, v in r["head%d" % i].items():
            out["head%d.%s" % (i, k)] = v
    return out


@pytest.mark.parametrize("stack", [(40, 128, 2), (13, 128, 3)], ids=["resident", "generic"])
def test_chunks_and_batch_composition_are_bitwise(stack):
    w, mel, st, _ = _case(stack, 8, scale=4.0)
    m = _model(stack, 8, w)
    x, s0 = torch.from_numpy(mel).cuda(), torch.from_numpy(st).cuda()
    pw = [m.fresh_prev_word(B_MAX), m.fresh_prev_word(B_MAX)]
    whole = _all_outputs(m.forward_heads(x, s0, prev_words=pw, decode2_thres=(0.4, 0.3)))
    assert int((whole["head1.tokens"] > 0).sum()) > 0 and int((whole["head2.tokens"] > 0).sum()) > 0
    pw2 = [m.fresh_prev_word(B_MAX), m.fresh_prev_word(B_MAX)]
    state, parts, pos = s0, [], 0
    for n in (1, 31, 33):
        r = m.forward_heads(x[:, pos:pos + n].contiguous(), state, prev_words=pw2, decode2_thres=(0.4, 0.3))
        state = r["state"]
        parts.append(_all_outputs(r))
        pos += n
    assert pos == T_MAX
    for k, v in whole.items():
        got = parts[-1][k] if k == "state" else torch.cat([p[k] for p in parts], 1)
        assert torch.equal(got, v), k
    assert torch.equal(pw[0], pw2[0]) and torch.equal(pw[1], pw2[1])
    # stream 0 alone == stream 0 among 17
    pw1 = [m.fresh_prev_word(1), m.fresh_prev_word(1)]
    alone = _all_outputs(m.forward_heads(x[:1].contiguous(), s0[:, :1].contiguous(), prev_words=pw1, decode2_thres=(0.4, 0.3)))
    for k, v in whole.items():
        assert torch.equal(alone[k], v[:, :1] if k == "state" else v[:1]), k
    assert int(pw1[0][0]) == int(pw[0][0]) and int(pw1[1][0]) == int(pw[1][0])
    m.close()


def _margin_ok(softmax_row, thres, eps=1e-4):
    """tests/test_gpu_parity.py: the frame's largest word probability is further than eps from the threshold and -- where it is
    above it, so that WHICH word matters -- further than eps from the runner-up."""
    srt = np.sort(softmax_row[1:5])
    return abs(srt[-1] - thres) > eps and (srt[-1] < thres or (srt[-1] - srt[-2]) > eps)


@pytest.mark.parametrize("stack", [(40, 128, 2), (13, 128, 2), (40, 128, 1)], ids=["resident", "generic", "resident-1-layer"])
def test_head1_agrees_with_kws_step_on_the_same_handle(stack):
    w, mel, st, _ = _case(stack, 8, scale=4.0)
    m = _model(stack, 8, w)
    x, s0 = torch.from_numpy(mel).cuda(), torch.from_numpy(st).cuda()
    pa, pb = m.fresh_prev_word(B_MAX), m.fresh_prev_word(B_MAX)
    a = m.forward(x, s0, prev_word=pa)
    assert "dense_heads" not in "".join(m.kernel_names())               # the plain step keeps its fused epilogue
    r = m.forward_heads(x, s0, heads=(1,), prev_words=(pb, None))
    b = r["head1"]
    d = {k: (u - v).abs().max().item() for k, u, v in (("state", a["state"], r["state"]), ("logits", a["logits"], b["logits"]),
                                                       ("softmax", a["softmax"], b["softmax"]))}
    print("kws_step vs kws_step_heads, head 1:", d, "bitwise:", {k: v == 0.0 for k, v in d.items()})
    assert max(d.values()) <= 2e-5, d
    sm, ta, tb = _np(a["softmax"]), _np(a["tokens"]), _np(b["tokens"])
    checked = 0
    for k in range(B_MAX):
        if all(_margin_ok(row, 0.4) for row in sm[k]):
            assert np.array_equal(ta[k], tb[k]), k
            assert int(pa[k]) == int(pb[k])
            checked += 1
    assert checked >= B_MAX // 2 and (ta > 0).sum() > 0
    m.close()


def test_tokens_follow_each_heads_own_softmax_and_threshold():
    stack = (13, 128, 2)
    w, mel, st, ref = _case(stack, 8, scale=4.0)
    thres = (0.4, 0.6)
    # on the restatement first: both heads emit words at their thresholds, so the device check below cannot pass vacuously
    for i, c in ((1, C1), (2, 8)):
        assert sum(int((HM.frame_tokens(ref["softmax%d" % i][k], c, thres[i - 1])[0] > 0).sum()) for k in range(B_MAX)) >= 1
    m = _model(stack, 8, w)
    pw = [m.fresh_prev_word(B_MAX), m.fresh_prev_word(B_MAX)]
    r = m.forward_heads(torch.from_numpy(mel), torch.from_numpy(st), prev_words=pw, decode2_thres=thres)
    for i, c in ((1, C1), (2, 8)):
        sm, tok = _np(r["head%d" % i]["softmax"]), _np(r["head%d" % i]["tokens"])
        assert (tok > 0).sum() >= 1
        for k in range(B_MAX):
            want, last = HM.frame_tokens(sm[k], c, np.float32(thres[i - 1]))
            assert np.array_equal(tok[k], want), (i, k)
            assert int(pw[i - 1][k]) == last
    assert not np.array_equal(_np(r["head1"]["tokens"]), _np(r["head2"]["tokens"]))
    m.close()


def test_optional_outputs_and_reservation():
    stack = (40, 128, 2)
    w, mel, st, _ = _case(stack, 8)
    m = _model(stack, 8, w)
    x, s0 = torch.from_numpy(mel).cuda(), torch.from_numpy(st).cuda()

    def run(**kw):
        pw = [m.fresh_prev_word(B_MAX), m.fresh_prev_word(B_MAX)]
        out = _all_outputs(dict({"nn_outputs": None, "head1": {}, "head2": {}}, **m.forward_heads(x, s0, prev_words=pw, **kw)))
        out["pw1"], out["pw2"] = pw
        return {k: v for k, v in out.items() if v is not None}
    full = run()
    assert set(full) == {"state", "nn_outputs", "pw1", "pw2"} | {"head%d.%s" % (i, k) for i in (1, 2) for k in ("logits", "softmax", "tokens")}
    for kw, gone in (({"heads": (2,)}, ("head1.", "pw1")), ({"heads": (1,)}, ("head2.", "pw2")), ({"want_nn_outputs": False}, ("nn_outputs",)),
                     ({"want_logits": False}, ("head1.logits", "head2.logits")), ({"want_softmax": False, "want_nn_outputs": False}, ("softmax", "nn_")),
                     ({"heads": ()}, ("head", "pw")), ({"heads": (), "want_nn_outputs": False}, ("head", "pw", "nn_"))):
        part = run(**kw)
        for k, v in full.items():
            if any(g in k for g in gone):
                assert k not in part or k.startswith("pw"), (kw, k)
            else:
                assert torch.equal(part[k], v), (kw, k)
    # one reservation covers both step kinds
    m2 = _model(stack, 8, w)
    m2.reserve(B_MAX, T_MAX)
    allocs = m2.scratch_stats()[1]
    for t in (T_MAX, 33, 1):
        m2.forward(x[:, :t].contiguous(), s0)
        m2.forward_heads(x[:, :t].contiguous(), s0, prev_words=[m2.fresh_prev_word(B_MAX), m2.fresh_prev_word(B_MAX)])
        m2.set_profiling(t == 33)
    torch.cuda.synchronize()
    m2.set_profiling(False)
    assert m2.scratch_stats()[1] == allocs
    m.close()
    m2.close()


def test_selftest_covers_the_heads_step():
    w, _, _, _ = _case((40, 128, 2), 8)
    m = _model((40, 128, 2), 8, w)
    m.selftest()
    m.close()


class _Restated(object):
    """predict_ctc's model, answering from the fp64 restatement."""

    def __init__(self, model, ref):
        self.config, self.num_classes2, self.zero_state, self.ref = model.config, model.num_classes2, model.zero_state, ref

    def run(self, fetches, feed_dict):
        return [torch.from_numpy(self.ref["softmax1"][0].astype(np.float32)), torch.from_numpy(self.ref["softmax2"][0].astype(np.float32)),
                torch.from_numpy(self.ref["top"][0].astype(np.float32))]


def _decisions_have_margin(sm, eps=1e-4):
    """Every comparison ctc_decode / ctc_decode_strict can make on these rows (thresholds 0.5, loose 0.2 -- also on word 3 alone --
    and 0.6; the largest word where it is above the lowest threshold) is decided by more than eps."""
    p = np.sort(sm[:, 1:-1], axis=1)
    top = p[:, -1]
    return all(np.abs(top - thr).min() > eps for thr in (0.5, 0.2, 0.6)) and np.abs(sm[:, 3] - 0.2).min() > eps and \
        bool(((top < 0.2) | (top - p[:, -2] > eps)).all())


def _utterance(seed):
    """Half a second of PCM (48 frames: two frame blocks of the heads kernel): ten tones of random pitch and level in noise."""
    rng = np.random.default_rng(100 + seed)
    t = np.arange(800) / 16000.0
    segs = []
    for _ in range(10):
        f, a = rng.uniform(300, 6000), rng.uniform(0.5, 8.0)
        segs.append(a * np.sin(2 * np.pi * f * t) + 0.3 * a * rng.standard_normal(800))
    return np.concatenate(segs).astype(np.float32)


def test_run_fetches_and_predict_ctc_end_to_end():
    from keyword_spotting_amd.custom_keyword import predict_ctc
    from keyword_spotting_amd.rnn_ctc import FEED_INPUT, FEED_STATE
    stack = (40, 128, 2)
    w, _, _, _ = _case(stack, 8, seed=31, scale=2.0)
    m = _model(stack, 8, w)
    compared = 0
    for seed in range(3):
        pcm = _utterance(seed)
        sm1, sm2, nn, state = m.run(["model/softmax1:0", "model/softmax2:0", "model/nn_outputs:0", "model/rnn_states:0"],
                                    {FEED_INPUT: pcm, FEED_STATE: m.zero_state(1)})
        assert sm1.shape == (48, C1) and sm2.shape == (48, 8) and nn.shape == (48, 128) and state.shape == (2, 1, 128)
        mel = _np(m.frontend.forward(torch.from_numpy(pcm)))[None]
        ref = HM.heads_forward(w, mel)
        assert np.abs(_np(sm1) - ref["softmax1"][0]).max() <= 2e-5 and np.abs(_np(sm2) - ref["softmax2"][0]).max() <= 2e-5
        assert np.abs(_np(nn) - ref["top"][0]).max() <= 1e-4 and np.abs(_np(state) - ref["state"]).max() <= 1e-4
        if not (_decisions_have_margin(ref["softmax1"][0]) and _decisions_have_margin(ref["softmax2"][0])):
            continue
        got, want = predict_ctc(m, pcm, "1233"), predict_ctc(_Restated(m, ref), pcm, "1233")
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert len(got[1]) > 1 and len(got[2]) > 1                    # both heads decoded words
        compared += 1
    assert compared >= 1
    m.close()
