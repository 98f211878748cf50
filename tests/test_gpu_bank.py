"""GPU checks of the utterance step on a bank of enrolled heads (kws_bank_* / kws_step_bank, custom_keyword.KeywordBank): head 2 of
stream b is head 1's logits with the columns of bank slot users[b] spliced in front of the blank.

Against the fp64 restatement tests/bank_model.py: logits and nn_outputs <= 1e-4, softmax <= 2e-5 (the heads' bounds of
tests/test_gpu_heads.py); per-head tokens exact against each head's own device softmax; head 1 and nn_outputs bitwise kws_step_heads'
on the same handle; seq_len rows and reset; chunks bitwise; ISOLATION -- rewriting slot j leaves every stream whose user is not j
bitwise unchanged, and a stream's rows do not depend on which other users share its group; all streams on one slot against
kws_step_heads on extend_head weights; enrol -> kws_bank_set -> kws_step_bank end to end.

Shapes: B in {1, 17} (a partial group, a second group), T in {1, 33, 65} (bank_heads_kernel takes 32 frames per workgroup: a block
boundary and its halo), (C, n_new) in {(6,2), (6,1), (3,5)}, capacity 5, users mixing repeats, every slot, -1 and an out-of-range value."""
import functools

import numpy as np
import pytest
import torch

import bank_model as BM
import heads_model as HM
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu

# (n_mel, hidden, layers): n_mel 40 at hidden 128 takes the resident kernels, everything else the generic ones
STACKS = [(40, 128, 1), (40, 128, 2), (13, 128, 1), (13, 128, 2), (13, 64, 2), (13, 256, 2)]
CN = [(6, 2), (6, 1), (3, 5)]
B_MAX, T_MAX, CAPACITY = 17, 65, 5
USERS = np.array([0, 1, 2, 3, 4, 4, 4, -1, 7, 0, 3, 2, 1, -1, 0, 0, 2], np.int32)          # 7: out of range, reads as -1
VALID = (USERS >= 0) & (USERS < CAPACITY)
THRES = (0.4, 0.3)


def _label_dict(c):
    """A label_dict that gives config.num_classes == c (space, c - 3 words, other, blank)."""
    return {"w%d" % i: i for i in range(1, c - 2)}


def _kernel(stack):
    return "auto" if stack[:2] == (40, 128) else "generic"


def _bank(stack, c, n_new, w, cols, bias):
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.custom_keyword import KeywordBank
    from keyword_spotting_amd.rnn_ctc import DeployModel
    one = DeployModel(get_config(n_mel=stack[0], hidden_size=stack[1], num_layers=stack[2], label_dict=_label_dict(c)), w, kernel=_kernel(stack))
    bank = KeywordBank(one, n_new, cols.shape[0], kernel=_kernel(stack))
    one.close()
    return bank.set(0, cols, bias)


@functools.lru_cache(maxsize=None)
def _case(stack, c, n_new, seed=11, scale=1.0):
    """Weights, bank, inputs and the fp64 restatement of the largest shape; the GRU is causal and streams are independent, so every
    smaller (B, T) is a slice of it.  Computed once, never modified."""
    w = G.random_weights(stack[0], stack[1], stack[2], c, seed)
    w["Wfc"] = (w["Wfc"] * scale).astype(np.float32)
    cols, bias = BM.random_bank(stack[1], n_new, CAPACITY, seed, scale=scale)
    mel = G.synthetic_mel(B_MAX, T_MAX, stack[0], seed=seed + 1)
    st = (0.3 * np.random.default_rng(seed + 2).standard_normal((stack[2], B_MAX, stack[1]))).astype(np.float32)
    return w, cols, bias, mel, st, BM.bank_forward(w, cols, bias, USERS, mel, st)


def _np(x):
    return x.cpu().numpy()


def _all_outputs(r):
    out = {"state": r["state"], "nn_outputs": r["nn_outputs"]}
    for i in (1, 2):
        for k, v in r["head%d" % i].items():
            out["head%d.%s" % (i, k)] = v
    return out


def _check_against(r, ref, b, t, what):
    for i in (1, 2):
        lg, sm = _np(r["head%d" % i]["logits"]), _np(r["head%d" % i]["softmax"])
        el = np.abs(lg - ref["logits%d" % i][:b, :t]).max()
        es = np.abs(sm - ref["softmax%d" % i][:b, :t]).max()
        print("%s head%d: max|dlogit| %.2e max|dsoftmax| %.2e" % (what, i, el, es))
        assert el <= 1e-4 and es <= 2e-5, (what, i, el, es)
        rows = sm.astype(np.float64).sum(-1)
        live = np.ones(b, bool) if i == 1 else VALID[:b]
        assert np.abs(rows[live] - 1).max(initial=0) <= 1e-6
        if i == 2:
            assert not lg[~live].any() and not sm[~live].any()              # no slot: exactly zero rows
    en = np.abs(_np(r["nn_outputs"]) - ref["top"][:b, :t]).max()
    print("%s max|dnn_outputs| %.2e" % (what, en))
    assert en <= 1e-4, (what, en)


@pytest.mark.parametrize("cn", CN, ids=lambda v: "c%d-n%d" % v)
@pytest.mark.parametrize("stack", STACKS, ids=lambda s: "mel%d-h%d-l%d" % s)
def test_bank_step_matches_the_restatement_and_head1_is_kws_step_heads(stack, cn):
    c, n_new = cn
    w, cols, bias, mel, st, ref = _case(stack, c, n_new)
    bank = _bank(stack, c, n_new, w, cols, bias)
    got_w, got_b = bank.get()
    assert np.array_equal(_np(got_w), cols) and np.array_equal(_np(got_b), bias)            # kws_bank_set / kws_bank_get
    for b in (1, B_MAX):
        for t in (1, 33, T_MAX):
            x, s0, users = torch.from_numpy(mel[:b, :t].copy()), torch.from_numpy(st[:, :b].copy()), USERS[:b]
            pw = [torch.full((b,), 2, dtype=torch.int32, device="cuda"), torch.full((b,), 1, dtype=torch.int32, device="cuda")]
            r = bank.forward(x, s0, users, prev_words=pw, decode2_thres=THRES)
            names = bank.stack.kernel_names()
            _check_against(r, ref, b, t, "B=%d T=%d" % (b, t))
            if t == T_MAX:
                assert np.abs(_np(r["state"]) - ref["state"][:, :b]).max() <= 1e-4
            # tokens: exact against each head's own device softmax; a stream without a slot has none and carries no word
            for i, classes, before in ((1, c, 2), (2, c + n_new, 1)):
                sm, tok = _np(r["head%d" % i]["softmax"]), _np(r["head%d" % i]["tokens"])
                for k in range(b):
                    if i == 2 and not VALID[k]:
                        assert not tok[k].any() and int(pw[1][k]) == -1
                        continue
                    want, last = HM.frame_tokens(sm[k], classes, np.float32(THRES[i - 1]), prev_word=before)
                    assert np.array_equal(tok[k], want), (i, k)
                    assert int(pw[i - 1][k]) == last
            # head 1 and nn_outputs: the bits of kws_step_heads on the same handle
            pw1 = torch.full((b,), 2, dtype=torch.int32, device="cuda")
            h = bank.stack.forward_heads(x, s0, heads=(1,), prev_words=(pw1, None), decode2_thres=THRES)
            for k in ("logits", "softmax", "tokens"):
                assert torch.equal(r["head1"][k], h["head1"][k]), k
            assert torch.equal(r["nn_outputs"], h["nn_outputs"]) and torch.equal(r["state"], h["state"]) and torch.equal(pw[0], pw1)
    family = "gru_layer_resident" if stack[:2] == (40, 128) else "gru_layer_generic"
    assert all(n.startswith(family) and ", false>" in n for n in names), names          # no layer is `last`
    assert names[-1].endswith(" + bank_heads_kernel<%d>" % (stack[1] // 16)) and "bank_heads" not in "".join(names[:-1]), names
    bank.close()


@pytest.mark.parametrize("stack", [(40, 128, 2), (13, 128, 2)], ids=["resident", "generic"])
def test_seq_len_rows_and_reset(stack):
    c, n_new = 6, 2
    w, cols, bias, mel, st, _ = _case(stack, c, n_new)
    b, t = B_MAX, 33
    lens = np.array([0, 1, t - 1, t] * 5, np.int32)[:b]
    ref = BM.bank_forward(w, cols, bias, USERS, mel[:, :t], st, lens)
    bank = _bank(stack, c, n_new, w, cols, bias)
    thres = (0.05, 0.05)          # below softmax(bias)'s largest word: a row past the length WOULD carry a word
    pw = [torch.full((b,), 2, dtype=torch.int32, device="cuda"), torch.full((b,), 2, dtype=torch.int32, device="cuda")]
    r = bank.forward(torch.from_numpy(mel[:, :t].copy()), torch.from_numpy(st), USERS, seq_len=torch.from_numpy(lens), prev_words=pw,
                     decode2_thres=thres)
    _check_against(r, ref, b, t, "seq_len")
    nn, l1, l2 = _np(r["nn_outputs"]), _np(r["head1"]["logits"]), _np(r["head2"]["logits"])
    for k, n in enumerate(lens):
        assert not nn[k, n:].any()                                                       # exactly the zero row
        assert np.array_equal(l1[k, n:], np.broadcast_to(w["bfc"], (t - n, c)))          # exactly bfc
        assert not _np(r["head1"]["tokens"])[k, n:].any() and not _np(r["head2"]["tokens"])[k, n:].any()
        if VALID[k]:      # head 1's bias around the slot's own bias, exactly
            want = np.concatenate([w["bfc"][:c - 1], bias[USERS[k]], w["bfc"][c - 1:]])
            assert np.array_equal(l2[k, n:], np.broadcast_to(want, (t - n, c + n_new))), k
        if n < t:
            assert int(pw[0][k]) == -1 and int(pw[1][k]) == -1                           # ... and no word to carry
    for i, classes in ((1, c), (2, c + n_new)):
        sm, tok = _np(r["head%d" % i]["softmax"]), _np(r["head%d" % i]["tokens"])
        for k, n in enumerate(lens):
            if i == 2 and not VALID[k]:
                continue
            want, last = HM.frame_tokens(sm[k], classes, np.float32(thres[i - 1]), prev_word=2, length=n)
            assert np.array_equal(tok[k], want), (i, k)
            assert int(pw[i - 1][k]) == last
    # reset_mask: zero state and both prev_word = -1
    mask = np.array([1, 0] * 9, np.uint8)[:b]
    st0 = st.copy()
    st0[:, mask == 1] = 0
    ref0 = BM.bank_forward(w, cols, bias, USERS, mel[:, :t], st0)
    pw = [torch.full((b,), 2, dtype=torch.int32, device="cuda"), torch.full((b,), 1, dtype=torch.int32, device="cuda")]
    r = bank.forward(torch.from_numpy(mel[:, :t].copy()), torch.from_numpy(st), USERS, reset_mask=torch.from_numpy(mask), prev_words=pw,
                     decode2_thres=thres)
    _check_against(r, ref0, b, t, "reset")
    for i, classes, before in ((1, c, 2), (2, c + n_new, 1)):
        sm, tok = _np(r["head%d" % i]["softmax"]), _np(r["head%d" % i]["tokens"])
        for k in range(b):
            if i == 2 and not VALID[k]:
                continue
            want, _ = HM.frame_tokens(sm[k], classes, np.float32(thres[i - 1]), prev_word=-1 if mask[k] else before)
            assert np.array_equal(tok[k], want), (i, k)
    bank.close()


@pytest.mark.parametrize("stack", [(40, 128, 2), (13, 128, 2), (13, 256, 2)], ids=["resident", "generic", "h256"])
def test_chunks_are_bitwise_and_streams_are_isolated(stack):
    c, n_new = 6, 2
    w, cols, bias, mel, st, _ = _case(stack, c, n_new, scale=4.0)
    bank = _bank(stack, c, n_new, w, cols, bias)
    x, s0 = torch.from_numpy(mel).cuda(), torch.from_numpy(st).cuda()

    def run(xs, state, users, chunks=(T_MAX,)):
        pw = [bank.stack.fresh_prev_word(xs.shape[0]), bank.stack.fresh_prev_word(xs.shape[0])]
        parts, pos = [], 0
        for n in chunks:
            r = bank.forward(xs[:, pos:pos + n].contiguous(), state, users, prev_words=pw, decode2_thres=THRES)
            state = r["state"]
            parts.append(_all_outputs(r))
            pos += n
        out = {k: parts[-1][k] if k == "state" else torch.cat([p[k] for p in parts], 1) for k in parts[0]}
        out["pw1"], out["pw2"] = pw
        return out
    whole = run(x, s0, USERS)
    assert int((whole["head1.tokens"] > 0).sum()) > 0 and int((whole["head2.tokens"] > 0).sum()) > 0
    # chunks of 1, 31 and 33 frames == one call
    for k, v in run(x, s0, USERS, (1, 31, 33)).items():
        assert torch.equal(v, whole[k]), k
    # a stream alone == the same stream inside B = 17, whatever users share its group (streams 0, 4 and 16: a second group)
    for s in (0, 4, 16):
        alone = run(x[s:s + 1].contiguous(), s0[:, s:s + 1].contiguous(), USERS[s:s + 1])
        for k, v in whole.items():
            assert torch.equal(alone[k], v[:, s:s + 1] if k == "state" else v[s:s + 1]), (s, k)
    # ... and with every OTHER stream moved to another slot
    for s in (0, 4, 16):
        others = np.where(np.arange(B_MAX) == s, USERS, (USERS + 1) % CAPACITY).astype(np.int32)
        moved = run(x, s0, others)
        for k, v in whole.items():
            assert torch.equal(moved[k][:, s] if k == "state" else moved[k][s], v[:, s] if k == "state" else v[s]), (s, k)
        assert not torch.equal(moved["head2.logits"], whole["head2.logits"])
    # rewriting slot j leaves every stream whose user is not j bitwise unchanged, and changes the streams on j
    j = 4
    new_cols, new_bias = BM.random_bank(stack[1], n_new, 1, seed=99, scale=4.0)
    bank.set(j, new_cols, new_bias)
    after = run(x, s0, USERS)
    keep = torch.from_numpy(USERS != j).cuda()
    for k, v in whole.items():
        if k == "state":
            assert torch.equal(after[k], v)
        else:
            assert torch.equal(after[k][keep], v[keep]), k
    on_j = torch.from_numpy(USERS == j).cuda()
    assert not torch.equal(after["head2.logits"][on_j], whole["head2.logits"][on_j])
    for k in ("head1.logits", "head1.softmax", "head1.tokens", "nn_outputs"):
        assert torch.equal(after[k], whole[k]), k
    bank.close()


@pytest.mark.parametrize("cn", CN, ids=lambda v: "c%d-n%d" % v)
def test_all_streams_on_one_slot_against_kws_step_heads_on_extend_head_weights(cn):
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.rnn_ctc import DeployModel
    c, n_new = cn
    stack = (40, 128, 2)
    w, cols, bias, mel, st, _ = _case(stack, c, n_new)
    bank = _bank(stack, c, n_new, w, cols, bias)
    x, s0 = torch.from_numpy(mel).cuda(), torch.from_numpy(st).cuda()
    for u in (0, 3):
        w2 = dict(w)
        w2["Wfc2"], w2["bfc2"] = weights.extend_head(w["Wfc"], w["bfc"], cols[u], bias[u])
        cfg = get_config(n_mel=stack[0], hidden_size=stack[1], num_layers=stack[2], label_dict=_label_dict(c))
        cfg.num_classes2 = c + n_new
        served = DeployModel(cfg, w2)
        want = served.forward_heads(x, s0)
        got = bank.forward(x, s0, np.full(B_MAX, u, np.int32))
        for k in ("logits", "softmax"):
            assert torch.equal(got["head1"][k], want["head1"][k]), k
        assert torch.equal(got["nn_outputs"], want["nn_outputs"])
        d = {k: (got["head2"][k] - want["head2"][k]).abs().max().item() for k in ("logits", "softmax")}
        print("c=%d n_new=%d slot %d: head 2 against kws_step_heads on extend_head weights (informational: the new classes are summed "
              "in another order there):" % (c, n_new, u), d)
        old = list(range(c - 1)) + [c + n_new - 1]           # the frozen logits are head 1's accumulator: the same bits in both
        assert torch.equal(got["head2"]["logits"][..., old], want["head2"]["logits"][..., old])
        served.close()
    bank.close()


@pytest.mark.parametrize("seed", [0, 2])
def test_enrol_set_serve_end_to_end(seed):
    """E = 2 users enrol the words 5 6 on different utterances in one fit; its device tensors go into the bank with one kws_bank_set;
    each user's training utterances decode to the new words through their own slot (utterances on which the fp64 restatement does)."""
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.custom_keyword import Enroller, KeywordBank, truncated_normal
    from keyword_spotting_amd.prediction import ctc_decode2, ctc_label
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg = get_config()
    model = DeployModel(cfg, weights.init_weights(cfg, seed=seed))
    mel = np.concatenate([G.synthetic_mel(3, 48, cfg.n_mel, seed=seed + 10), G.synthetic_mel(3, 48, cfg.n_mel, seed=seed + 20)])
    init = (np.stack([truncated_normal((1, cfg.hidden_size, 2), seed)[0], truncated_normal((1, cfg.hidden_size, 2), 1)[0]]),
            np.zeros((2, 2), np.float32))
    enroller = Enroller(model, 2, enrolments=2, utterances_per_enrolment=3)
    wn, bn, _ = enroller.fit(torch.from_numpy(mel), [48] * 6, list(ctc_label([5, 6])), 300, lr=0.03, init=init)
    enroller.close()
    assert wn.is_cuda and tuple(wn.shape) == (2, cfg.hidden_size, 2)
    bank = KeywordBank(model, 2, 4)
    bank.set(1, wn, bn)                                      # users 0 and 1 live in slots 1 and 2; slots 0 and 3 stay zero
    users = np.array([1, 1, 1, 2, 2, 2], np.int32)
    r = bank.forward(torch.from_numpy(mel), bank.zero_state(6), users, want_nn_outputs=False, want_logits=False)
    sm2 = _np(r["head2"]["softmax"])
    for i in range(6):
        words = [int(v) for v in ctc_decode2(sm2[i], 8)[1::2]]
        assert 5 in words and 6 in words[words.index(5) + 1:], (i, words)
    # through the OTHER user's slot the same utterances give other rows
    swapped = bank.forward(torch.from_numpy(mel), bank.zero_state(6), users[::-1].copy(), want_nn_outputs=False, want_logits=False)
    assert not torch.equal(swapped["head2"]["softmax"], r["head2"]["softmax"]) and torch.equal(swapped["head1"]["softmax"], r["head1"]["softmax"])
    bank.close()
    model.close()
