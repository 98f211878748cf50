"""GPU checks of the bank stream manager (kws_stream_create_bank / kws_step_bank_window, StreamManager(bank=, users=, label2=)): one
manager serves streams whose users each enrolled their own keyword -- head 2 of stream b comes from bank slot users[b].

  1. manager == host mirror (HotwordDetector(bank=, users=, label2=)), exactly: hit bitmasks and states, every chunk
  2. manager == the fp64 policy loop (tests/bank_model.policy_loop) up to a stream's first frame at a decision edge
  3. the optional softmax outputs are bitwise kws_step_bank's rows at T in {1, 33, 0}
  4. the PCM path with ragged lengths, skips and recycling, a recycled slot handed to another user
  5. launch names; 6. a bank manager, a heads manager and a plain manager on one model handle; 7. the LDS refusal

Inputs.  17 streams over 4 users plus -1: USERS below.  Streams 8..15 are fed the audio of streams 0..7 under ANOTHER user, so
that what differs between the two is the bank slot alone.  Head 1: oracle.random_weights with Wfc scaled by 3, label "12"; the
bank: bank_model.random_bank scaled by 3 (drawn as tests/test_gpu_heads.py draws head 2), label2 "5": the first new word of every
user (C = 6).  Thresholds 0.4 / 0.5.  The seeds were chosen with the fp64 restatement alone (no GPU) so that head-1-only,
head-2-only and both-heads chunks each occur >= 3 times and at least 3 (chunk, stream pair) cases exist where two streams with
the same audio and different users differ in hit_2; at least half of all (stream, chunk) pairs lie before the stream's first
decision edge.  The tests assert those conditions on the restatement and fail if they do not hold.
Shapes: chunks of 21-23 frames, windows of 1 / 15 / 17 chunks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bank_model as BM
from oracle import decode_oracle as D
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu

C1 = 6
THRES = (0.4, 0.5)
LABEL1, LABEL2 = "12", "5"
B, CAPACITY = 17, 4
USERS = np.array([0, 1, 2, 3, 0, 1, 2, -1, 1, 2, 3, 0, -1, 3, 0, 1, 2], np.int32)
PAIRS = [(i, i + 8) for i in range(8)]          # the same audio, another user
# name: ((n_mel, hidden, layers), n_new, window_chunks, seed)
CASES = {
    "resident": ((40, 128, 2), 2, 15, 2),
    "single-layer-window17": ((13, 128, 1), 1, 17, 14),
    "h64": ((13, 64, 2), 2, 15, 2),
    "h256-window1": ((13, 256, 2), 2, 1, 7),
}
N_CHUNKS = 60


def _label_dict(c):
    """A label_dict that gives config.num_classes == c (space, c - 3 words, other, blank)."""
    return {"w%d" % i: i for i in range(1, c - 2)}


def _kernel(stack):
    return "auto" if stack[:2] == (40, 128) else "generic"


def _weights(stack, seed, c1=C1):
    w = G.random_weights(stack[0], stack[1], stack[2], c1, seed)
    w["Wfc"] = (w["Wfc"] * 3).astype(np.float32)
    return w


def _bank(stack, n_new, w, cols, bias, c1=C1):
    """A KeywordBank on a one-head model of `w` with its slots set -> the bank (its stack is the model handle of the bank calls)."""
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.custom_keyword import KeywordBank
    from keyword_spotting_amd.rnn_ctc import DeployModel
    one = DeployModel(get_config(n_mel=stack[0], hidden_size=stack[1], num_layers=stack[2], label_dict=_label_dict(c1)), w, kernel=_kernel(stack))
    bank = KeywordBank(one, n_new, cols.shape[0], kernel=_kernel(stack))
    one.close()
    return bank.set(0, cols, bias)


def _close(*banks):
    for bank in banks:
        bank.close()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    stack, n_new, _, seed = CASES[name]
    chunks = D.chunk_frame_counts([3600] * N_CHUNKS)
    mel = G.synthetic_mel(B, sum(chunks), stack[0], seed=seed + 1)
    for i, j in PAIRS:
        mel[j] = mel[i]
    speech = np.random.default_rng(seed + 2).random((len(chunks), B)) > 0.05          # occasional silence
    for i, j in PAIRS:
        speech[:, j] = speech[:, i]
    cols, bias = BM.random_bank(stack[1], n_new, CAPACITY, seed, scale=3.0)
    return _weights(stack, seed), cols, bias, mel, chunks, speech


@functools.lru_cache(maxsize=None)
def _policy(name):
    """The fp64 restatement of the whole loop; computed once, never modified."""
    w, cols, bias, mel, chunks, speech = _inputs(name)
    return BM.policy_loop(w, cols, bias, USERS, mel, chunks, speech, (LABEL1, LABEL2), THRES, CASES[name][2])


def _kinds(mask):
    return [int((mask == k).sum()) for k in (1, 2, 3)]


def _pair_differences(mask):
    """(chunk, stream pair) cases where two streams with the same audio and two different users (both with a slot) differ in hit_2."""
    return sum(int(((mask[:, i] ^ mask[:, j]) & 2 > 0).sum()) for i, j in PAIRS if USERS[i] >= 0 and USERS[j] >= 0 and USERS[i] != USERS[j])


def _input_conditions(name):
    pol = _policy(name)
    kinds, pairs = _kinds(pol["mask"]), _pair_differences(pol["mask"])
    print(name, "restatement: head 1 alone / head 2 alone / both:", kinds, "same audio, other user, other hit_2:", pairs)
    assert min(kinds) >= 3, kinds
    assert pairs >= 3, pairs
    assert not (pol["mask"][:, USERS < 0] & 2).any()          # a stream without a slot never reports head 2
    return pol


@functools.lru_cache(maxsize=None)
def _run(name):
    """Manager and host mirror on two banks with the same contents over the case's chunks -> per chunk the two bitmasks and whether
    the states were equal; and the kernel names after the last feed."""
    from keyword_spotting_amd.detector import HotwordDetector, StreamManager
    stack, n_new, window, _ = CASES[name]
    w, cols, bias, mel, chunks, speech = _inputs(name)
    x = torch.from_numpy(mel).cuda()
    kw = dict(label=LABEL1, label2=LABEL2, decode_thres=THRES[0], decode_thres2=THRES[1], window_chunks=window, users=USERS)
    b_mgr, b_det = _bank(stack, n_new, w, cols, bias), _bank(stack, n_new, w, cols, bias)
    mgr, det = StreamManager(None, B, bank=b_mgr, **kw), HotwordDetector(None, batch=B, bank=b_det, **kw)
    got, want, same_state, pos = [], [], [], 0
    for ci, n in enumerate(chunks):
        chunk = x[:, pos:pos + n].clone()
        det.feed(chunk, speech=speech[ci])
        want.append(det.hit_mask.copy())
        got.append(mgr.feed(chunk, speech=torch.from_numpy(speech[ci])).cpu().numpy().copy())
        same_state.append(torch.equal(mgr.state, det.state))
        pos += n
    names = b_mgr.stack.kernel_names()
    mgr.close()
    _close(b_mgr, b_det)
    return dict(got=np.stack(got), want=np.stack(want), same_state=same_state, names=names)


@pytest.mark.parametrize("name", list(CASES))
def test_manager_equals_the_host_mirror_exactly(name):
    _input_conditions(name)
    r = _run(name)
    for ci in range(N_CHUNKS):
        np.testing.assert_array_equal(r["got"][ci], r["want"][ci], err_msg="%s chunk %d" % (name, ci))
        assert r["same_state"][ci], (name, ci)
    dk = _kinds(r["want"])
    print(name, "device: head 1 alone / head 2 alone / both:", dk, "pair differences:", _pair_differences(r["want"]))
    assert min(dk) >= 3 and _pair_differences(r["want"]) >= 3
    assert not (r["got"][:, USERS < 0] & 2).any()


@pytest.mark.parametrize("name", list(CASES))
def test_manager_follows_the_fp64_policy_loop(name):
    pol = _input_conditions(name)
    ok = np.cumprod(pol["margin_ok"], 0).astype(bool)          # a stream is compared up to its first chunk with a frame at an edge
    assert ok.mean() >= 0.5, ok.mean()                         # the cap, met by the restatement alone
    r = _run(name)
    differ = (r["got"] != pol["mask"]) & ok
    print(name, "compared %.0f %% of the (stream, chunk) pairs, %d hits among them" % (100 * ok.mean(), int((pol["mask"][ok] > 0).sum())))
    assert not differ.any(), np.argwhere(differ)[:5]
    assert int(((pol["mask"] & 2 > 0) & ok).sum()) >= 1        # head 2 fires inside what was compared


@pytest.mark.parametrize("name", list(CASES))
def test_launch_names(name):
    stack = CASES[name][0]
    names = _run(name)["names"]
    family = "gru_layer_resident" if stack[:2] == (40, 128) else "gru_layer_generic"
    assert len(names) == stack[2] and all(n.startswith(family) and ", false>" in n for n in names), names          # no layer is `last`
    assert names[-1].endswith(" + bank_heads_window_kernel<%d>" % (stack[1] // 16)), names
    assert "bank_heads" not in "".join(names[:-1]) and not any("window_inc" in n or "dense_heads" in n for n in names), names


@pytest.mark.parametrize("name", list(CASES))
def test_softmax_outputs_are_bitwise_kws_step_bank(name):
    """max_frames = 40, mel chunks of 1 and 33 frames (the 32-frame block of the kernel's loop) and of none: both optional softmax
    outputs against KeywordBank.forward on the same handles from the same state; hits and states against the mirror."""
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.detector import HotwordDetector, StreamManager
    lib = _lib.load()
    stack, n_new, window, seed = CASES[name]
    w, cols, bias = _inputs(name)[:3]
    kw = dict(label=LABEL1, label2=LABEL2, decode_thres=THRES[0], decode_thres2=THRES[1], window_chunks=window, users=USERS)
    b_mgr, b_det = _bank(stack, n_new, w, cols, bias), _bank(stack, n_new, w, cols, bias)
    mgr, det = StreamManager(None, B, max_frames=40, bank=b_mgr, **kw), HotwordDetector(None, batch=B, bank=b_det, **kw)
    mgr.state.copy_(torch.from_numpy((0.3 * np.random.default_rng(seed).standard_normal(tuple(mgr.state.shape))).astype(np.float32)))
    det.state.copy_(mgr.state)
    lens = [1, 33, 0, 33, 1, 33, 33]
    x = torch.from_numpy(G.synthetic_mel(B, sum(lens), stack[0], seed=seed + 5)).cuda()
    rng = np.random.default_rng(seed + 6)
    pos = 0
    for n in lens:
        chunk = x[:, pos:pos + n].clone()
        speech = rng.random(B) > 0.1
        before = mgr.state.clone()
        silent = torch.from_numpy(~speech).cuda().to(torch.uint8)
        reset = torch.maximum(mgr.restart, silent)
        sm1, sm2 = torch.empty(B, n, C1, device="cuda"), torch.empty(B, n, C1 + n_new, device="cuda")
        model = b_mgr.stack
        with torch.cuda.device(model.device):
            _lib.check(lib.kws_step_bank_window(model._handle, b_mgr._handle, _lib.ptr(mgr.users), _lib.ptr(chunk), _lib.ptr(mgr.state),
                                                _lib.ptr(mgr.state), _lib.ptr(reset), B, n, mgr._win, mgr._win2, mgr.label, mgr.label2,
                                                _lib.ptr(silent), _lib.ptr(sm1), _lib.ptr(sm2), _lib.ptr(mgr.hit), _lib.ptr(mgr.restart),
                                                _lib.current_stream_ptr()))
        got = mgr.hit.cpu().numpy()
        ref = b_mgr.forward(chunk, before, mgr.users, reset_mask=reset, want_nn_outputs=False, want_logits=False)
        assert torch.equal(sm1, ref["head1"]["softmax"]) and torch.equal(sm2, ref["head2"]["softmax"]), (name, n)
        assert not sm2[torch.from_numpy(USERS < 0).cuda()].any()
        assert torch.equal(mgr.state, ref["state"])
        det.feed(chunk, speech=speech)
        np.testing.assert_array_equal(got, det.hit_mask, err_msg="%s T=%d" % (name, n))
        assert torch.equal(mgr.state, det.state)
        pos += n
    mgr.close()
    _close(b_mgr, b_det)


# ---- the PCM path -----------------------------------------------------------------------------------------------------
_PCM = {}


def _pcm_setup():
    """(front-end, weights, columns, bias, (label1, label2)) at the reference shape: each head's most frequent word on noise through the
    real front-end as its one-digit label -- head 2's among the NEW words (digits C1 - 1, C1), over all users."""
    if not _PCM:
        from keyword_spotting_amd import get_config
        from keyword_spotting_amd.frontend import MelFrontend
        stack, n_new, seed = (40, 128, 2), 2, 7319
        fe = MelFrontend(get_config())
        w = _weights(stack, seed)
        noise = torch.from_numpy((np.random.default_rng(8100).standard_normal((48, 16000)) * 0.2).astype(np.float32))
        cols, bias = BM.random_bank(stack[1], n_new, CAPACITY, seed, scale=4.0)
        bank = _bank(stack, n_new, w, cols, bias)
        mel, users = fe.forward(noise), np.arange(48) % CAPACITY
        for bank_seed in range(seed, seed + 60):       # the first bank whose users say their new words often enough on this noise
            cols, bias = BM.random_bank(stack[1], n_new, CAPACITY, bank_seed, scale=4.0)
            r = bank.set(0, cols, bias).forward(mel, bank.zero_state(48), users, want_nn_outputs=False, want_logits=False)
            words = [np.concatenate([D.ctc_decode2(r["head%d" % i]["softmax"][k].cpu().numpy(), c, THRES[i - 1])[1::2] for k in range(48)])
                     for i, c in ((1, C1), (2, C1 + n_new))]
            new = words[1][words[1] >= C1 - 1]          # the new words are the digits C1 - 1 .. C1 + n_new - 2
            if len(words[0]) >= 40 and len(new) >= 40:
                break
        else:
            bank.close()
            raise AssertionError("no bank among 60 seeds whose users emit their new words on this noise")
        bank.close()
        print("PCM setup: bank seed %d, %d head-1 words, %d new words" % (bank_seed, len(words[0]), len(new)))
        _PCM["v"] = (fe, w, cols, bias, (str(int(np.bincount(words[0]).argmax())), str(int(np.bincount(new).argmax()))))
    return _PCM["v"]


def _bank_manager(bank, b, users, labels, **kw):
    from keyword_spotting_amd.detector import StreamManager
    return StreamManager(None, b, bank=bank, users=users, label=labels[0], label2=labels[1], decode_thres=THRES[0], decode_thres2=THRES[1], **kw)


def test_ragged_lengths_skips_and_recycling_to_another_user():
    """Stream s of a ragged bank manager gets, bit for bit, what a lock-step bank manager gets when fed stream s's chunks alone under
    stream s's user -- on the periods where it had data, and nothing on the others.  Mid-run two streams are recycled and handed to
    ANOTHER user (users[s] rewritten on the device): from there on their oracle is a fresh manager under the new user."""
    fe, w, cols, bias, labels = _pcm_setup()
    stack, n_new = (40, 128, 2), 2
    periods, n_max, at = 12, 5000, 6
    recycled = {2: 3, 7: 1, 16: -1}                                   # stream -> its user after the recycle (7 had none; 16 loses its)
    rng = np.random.default_rng(8300)
    lens = rng.choice([0, 150, 1800, 3600, 5000], size=(B, periods), p=[0.15, 0.1, 0.2, 0.4, 0.15]).astype(np.int32)
    lens[3, :2] = 150                                                 # a stream that opens with sub-frame chunks
    chunks = []
    for p in range(periods):
        pad = rng.integers(-32768, 32767, (B, n_max)).astype(np.int16)          # loud padding that must never reach a result
        data = (rng.integers(-6000, 6000, (B, n_max)) * rng.choice([0.25, 1.0, 3.0], (B, 1))).astype(np.int16)
        data[rng.random(B) < 0.05] //= 4096
        chunks.append(np.where(np.arange(n_max)[None, :] < lens[:, p:p + 1], data, pad).astype(np.int16))
    b_rag, b_ora = _bank(stack, n_new, w, cols, bias), _bank(stack, n_new, w, cols, bias)
    rag = _bank_manager(b_rag, B, USERS, labels)
    hits = np.zeros((B, periods), np.int32)
    for p in range(periods):
        if p == at:
            rag.recycle(list(recycled))
            for s, u in recycled.items():
                rag.users[s] = u
        hits[:, p] = rag.feed_pcm(torch.from_numpy(chunks[p]).cuda(), fe, lengths=torch.from_numpy(lens[:, p])).cpu().numpy()
    torch.cuda.synchronize()
    assert "bank_heads_window_kernel<8>" in b_rag.stack.kernel_names()[-1]
    print("ragged bank manager: head 1 alone / head 2 alone / both:", _kinds(hits))
    assert (hits & 1).sum() > 0 and (hits & 2).sum() > 0, "no trigger: the run does not cover both heads"
    assert (lens == 0).any()
    for s in (0, 2, 3, 7, 9, 12, 16):                                 # every recycled stream, users 0..3 and -1 among the others
        user = int(USERS[s])
        oracle = _bank_manager(b_ora, B, np.full(B, user, np.int32), labels)
        for p in range(periods):
            if p == at and s in recycled:
                oracle.close()
                user = recycled[s]
                oracle = _bank_manager(b_ora, B, np.full(B, user, np.int32), labels)
            n = int(lens[s, p])
            if n == 0:
                assert hits[s, p] == 0, (s, p)
                continue
            row = torch.from_numpy(np.repeat(chunks[p][s:s + 1, :n], B, 0)).cuda()
            want = int(oracle.feed_pcm(row, fe)[0].item())
            assert hits[s, p] == want, (s, p, n)
            assert user >= 0 or not want & 2
        torch.cuda.synchronize()
        assert torch.equal(rag.state[:, s], oracle.state[:, 0]), s
        assert int(rag.restart[s]) == int(oracle.restart[0]), s
        oracle.close()
    rag.close()
    _close(b_rag, b_ora)


def test_bank_heads_and_plain_managers_coexist_on_one_model():
    """A bank manager, a two-head manager (the handle's own second head) and a plain manager on ONE model handle, fed in turn, each
    equal to itself alone on a handle of its own."""
    from keyword_spotting_amd.detector import StreamManager
    fe, w, cols, bias, labels = _pcm_setup()
    stack, n_new = (40, 128, 2), 2
    shared, alone = _bank(stack, n_new, w, cols, bias), [_bank(stack, n_new, w, cols, bias) for _ in range(3)]

    def trio(banks):
        return [_bank_manager(banks[0], B, USERS, labels),
                StreamManager(banks[1].stack, B, label=labels[0], label2=labels[1], decode_thres=THRES[0], decode_thres2=THRES[1]),
                StreamManager(banks[2].stack, B, label=labels[0], decode_thres=THRES[0])]
    together, apart = trio([shared] * 3), trio(alone)
    rng = np.random.default_rng(8500)
    fired = [0, 0, 0]
    for k in range(14):
        x = torch.from_numpy(rng.integers(-6000, 6000, (B, 3600)).astype(np.int16)).cuda()
        for i, (m, ref) in enumerate(zip(together, apart)):
            got = m.feed_pcm(x, fe).clone()
            assert torch.equal(got, ref.feed_pcm(x, fe)) and torch.equal(m.state, ref.state), (k, i)
            fired[i] += int((got > 0).sum())
    print("hits of the bank / two-head / plain manager:", fired)
    assert fired[0] > 0 and fired[2] > 0
    for m in together + apart:
        m.close()
    _close(shared, *alone)


def test_refusals_on_live_handles():
    """What needs live handles to be refused: a bank of another shape than the model, window 2 with another class count than
    C + n_new, a model without a second head, slots past the capacity, and the LDS total with its byte counts."""
    from keyword_spotting_amd import _lib, get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    lib = _lib.load()
    stack, n_new, c1 = (13, 256, 1), 5, 3
    w = _weights(stack, 5, c1)
    cols, bias = BM.random_bank(stack[1], n_new, 2, 5)
    bank = _bank(stack, n_new, w, cols, bias, c1)
    model = bank.stack
    one = DeployModel(get_config(n_mel=13, hidden_size=256, num_layers=1, label_dict=_label_dict(c1)), w, kernel="generic")
    b = 2
    state, restart = model.zero_state(b), torch.zeros(b, dtype=torch.uint8, device="cuda")
    users, hit = torch.zeros(b, dtype=torch.int32, device="cuda"), torch.zeros(b, dtype=torch.int32, device="cuda")
    bad = _lib.KWS_ERR_INVALID_ARGUMENT

    def handle(create, *args):
        h = ctypes.c_void_p()
        _lib.check(create(*args, ctypes.byref(h)))
        return h
    other_h, other_c = handle(lib.kws_bank_create, 128, c1, n_new, 2), handle(lib.kws_bank_create, 256, 4, 1, 2)
    w3, w8, w7 = (handle(lib.kws_window_create, b, 15, 32, c, 0.4) for c in (3, 8, 7))
    mel = torch.from_numpy(G.synthetic_mel(b, 4, 13, seed=1)).cuda()

    def step(mdl, bk, win2, t=4, win1=w3):
        rc = lib.kws_step_bank_window(mdl, bk, _lib.ptr(users), _lib.ptr(mel), _lib.ptr(state), _lib.ptr(state), None, b, t, win1, win2,
                                      b"1", b"3", None, None, None, _lib.ptr(hit), _lib.ptr(restart), None)
        return rc, lib.kws_last_error().decode()
    allocs = model.scratch_stats()[1]
    for bk in (other_h, other_c):
        rc, msg = step(model._handle, bk, w8)
        assert rc == bad and "the bank was created for" in msg, msg
        assert lib.kws_step_bank(model._handle, bk, _lib.ptr(users), _lib.ptr(mel), _lib.ptr(state), _lib.ptr(state), None, None, None, None, None,
                                 b, 4, None) == bad
    rc, msg = step(model._handle, bank._handle, w7)
    assert rc == bad and "head 2 needs B=2 C=8" in msg, msg
    rc, msg = step(one._handle, bank._handle, w8)
    assert rc == bad and "second class head" in msg, msg
    assert lib.kws_bank_set(bank._handle, 1, 2, _lib.ptr(bank.get()[0]), _lib.ptr(bank.get()[1]), None) == bad
    assert b"capacity 2" in lib.kws_last_error()
    assert lib.kws_bank_get(bank._handle, -1, 1, _lib.ptr(bank.get()[0]), _lib.ptr(bank.get()[1]), None) == bad
    # windows of 40 chunks x chunks of 200 frames x the columns of H = 256, n_new = 5: each part fits, the total does not
    l3, l8 = (handle(lib.kws_window_create, b, 40, 208, c, 0.4) for c in (3, 8))
    long_mel = torch.zeros(b, 200, 13, device="cuda")
    heads = 32768 + 2 * 16 * 208 + 512 + 2 * 16 * (40 * 32 + 32)
    stage = (16 * 256 * 5 + 128) * 4
    assert heads <= 160 * 1024 < heads + stage
    rc = lib.kws_step_bank_window(model._handle, bank._handle, _lib.ptr(users), _lib.ptr(long_mel), _lib.ptr(state), _lib.ptr(state), None, b, 200,
                                  l3, l8, b"1", b"3", None, None, None, _lib.ptr(hit), _lib.ptr(restart), None)
    msg = lib.kws_last_error().decode()
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "bytes of LDS" in msg and str(heads + stage) in msg and "columns %d" % stage in msg, msg
    assert model.scratch_stats()[1] == allocs                                         # refused before any device work on the model
    for h in (w3, w8, w7, l3, l8):
        lib.kws_window_destroy(h)
    for h in (other_h, other_c):
        lib.kws_bank_destroy(h)
    one.close()
    bank.close()
