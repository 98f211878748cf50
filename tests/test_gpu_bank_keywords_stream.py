"""GPU checks of the bank stream manager on a bank whose slots carry keywords of their own (kws_bank_set_keyword; the keyword form
bank_keyword_window_kernel): window 2 of stream b walks the label of ITS slot over ITS slot's C + n_used classes.

  1. manager == host mirror (HotwordDetector(bank=...): per-stream label and slice), exactly: hit bitmasks and states, every chunk
  2. manager == the fp64 policy loop (tests/bank_keywords_model.policy_loop) up to a stream's first frame at a decision edge
  3. softmax2 rows bitwise kws_step_bank's at T in {1, 33, 0}
  4. the PCM path: ragged lengths, skips, a stream recycled to a slot with another label
  5. every slot at (label2, n_new) == a bank without keywords; launch names with and without keywords; a keyword bank manager, a plain bank manager and a heads manager on one model handle
  6. the refusals that need a live bank, and the LDS refusal with its byte counts
  7. enrol with n_new = 1 and n_new = 2 -> one bank of n_new = 2 -> each user's rows against DeployModel on their own extended weights

Inputs of 1 and 2.  C = 6, n_new = 2, capacity 5: slots 0..3 carry "5" (n_used 1), "56", "55", "1256" (n_used 2), slot 4 none; label2 = "6"
for slot 4.  17 streams: USERS below, -1 among them.  Streams 8..15 are fed the audio of streams 0..7 and sit on a slot with the SAME
columns (slots 0, 1, 4 share one set, slots 2, 3 another) under ANOTHER label, so what differs between the two is the keyword alone.
For each of the four patterns to occur in 60 chunks the model is DESIGNED, not drawn: the gate biases are -30 (the cell forgets at
once), the candidate weights copy input k to hidden unit k, head 1 reads words 1..4 from units 1..4 and the bank's two columns read
units 5 and 6 -- a frame of "symbol" k decodes to word k, symbol 0 to none -- and every stream's audio is a random sequence of the
motifs 1 2 5 6 / 5 _ 5 / 5 6 / 6 / 5 / 1 2 in segments of 3..5 frames.  (The kernels compute what they always compute; what the
stack does with real weights is tests/test_gpu_bank_stream.py's and test_gpu_bank_keywords.py's.)  The conditions below are asserted
on the fp64 restatement alone: at least half of all (chunk, stream) pairs are compared, every label fires, and at least 3
(chunk, stream pair) cases with the same audio and columns but different labels differ in hit_2."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bank_keywords_model as KM
import bank_model as BM
from oracle import decode_oracle as D
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu

C1, N_NEW = 6, 2
THRES = (0.4, 0.5)
LABEL1, LABEL2 = "12", "6"
B, CAPACITY = 17, 5
KEYWORDS = [("5", 1), ("56", 2), ("55", 2), ("1256", 2), (None, 2)]
SHARE = [0, 0, 1, 1, 0]                              # the column set of each slot
USERS = np.array([0, 1, 2, 3, 4, 0, 2, -1, 1, 0, 3, 2, 1, 4, 3, 0, 4], np.int32)
PAIRS = [(i, i + 8) for i in range(8)]               # the same audio and columns, another label
MOTIFS = [[1, 2, 5, 6], [5, 0, 5], [5, 6], [6, 0], [5, 0], [1, 2, 0], [0]]
# name: ((n_mel, hidden, layers), window_chunks, seed)
CASES = {
    "resident-window15": ((40, 128, 2), 15, 1),
    "single-layer-window3": ((13, 128, 1), 3, 2),
    "h64-window1": ((13, 64, 2), 1, 3),
}
N_CHUNKS = 60


def _label_dict(c):
    return {"w%d" % i: i for i in range(1, c - 2)}


def _kernel(stack):
    return "auto" if stack[:2] == (40, 128) else "generic"


def _designed(stack, seed):
    """(weights, columns [CAPACITY,H,2], bias): symbol k on input k -> hidden unit k of every layer -> word k (module docstring)."""
    n_mel, hidden, layers = stack
    w = G.random_weights(n_mel, hidden, layers, C1, seed)
    for lay in w["layers"]:
        lay["bg"] = np.full_like(lay["bg"], -30.0)
        lay["Wc"] = np.zeros_like(lay["Wc"])
        lay["bc"] = np.zeros_like(lay["bc"])
        for k in range(7):
            lay["Wc"][k, k] = 3.0
    w["Wfc"] = np.zeros_like(w["Wfc"])
    for k in range(5):
        w["Wfc"][k, k] = 6.0
    w["Wfc"][0, 1] = 1.5                               # "none": the space class, word 1 a clear but distant second
    w["bfc"] = np.array([0, 0.5, 0.4, 0.3, 0.2, 0], np.float32)          # no two word classes tie where nothing is said
    rng = np.random.default_rng(seed)
    sets = 0.02 * rng.standard_normal((2, hidden, N_NEW)).astype(np.float32)
    sets[:, 5, 0] = 6.0
    sets[:, 6, 1] = 6.0
    bias = np.array([[0.1, 0.0], [0.05, -0.05]], np.float32)
    return w, sets[SHARE].copy(), bias[SHARE].copy()


def _motif_audio(n_mel, frames, seed):
    rng = np.random.default_rng(seed)
    mel = np.abs(0.01 * rng.standard_normal((B, frames, n_mel))).astype(np.float32)
    for s in range(B):
        t = 0
        while t < frames:
            for k in MOTIFS[rng.integers(len(MOTIFS))]:
                n = int(rng.integers(3, 6))
                mel[s, t:t + n, k] += 2.0
                t += n
    return mel


@functools.lru_cache(maxsize=None)
def _inputs(name):
    stack, _, seed = CASES[name]
    chunks = D.chunk_frame_counts([3600] * N_CHUNKS)
    mel = _motif_audio(stack[0], sum(chunks), seed + 1)
    speech = np.random.default_rng(seed + 2).random((len(chunks), B)) > 0.05          # occasional silence
    for i, j in PAIRS:
        mel[j] = mel[i]
        speech[:, j] = speech[:, i]
    w, cols, bias = _designed(stack, seed)
    return w, cols, bias, mel, chunks, speech


def _per_stream(keywords=KEYWORDS, users=USERS):
    per = KM.stream_keywords(keywords, users, N_NEW, LABEL2)
    return [k[0] for k in per], [k[1] for k in per]


@functools.lru_cache(maxsize=None)
def _policy(name):
    """The fp64 restatement of the whole loop; computed once, never modified."""
    w, cols, bias, mel, chunks, speech = _inputs(name)
    labels2, n_used = _per_stream()
    return KM.policy_loop(w, cols, bias, USERS, n_used, mel, chunks, speech, LABEL1, labels2, THRES, CASES[name][1])


def _fires(mask):
    """hit_2 counts per label, over the streams that walk it."""
    labels2, _ = _per_stream()
    out = {}
    for s, label in enumerate(labels2):
        if USERS[s] >= 0:
            out[label] = out.get(label, 0) + int((mask[:, s] & 2 > 0).sum())
    return out


def _pair_differences(mask):
    return sum(int(((mask[:, i] ^ mask[:, j]) & 2 > 0).sum()) for i, j in PAIRS if USERS[i] >= 0 and USERS[j] >= 0)


def _input_conditions(name):
    pol = _policy(name)
    ok = np.cumprod(pol["margin_ok"], 0).astype(bool)          # a stream is compared up to its first chunk with a frame at an edge
    fires, pairs = _fires(pol["mask"]), _pair_differences(pol["mask"])
    print(name, "restatement: compared %.0f %%, hit_2 per label %s, hit_1 %d, same audio and columns, other label, other hit_2: %d"
          % (100 * ok.mean(), fires, int((pol["mask"] & 1 > 0).sum()), pairs))
    assert ok.mean() >= 0.5, ok.mean()
    assert set(fires) == {"5", "56", "55", "1256", LABEL2} and min(fires.values()) >= 1, fires
    assert pairs >= 3, pairs
    assert not (pol["mask"][:, USERS < 0] & 2).any()          # a stream without a slot never reports head 2
    return pol, ok


def _bank(stack, w, cols, bias, keywords=KEYWORDS, c1=C1, n_new=N_NEW):
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.custom_keyword import KeywordBank
    from keyword_spotting_amd.rnn_ctc import DeployModel
    one = DeployModel(get_config(n_mel=stack[0], hidden_size=stack[1], num_layers=stack[2], label_dict=_label_dict(c1)), w, kernel=_kernel(stack))
    bank = KeywordBank(one, n_new, cols.shape[0], kernel=_kernel(stack))
    one.close()
    bank.set(0, cols, bias)
    for slot, (label, n_used) in enumerate(keywords or ()):
        if label is not None:
            bank.set_keyword(slot, label, n_used)
    return bank


def _close(*banks):
    for bank in banks:
        bank.close()


@functools.lru_cache(maxsize=None)
def _run(name):
    """Manager and host mirror on two banks with the same contents -> per chunk the two bitmasks and whether the states were equal."""
    from keyword_spotting_amd.detector import HotwordDetector, StreamManager
    stack, window, _ = CASES[name]
    w, cols, bias, mel, chunks, speech = _inputs(name)
    x = torch.from_numpy(mel).cuda()
    kw = dict(label=LABEL1, label2=LABEL2, decode_thres=THRES[0], decode_thres2=THRES[1], window_chunks=window, users=USERS)
    b_mgr, b_det = _bank(stack, w, cols, bias), _bank(stack, w, cols, bias)
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
    fires = _fires(r["want"])
    print(name, "device: hit_2 per label", fires, "pair differences:", _pair_differences(r["want"]))
    assert min(fires.values()) >= 1 and _pair_differences(r["want"]) >= 3
    assert not (r["got"][:, USERS < 0] & 2).any()


@pytest.mark.parametrize("name", list(CASES))
def test_manager_follows_the_fp64_policy_loop(name):
    pol, ok = _input_conditions(name)
    r = _run(name)
    differ = (r["got"] != pol["mask"]) & ok
    print(name, "compared %.0f %% of the (stream, chunk) pairs, %d hits among them" % (100 * ok.mean(), int((pol["mask"][ok] > 0).sum())))
    assert not differ.any(), np.argwhere(differ)[:5]
    fires_compared = _fires(np.where(ok, pol["mask"], 0))
    assert min(fires_compared.values()) >= 1, fires_compared          # every label fires inside what was compared


def test_every_slot_at_label2_is_the_plain_bank_manager():
    """A keyword of its own that equals the manager's -- (label2, n_new) on every slot -- walks a staged copy of the same matcher over
    the same width: hits and states bitwise those of a manager on a bank without keywords, through the other kernel."""
    from keyword_spotting_amd.detector import StreamManager
    name = "resident-window15"
    stack, window, _ = CASES[name]
    w, cols, bias, mel, chunks, speech = _inputs(name)
    same = _bank(stack, w, cols, bias, keywords=[(LABEL2, N_NEW)] * CAPACITY)
    plain = _bank(stack, w, cols, bias, keywords=None)
    kw = dict(label=LABEL1, label2=LABEL2, decode_thres=THRES[0], decode_thres2=THRES[1], window_chunks=window, users=USERS)
    m_same, m_plain = StreamManager(None, B, bank=same, **kw), StreamManager(None, B, bank=plain, **kw)
    x = torch.from_numpy(mel).cuda()
    pos, fired = 0, 0
    for ci, n in enumerate(chunks[:20]):
        chunk, sp = x[:, pos:pos + n].clone(), torch.from_numpy(speech[ci])
        got = m_same.feed(chunk, speech=sp).clone()
        assert torch.equal(got, m_plain.feed(chunk, speech=sp)) and torch.equal(m_same.state, m_plain.state), ci
        fired += int((got & 2 > 0).sum())
        pos += n
    assert fired > 0
    assert "bank_keyword_window_kernel" in same.stack.kernel_names()[-1] and "bank_heads_window_kernel" in plain.stack.kernel_names()[-1]
    m_same.close()
    m_plain.close()
    _close(same, plain)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_names_with_and_without_keywords(name):
    stack = CASES[name][0]
    names = _run(name)["names"]
    family = "gru_layer_resident" if stack[:2] == (40, 128) else "gru_layer_generic"
    assert len(names) == stack[2] and all(n.startswith(family) and ", false>" in n for n in names), names
    assert names[-1].endswith(" + bank_keyword_window_kernel<%d>" % (stack[1] // 16)), names
    assert "bank_" not in "".join(names[:-1]) and not any("window_inc" in n or "dense_heads" in n for n in names), names
    # a bank on which no keyword was ever set launches the kernels it always did
    from keyword_spotting_amd.detector import StreamManager
    w, cols, bias, mel = _inputs(name)[:4]
    plain = _bank(stack, w, cols, bias, keywords=None)
    mgr = StreamManager(None, B, bank=plain, users=USERS, label=LABEL1, label2=LABEL2)
    mgr.feed(torch.from_numpy(mel[:, :22].copy()).cuda())
    assert plain.stack.kernel_names()[-1].endswith(" + bank_heads_window_kernel<%d>" % (stack[1] // 16))
    plain.forward(torch.from_numpy(mel[:, :5].copy()), plain.zero_state(B), USERS)
    assert plain.stack.kernel_names()[-1].endswith(" + bank_heads_kernel<%d>" % (stack[1] // 16))
    mgr.close()
    _close(plain)


@pytest.mark.parametrize("name", list(CASES))
def test_softmax_outputs_are_bitwise_kws_step_bank(name):
    """Mel chunks of 1 and 33 frames (the 32-frame block of the kernel's loop) and of none: softmax2 against KeywordBank.forward on the
    same handles from the same state -- rows of C + n_new entries, zeros past each stream's width; hits and states against the mirror."""
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.detector import HotwordDetector, StreamManager
    lib = _lib.load()
    stack, window, seed = CASES[name]
    w, cols, bias = _inputs(name)[:3]
    _, n_used = _per_stream()
    kw = dict(label=LABEL1, label2=LABEL2, decode_thres=THRES[0], decode_thres2=THRES[1], window_chunks=window, users=USERS)
    b_mgr, b_det = _bank(stack, w, cols, bias), _bank(stack, w, cols, bias)
    mgr, det = StreamManager(None, B, max_frames=40, bank=b_mgr, **kw), HotwordDetector(None, batch=B, bank=b_det, **kw)
    lens = [1, 33, 0, 33, 1, 33, 33]
    x = torch.from_numpy(_motif_audio(stack[0], sum(lens), seed + 5)).cuda()
    rng = np.random.default_rng(seed + 6)
    pos = 0
    for n in lens:
        chunk = x[:, pos:pos + n].clone()
        speech = rng.random(B) > 0.1
        before = mgr.state.clone()
        silent = torch.from_numpy(~speech).cuda().to(torch.uint8)
        reset = torch.maximum(mgr.restart, silent)
        sm1, sm2 = torch.empty(B, n, C1, device="cuda"), torch.empty(B, n, C1 + N_NEW, device="cuda")
        model = b_mgr.stack
        with torch.cuda.device(model.device):
            _lib.check(lib.kws_step_bank_window(model._handle, b_mgr._handle, _lib.ptr(mgr.users), _lib.ptr(chunk), _lib.ptr(mgr.state),
                                                _lib.ptr(mgr.state), _lib.ptr(reset), B, n, mgr._win, mgr._win2, mgr.label, mgr.label2,
                                                _lib.ptr(silent), _lib.ptr(sm1), _lib.ptr(sm2), _lib.ptr(mgr.hit), _lib.ptr(mgr.restart),
                                                _lib.current_stream_ptr()))
        got = mgr.hit.cpu().numpy()
        ref = b_mgr.forward(chunk, before, mgr.users, reset_mask=reset, want_nn_outputs=False, want_logits=False)
        assert torch.equal(sm1, ref["head1"]["softmax"]) and torch.equal(sm2, ref["head2"]["softmax"]), (name, n)
        for s in range(B):
            assert not sm2[s, :, C1 + n_used[s]:].any() and (USERS[s] >= 0 or not sm2[s].any()), s
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
    """(front-end, weights, columns, bias) at the reference shape: random weights scaled by 3 and a random bank scaled by 4 (what
    tests/test_gpu_bank_stream.py feeds noise to); slots 0..3 on two column sets as above."""
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.frontend import MelFrontend
    stack, seed = (40, 128, 2), 7319
    if "v" in _PCM:
        return _PCM["v"]
    fe = MelFrontend(get_config())
    w = G.random_weights(stack[0], stack[1], stack[2], C1, seed)
    w["Wfc"] = (w["Wfc"] * 3).astype(np.float32)
    noise = torch.from_numpy((np.random.default_rng(8100).standard_normal((48, 16000)) * 0.2).astype(np.float32))
    mel, users = fe.forward(noise), np.arange(48) % CAPACITY
    base, bb = BM.random_bank(stack[1], N_NEW, 2, seed, scale=4.0)
    bank = _bank(stack, w, base[SHARE].copy(), bb[SHARE].copy(), keywords=None)
    for bank_seed in range(seed, seed + 60):       # the first bank whose users say BOTH new words often enough on this noise
        base, bb = BM.random_bank(stack[1], N_NEW, 2, bank_seed, scale=4.0)
        r = bank.set(0, base[SHARE].copy(), bb[SHARE].copy()).forward(mel, bank.zero_state(48), users, want_nn_outputs=False, want_logits=False)
        words = np.concatenate([D.ctc_decode2(r["head2"]["softmax"][k].cpu().numpy(), C1 + N_NEW, 0.3)[1::2] for k in range(48)])
        if (words == 5).sum() >= 20 and (words == 6).sum() >= 20:
            break
    else:
        bank.close()
        raise AssertionError("no bank among 60 seeds whose users emit both new words on this noise")
    bank.close()
    print("PCM setup: bank seed %d, %d x word 5, %d x word 6" % (bank_seed, (words == 5).sum(), (words == 6).sum()))
    _PCM["v"] = (fe, w, base[SHARE].copy(), bb[SHARE].copy())
    return _PCM["v"]


def _manager(bank, users, labels=("1", "6"), **kw):
    from keyword_spotting_amd.detector import StreamManager
    return StreamManager(None, B, bank=bank, users=users, label=labels[0], label2=labels[1], decode_thres=THRES[0], decode_thres2=0.3, **kw)


PCM_KEYWORDS = [("5", 1), ("6", 2), ("55", 2), ("56", 2), (None, 2)]


def test_ragged_lengths_skips_and_recycling_to_a_slot_with_another_label():
    """Stream s of a ragged keyword-bank manager gets, bit for bit, what a lock-step manager gets when fed stream s's chunks alone on
    stream s's slot -- on the periods where it had data, nothing on the others.  Mid-run three streams are recycled and moved to a slot
    with ANOTHER label (users[s] rewritten on the device): from their first chunk on their oracle is a fresh manager on the new slot;
    their neighbours are untouched (their oracle runs through)."""
    fe, w, cols, bias = _pcm_setup()
    stack = (40, 128, 2)
    periods, n_max, at = 12, 5000, 6
    recycled = {2: 0, 7: 1, 16: 3}                                    # stream -> its slot after the recycle (7 had none)
    rng = np.random.default_rng(8300)
    lens = rng.choice([0, 150, 1800, 3600, 5000], size=(B, periods), p=[0.15, 0.1, 0.2, 0.4, 0.15]).astype(np.int32)
    lens[3, :2] = 150                                                 # a stream that opens with sub-frame chunks
    chunks = []
    for p in range(periods):
        pad = rng.integers(-32768, 32767, (B, n_max)).astype(np.int16)          # loud padding that must never reach a result
        data = (rng.integers(-6000, 6000, (B, n_max)) * rng.choice([0.25, 1.0, 3.0], (B, 1))).astype(np.int16)
        chunks.append(np.where(np.arange(n_max)[None, :] < lens[:, p:p + 1], data, pad).astype(np.int16))
    b_rag, b_ora = _bank(stack, w, cols, bias, PCM_KEYWORDS), _bank(stack, w, cols, bias, PCM_KEYWORDS)
    rag = _manager(b_rag, USERS)
    hits = np.zeros((B, periods), np.int32)
    for p in range(periods):
        if p == at:
            rag.recycle(list(recycled))
            for s, u in recycled.items():
                rag.users[s] = u
        hits[:, p] = rag.feed_pcm(torch.from_numpy(chunks[p]).cuda(), fe, lengths=torch.from_numpy(lens[:, p])).cpu().numpy()
    torch.cuda.synchronize()
    assert "bank_keyword_window_kernel<8>" in b_rag.stack.kernel_names()[-1]
    print("ragged keyword-bank manager: hit_1 %d, hit_2 %d" % (int((hits & 1 > 0).sum()), int((hits & 2 > 0).sum())))
    assert (hits & 2).sum() > 0, "no head-2 trigger: the run does not cover the keywords"
    assert (lens == 0).any()
    fired2 = set()
    for s in (0, 1, 2, 3, 7, 9, 12, 16):                              # every recycled stream and neighbours of each
        user = int(USERS[s])
        oracle = _manager(b_ora, np.full(B, user, np.int32))
        for p in range(periods):
            if p == at and s in recycled:
                oracle.close()
                user = recycled[s]
                oracle = _manager(b_ora, np.full(B, user, np.int32))
            n = int(lens[s, p])
            if n == 0:
                assert hits[s, p] == 0, (s, p)
                continue
            row = torch.from_numpy(np.repeat(chunks[p][s:s + 1, :n], B, 0)).cuda()
            want = int(oracle.feed_pcm(row, fe)[0].item())
            assert hits[s, p] == want, (s, p, n)
            assert user >= 0 or not want & 2
            if want & 2:
                fired2.add(user)
        torch.cuda.synchronize()
        assert torch.equal(rag.state[:, s], oracle.state[:, 0]), s
        assert int(rag.restart[s]) == int(oracle.restart[0]), s
        oracle.close()
    print("slots whose keyword fired among the checked streams:", sorted(fired2))
    rag.close()
    _close(b_rag, b_ora)


def test_keyword_bank_plain_bank_and_heads_managers_coexist_on_one_model():
    """A keyword-bank manager, a plain bank manager (another bank, no keywords) and a two-head manager on ONE model handle, fed in turn,
    each equal to itself alone on a handle of its own; the two bank managers report their own launch names."""
    from keyword_spotting_amd.detector import StreamManager
    fe, w, cols, bias = _pcm_setup()
    stack = (40, 128, 2)
    kw = dict(decode_thres=THRES[0], decode_thres2=0.3)

    def trio(stacks):
        """managers on the model handles `stacks` (three banks' own stacks, or one shared)"""
        out = []
        for i, keywords in enumerate((PCM_KEYWORDS, None)):
            bank = _bank(stack, w, cols, bias, keywords)
            if stacks[i] is not None:
                bank.stack.close()
                bank.stack = stacks[i]
            out.append((StreamManager(None, B, bank=bank, users=USERS, label="1", label2="6", **kw), bank))
        return out
    shared = _bank(stack, w, cols, bias, None)
    together, apart = trio([shared.stack, shared.stack]), trio([None, None])
    heads = [StreamManager(shared.stack, B, label="1", label2="6", **kw), StreamManager(apart[0][1].stack, B, label="1", label2="6", **kw)]
    rng = np.random.default_rng(8500)
    fired = [0, 0, 0]
    for k in range(10):
        x = torch.from_numpy(rng.integers(-6000, 6000, (B, 3600)).astype(np.int16)).cuda()
        for i in range(2):
            got = together[i][0].feed_pcm(x, fe).clone()
            name = shared.stack.kernel_names()[-1]
            assert name.endswith(" + bank_keyword_window_kernel<8>" if i == 0 else " + bank_heads_window_kernel<8>"), name
            assert torch.equal(got, apart[i][0].feed_pcm(x, fe)) and torch.equal(together[i][0].state, apart[i][0].state), (k, i)
            fired[i] += int((got & 2 > 0).sum())
        got = heads[0].feed_pcm(x, fe).clone()
        assert shared.stack.kernel_names()[-1].endswith(" + heads_window_kernel<8>")
        assert torch.equal(got, heads[1].feed_pcm(x, fe)) and torch.equal(heads[0].state, heads[1].state), k
        fired[2] += int((got > 0).sum())
    print("head-2 hits of the keyword bank / plain bank manager, hits of the two-head manager:", fired)
    assert fired[0] > 0 and fired[1] > 0
    for m in heads:
        m.close()
    for m, bank in together:
        m.close()
        bank.stack = None
        bank.close()
    for m, bank in apart:
        m.close()
        bank.close()
    shared.close()


def test_refusals_on_a_live_bank_and_the_lds_total():
    """kws_bank_set_keyword's refusals that need a live bank, by code and message, none of them changing the slot; and the LDS total of
    the keyword form with its byte counts: a shape that a bank without keywords still takes."""
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    stack, n_new, c1 = (13, 256, 1), 4, 3
    w = G.random_weights(stack[0], stack[1], stack[2], c1, 5)
    cols, bias = BM.random_bank(stack[1], n_new, 2, 5)
    bank = _bank(stack, w, cols, bias, keywords=None, c1=c1, n_new=n_new)
    bad = _lib.KWS_ERR_INVALID_ARGUMENT
    err = lambda: lib.kws_last_error().decode()

    def set_keyword(slot, n_used, label):
        return lib.kws_bank_set_keyword(bank._handle, slot, n_used, label, None)
    for slot in (-1, 2):
        assert set_keyword(slot, 1, b"2") == bad and "capacity 2" in err()
    for n_used in (0, 5):
        assert set_keyword(0, n_used, b"2") == bad and "n_used=%d" % n_used in err()
    assert set_keyword(0, 2, None) == bad and "n_used=2 without a label" in err()
    assert set_keyword(0, 4, b"2" * 16) == bad and "15 digits" in err()
    for label in (b"20", b"2a", b"2 "):
        assert set_keyword(0, 4, label) == bad and "digits 1..9" in err(), label
    assert set_keyword(0, 1, b"23") == bad and "digit 3" in err() and "words 1..2" in err()          # C + n_used - 2 = 2
    assert set_keyword(0, 4, b"26") == bad and "digit 6" in err() and "words 1..5" in err()
    assert bank.keyword(0) == (None, n_new) and not bank.has_keywords()
    n, own, label = ctypes.c_int(), ctypes.c_int(), ctypes.create_string_buffer(16)
    assert lib.kws_bank_get_keyword(bank._handle, 2, ctypes.byref(n), label, ctypes.byref(own)) == bad and "capacity 2" in err()
    assert set_keyword(0, 2, b"23") == _lib.KWS_OK and set_keyword(1, 4, b"2" * 15) == _lib.KWS_OK
    assert bank.keyword(0) == ("23", 2) and bank.keyword(1) == ("2" * 15, 4)
    assert set_keyword(0, n_new, None) == _lib.KWS_OK and bank.keyword(0) == (None, n_new)
    # windows of 54 chunks x chunks of 200 frames x the columns of H = 256, n_new = 4: the plain form fits, the keyword form does not
    model, b = bank.stack, 2
    state, restart = model.zero_state(b), torch.zeros(b, dtype=torch.uint8, device="cuda")
    users, hit = torch.zeros(b, dtype=torch.int32, device="cuda"), torch.zeros(b, dtype=torch.int32, device="cuda")
    wins = []
    for c in (3, 7):
        h = ctypes.c_void_p()
        _lib.check(lib.kws_window_create(b, 54, 208, c, 0.4, ctypes.byref(h)))
        wins.append(h)
    long_mel = torch.zeros(b, 200, 13, device="cuda")
    heads = 32768 + 2 * 16 * 208 + 512 + 2 * 16 * (54 * 32 + 32)
    stage, keywords = (16 * 256 * n_new + 128) * 4, 16 * 256 + 128
    assert heads + stage <= 160 * 1024 < heads + stage + keywords
    plain = _bank(stack, w, cols, bias, keywords=None, c1=c1, n_new=n_new)

    def step(bk):
        return lib.kws_step_bank_window(bk.stack._handle, bk._handle, _lib.ptr(users), _lib.ptr(long_mel), _lib.ptr(state), _lib.ptr(state), None,
                                        b, 200, wins[0], wins[1], b"1", b"2", None, None, None, _lib.ptr(hit), _lib.ptr(restart), None)
    allocs = model.scratch_stats()[1]
    rc = step(bank)
    msg = err()
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "bytes of LDS" in msg and str(heads + stage + keywords) in msg, msg
    assert "columns %d" % stage in msg and "keyword matchers %d" % keywords in msg, msg
    assert model.scratch_stats()[1] == allocs                                         # refused before any device work on the model
    assert step(plain) == _lib.KWS_OK                                                # the same shape without keywords: today's kernel
    torch.cuda.synchronize()
    for h in wins:
        lib.kws_window_destroy(h)
    _close(bank, plain)


def test_enrol_one_and_two_words_into_one_bank_end_to_end():
    """User A enrols ONE new word ("5", an Enroller of n_new = 1), user B two ("56", n_new = 2); both go into one bank of n_new = 2 with
    KeywordBank.set(labels=).  Each user's bank rows against DeployModel on that user's own extended_weights: head-2 logits within
    1e-4 (the new classes are summed in another order there), tokens equal."""
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.custom_keyword import Enroller, KeywordBank, truncated_normal
    from keyword_spotting_amd.prediction import ctc_label
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg = get_config()
    c, h = cfg.num_classes, cfg.hidden_size
    model = DeployModel(cfg, weights.init_weights(cfg, seed=0))
    mel = G.synthetic_mel(6, 48, cfg.n_mel, seed=10)
    bank = KeywordBank(model, 2, 3)
    served = []
    for slot, (n_u, words, label) in enumerate(((1, [5], "5"), (2, [5, 6], "56"))):
        enroller = Enroller(model, n_u, enrolments=1, utterances_per_enrolment=3)
        init = (truncated_normal((1, h, n_u), slot), np.zeros((1, n_u), np.float32))
        wn, bn, _ = enroller.fit(torch.from_numpy(mel[3 * slot:3 * slot + 3]), [48] * 3, list(ctc_label(words)), 100, lr=0.03, init=init)
        assert tuple(wn.shape) == (1, h, n_u)
        bank.set(slot, wn, bn, labels=[label])
        served.append(DeployModel(enroller.heads_config(), enroller.extended_weights(wn[0].cpu().numpy(), bn[0].cpu().numpy())))
        enroller.close()
    assert bank.keyword(0) == ("5", 1) and bank.keyword(1) == ("56", 2) and bank.keyword(2) == (None, 2)
    got_w, got_b = bank.get(0, 1)
    assert not got_w[..., 1].any() and not got_b[..., 1].any()                        # user A's second column: the zero padding
    users = np.array([0, 0, 0, 1, 1, 1], np.int32)
    x = torch.from_numpy(mel)
    pw = [bank.stack.fresh_prev_word(6), bank.stack.fresh_prev_word(6)]
    r = bank.forward(x, bank.zero_state(6), users, prev_words=pw, decode2_thres=(0.4, 0.4))
    for slot, n_u in ((0, 1), (1, 2)):
        rows = slice(3 * slot, 3 * slot + 3)
        pw_s = [served[slot].fresh_prev_word(3), served[slot].fresh_prev_word(3)]
        want = served[slot].forward_heads(x[rows], served[slot].zero_state(3), prev_words=pw_s, decode2_thres=(0.4, 0.4))
        d = (r["head2"]["logits"][rows][..., :c + n_u] - want["head2"]["logits"]).abs().max().item()
        print("user on slot %d (n_new = %d): head 2 max|dlogit| against DeployModel on its extended weights %.2e" % (slot, n_u, d))
        assert d <= 1e-4
        assert not r["head2"]["logits"][rows][..., c + n_u:].any()
        assert torch.equal(r["head2"]["tokens"][rows], want["head2"]["tokens"]) and torch.equal(pw[1][rows], pw_s[1])
        assert torch.equal(r["head1"]["logits"][rows], want["head1"]["logits"])
        served[slot].close()
    assert int((r["head2"]["tokens"] > 0).sum()) > 0
    bank.close()
    model.close()
