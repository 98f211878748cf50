"""GPU checks of the two-head stream manager (kws_stream_create_heads / kws_step_heads_window, StreamManager(label2=...)): one
manager on a customised-keyword model decodes both heads per chunk, the stack run once, one launch behind it.

  1. manager == host mirror (HotwordDetector(label2=...)), exactly: hit bitmasks and states, every chunk
  2. manager == the fp64 policy loop (tests/heads_stream_model.policy_loop) up to a stream's first frame at a decision edge
  3. the optional softmax outputs are bitwise kws_step_heads' rows, every stack, T in {1, 33} (the kernel's 32-frame block), T = 0
  4. the PCM path: float / int16 / sub-frame chunks against the mirror; ragged lengths (0 = skip) and recycling against lock-step
     two-head managers fed each stream's chunks alone
  5. launch shape and scratch; 6. unchanged ground: no label2 -> head 1 through the fused tail; 7. refusals

Inputs.  Weights: heads_model.random_heads_weights, both heads scaled by 3 so that words fire (as test_gpu_detector._keyword_weights).
Labels: head 1 "12"; head 2 at C2 = 8 a label with a word only it has, at C2 = 3 its single word "1".  Thresholds 0.4 / 0.5.  The
seeds were chosen with the fp64 restatement alone (no GPU): on each 17-stream case every kind of chunk -- head 1 alone, head 2
alone, both -- occurs at least 3 times, at least half of all (stream, chunk) pairs lie before the stream's first decision edge,
and the coupling is observable: some head-2-only hit is followed by a chunk where head 1 would have fired had its window not been
cleared.  The tests assert those conditions on the restatement before they compare the device with anything.
The case h256-b1-window1 is EXEMPT from those input conditions, and says so here: it exists for the shapes (one stream: a partial
group; a one-chunk window; hidden 256), its 60 (stream, chunk) pairs are a seventeenth of the other cases', and no seed among the
150 searched gives one stream three chunks on which both heads fire; it asserts head 1 alone >= 3, head 2 alone >= 3, both >= 1.  The
coupling cannot be observable there at all: a one-chunk window holds nothing of an earlier chunk, so a cleared and an uncleared
window are the same window one chunk later.  The three 17-stream cases carry the issue's conditions.
Shapes: B in {1, 17} (a partial group, a second group), chunks of 21-23 frames (D.chunk_frame_counts), windows of 1 / 15 / 17
chunks (17: a second ring slot per lane)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import heads_model as HM
import heads_stream_model as SM
from oracle import decode_oracle as D
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu

C1 = 6
THRES = (0.4, 0.5)
LABEL1 = "12"
# name: ((n_mel, hidden, layers), C2, B, window_chunks, seed, label2)
CASES = {
    "resident": ((40, 128, 2), 8, 17, 15, 9, "25"),
    "h64-window17": ((13, 64, 2), 3, 17, 17, 13, "1"),
    "single-layer": ((13, 128, 1), 3, 17, 15, 27, "1"),
    "h256-b1-window1": ((13, 256, 2), 8, 1, 1, 26, "5"),
}
N_CHUNKS = 60


def _config(stack, c2):
    from keyword_spotting_amd import get_config
    cfg = get_config(n_mel=stack[0], hidden_size=stack[1], num_layers=stack[2])
    if c2:
        cfg.num_classes2 = c2
    return cfg


def _model(stack, c2, w):
    """n_mel 40 at hidden 128: AUTO, the resident kernels on every layer; the other stacks: the generic kernels (tests/test_gpu_heads.py)."""
    from keyword_spotting_amd.rnn_ctc import DeployModel
    return DeployModel(_config(stack, c2), w, kernel="auto" if stack[:2] == (40, 128) else "generic")


def _weights(stack, c2, seed):
    w = HM.random_heads_weights(stack[0], stack[1], stack[2], C1, c2, seed=seed)
    w["Wfc"] = (w["Wfc"] * 3).astype(np.float32)
    w["Wfc2"] = (w["Wfc2"] * 3).astype(np.float32)
    return w


@functools.lru_cache(maxsize=None)
def _inputs(name):
    stack, c2, b, _, seed, _ = CASES[name]
    chunks = D.chunk_frame_counts([3600] * N_CHUNKS)
    mel = G.synthetic_mel(b, sum(chunks), stack[0], seed=seed + 1)
    speech = np.random.default_rng(seed + 2).random((len(chunks), b)) > 0.05          # occasional silence
    return _weights(stack, c2, seed), mel, chunks, speech


@functools.lru_cache(maxsize=None)
def _policy(name):
    """The fp64 restatement of the whole loop; computed once, never modified."""
    _, _, _, window, _, label2 = CASES[name]
    w, mel, chunks, speech = _inputs(name)
    return SM.policy_loop(w, mel, chunks, speech, (LABEL1, label2), THRES, window)


@functools.lru_cache(maxsize=None)
def _run(name):
    """Manager and host mirror on two handles with the same weights over the case's chunks -> per chunk the two bitmasks and
    whether the states were equal; and the kernel names after the last feed."""
    from keyword_spotting_amd.detector import HotwordDetector, StreamManager
    stack, c2, b, window, _, label2 = CASES[name]
    w, mel, chunks, speech = _inputs(name)
    x = torch.from_numpy(mel).cuda()
    kw = dict(label=LABEL1, label2=label2, decode_thres=THRES[0], decode_thres2=THRES[1], window_chunks=window)
    m_mgr, m_det = _model(stack, c2, w), _model(stack, c2, w)
    mgr, det = StreamManager(m_mgr, b, **kw), HotwordDetector(m_det, batch=b, **kw)
    got, want, same_state, pos = [], [], [], 0
    for ci, n in enumerate(chunks):
        chunk = x[:, pos:pos + n].clone()               # (a copy: at B = 1 the slice itself is contiguous, but not 16-byte aligned)
        fired = det.feed(chunk, speech=speech[ci])
        want.append(det.hit_mask.copy())
        assert sorted(fired) == np.nonzero(det.hit_mask)[0].tolist()
        got.append(mgr.feed(chunk, speech=torch.from_numpy(speech[ci])).cpu().numpy().copy())
        same_state.append(torch.equal(mgr.state, det.state))
        pos += n
    names = m_mgr.kernel_names()
    mgr.close()
    m_mgr.close()
    m_det.close()
    return dict(got=np.stack(got), want=np.stack(want), same_state=same_state, names=names)


def _kinds(mask):
    return [int((mask == k).sum()) for k in (1, 2, 3)]


@pytest.mark.parametrize("name", list(CASES))
def test_manager_equals_the_host_mirror_exactly(name):
    b = CASES[name][2]
    pol = _policy(name)
    kinds = _kinds(pol["mask"])
    print(name, "restatement: head 1 alone / head 2 alone / both:", kinds, "coupling observable:", int(pol["observable"].sum()))
    if b > 1:           # what the seeds were chosen for, on the restatement alone
        assert min(kinds) >= 3, kinds
        assert pol["observable"].sum() >= 1          # head 1 would have fired, had a head-2-only hit left its window alone
    else:               # one stream, a one-chunk window: exempt from the conditions above (module docstring)
        assert kinds[0] >= 3 and kinds[1] >= 3 and kinds[2] >= 1, kinds
    r = _run(name)
    for ci in range(N_CHUNKS):
        np.testing.assert_array_equal(r["got"][ci], r["want"][ci], err_msg="%s chunk %d" % (name, ci))
        assert r["same_state"][ci], (name, ci)
    dk = _kinds(r["want"])
    print(name, "device: head 1 alone / head 2 alone / both:", dk)
    assert min(dk) >= (3 if b > 1 else 1), dk


@pytest.mark.parametrize("name", ["resident", "h64-window17", "single-layer"])
def test_manager_follows_the_fp64_policy_loop(name):
    pol = _policy(name)
    ok = np.cumprod(pol["margin_ok"], 0).astype(bool)          # a stream is compared up to its first chunk with a frame at an edge
    assert ok.mean() >= 0.5, ok.mean()                         # the cap, met by the restatement alone
    r = _run(name)
    differ = (r["got"] != pol["mask"]) & ok
    print(name, "compared %.0f %% of the (stream, chunk) pairs, %d hits among them" % (100 * ok.mean(), int((pol["mask"][ok] > 0).sum())))
    assert not differ.any(), np.argwhere(differ)[:5]
    assert (pol["observable"] & ok).sum() >= 1                 # the coupling lies inside what was compared
    assert min(int(((pol["mask"] == k) & ok).sum()) for k in (1, 2, 3)) >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_softmax_outputs_are_bitwise_kws_step_heads_and_block_boundaries(name):
    """max_frames = 40, mel chunks of 1 and 33 frames (the 32-frame block of the kernel's loop) and of none: both optional softmax
    outputs against forward_heads on the same handle from the same state; hits and states against the mirror on another handle."""
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.detector import HotwordDetector, StreamManager
    lib = _lib.load()
    stack, c2, b, window, seed, label2 = CASES[name]
    b = 17
    w = _weights(stack, c2, seed)
    kw = dict(label=LABEL1, label2=label2, decode_thres=THRES[0], decode_thres2=THRES[1], window_chunks=window)
    m_mgr, m_det = _model(stack, c2, w), _model(stack, c2, w)
    mgr, det = StreamManager(m_mgr, b, max_frames=40, **kw), HotwordDetector(m_det, batch=b, **kw)
    mgr.state.copy_(torch.from_numpy((0.3 * np.random.default_rng(seed).standard_normal(tuple(mgr.state.shape))).astype(np.float32)))
    det.state.copy_(mgr.state)
    lens = [1, 33, 0, 33, 1, 33, 33]
    x = torch.from_numpy(G.synthetic_mel(b, sum(lens), stack[0], seed=seed + 5)).cuda()
    rng = np.random.default_rng(seed + 6)
    pos, hits = 0, 0
    for n in lens:
        chunk = x[:, pos:pos + n].clone()
        speech = rng.random(b) > 0.1
        before = mgr.state.clone()
        reset = torch.maximum(mgr.restart, torch.from_numpy(~speech).cuda().to(torch.uint8))
        # the manager's own iteration (StreamManager.feed), through the C entry point so that the optional outputs are reachable
        silent = torch.from_numpy(~speech).cuda().to(torch.uint8)
        sm1, sm2 = torch.empty(b, n, C1, device="cuda"), torch.empty(b, n, c2, device="cuda")
        with torch.cuda.device(m_mgr.device):
            _lib.check(lib.kws_step_heads_window(m_mgr._handle, _lib.ptr(chunk), _lib.ptr(mgr.state), _lib.ptr(mgr.state), _lib.ptr(reset), b, n,
                                                 mgr._win, mgr._win2, mgr.label, mgr.label2, _lib.ptr(silent), _lib.ptr(sm1), _lib.ptr(sm2),
                                                 _lib.ptr(mgr.hit), _lib.ptr(mgr.restart), _lib.current_stream_ptr()))
        got = mgr.hit.cpu().numpy()
        ref = m_mgr.forward_heads(chunk, before, reset_mask=reset, want_nn_outputs=False, want_logits=False)
        assert torch.equal(sm1, ref["head1"]["softmax"]) and torch.equal(sm2, ref["head2"]["softmax"]), (name, n)
        assert torch.equal(mgr.state, ref["state"])
        det.feed(chunk, speech=speech)
        np.testing.assert_array_equal(got, det.hit_mask, err_msg="%s T=%d" % (name, n))
        assert torch.equal(mgr.state, det.state)
        hits += int((got > 0).sum())
        pos += n
    print(name, "hits over the %d chunks:" % len(lens), hits)
    mgr.close()
    for m in (m_mgr, m_det):
        m.close()


# ---- the PCM path -----------------------------------------------------------------------------------------------------
_PCM = {}


def _pcm_setup():
    """(config, front-end, weights, (label1, label2)): a two-head model at the reference shape whose heads both say something on
    noise through the real front-end, each head's most frequent word as its one-digit label (as tests/test_gpu_ragged.py)."""
    if not _PCM:
        from keyword_spotting_amd.frontend import MelFrontend
        stack, c2 = (40, 128, 2), 8
        cfg = _config(stack, c2)
        fe = MelFrontend(cfg)
        noise = torch.from_numpy((np.random.default_rng(8100).standard_normal((48, 16000)) * 0.2).astype(np.float32))
        for seed in range(7319, 7380):       # (7319: the first whose fp64 restatement emits varied words from both heads on this noise)
            w = _weights(stack, c2, seed)
            probe = _model(stack, c2, w)
            r = probe.forward_heads(fe.forward(noise), probe.zero_state(48), want_nn_outputs=False, want_logits=False)
            probe.close()
            words = [np.concatenate([D.ctc_decode2(r["head%d" % i]["softmax"][k].cpu().numpy(), c, THRES[i - 1])[1::2] for k in range(48)])
                     for i, c in ((1, C1), (2, c2))]
            if min(len(v) for v in words) >= 80:
                _PCM["v"] = (cfg, fe, w, tuple(str(int(np.bincount(v).argmax())) for v in words))
                break
        else:
            raise AssertionError("no seed gives a model whose heads both emit words")
    return _PCM["v"]


def _two_head_manager(model, b, labels, **kw):
    from keyword_spotting_amd.detector import StreamManager
    return StreamManager(model, b, label=labels[0], label2=labels[1], decode_thres=THRES[0], decode_thres2=THRES[1], **kw)


def test_pcm_feeds_equal_the_mirror():
    """float PCM, int16 PCM, sub-frame chunks (zero frames: an empty entry into both windows), quiet chunks (VAD clears both)."""
    from keyword_spotting_amd.detector import HotwordDetector
    cfg, fe, w, labels = _pcm_setup()
    b = 17
    m_mgr, m_det = _model((40, 128, 2), 8, w), _model((40, 128, 2), 8, w)
    mgr = _two_head_manager(m_mgr, b, labels)
    det = HotwordDetector(m_det, batch=b, label=labels[0], label2=labels[1], decode_thres=THRES[0], decode_thres2=THRES[1])
    rng = np.random.default_rng(8200)
    sizes = [150, 150, 3600, 3600, 1800, 150] + [3600] * 18
    masks = []
    for k, n in enumerate(sizes):
        gain = rng.choice([0.25, 1.0, 3.0], (b, 1))                   # loudness changes from chunk to chunk: the words do too
        if k % 2:
            chunk = (rng.integers(-6000, 6000, (b, n)) * gain).astype(np.int16)
            chunk[rng.random(b) < 0.06] //= 4096                      # below vad(data, 30)
        else:
            chunk = (rng.standard_normal((b, n)) * 0.2 * gain).astype(np.float32)
            chunk[rng.random(b) < 0.06] *= 1e-4
        x = torch.from_numpy(chunk).cuda()
        det.feed_pcm(x, fe)
        got = mgr.feed_pcm(x, fe).cpu().numpy()
        np.testing.assert_array_equal(got, det.hit_mask, err_msg="chunk %d (%d samples)" % (k, n))
        assert torch.equal(mgr.state, det.state), k
        masks.append(got.copy())
    masks = np.stack(masks)
    print("PCM feeds: head 1 alone / head 2 alone / both:", _kinds(masks))
    assert ((masks & 1) > 0).sum() >= 1 and ((masks & 2) > 0).sum() >= 1
    names = m_mgr.kernel_names()
    assert names[-1].endswith(" + heads_window_kernel<8>"), names
    mgr.close()
    m_mgr.close()
    m_det.close()


def test_ragged_lengths_and_recycling_equal_per_stream_lockstep_replay():
    """Stream b of a ragged two-head manager gets, bit for bit, what a lock-step two-head manager gets when fed stream b's chunks
    alone (tests/test_gpu_ragged.py's argument) -- on the periods where it had data, and nothing on the others (hit 0, restart
    kept).  Mid-run some streams are recycled: from there on their oracle is a fresh manager, so both windows behave as fresh."""
    cfg, fe, w, labels = _pcm_setup()
    b, periods, n_max, recycled, at = 17, 12, 5000, (2, 16), 6
    rng = np.random.default_rng(8300)
    lens = rng.choice([0, 150, 1800, 3600, 5000], size=(b, periods), p=[0.15, 0.1, 0.2, 0.4, 0.15]).astype(np.int32)
    lens[3, :2] = 150                                                 # a stream that opens with sub-frame chunks
    chunks = []
    for p in range(periods):
        pad = rng.integers(-32768, 32767, (b, n_max)).astype(np.int16)          # loud padding that must never reach a result
        data = (rng.integers(-6000, 6000, (b, n_max)) * rng.choice([0.25, 1.0, 3.0], (b, 1))).astype(np.int16)
        data[rng.random(b) < 0.05] //= 4096
        chunks.append(np.where(np.arange(n_max)[None, :] < lens[:, p:p + 1], data, pad).astype(np.int16))
    m_rag, m_ora = _model((40, 128, 2), 8, w), _model((40, 128, 2), 8, w)
    rag = _two_head_manager(m_rag, b, labels)
    hits = np.zeros((b, periods), np.int32)
    for p in range(periods):
        if p == at:
            rag.recycle(list(recycled))
        hits[:, p] = rag.feed_pcm(torch.from_numpy(chunks[p]).cuda(), fe, lengths=torch.from_numpy(lens[:, p])).cpu().numpy()
    torch.cuda.synchronize()
    assert "heads_window_kernel<8>" in m_rag.kernel_names()[-1] and "window_inc" not in "".join(m_rag.kernel_names())
    assert (hits & 1).sum() > 0 and (hits & 2).sum() > 0, "no trigger: the run does not cover the coupled clear"
    assert (lens == 0).any()
    after = 0
    for s in range(b):
        oracle = _two_head_manager(m_ora, b, labels)
        for p in range(periods):
            if p == at and s in recycled:
                oracle.close()
                oracle = _two_head_manager(m_ora, b, labels)
            n = int(lens[s, p])
            if n == 0:
                assert hits[s, p] == 0, (s, p)
                continue
            row = torch.from_numpy(np.repeat(chunks[p][s:s + 1, :n], b, 0)).cuda()
            want = int(oracle.feed_pcm(row, fe)[0].item())
            assert hits[s, p] == want, (s, p, n)
            after += int(want > 0 and p >= at and s in recycled)
        torch.cuda.synchronize()
        assert torch.equal(rag.state[:, s], oracle.state[:, 0]), s
        assert int(rag.restart[s]) == int(oracle.restart[0]), s
        oracle.close()
    print("hits of recycled streams after the recycle:", after)
    rag.close()
    m_rag.close()
    m_ora.close()


# ---- launch shape, unchanged ground, refusals --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resident", "single-layer", "h256-b1-window1"])
def test_launch_shape_and_scratch(name):
    stack = CASES[name][0]
    names = _run(name)["names"]
    family = "gru_layer_resident" if stack[:2] == (40, 128) else "gru_layer_generic"
    assert len(names) == stack[2] and all(n.startswith(family) and ", false>" in n for n in names), names          # no layer is `last`
    assert names[-1].endswith(" + heads_window_kernel<%d>" % (stack[1] // 16)), names
    assert not any("window_inc_kernel" in n or "dense_heads_kernel" in n or "window tail" in n for n in names), names
    assert "heads_window" not in "".join(names[:-1])


def test_feeds_never_regrow_the_scratch_and_profiling_times_the_launch():
    cfg, fe, w, labels = _pcm_setup()
    b = 17
    model = _model((40, 128, 2), 8, w)
    mgr = _two_head_manager(model, b, labels)
    mgr._stream_on(fe)                                                # kws_stream_create_heads: reserves what a heads step needs
    allocs = model.scratch_stats()[1]
    rng = np.random.default_rng(8400)
    model.set_profiling(True)
    for n, ragged in ((3600, False), (150, False), (5000, False), (3600, True), (5000, True)):
        x = torch.from_numpy(rng.integers(-6000, 6000, (b, n)).astype(np.int16)).cuda()
        mgr.feed_pcm(x, fe, lengths=torch.from_numpy(rng.integers(0, n + 1, b).astype(np.int32)) if ragged else None)
        mgr.feed(torch.from_numpy(G.synthetic_mel(b, 22, 40, seed=n)))
    times = model.kernel_times()
    model.set_profiling(False)
    assert model.scratch_stats()[1] == allocs
    assert times[0][1] == times[1][1] == 9 and times[1][0] > 0        # (the sub-frame chunk launches no layer) the top slot holds layer + heads_window
    mgr.close()
    model.close()


def test_without_label2_a_heads_handle_streams_head_1_as_before_and_both_kinds_coexist():
    from keyword_spotting_amd.detector import StreamManager
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg, fe, w, labels = _pcm_setup()
    b = 17
    one = {k: v for k, v in w.items() if k not in ("Wfc2", "bfc2")}
    m_heads, m_one, m_alone = _model((40, 128, 2), 8, w), DeployModel(_config((40, 128, 2), 0), one), _model((40, 128, 2), 8, w)
    plain, ref = StreamManager(m_heads, b, label=labels[0], decode_thres=THRES[0]), StreamManager(m_one, b, label=labels[0], decode_thres=THRES[0])
    both, alone = _two_head_manager(m_heads, b, labels), _two_head_manager(m_alone, b, labels)      # `both` shares the handle with `plain`
    rng = np.random.default_rng(8500)
    fired = 0
    for k in range(16):
        x = torch.from_numpy(rng.integers(-6000, 6000, (b, 3600)).astype(np.int16)).cuda()
        got = plain.feed_pcm(x, fe).clone()
        assert "window tail" in m_heads.kernel_names()[-1] and "heads" not in "".join(m_heads.kernel_names())      # the fused tail, as on the parent
        assert torch.equal(got, ref.feed_pcm(x, fe)) and torch.equal(plain.state, ref.state), k
        assert int(got.max()) <= 1
        fired += int(got.sum())
        got2 = both.feed_pcm(x, fe).clone()
        assert torch.equal(got2, alone.feed_pcm(x, fe)) and torch.equal(both.state, alone.state), k
    assert fired > 0
    for m in (plain, ref, both, alone):
        m.close()
    for m in (m_heads, m_one, m_alone):
        m.close()


def test_refusals():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.detector import StreamManager
    from keyword_spotting_amd.rnn_ctc import DeployModel
    cfg, fe, w, labels = _pcm_setup()
    lib = _lib.load()
    b = 2
    model = _model((40, 128, 2), 8, w)
    one = DeployModel(_config((40, 128, 2), 0), {k: v for k, v in w.items() if k not in ("Wfc2", "bfc2")})
    state, restart = model.zero_state(b), torch.zeros(b, dtype=torch.uint8, device="cuda")

    def window(c, chunks=15, frames=32, batch=b):
        h = ctypes.c_void_p()
        _lib.check(lib.kws_window_create(batch, chunks, frames, c, 0.4, ctypes.byref(h)))
        return h

    def create(mdl, w1, w2, samples=3600, l1=b"12", l2=b"5"):
        out = ctypes.c_void_p()
        rc = lib.kws_stream_create_heads(mdl._handle, fe._handle, w1, w2, b, samples, 30.0, l1, l2, _lib.ptr(state), _lib.ptr(restart),
                                         ctypes.byref(out))
        if rc == _lib.KWS_OK:
            lib.kws_stream_destroy(out)
        return rc, lib.kws_last_error().decode()
    w6, w8, w3, wb = window(6), window(8), window(3), window(8, batch=b + 1)
    allocs = model.scratch_stats()[1]
    assert create(model, w6, w3)[0] == _lib.KWS_ERR_INVALID_ARGUMENT                  # window 2 has another class count than head 2
    assert create(model, w8, w8)[0] == _lib.KWS_ERR_INVALID_ARGUMENT                  # window 1 ... than head 1 (and the same handle twice)
    assert create(model, w6, wb)[0] == _lib.KWS_ERR_INVALID_ARGUMENT                  # another batch
    assert create(model, w6, w8, samples=33 * 160 + 400)[0] == _lib.KWS_ERR_INVALID_ARGUMENT      # more frames per chunk than the windows hold
    assert create(model, w6, w8, l2=b"05")[0] == _lib.KWS_ERR_INVALID_ARGUMENT        # a bad label
    rc, msg = create(one, w6, w8)
    assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "second class head" in msg          # a model without a second head
    with pytest.raises(_lib.InvalidArgumentError):
        StreamManager(one, b, label="12", label2="5")
    # long chunks x the windows that hold them: more LDS than a workgroup may hold, refused with the byte counts
    l6, l8 = window(6, chunks=4, frames=6000), window(8, chunks=4, frames=6000)
    rc, msg = create(model, l6, l8, samples=6000 * 160)
    assert rc == _lib.KWS_ERR_UNSUPPORTED and "bytes of LDS" in msg and str(32768 + 32 * 6000 + 512 + 2 * 16 * (4 * 32 + 32)) in msg, msg
    assert model.scratch_stats()[1] == allocs                                         # refused before any device work on the model
    # a label rebinding: the windows of a manager that ran with "5" do not continue with "6"
    mgr = StreamManager(model, b, label="12", label2="5")
    mel = torch.from_numpy(G.synthetic_mel(b, 3, 40, seed=1)).cuda()
    mgr.feed(mel)
    silent = torch.zeros(b, dtype=torch.uint8, device="cuda")
    for l1, l2 in ((b"12", b"6"), (b"13", b"5")):
        rc = lib.kws_step_heads_window(model._handle, _lib.ptr(mel), _lib.ptr(mgr.state), _lib.ptr(mgr.state), None, b, 3, mgr._win, mgr._win2,
                                       l1, l2, _lib.ptr(silent), None, None, _lib.ptr(mgr.hit), _lib.ptr(mgr.restart), None)
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and "cannot continue" in lib.kws_last_error().decode()
    mgr.feed(mel)                                                                     # ... and go on with their own
    mgr.close()
    for h in (w6, w8, w3, wb, l6, l8):
        lib.kws_window_destroy(h)
    model.close()
    one.close()
