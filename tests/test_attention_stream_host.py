"""The self-attention model's sliding-window stream manager without a GPU: the refusals of kws_attention_stream_*, the window policy of
the float64 restatement (tests/attention_stream_model.py) against a plain SimpleQueue, the float64 policy loop against its pieces
composed by hand, and the conditions the GPU cases (tests/test_gpu_attention_stream.py) lean on, from the restatement alone.

The chosen inputs (attention_stream_model.CASES; random-initialised weights never say "1233", so W_out is scaled by 30, the labels are
short and the seeds were searched on the CPU) and what the float64 loop counts over them, 30 chunks per case:

    case     streams  label  triggers  silence clears  evictions  of a zero-frame slot  triggers after an eviction  rows (max)  compared
    w15_c1   17       2121   8         26              47         2                     4                           374         495 / 510
    w3_c2    33       2      190       122             135        15                    49                          37          990 / 990
    w1_c2    1        34     5         4               20         1                     3                           17          30 / 30
    w3_c1    17       121    46        81              184        8                     31                          65          510 / 510
"""
import ctypes

import numpy as np
import pytest

import attention_model as AM
import attention_stream_model as SM
from conftest import have_gpu
from oracle import decode_oracle as DO
from oracle import frontend_oracle as FO


def _lib():
    from keyword_spotting_amd import _lib
    return _lib, _lib.load()


def test_symbols_are_bound_and_exported():
    _l, lib = _lib()
    for sym in ("create", "destroy", "feed", "recycle", "window", "carry", "stats"):
        assert "kws_attention_stream_" + sym in _l.EXPORTED_SYMBOLS and hasattr(lib, "kws_attention_stream_" + sym)
    import keyword_spotting_amd as K
    assert "AttentionStreamManager" in K.__all__ and "AttentionHotwordDetector" in K.__all__
    from keyword_spotting_amd import attention_stream
    assert K.AttentionStreamManager is attention_stream.AttentionStreamManager
    assert K.AttentionHotwordDetector is attention_stream.AttentionHotwordDetector


def test_refusals_that_need_no_handle():
    """Null pointers, the shape arguments, the label's form and handles that are not alive: all decided before anything is dereferenced
    or the device is touched, so they are reached with made-up handle values and no GPU."""
    _l, lib = _lib()
    bad, unsupported = _l.KWS_ERR_INVALID_ARGUMENT, _l.KWS_ERR_UNSUPPORTED
    buf = (ctypes.c_char * 64)()
    dummy = ctypes.cast(buf, ctypes.c_void_p)
    out = ctypes.c_void_p(1)

    def create(model=dummy, fe=dummy, B=2, chunk=3600, nq=15, label=b"12", o=None):
        rc = lib.kws_attention_stream_create(model, fe, B, chunk, nq, 30.0, 0.4, label, ctypes.byref(out) if o is None else o)
        return rc, lib.kws_last_error().decode()

    assert lib.kws_attention_stream_create(dummy, dummy, 2, 3600, 15, 30.0, 0.4, b"12", None) == bad
    assert "out handle pointer is null" in lib.kws_last_error().decode()
    for kw, word in ((dict(model=None), "model"), (dict(fe=None), "frontend"), (dict(label=None), "label")):
        out.value = 1
        rc, msg = create(**kw)
        assert rc == bad and "null argument: " + word in msg and not out.value, (kw, msg)      # out is cleared
    for B in (0, -3):
        rc, msg = create(B=B)
        assert rc == bad and "B=%d" % B in msg, msg
    for nq in (0, -1, 65, 1000):
        rc, msg = create(nq=nq)
        assert rc == unsupported and "window_chunks=%d" % nq in msg and "1..64" in msg, msg
    rc, msg = create(chunk=0)
    assert rc == bad and "max_chunk_samples=0" in msg, msg
    rc, msg = create(label=b"")
    assert rc == bad and "label is empty" in msg, msg
    rc, msg = create(label=b"1212121212121212")
    assert rc == bad and "label longer than 15" in msg, msg
    for label in (b"1x", b"10", b"12 "):
        rc, msg = create(label=label)
        assert rc == bad and "label must be digits 1..9" in msg, msg
    rc, msg = create()
    assert rc == bad and "not alive" in msg, msg
    # every other entry point: the null handle and null pointers
    assert lib.kws_attention_stream_destroy(None) == _l.KWS_OK
    assert lib.kws_attention_stream_feed(None, dummy, 1, None, 0, dummy, None, None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_attention_stream_recycle(None, dummy, None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_attention_stream_window(None, None, dummy, dummy, None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_attention_stream_carry(None, dummy, dummy, None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_attention_stream_stats(None, None, None) == bad and b"handle is null" in lib.kws_last_error()


@pytest.mark.skipif(not have_gpu(), reason="these refusals read the borrowed handles' configs, and a handle needs a device to exist")
def test_refusals_that_read_the_handles():
    """The refusals that compare the model's config with the front-end's: n_mel, max_frames, the front-end's kind and FFT size, a label
    digit outside 1..C-2 -- taken in kws_attention_stream_create before its first device call.  (Also in test_gpu_attention_stream.py.)"""
    import attention_stream_refusals
    attention_stream_refusals.check()


@pytest.mark.parametrize("nq", [1, 3, 15])
def test_window_policy_is_a_simple_queue_of_chunks(nq):
    """WindowPolicy (one linear array + slot lengths) against SimpleQueue.add / clear / get_all re-concatenated each step, over random
    slot lengths including 0, silences and triggers."""
    from keyword_spotting_amd.queue import SimpleQueue
    rng = np.random.default_rng(100 + nq)
    F = 5
    for trial in range(20):
        win, q = SM.WindowPolicy(nq, F), SimpleQueue(nq)
        evictions = zero = 0
        for step in range(80):
            event = rng.random()
            if event < 0.08:                # silence: cleared before the chunk is added
                win.clear(), q.clear()
            f = int(rng.choice([0, 0, 1, 2, 7, 31]))
            chunk = rng.standard_normal((f, F))
            full = q.full()
            zero += bool(full and q.get_all()[0].shape[0] == 0)
            evictions += full
            assert win.add(chunk) == full
            q.add(chunk)
            want = np.concatenate(q.get_all(), 0) if q.get_all() else np.zeros((0, F))
            np.testing.assert_array_equal(win.frames, want)
            assert win.slots == [c.shape[0] for c in q.get_all()] and len(win.slots) <= nq
            if 0.08 <= event < 0.14:        # trigger: cleared after the decision
                win.clear(), q.clear()
                assert win.frames.shape[0] == 0 and win.slots == []
        assert win.evictions == evictions and win.zero_evictions == zero
    assert evictions > 0


def test_policy_loop_is_its_pieces_composed_by_hand():
    """PolicyLoop.feed on explicit windows: oracle/frontend_oracle on [carry | chunk], tests/attention_model.forward on the concatenated
    window, oracle/decode_oracle on all of its rows."""
    case = "w3_c2"
    k = SM.CASES[case]
    cfg, w = SM.case_config(case), SM.case_weights(case)
    loop = SM.PolicyLoop(cfg, w, 2, SM.VAD_THRES, k["label"], k["thres"])
    rng = np.random.default_rng(5)
    a, b, c, d = (rng.standard_normal(n) * 0.2 for n in (1800, 150, 3600, 1000))
    mel = lambda x: FO.melspec(x[None], cfg.samplerate, cfg.fft_size, cfg.hop_size, cfg.n_mel, float(cfg.fmin), float(cfg.fmax))[0]

    def decided(window):
        sm = AM.forward(cfg, w, window)[1]
        return sm, DO.ctc_predict(DO.ctc_decode2(sm, cfg.num_classes, k["thres"]), k["label"])

    r = loop.feed(a)                        # 1800 samples: 9 frames, 360 carried
    ma = mel(a)
    assert (r["frames"], r["len"], r["chunks"], r["carry"]) == (9, 9, 1, 360) and not r["silent"] and not r["evicted"]
    sm, hit = decided(ma)
    np.testing.assert_array_equal(r["softmax"], sm)
    assert r["hit"] == hit and r["rows"] == AM.frames_out(9, cfg.combine_frame)
    loop.win.frames, loop.win.slots = ma, [9]              # (whatever was decided: go on from the full window)
    r = loop.feed(np.zeros(0))
    assert r["skipped"] and r["hit"] == 0 and loop.res.shape[0] == 360 and loop.win.slots == [9]
    r = loop.feed(b)                        # 360 + 150 = 510 samples: 1 frame, 350 carried
    mb = mel(np.concatenate([a[-360:], b]))
    assert (r["frames"], r["len"], r["chunks"], r["carry"]) == (1, 10, 2, 350)
    np.testing.assert_array_equal(r["softmax"], decided(np.concatenate([ma, mb], 0))[0])
    loop.win.frames, loop.win.slots = np.concatenate([ma, mb], 0), [9, 1]
    r = loop.feed(c)                        # the window is full: slot a goes with its 9 frames
    mc = mel(np.concatenate([np.concatenate([a[-360:], b])[-350:], c]))
    assert r["evicted"] and not r["zero_evicted"] and r["len"] == 1 + mc.shape[0] and r["chunks"] == 2
    sm, hit = decided(np.concatenate([mb, mc], 0))
    np.testing.assert_array_equal(r["softmax"], sm)
    assert r["hit"] == hit
    r = loop.feed(d * 1e-6)                 # silence: the window is emptied first, the chunk still takes a slot
    assert r["silent"] and r["chunks"] == 1 and r["len"] == r["frames"] and not r["evicted"]
    loop.recycle()
    r = loop.feed(b)                        # a fresh stream: 150 samples complete no frame
    assert (r["frames"], r["len"], r["chunks"], r["carry"], r["hit"], r["rows"]) == (0, 0, 1, 150, 0, 0)


@pytest.mark.parametrize("case", sorted(SM.CASES))
def test_conditions_the_gpu_cases_lean_on(case):
    c = SM.case_counts(case)
    print(case, c)
    assert c["triggers"] >= 3 and c["silences"] >= 3 and c["evictions"] >= 3, c
    assert c["zero_evictions"] >= 1 and c["trigger_after_eviction"] >= 1, c
    assert 2 * c["compared"] >= c["pairs"], c                  # at least half of all (stream, chunk) pairs precede their stream's first edge
    k = SM.CASES[case]
    if k["nq"] == 15 and k["c"] == 1:
        assert c["max_rows"] > 256, c                          # the decide kernel takes several passes of 64 rows, and more than four
    lens = SM.case_inputs(case)[1]
    assert set(np.unique(np.concatenate(lens))) <= set(SM.LENGTHS)
    if k["ragged"]:
        assert set(np.unique(np.concatenate(lens))) == set(SM.LENGTHS)


def test_the_cases_cover_the_axes():
    ks = list(SM.CASES.values())
    assert {k["L"] for k in ks} == {1, 2} and {k["c"] for k in ks} == {1, 2} and {k["n_mel"] for k in ks} == {40, 60}
    assert {k["C"] for k in ks} == {4, 6} and {k["B"] for k in ks} == {1, 17, 33} and {k["nq"] for k in ks} == {1, 3, 15}
    assert {(k["int16"], k["ragged"]) for k in ks} == {(False, True), (True, True), (False, False), (True, False)}
    assert any(k["nq"] == 15 and k["c"] == 1 for k in ks)
