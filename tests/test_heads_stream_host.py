"""The two-head stream manager without a GPU.

1. The coupled incremental windows (two tests/window_model.IncrementalWindow plus the cross-clear: what heads_window_kernel keeps
   per stream) decide what the reference's policy decides -- a SimpleQueue per head, re-scanned with ctc_decode2 / ctc_predict, the
   two decisions ORed and BOTH queues cleared on a detection (detector.py:195-209 per head, README "decode respectively",
   server_demo.py:122-129) -- on random per-frame word traces with chunk lengths including 0, silence, and window sizes 1, 15, 17.
   In the incremental form "the other head fired" must be the same state change as "this head fired", evictions included.
2. The two new entry points refuse null handles and null pointers before any device work, and the Python layer refuses label2 on
   a model without a second head before it touches the device."""
import ctypes

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from heads_stream_model import CoupledRescan, CoupledWindows

LABELS1 = ["12", "1233", "1", "121", "33"]
LABELS2 = ["5", "25", "1", "56", "66"]          # head 2 (8 classes) has the words 0..5: digits 1..6


def _chunk(max_word):
    plain = st.lists(st.integers(-1, max_word), min_size=0, max_size=7)
    # long runs of one word make words straddle chunk boundaries and evictions
    held = st.builds(lambda w, n, tail: [w] * n + tail, st.integers(-1, max_word), st.integers(0, 6), st.lists(st.integers(-1, max_word), max_size=2))
    return st.one_of(plain, held)


@st.composite
def _trace(draw):
    """Chunks of both heads: the same number of frames in both (one stack, two projections), words drawn per head."""
    out = []
    for _ in range(draw(st.integers(1, 40))):
        w1 = draw(_chunk(3))
        w2 = draw(st.lists(st.integers(-1, 5), min_size=len(w1), max_size=len(w1)))
        if w2 and draw(st.booleans()):                    # a plateau in head 2 as well
            w2 = [w2[0]] * len(w2)
        out.append((w1, w2, draw(st.booleans())))
    return out


@settings(max_examples=500, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(trace=_trace(), max_chunks=st.sampled_from([1, 2, 3, 15, 17]), label1=st.sampled_from(LABELS1), label2=st.sampled_from(LABELS2),
       clear_rate=st.sampled_from([0, 0, 1]))
def test_coupled_incremental_windows_equal_the_coupled_rescan(trace, max_chunks, label1, label2, clear_rate):
    inc, ref = CoupledWindows(max_chunks, label1, label2), CoupledRescan(max_chunks, label1, label2)
    for k, (w1, w2, flag) in enumerate(trace):
        clear = bool(flag and clear_rate and k % 3 == 0)
        assert inc.step(w1, w2, clear) == ref.step(w1, w2, clear), (k, w1, w2, clear, max_chunks, label1, label2)


def _random_run(rng, max_chunks, label1, label2, steps, cross_clear=True):
    """Chunks of realistic length (0..23 frames) with word plateaus per head -> (masks of the incremental form, of the re-scan)."""
    inc, ref = CoupledWindows(max_chunks, label1, label2, cross_clear), CoupledRescan(max_chunks, label1, label2)
    word, got, want = [-1, -1], [], []
    for _ in range(steps):
        n = int(rng.choice([0, 1, 3, 21, 22, 23]))
        words = ([], [])
        for _ in range(n):
            for k, top in ((0, 4), (1, 6)):
                if rng.random() < 0.12:
                    word[k] = int(rng.integers(-1, top))
                words[k].append(word[k])
        clear = bool(rng.random() < 0.03)
        got.append(inc.step(words[0], words[1], clear))
        want.append(ref.step(words[0], words[1], clear))
    return got, want


def test_coupled_windows_on_long_random_streams():
    """Thousands of evictions with words held across them, window sizes 1 / 15 / 17, every kind of hit."""
    rng = np.random.default_rng(23)
    kinds = np.zeros(4, int)
    for trial in range(24):
        got, want = _random_run(rng, int(rng.choice([1, 15, 17])), str(rng.choice(["12", "33", "121"])), str(rng.choice(["5", "25", "56"])), 300)
        assert got == want, trial
        kinds += np.bincount(want, minlength=4)
    assert (kinds[1:] >= 3).all(), kinds                  # head 1 alone, head 2 alone, both in one chunk


def test_the_cross_clear_is_what_the_comparison_sees():
    """The same runs without the cross-clear (a head-2 hit leaves head 1's window alone) differ from the policy: the property above
    is not vacuous."""
    rng = np.random.default_rng(23)
    differ = 0
    for trial in range(24):
        got, want = _random_run(rng, int(rng.choice([1, 15, 17])), str(rng.choice(["12", "33", "121"])), str(rng.choice(["5", "25", "56"])), 300,
                                cross_clear=False)
        differ += got != want
    assert differ >= 3


def test_null_and_invalid_arguments_are_rejected():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_stream_create_heads", "kws_step_heads_window"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED_SYMBOLS
    dummy, out = ctypes.c_void_p(1), ctypes.c_void_p(7)
    bad = _lib.KWS_ERR_INVALID_ARGUMENT
    # kws_stream_create_heads: no out pointer; null handles / pointers (out is cleared); handles that are not alive
    assert lib.kws_stream_create_heads(dummy, dummy, dummy, dummy, 1, 3600, 30.0, b"12", b"5", dummy, dummy, None) == bad
    assert lib.kws_stream_create_heads(None, None, None, None, 1, 3600, 30.0, None, None, None, None, ctypes.byref(out)) == bad
    assert out.value is None
    for hole in range(4):
        args = [dummy] * 4
        args[hole] = None
        out = ctypes.c_void_p(7)
        assert lib.kws_stream_create_heads(*args, 1, 3600, 30.0, b"12", b"5", dummy, dummy, ctypes.byref(out)) == bad
        assert out.value is None
    assert lib.kws_stream_create_heads(dummy, dummy, dummy, dummy, 1, 3600, 30.0, b"12", None, dummy, dummy, ctypes.byref(out)) == bad
    assert lib.kws_stream_create_heads(dummy, dummy, dummy, dummy, 1, 3600, 30.0, b"12", b"5", dummy, dummy, ctypes.byref(out)) == bad
    assert b"not alive" in lib.kws_last_error()
    # kws_step_heads_window: null model; null windows / labels / hit / state; handles that are not alive
    assert lib.kws_step_heads_window(None, dummy, dummy, dummy, None, 1, 1, dummy, dummy, b"12", b"5", None, None, None, dummy, None, None) == bad
    for kw in ({"w1": None}, {"w2": None}, {"l1": None}, {"l2": None}, {"hit": None}, {"si": None}, {"so": None}, {"mel": None}):
        a = dict(mel=dummy, si=dummy, so=dummy, w1=dummy, w2=dummy, l1=b"12", l2=b"5", hit=dummy)
        a.update(kw)
        assert lib.kws_step_heads_window(dummy, a["mel"], a["si"], a["so"], None, 1, 1, a["w1"], a["w2"], a["l1"], a["l2"], None, None, None,
                                         a["hit"], None, None) == bad, kw
        assert b"null pointer" in lib.kws_last_error()
    assert lib.kws_step_heads_window(dummy, dummy, dummy, dummy, None, 0, 1, dummy, dummy, b"12", b"5", None, None, None, dummy, None, None) == bad
    assert lib.kws_step_heads_window(dummy, dummy, dummy, dummy, None, 1, 1, dummy, dummy, b"12", b"5", None, None, None, dummy, None, None) == bad
    assert b"not alive" in lib.kws_last_error()


def test_stream_server_passes_label2_through(monkeypatch):
    """StreamServer(label2=..., decode_thres2=...) hands both to every StreamManager it creates; without label2 neither is passed."""
    from keyword_spotting_amd import serving

    class Stub(object):
        def __init__(self, *a, **kw):
            self.args, self.kw = a, kw

        def close(self):
            pass
    for name in ("DeployModel", "MelFrontend", "StreamManager"):
        monkeypatch.setattr(serving, name, Stub)
    monkeypatch.setattr(serving.torch.cuda, "Stream", lambda device=None: None)
    srv = serving.StreamServer(object(), weights={}, handles=1, label="12", label2="5", decode_thres2=0.6)
    assert srv._mgr_args["label2"] == "5" and srv._mgr_args["decode_thres2"] == 0.6 and srv._mgr_args["label"] == "12"
    mgr = Stub(srv.models[0], 4, **srv._mgr_args)
    assert mgr.kw["label2"] == "5"
    plain = serving.StreamServer(object(), weights={}, handles=1, label="12")
    assert "label2" not in plain._mgr_args and "decode_thres2" not in plain._mgr_args


class _OneHead(object):
    """A model without a second head; anything else the constructors ask of it means they went on."""
    num_classes2 = 0

    def __getattr__(self, name):
        raise AssertionError("touched the model (%s) before label2 was checked" % name)


def test_label2_needs_a_second_head_before_any_device_call():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.detector import _second_head
    with pytest.raises(_lib.InvalidArgumentError):
        _second_head(_OneHead(), "5", None, 0.4)
    with pytest.raises(_lib.InvalidArgumentError):
        _second_head(_OneHead(), None, 0.5, 0.4)             # a threshold for a head that is not decoded
    assert _second_head(_OneHead(), None, None, 0.4) == (None, None)

    class TwoHeads(object):
        num_classes2 = 8
    assert _second_head(TwoHeads(), "25", None, 0.4) == ("25", 0.4) and _second_head(TwoHeads(), "5", 0.6, 0.4) == ("5", 0.6)
