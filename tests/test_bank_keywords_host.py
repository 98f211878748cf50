"""CPU checks of per-slot keywords in the bank of enrolled heads (kws_bank_set_keyword / kws_bank_get_keyword, KeywordBank.set_keyword):
the bound symbols and the refusals that need no live handle; the fp64 restatement tests/bank_keywords_model.py reduces to
tests/bank_model.py when every slot has (label2, n_new); why the host mirror slices a queued row to its slot's width before decoding;
KeywordBank.set's padding and label plumbing on a stub library; and the incremental window with one matcher per stream against the
re-scan.  (Refusals that need a live bank -- slot, n_used, the label's digits -- are in tests/test_gpu_bank_keywords_stream.py.)"""
import contextlib
import ctypes

import numpy as np
import pytest

import bank_keywords_model as KM
import bank_model as BM
import window_model as WM
from oracle import decode_oracle as D
from oracle import gru_oracle as G


def test_symbols_are_bound_and_dead_handles_are_refused_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_bank_set_keyword", "kws_bank_get_keyword"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED_SYMBOLS
    bad = _lib.KWS_ERR_INVALID_ARGUMENT
    err = lambda: lib.kws_last_error().decode()
    dummy = ctypes.c_void_p(256)                      # a non-null address that is no live handle and is never read
    n_used, own, label = ctypes.c_int(7), ctypes.c_int(7), ctypes.create_string_buffer(16)
    assert lib.kws_bank_set_keyword(None, 0, 1, b"5", None) == bad and "bank is null" in err()
    assert lib.kws_bank_set_keyword(dummy, 0, 1, b"5", None) == bad and "not alive" in err()
    assert lib.kws_bank_set_keyword(dummy, 0, 1, None, None) == bad and "not alive" in err()
    assert lib.kws_bank_get_keyword(None, 0, ctypes.byref(n_used), label, ctypes.byref(own)) == bad and "bank is null" in err()
    assert lib.kws_bank_get_keyword(dummy, 0, ctypes.byref(n_used), label, ctypes.byref(own)) == bad and "not alive" in err()
    assert n_used.value == 7 and own.value == 7       # a refused call writes nothing


@pytest.mark.parametrize("c,n_new", [(6, 2), (3, 5)])
def test_every_slot_at_label2_and_full_width_is_the_old_model(c, n_new):
    hidden, b, t, capacity = 64, 6, 40, 3
    w = G.random_weights(13, hidden, 2, c, seed=3)
    w["Wfc"] = (w["Wfc"] * 3).astype(np.float32)
    cols, bias = BM.random_bank(hidden, n_new, capacity, seed=4, scale=3.0)
    mel = G.synthetic_mel(b, t, 13, seed=5)
    st = (0.3 * np.random.default_rng(6).standard_normal((2, b, hidden))).astype(np.float32)
    users = np.array([0, 1, 2, -1, 7, 1])
    lens = np.array([0, 1, t - 1, t, t, 7], np.int64)
    full = np.full(b, n_new)
    for relu, clip in ((False, -1.0), (True, 20.0)):
        got = KM.bank_forward(w, cols, bias, users, full, mel, st, lens, use_relu=relu, value_clip=clip)
        want = BM.bank_forward(w, cols, bias, users, mel, st, lens, use_relu=relu, value_clip=clip)
        for k in want:
            assert np.abs(got[k] - want[k]).max() <= 1e-12, (k, relu)
    chunks, labels = [10, 0, 10, 10, 10], ("1", str(c - 1))
    speech = np.random.default_rng(7).random((len(chunks), b)) > 0.1
    keywords = [(None, n_new), (labels[1], n_new), (None, n_new)]
    per = KM.stream_keywords(keywords, users, n_new, labels[1])
    assert per == [(labels[1], n_new)] * b
    got = KM.policy_loop(w, cols, bias, users, [k[1] for k in per], mel, chunks, speech, labels[0], [k[0] for k in per], (0.4, 0.3), 2)
    want = BM.policy_loop(w, cols, bias, users, mel, chunks, speech, labels, (0.4, 0.3), 2)
    assert np.array_equal(got["mask"], want["mask"]) and np.array_equal(got["margin_ok"], want["margin_ok"])
    assert (want["mask"] & 2).any()
    # ... and a narrower slot is another head: its rows are the softmax over C + n_used classes, zero-padded
    narrow = KM.bank_forward(w, cols, bias, users, np.ones(b, int), mel, st)
    assert not narrow["softmax2"][..., c + 1:].any() and not narrow["logits2"][..., c + 1:].any()
    live = (users >= 0) & (users < capacity)
    assert np.abs(narrow["softmax2"][live].sum(-1) - 1).max() <= 1e-12
    assert np.array_equal(narrow["logits2"][live][..., c], want_blank(w, cols, bias, users, mel, st)[live])


def want_blank(w, cols, bias, users, mel, st):
    """head 1's blank logit: where a slot of width 1 has its blank (column C)"""
    return BM.bank_forward(w, cols, bias, users, mel, st)["logits1"][..., -1]


def test_a_padded_row_must_be_sliced_to_the_slots_width_before_decoding():
    """C = 6, n_new = 2, a slot with n_used = 1: its rows have 7 classes -- words 1..5, blank at column 6 -- zero-padded to 8.  Read at
    the bank's width 8 the blank column 6 is word class 6: a frame that is confidently BLANK decodes to word 6."""
    c, n_new, n_used, thres = 6, 2, 1, 0.4
    row = np.zeros((3, c + n_new))
    row[0, [5, 6]] = 0.9, 0.1                    # the new word 5
    row[1, [5, 6]] = 0.05, 0.95                  # blank, above the threshold
    row[2, [0, 6]] = 0.5, 0.5
    sliced = D.ctc_decode2(row[:, :c + n_used], c + n_used, thres)
    padded = D.ctc_decode2(row, c + n_new, thres)
    assert [int(v) for v in sliced[1::2]] == [5]
    assert [int(v) for v in padded[1::2]] == [5, 6]
    assert D.ctc_predict(padded, "56") and not D.ctc_predict(sliced, "56")
    # the restatement's rows are of that kind: a narrow slot's blank sits where the full width has a word class
    assert KM.stream_keywords([("5", 1)], [0, -1], n_new, "56") == [("5", 1), ("56", n_new)]


class _StubLib(object):
    """Records kws_bank_set / kws_bank_set_keyword; kws_bank_get_keyword answers from what was set."""

    def __init__(self, n_new):
        self.n_new, self.sets, self.keywords = n_new, [], {}

    def kws_bank_set(self, handle, first, count, wn, bn, stream):
        per = 4 * self.n_new
        w = np.ctypeslib.as_array((ctypes.c_float * (count * per)).from_address(wn.value)).reshape(count, 4, self.n_new).copy()
        b = np.ctypeslib.as_array((ctypes.c_float * (count * self.n_new)).from_address(bn.value)).reshape(count, self.n_new).copy()
        self.sets.append((first, w, b))
        return 0

    def kws_bank_set_keyword(self, handle, slot, n_used, label, stream):
        self.keywords[slot] = (label, n_used)
        return 0

    def kws_bank_get_keyword(self, handle, slot, n_used, label, own):
        lab, n = self.keywords.get(slot, (None, self.n_new))
        n_used._obj.value, own._obj.value = n, int(lab is not None)
        label.value = lab or b""
        return 0


def test_keyword_bank_set_pads_narrow_columns_and_sets_the_slots_keywords(monkeypatch):
    import torch
    from keyword_spotting_amd import _lib, get_config
    from keyword_spotting_amd.custom_keyword import KeywordBank
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(_lib, "current_stream_ptr", lambda: None)
    bank = object.__new__(KeywordBank)
    bank.config, bank.device, bank.n_new, bank.capacity = get_config(hidden_size=4), "cpu", 2, 8
    bank._lib, bank._handle, bank._has_keywords, bank.stack = _StubLib(2), ctypes.c_void_p(1), False, None
    rng = np.random.default_rng(0)
    full_w, full_b = rng.standard_normal((2, 4, 2)).astype(np.float32), rng.standard_normal((2, 2)).astype(np.float32)
    # today's full-width call: one kws_bank_set, no keyword
    bank.set(1, full_w, full_b)
    first, w, b = bank._lib.sets[-1]
    assert first == 1 and np.array_equal(w, full_w) and np.array_equal(b, full_b) and not bank._lib.keywords and not bank.has_keywords()
    assert bank.keyword(1) == (None, 2)
    # columns of a one-word enroller: zero-padded, each slot's keyword (label, 1)
    one_w, one_b = rng.standard_normal((2, 4, 1)).astype(np.float32), rng.standard_normal((2, 1)).astype(np.float32)
    bank.set(3, one_w, one_b, labels=["5", "55"])
    first, w, b = bank._lib.sets[-1]
    assert first == 3 and np.array_equal(w[..., :1], one_w) and not w[..., 1:].any()
    assert np.array_equal(b[:, :1], one_b) and not b[:, 1:].any()
    assert bank._lib.keywords == {3: (b"5", 1), 4: (b"55", 1)} and bank.has_keywords()
    assert bank.keyword(3) == ("5", 1) and bank.keyword(4) == ("55", 1) and bank.keyword(5) == (None, 2)
    # one label for all; full-width columns with labels; one slot as [H, n_u]
    bank.set(5, full_w, full_b, labels="1256")
    assert bank._lib.keywords[5] == (b"1256", 2) and bank._lib.keywords[6] == (b"1256", 2)
    bank.set(7, one_w[0], one_b[0], labels=["5"])
    assert bank._lib.sets[-1][1].shape == (1, 4, 2) and bank._lib.keywords[7] == (b"5", 1)
    bank.set_keyword(7, None)
    assert bank._lib.keywords[7] == (None, 2)
    # refused before the library is called: narrow columns without labels, a label count that does not match, columns too wide
    n_sets = len(bank._lib.sets)
    with pytest.raises(_lib.InvalidArgumentError, match="need labels"):
        bank.set(0, one_w, one_b)
    with pytest.raises(_lib.InvalidArgumentError, match="labels: 1 for 2"):
        bank.set(0, one_w, one_b, labels=["5"])
    with pytest.raises(_lib.InvalidArgumentError, match="columns / bias must be"):
        bank.set(0, np.zeros((1, 4, 3), np.float32), np.zeros((1, 3), np.float32))
    assert len(bank._lib.sets) == n_sets


LABELS = ["5", "55", "56", "565", "1256", "565656565656565"]


def test_incremental_window_with_a_matcher_per_stream_equals_the_rescan():
    """Six streams, one label each (the 15-digit one fills the matcher's 16 states), the same frame words for all of them: windows of 3
    chunks so that evictions occur, chunks of 0..6 frames, words 1..6 and none.  The incremental ring (window_model.IncrementalWindow,
    what window_device.h keeps) of stream s, built with ITS matcher, against the reference's re-scan of its queued frames for ITS label."""
    assert len(LABELS[-1]) == 15
    rng = np.random.default_rng(11)
    hits = np.zeros(len(LABELS), int)
    for trial in range(30):
        inc = [WM.IncrementalWindow(3, [int(d) for d in lab]) for lab in LABELS]
        queues = [D.SimpleQueue(3) for _ in LABELS]
        clean = trial % 3 == 0                                                 # every third trial: long clean 5 6 5 6 ... runs (the 15 digits)
        run = np.tile([5, 6], 300) if clean else rng.choice([5, 6, 1, 2], 600, p=[0.4, 0.4, 0.1, 0.1])
        pos = 0
        for step in range(60):
            n = int(rng.integers(4, 8)) if clean else int(rng.integers(0, 7))
            words = np.where(rng.random(n) < (0.02 if clean else 0.15), -1, run[pos:pos + n] - 1)
            if not clean and rng.random() < 0.3:
                words = np.repeat(words, 2)[:n]                                   # repeated words: no new emission
            pos += n
            clear = rng.random() < 0.05
            for s, lab in enumerate(LABELS):
                got = inc[s].step([int(v) for v in words], clear_before=clear)
                if clear:
                    queues[s].clear()
                queues[s].add(np.asarray(words, int))
                frames = np.concatenate(queues[s].get_all())
                seq, pre = [], -1
                for v in frames:                                                  # utils/prediction.py:74-80 over the window's frames
                    if v >= 0 and v != pre:
                        seq.append(int(v) + 1)
                    pre = v
                want = int(lab in "".join(str(v) for v in seq))
                assert got == want, (trial, step, lab, seq)
                if want:
                    queues[s].clear()
                hits[s] += want
    print("hits per label:", dict(zip(LABELS, hits)))
    assert (hits > 0).all(), hits
