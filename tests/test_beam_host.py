"""CPU checks of the CTC prefix beam search: the fp64 restatement tests/beam_model.py against brute-force enumeration of all C^T
paths and against torch's CTC loss in fp64, its pruning, merge_repeated and L_max rules, the re-entry event the device tests rely on,
every refusal kws_ctc_beam_search raises before it touches a device, and the host side of the Python wrapper."""
import ctypes
import inspect

import numpy as np
import pytest

import beam_model as M
from conftest import have_gpu

# (T, C, the number of labellings an unpruned beam has to hold where the device tests rely on it)
UNPRUNED = [(1, 3, None), (2, 3, None), (5, 3, None), (4, 3, 15), (3, 4, 25)]


def _logits(seed, t, c):
    return M.make_logits(seed, t, c, 0)


@pytest.mark.parametrize("t,c,count", UNPRUNED)
def test_unpruned_restatement_is_brute_force(t, c, count):
    for seed in range(3):
        x = _logits(seed, t, c)
        exact = M.brute_force(x)
        assert count is None or len(exact) == count
        count = len(exact)
        r = M.beam_search(x, beam_width=count, top_paths=count, merge_repeated=False)
        assert sorted(r["paths"]) == sorted(exact)
        err = max(abs(float(s) - exact[p]) for p, s in zip(r["paths"], r["scores"]))
        assert err <= 1e-10, err
        assert list(r["scores"]) == sorted(r["scores"], reverse=True)
        assert abs(np.logaddexp.reduce(r["scores"])) <= 1e-10          # the labellings' probabilities sum to one


def test_negative_control_is_caught_by_brute_force():
    """lp_b (+) lp_nb instead of lp_b for the extension by the last label counts paths that need a blank between the repeats"""
    x = _logits(0, 4, 3)
    exact = M.brute_force(x)
    r = M.beam_search(x, beam_width=15, top_paths=15, merge_repeated=False, repeat_from_total=True)
    # (labellings no path of four frames collapses to appear too: their truth is -inf)
    err = {p: abs(float(s) - exact.get(p, -np.inf)) for p, s in zip(r["paths"], r["scores"])}
    assert max(err.values()) > 1e-3
    assert all(any(a == b for a, b in zip(p, p[1:])) for p, e in err.items() if e > 1e-10)      # only labellings with a repeat


def test_top_path_score_is_torchs_ctc_loss():
    x = _logits(1, 12, 4)
    r = M.beam_search(x, beam_width=32, top_paths=32, merge_repeated=False)
    exact_w = M.beam_search(x, beam_width=10 ** 9, top_paths=3, merge_repeated=False)              # nothing pruned
    for p, s in zip(exact_w["paths"], exact_w["scores"]):
        assert abs(float(s) - M.torch_log_prob(x, p)) <= 1e-10
    for p, s in zip(r["paths"], r["scores"]):                                                     # pruned: never above the truth
        assert float(s) <= M.torch_log_prob(x, p) + 1e-10


@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_pruned_scores_are_lower_bounds(w):
    for seed in range(4):
        x = M.make_logits(seed, 48, 6, w)
        r = M.beam_search(x, beam_width=w, top_paths=w, merge_repeated=False)
        assert len(set(r["paths"])) == w
        for p, s in zip(r["paths"], r["scores"]):
            assert float(s) <= M.torch_log_prob(x, p) + 1e-10
        assert r["gap"] >= 0


def test_merge_repeated_and_l_max():
    x = np.full((6, 3), -4.0, np.float32)
    for t, c in enumerate([0, 2, 0, 2, 1, 1]):          # label 0, blank, label 0, blank, label 1 twice: the labelling (0, 0, 1)
        x[t, c] = 4.0
    plain = M.beam_search(x, beam_width=4, top_paths=2, merge_repeated=False)
    merged = M.beam_search(x, beam_width=4, top_paths=2, merge_repeated=True)
    assert plain["paths"][0] == (0, 0, 1) and merged["paths"][0] == (0, 1) and merged["raw"][0] == (0, 0, 1)
    assert np.array_equal(plain["scores"], merged["scores"])
    for l_max in (1, 2):                                # no prefix grows past L_max; what is kept still scores below the truth
        r = M.beam_search(x, beam_width=4, top_paths=4, l_max=l_max, merge_repeated=False)
        assert max(len(p) for p in r["paths"]) == l_max
        for p, s in zip(r["paths"], r["scores"]):
            if s > -np.inf:
                assert float(s) <= M.torch_log_prob(x, p) + 1e-10
    d, n = M.dense(merged["paths"], 4)
    assert d.tolist()[0] == [0, 1, -1, -1] and n[0] == 2
    empty = M.beam_search(x, seq_len=0, beam_width=2, top_paths=2)
    assert empty["paths"] == [(), ()] and empty["scores"][0] == 0 and empty["scores"][1] == -np.inf
    assert M.beam_search(x, seq_len=99, beam_width=2)["scores"][0] == M.beam_search(x, beam_width=2)["scores"][0]
    assert M.beam_search(x, seq_len=3, beam_width=2)["scores"][0] == M.beam_search(x[:3], beam_width=2)["scores"][0]


@pytest.mark.parametrize("t,c,w", [(48, 3, 2), (48, 4, 3)])
def test_a_prefix_comes_back_beside_its_surviving_child(t, c, w):
    """the event that makes identity-by-content matter occurs on the inputs tests/test_gpu_beam.py uses"""
    count = sum(M.beam_search(M.make_logits(seed, t, c, w), beam_width=w, top_paths=w)["reentries"] for seed in range(12))
    print("BEAM-REENTRIES T=%d C=%d W=%d: %d over 12 seeds" % (t, c, w, count))
    assert count > 0


def test_a_prefix_comes_back_and_its_child_stays():
    """... and on the flat inputs (peak 1.0) the returning prefix and its extension are both kept: the merge by content is exercised"""
    runs = [M.beam_search(M.make_logits(seed, 24, 3, 3, peak=1.0), beam_width=3, top_paths=3) for seed in M.REJOIN_SEEDS]
    assert all(r["rejoined"] > 0 for r in runs)


def test_float32_restatement_stays_close():
    x = M.make_logits(0, 48, 6, 5)
    r64, r32 = M.beam_search(x, beam_width=5, top_paths=5), M.beam_search(x, beam_width=5, top_paths=5, dtype=np.float32)
    assert r32["scores"].dtype == np.float32
    assert np.abs(r32["scores"].astype(np.float64) - r64["scores"]).max() <= 1e-3


def test_symbol_is_bound():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert "kws_ctc_beam_search" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "kws_ctc_beam_search")
    assert len(lib.kws_ctc_beam_search.argtypes) == 13


def test_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    x = ctypes.c_void_p(256)            # a non-null, aligned address that is never read: every refusal below comes first

    def call(logits=x, seq=None, b=2, t=48, c=6, w=5, k=1, l_max=64, merge=1, paths=x, lengths=x, log_prob=x):
        return lib.kws_ctc_beam_search(logits, seq, b, t, c, w, k, l_max, merge, paths, lengths, log_prob, None)
    bad = _lib.KWS_ERR_INVALID_ARGUMENT
    for kw in ({"logits": None}, {"paths": None}, {"lengths": None}, {"log_prob": None}):
        assert call(**kw) == bad and b"null pointer" in lib.kws_last_error()
    assert call(c=2) == bad and b"C=2" in lib.kws_last_error()
    assert call(c=9) == bad and b"C=9" in lib.kws_last_error()
    assert call(w=0) == bad and b"beam_width=0" in lib.kws_last_error()
    assert call(w=33) == bad and b"beam_width=33" in lib.kws_last_error()
    assert call(k=0) == bad and b"top_paths=0" in lib.kws_last_error()
    assert call(k=6) == bad and b"top_paths=6 out of range [1,beam_width=5]" in lib.kws_last_error()
    assert call(l_max=0) == bad and b"L_max=0" in lib.kws_last_error()
    assert call(l_max=65) == bad and b"L_max=65" in lib.kws_last_error()
    assert call(b=0) == bad and b"B=0" in lib.kws_last_error()
    assert call(t=0) == bad and b"T=0" in lib.kws_last_error()
    assert call(logits=ctypes.c_void_p(264)) == bad and b"16-byte aligned" in lib.kws_last_error()
    assert call(seq=ctypes.c_void_p(258)) == bad and call(log_prob=ctypes.c_void_p(257)) == bad
    assert call(t=4885) == _lib.KWS_ERR_UNSUPPORTED                      # 32 x 4885 + 7552 = 163872 > 163840
    assert b"163872 bytes exceed the 163840" in lib.kws_last_error() and b"7552 bytes of beam" in lib.kws_last_error()
    if not have_gpu():
        assert call() == _lib.KWS_ERR_NO_DEVICE
        assert call(t=4884, w=32, k=32, c=8, seq=x) == _lib.KWS_ERR_NO_DEVICE


def test_python_wrapper_host_side():
    from keyword_spotting_amd import prediction as P
    sig = inspect.signature(P.ctc_beam_search_decode)
    assert list(sig.parameters)[:6] == ["inputs", "lengths", "beam_width", "top_paths", "merge_repeated", "max_len"]
    defaults = {k: v.default for k, v in sig.parameters.items()}
    assert defaults["beam_width"] is None and defaults["top_paths"] == 1 and defaults["merge_repeated"] is True and defaults["max_len"] == 64
    assert list(inspect.signature(P.decode_best).parameters)[0] == "inputs"
    # a dense row -> the other decoders' form: the space class 0 and the -1 padding go, the words stand between zeros
    assert P.path_to_seq([0, 1, 0, 2, 0, 3, 0, 3, 0, -1, -1]).tolist() == P.ctc_label([1, 2, 3, 3]).tolist()
    assert P.path_to_seq([-1, -1]).tolist() == [0] and P.path_to_seq([0, -1, 5]).tolist() == [0]
    assert P.path_to_seq(np.array([3, 4], np.int32)).dtype == np.int32 and P.path_to_seq([3, 4]).tolist() == [0, 3, 0, 4, 0]
