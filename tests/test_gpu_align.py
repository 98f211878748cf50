"""CTC forced alignment on the device: kws_ctc_align against the restatement tests/align_model.py on the SAME float32 arrays.  The
yardstick is the deviation of the float32-CPU restatement from the fp64 one: score bound = max(4 x that deviation, 16 * 2^-23 * |score|)
(the convention of tests/test_gpu_enroll.py and tests/test_gpu_beam.py).  A case is DECIDED when the float32-CPU run returns the fp64
path and the fp64 selection gap (best - second-best path score) is >= 8 x the bound: then the device must return exactly the
restatement's states and spans, with the score within the bound.  Undecided cases (a near-tie somewhere along the path) still have to
satisfy the invariants; their share is capped at 4 of 12 per shape and 15 % overall.  Posteriors: per utterance within max(4 x the
float32-CPU deviation, 16 * 2^-23)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import align_model as M

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -23
SHAPES = [(1, 3, 0), (1, 3, 1), (2, 3, 1), (3, 3, 2), (5, 4, 2), (9, 6, 4), (40, 6, 4), (63, 8, 31), (64, 3, 8), (65, 6, 4), (150, 6, 9), (300, 8, 31),
          (300, 6, 4)]
SEEDS = range(12)
ALL = ("states", "spans", "loss", "post")


def run(x, seq_len, labels, want=ALL, s_max=None, stream=None):
    """x [B,T,C] float32, seq_len [B], labels: B lists -> dict of numpy arrays (score and what `want` names; the others are passed as NULL)"""
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    xd = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    b, t, c = (int(v) for v in xd.shape)
    s_max = max([len(l) for l in labels] + [0]) if s_max is None else s_max
    lab = np.zeros((b, max(s_max, 1)), np.int32)[:, :s_max].copy()
    for i, l in enumerate(labels):
        lab[i, :len(l)] = l
    lab_len = np.array([len(l) for l in labels], np.int32)
    sl = np.ascontiguousarray(seq_len, np.int32)
    out = {"score": torch.full((b,), 7.0, device="cuda"),
           "states": torch.full((b, t), -7, dtype=torch.int32, device="cuda") if "states" in want else None,
           "spans": torch.full((b, s_max, 2), -7, dtype=torch.int32, device="cuda") if "spans" in want else None,
           "loss": torch.full((b,), 7.0, device="cuda") if "loss" in want else None,
           "post": torch.full((b, t, s_max), 7.0, device="cuda") if "post" in want else None}
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        _lib.check(lib.kws_ctc_align(_lib.ptr(xd), sl.ctypes.data_as(ctypes.c_void_p), lab.ctypes.data_as(ctypes.c_void_p) if s_max else None,
                                     lab_len.ctypes.data_as(ctypes.c_void_p), b, t, c, s_max, _lib.ptr(out["states"]), _lib.ptr(out["spans"]),
                                     _lib.ptr(out["score"]), _lib.ptr(out["loss"]), _lib.ptr(out["post"]), ctypes.c_void_p(s.cuda_stream)))
    s.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def judge(x, n, label):
    """the two CPU runs of one utterance -> dict(r64, r32, bound, post_bound, decided)"""
    r64, r32 = M.align(x, n, label), M.align(x, n, label, dtype=np.float32)
    same = np.array_equal(r64["states"], r32["states"])
    s64 = float(r64["score"])
    dev = abs(float(r32["score"]) - s64) if r64["valid"] and r32["valid"] else 0.0
    bound = max(4.0 * dev, FLOOR * abs(s64)) if r64["valid"] else 0.0
    post_bound = max(4.0 * float(np.abs(r32["post"].astype(np.float64) - r64["post"]).max()) if r64["post"].size else 0.0, FLOOR)
    return dict(r64=r64, r32=r32, bound=bound, post_bound=post_bound, decided=bool(same and r64["gap"] >= 8.0 * bound))


@functools.lru_cache(maxsize=None)
def case(seed, shape):
    t, c, s = shape
    x, label = M.make_logits(seed, t, c), M.make_label(seed, t, c, s)
    return dict(judge(x, t, label), x=x, label=label)


def check(x, n, label, got, j):
    """one utterance's device result (dict of its rows) against the rules -> (|score error| / bound of a decided case, post error / bound)"""
    r64, bound = j["r64"], j["bound"]
    t_all, c = x.shape
    states, spans, score = got["states"], got["spans"], float(got["score"])
    s_lab, ns = len(label), 2 * len(label) + 1
    assert (states[n:] == -1).all() and (spans[s_lab:] == -1).all()
    assert not got["post"][n:].any() and not got["post"][:, s_lab:].any()
    assert got["post"].size == 0 or (got["post"].min() >= 0 and got["post"].max() <= 1)
    if n == 0:
        assert score == 0 and got["loss"] == 0 and (states == -1).all() and (spans == -1).all() and not got["post"].any()
        return 0.0, 0.0
    if not r64["valid"]:
        assert score == -np.inf and got["loss"] == np.inf and (states == -1).all() and (spans == -1).all() and not got["post"].any()
        return 0.0, 0.0
    # ---- invariants, on every case
    st = states[:n]
    ext, skip = M.extended(label, c - 1)
    assert st[0] in (0, 1) and st[-1] in (ns - 1, max(ns - 2, 0)) and st.min() >= 0 and st.max() < ns
    step = np.diff(st)
    assert ((step >= 0) & (step <= 2)).all() and skip[st[1:][step == 2]].all()               # s-2 -> s only where skip_in allows
    sp = spans[:s_lab]
    assert np.array_equal(sp, M.spans_of(states, s_lab)) and (sp >= 0).all()                 # consistent with states; every label has one
    assert (sp[:, 0] <= sp[:, 1]).all() and (sp[1:, 0] > sp[:-1, 1]).all()                   # disjoint and increasing
    lp = M.log_softmax(x[:n])
    along = float(lp[np.arange(n), ext[st]].sum())
    assert abs(along - score) <= bound, (along, score, bound)
    assert score >= float(r64["score"]) - bound
    assert score <= -float(got["loss"]) + bound
    post_err = float(np.abs(got["post"][:, :s_lab].astype(np.float64) - r64["post"]).max()) if r64["post"].size else 0.0
    assert post_err <= j["post_bound"], (post_err, j["post_bound"])
    if not j["decided"]:
        return 0.0, post_err / j["post_bound"]
    assert np.array_equal(states, r64["states"]) and np.array_equal(spans[:s_lab], r64["spans"])
    err = abs(score - float(r64["score"]))
    assert err <= bound, (err, bound)
    return (err / bound if bound > 0 else 0.0), post_err / j["post_bound"]


def row(got, i):
    return {k: v[i] for k, v in got.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


def test_entry_point_exists():
    from keyword_spotting_amd import _lib
    assert hasattr(_lib.load(), "kws_ctc_align")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-C%d-S%d" % s)
def test_against_the_restatement(shape):
    from keyword_spotting_amd.custom_keyword import ctc_loss
    t, c, s = shape
    cases = [case(seed, shape) for seed in SEEDS]
    xs, labels = np.stack([k["x"] for k in cases]), [k["label"] for k in cases]
    got = run(xs, [t] * len(cases), labels)                                     # the twelve seeds in one launch
    undecided, worst, worst_post = 0, 0.0, 0.0
    for i, k in enumerate(cases):
        ratio, post_ratio = check(k["x"], t, k["label"], row(got, i), k)
        worst, worst_post = max(worst, ratio), max(worst_post, post_ratio)
        undecided += not k["decided"]
    print("ALIGN-RATIO T=%d C=%d S=%d: worst score error / bound %.3f, worst posterior error / bound %.3f over %d cases, %d undecided"
          % (t, c, s, worst, worst_post, len(cases), undecided))
    loss, _ = ctc_loss(torch.from_numpy(xs), [t] * len(cases), labels, want_grad=False)
    assert np.array_equal(loss.cpu().numpy().view(np.int32), got["loss"].view(np.int32))      # bitwise kws_ctc_loss's
    assert undecided <= 4


def test_undecided_share_overall():
    undecided = sum(not case(seed, shape)["decided"] for shape in SHAPES for seed in SEEDS)
    print("ALIGN-UNDECIDED %d of %d" % (undecided, len(SHAPES) * len(SEEDS)))
    assert undecided <= 0.15 * len(SHAPES) * len(SEEDS)


@pytest.mark.parametrize("shape", [(5, 4, 2), (9, 6, 4), (40, 6, 4), (64, 3, 8), (65, 8, 31)], ids=lambda s: "T%d-C%d-S%d" % s)
def test_all_zero_logits_pin_the_tie_rule(shape):
    """every row is flat, every path to a (frame, state) adds the same numbers in the same order: every tie is exact, on the device as in
    the restatement, and the path is the tie rule's alone"""
    t, c, s = shape
    x = np.zeros((t, c), np.float32)
    for seed in range(3):
        label = M.make_label(seed, t, c, s)
        r64 = M.align(x, t, label)
        assert r64["gap"] == 0
        got = row(run(x[None], [t], [label]), 0)
        assert np.array_equal(got["states"], r64["states"]) and np.array_equal(got["spans"], r64["spans"])
        assert abs(float(got["score"]) - float(r64["score"])) <= FLOOR * abs(float(r64["score"]))


@pytest.mark.parametrize("t,c", [(1, 3), (7, 3), (30, 6), (30, 8)])
def test_greedy_identity(t, c):
    """aligning the collapsed argmax labelling returns the argmax path, score = sum of the row maxima"""
    for seed in range(4):
        x = M.make_logits(seed, t, c)
        lp = M.log_softmax(x)
        path = lp.argmax(axis=1)
        label = list(M.collapse(path, c - 1))
        j = judge(x, t, label)
        got = row(run(x[None], [t], [label]), 0)
        check(x, t, label, got, j)
        assert abs(float(got["score"]) - lp.max(axis=1).sum()) <= j["bound"]
        if j["decided"]:
            assert np.array_equal(got["states"], M.path_states(path, c - 1))


def _mixed():
    """48 utterances of T = 40, C = 6 with every kind of slot: full, short, empty, one frame, labels of 0..4 entries, one without a path"""
    rng = np.random.default_rng(5)
    xs = np.stack([M.make_logits(100 + i, 40, 6) for i in range(48)])
    seq = [int(v) for v in rng.integers(0, 41, 48)]
    labels = [M.make_label(i, 40, 6, int(rng.integers(0, 5))) for i in range(48)]
    seq[0], seq[1], seq[2], seq[3] = 40, 0, 1, 40
    labels[2], seq[4], labels[4] = [3], 2, [1, 1]                               # one frame, one label; two frames cannot hold a repeat
    return xs, seq, labels


def test_one_launch_of_48_equals_the_utterances_alone():
    xs, seq, labels = _mixed()
    got = run(xs, seq, labels, s_max=4)
    assert same_bits(got, run(xs, seq, labels, s_max=4))                        # a rerun: the same bits
    for i in range(48):
        alone = run(xs[i:i + 1], seq[i:i + 1], labels[i:i + 1], s_max=4)
        assert same_bits(row(alone, 0), row(got, i)), i
        check(xs[i], seq[i], labels[i], row(got, i), judge(xs[i], seq[i], labels[i]))


def test_nan_beyond_seq_len_changes_nothing():
    xs, seq, labels = _mixed()
    dirty = xs.copy()
    for i, n in enumerate(seq):
        dirty[i, n:] = np.nan
    assert same_bits(run(dirty, seq, labels, s_max=4), run(xs, seq, labels, s_max=4))


def test_empty_slots_and_utterances_without_a_path():
    xs, seq, labels = _mixed()
    got = run(xs, seq, labels, s_max=4)
    e = row(got, 1)                                                             # seq_len 0
    assert e["score"] == 0 and e["loss"] == 0 and (e["states"] == -1).all() and (e["spans"] == -1).all() and not e["post"].any()
    n = row(got, 4)                                                             # [1, 1] in two frames
    assert n["score"] == -np.inf and n["loss"] == np.inf and (n["states"] == -1).all() and (n["spans"] == -1).all() and not n["post"].any()
    one = row(got, 2)                                                           # one frame, one label: the path is state 1
    assert one["states"][0] == 1 and (one["states"][1:] == -1).all() and one["spans"][0].tolist() == [0, 0] and (one["spans"][1:] == -1).all()
    assert one["post"][0, 0] == 1 and one["score"] == -one["loss"]
    none = run(xs[:3], [40, 40, 40], [[], [], []], s_max=0)                     # no labels at all: S_max = 0, labels NULL
    assert not none["states"].any() and none["spans"].shape == (3, 0, 2) and same_bits({"a": none["score"]}, {"a": -none["loss"]})


def test_null_optional_outputs():
    xs, seq, labels = _mixed()
    full = run(xs, seq, labels, s_max=4)
    for want in ((), ("states",), ("spans",), ("loss",), ("post",), ("states", "spans"), ("spans", "post")):
        part = run(xs, seq, labels, want=want, s_max=4)
        assert sorted(part) == sorted(want + ("score",))
        assert same_bits(part, {k: full[k] for k in part}), want


def test_non_default_stream_and_the_python_entry_point():
    from keyword_spotting_amd.custom_keyword import ctc_align, frame_labels
    xs, seq, labels = _mixed()
    full = run(xs, seq, labels, s_max=4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert same_bits(run(xs, seq, labels, s_max=4, stream=side), full)
    al = ctc_align(torch.from_numpy(xs), seq, labels, want_post=True)
    torch.cuda.synchronize()
    assert same_bits({k: getattr(al, k).cpu().numpy() for k in full}, full)
    assert ctc_align(xs, seq, labels).post is None
    classes = frame_labels(al.states, labels, 5)
    for i in range(48):
        assert np.array_equal(classes[i], M.frame_classes(full["states"][i], labels[i], 5))
        if full["score"][i] > -np.inf and seq[i]:
            assert M.collapse(classes[i][:seq[i]], 5) == tuple(labels[i])       # the frame-wise targets spell the transcript


def test_enroller_align_finds_the_enrolled_words():
    """the toy task of tests/test_gpu_enroll.py: a short fit of two new words on three utterances, then where the new head finds them"""
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.custom_keyword import Enroller
    from keyword_spotting_amd.prediction import ctc_label
    from keyword_spotting_amd.rnn_ctc import DeployModel
    from oracle import gru_oracle as G
    cfg = get_config()
    model = DeployModel(cfg, weights.init_weights(cfg, seed=0))
    mel = torch.from_numpy(G.synthetic_mel(3, 48, cfg.n_mel, seed=10))
    lengths, label = [48, 40, 33], [int(v) for v in ctc_label([5, 6])]
    enroller = Enroller(model, 2, enrolments=1, utterances_per_enrolment=3)
    try:
        wn, bn, trace = enroller.fit(mel, lengths, label, steps=60, lr=0.03)
        al = enroller.align(mel, lengths, label, wn, bn)
        # the loss of the assembled logits is the loss the next fit step reports; the two projections sum H = 128 products in different
        # orders (<= H 2^-24 |nn| |w| ~ 1e-5 per logit, a loss moves by at most one per logit and frame: 48 x 1e-5), so 1e-3 relative
        _, _, again = enroller.fit(mel, lengths, label, steps=1, lr=0.03, init=(wn, bn))
        torch.cuda.synchronize()
    finally:
        enroller.close()
        model.close()
    states, spans, post = al.states.cpu().numpy(), al.spans.cpu().numpy(), al.post.cpu().numpy()
    loss, next_loss = al.loss.cpu().numpy(), again[0].cpu().numpy()
    assert np.abs(loss - next_loss).max() <= 1e-3 * max(1.0, float(np.abs(next_loss).max())), (loss, next_loss)
    assert tuple(states.shape) == (3, 48) and tuple(spans.shape) == (3, 5, 2) and tuple(post.shape) == (3, 48, 5)
    for i, n in enumerate(lengths):
        assert (spans[i, :, 0] >= 0).all() and (spans[i, :, 1] < n).all()                      # within the recording
        assert (spans[i, :, 0] <= spans[i, :, 1]).all() and (spans[i, 1:, 0] > spans[i, :-1, 1]).all()
        assert np.array_equal(spans[i], M.spans_of(states[i], 5)) and (states[i, n:] == -1).all()
        assert post[i].min() >= 0 and post[i].max() <= 1 and not post[i, n:].any()
        for k in (1, 3):                                                                       # the two new words, classes 5 and 6
            print("ALIGN-ENROLL utterance %d word %d: span %d..%d, peak posterior %.3f at frame %d"
                  % (i, label[k], spans[i, k, 0], spans[i, k, 1], post[i, :, k].max(), post[i, :, k].argmax()))
