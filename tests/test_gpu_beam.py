"""CTC prefix beam search on the device: kws_ctc_beam_search against the fp64 restatement tests/beam_model.py on the SAME float32
arrays.  The yardstick is the deviation of the float32-CPU restatement from the fp64 one: bound = 4 x that deviation, floored at
16 * 2^-23 * max|reference| (the convention of tests/test_gpu_enroll.py).  A case is DECIDED when the float32-CPU run returns the fp64
paths and the fp64 selection gap is >= 8 x the bound: then the device must return exactly the restatement's paths, lengths and order
with scores within the bound.  Undecided cases (a near-tie somewhere along the way) still have to satisfy the invariants; their share
is capped at 4 of 12 per shape and 15 % overall."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_model as M

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -23
SHAPES = [(1, 3, 1, 1), (2, 3, 4, 4), (4, 3, 15, 15), (3, 4, 25, 25), (7, 6, 5, 1), (48, 3, 2, 2), (48, 4, 3, 3), (48, 6, 5, 5), (48, 8, 16, 16),
          (48, 8, 32, 4), (33, 4, 32, 32), (100, 6, 5, 1)]
SEEDS = range(12)


def run(x, seq_len=None, w=5, k=1, l_max=64, merge=False, stream=None):
    """x [B,T,C] float32 -> (paths [B,K,L], lengths [B,K], log_prob [B,K]) as numpy; seq_len: list, None (NULL)"""
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    xd = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    b, t, c = (int(v) for v in xd.shape)
    sl = None if seq_len is None else torch.tensor(list(seq_len), dtype=torch.int32).cuda()
    paths = torch.full((b, k, l_max), -7, dtype=torch.int32, device="cuda")
    lens = torch.full((b, k), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((b, k), 7.0, device="cuda")
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        _lib.check(lib.kws_ctc_beam_search(_lib.ptr(xd), _lib.ptr(sl), b, t, c, w, k, l_max, 1 if merge else 0, _lib.ptr(paths), _lib.ptr(lens),
                                           _lib.ptr(lp), ctypes.c_void_p(s.cuda_stream)))
    s.synchronize()
    return paths.cpu().numpy(), lens.cpu().numpy(), lp.cpu().numpy()


def judge(x, w, k, seq_len=None, l_max=64, merge=False):
    """the two CPU runs of one utterance -> (r64, bound, decided)"""
    r64 = M.beam_search(x, seq_len, w, k, l_max, merge)
    r32 = M.beam_search(x, seq_len, w, k, l_max, merge, dtype=np.float32)
    same = r32["raw"] == r64["raw"]
    fin = np.isfinite(r64["scores"])
    dev = float(np.abs(r32["scores"][fin].astype(np.float64) - r64["scores"][fin]).max()) if same and fin.any() else 0.0
    bound = max(4.0 * dev, FLOOR * float(np.abs(r64["scores"][fin]).max()) if fin.any() else 0.0)
    return r64, bound, bool(same and r64["gap"] >= 8.0 * bound)


@functools.lru_cache(maxsize=None)
def case(seed, shape):
    t, c, w, k = shape
    x = M.make_logits(seed, t, c, w)
    return (x,) + judge(x, w, k)


def check(x, got, r64, bound, decided, l_max=64, merge=False, seq_len=None):
    """one utterance's device result against the rules; -> |score error| / bound of a decided case (0 otherwise)"""
    paths, lens, lp = got
    k = len(lp)
    n = int(np.isfinite(lp).sum())
    assert np.isfinite(lp[:n]).all() and (lp[n:] == -np.inf).all() and (lens[n:] == 0).all()
    assert (np.diff(lp[:n]) <= 0).all()                                                 # descending
    rows = []
    for i in range(k):
        assert (paths[i, :lens[i]] >= 0).all() and (paths[i, lens[i]:] == -1).all()     # labels, then the -1 padding
        assert (paths[i, :lens[i]] < x.shape[1] - 1).all()
        rows.append(tuple(int(v) for v in paths[i, :lens[i]]))
    if not merge:
        assert len(set(rows[:n])) == n                                                  # distinct
        for i in range(n):                                                              # never above the labelling's exact log-probability
            assert lp[i] <= M.torch_log_prob(x, rows[i], seq_len) + bound, (i, rows[i])
    if not decided:
        return 0.0
    want, want_len = M.dense(r64["paths"], l_max)
    assert np.array_equal(paths, want) and np.array_equal(lens, want_len)
    assert np.array_equal(np.isfinite(lp), np.isfinite(r64["scores"]))
    fin = np.isfinite(lp)
    err = float(np.abs(lp[fin].astype(np.float64) - r64["scores"][fin]).max()) if fin.any() else 0.0
    assert err <= bound, (err, bound)
    return err / bound if bound > 0 else 0.0


def test_entry_point_exists():
    from keyword_spotting_amd import _lib
    assert hasattr(_lib.load(), "kws_ctc_beam_search")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-C%d-W%d-K%d" % s)
def test_against_the_restatement(shape):
    t, c, w, k = shape
    undecided, worst = 0, 0.0
    for seed in SEEDS:
        x, r64, bound, decided = case(seed, shape)
        paths, lens, lp = run(x[None], [t], w, k)
        worst = max(worst, check(x, (paths[0], lens[0], lp[0]), r64, bound, decided))
        undecided += not decided
    print("BEAM-RATIO T=%d C=%d W=%d K=%d: worst score error / bound %.3f over %d decided cases, %d undecided" %
          (t, c, w, k, worst, len(SEEDS) - undecided, undecided))
    assert undecided <= 4


def test_undecided_share_overall():
    undecided = sum(not case(seed, shape)[3] for shape in SHAPES for seed in SEEDS)
    print("BEAM-UNDECIDED %d of %d" % (undecided, len(SHAPES) * len(SEEDS)))
    assert undecided <= 0.15 * len(SHAPES) * len(SEEDS)


@pytest.mark.parametrize("seed", M.REJOIN_SEEDS)
def test_a_returning_prefix_merges_with_its_surviving_child(seed):
    """flat inputs on which a prefix comes back as an extension of its parent while its own extension stays: identity by content"""
    x = M.make_logits(seed, 24, 3, 3, peak=1.0)
    r64, bound, decided = judge(x, 3, 3)
    assert r64["rejoined"] > 0
    paths, lens, lp = run(x[None], [24], 3, 3)
    check(x, (paths[0], lens[0], lp[0]), r64, bound, decided)


@pytest.mark.parametrize("shape", [(4, 3, 15, 15), (3, 4, 25, 25)], ids=lambda s: "T%d-C%d" % s[:2])
def test_unpruned_top_path_is_the_ctc_loss_kernels(shape):
    """rank 0's log_prob = -kws_ctc_loss of that labelling, within the sum of the two kernels' bounds"""
    from keyword_spotting_amd.custom_keyword import ctc_loss
    t, c, w, k = shape
    for seed in range(4):
        x, r64, bound, _ = case(seed, shape)
        paths, lens, lp = run(x[None], [t], w, k)
        label = [int(v) for v in paths[0, 0, :lens[0, 0]]]
        xt = torch.from_numpy(x)
        tgt = torch.tensor([label], dtype=torch.long).reshape(1, len(label))
        ref = [float(torch.nn.functional.ctc_loss(torch.log_softmax(xt.to(d), -1).unsqueeze(1), tgt, torch.tensor([t]), torch.tensor([len(label)]),
                                                  blank=c - 1, reduction="none")[0]) for d in (torch.float64, torch.float32)]
        bound_loss = max(4.0 * abs(ref[1] - ref[0]), FLOOR * abs(ref[0]))
        loss, _ = ctc_loss(xt[None], [t], [label], want_grad=False)
        assert abs(float(lp[0, 0]) + float(loss[0].item())) <= bound + bound_loss


def test_batch_composition_and_reruns_leave_the_bits_alone():
    shape = (48, 6, 5, 5)
    xs = np.stack([case(seed, shape)[0] for seed in SEEDS])
    alone = [run(xs[i:i + 1], [48], 5, 5) for i in range(3)]
    for b in (5, 67):
        batch = np.stack([xs[i % 12] for i in range(b)])
        got = run(batch, [48] * b, 5, 5)
        again = run(batch, [48] * b, 5, 5)
        assert all(np.array_equal(a, g) for a, g in zip(got, again))
        for i in range(b):
            if i % 12 < 3:
                assert all(np.array_equal(a[0], g[i]) for a, g in zip(alone[i % 12], got))


def test_sequence_lengths():
    shape = (48, 6, 5, 5)
    t = 48
    xs = np.stack([case(seed, shape)[0] for seed in range(8)])
    seq = [0, 1, t - 1, t, t + 5, -3, 20, 33]
    clamped = [0, 1, t - 1, t, t, 0, 20, 33]
    dirty = xs.copy()
    for i, n in enumerate(clamped):
        dirty[i, n:] = np.nan                                   # what lies past seq_len is never read
    got = run(dirty, seq, 5, 5)
    for i, n in enumerate(clamped):
        r64, bound, decided = judge(xs[i], 5, 5, seq_len=n)
        check(xs[i], tuple(g[i] for g in got), r64, bound, decided, seq_len=n)
        alone = run(xs[i:i + 1, :max(n, 1)], [n], 5, 5)
        assert all(np.array_equal(a[0], g[i]) for a, g in zip(alone, got))          # ... nor do the neighbours' rows matter
    assert got[2][0, 0] == 0 and got[1][0, 0] == 0 and (got[0][0] == -1).all() and (got[2][0, 1:] == -np.inf).all()
    null = run(xs, None, 5, 5)
    full = run(xs, [t] * 8, 5, 5)
    assert all(np.array_equal(a, g) for a, g in zip(null, full))


def test_merge_repeated_l_max_and_missing_ranks():
    x = np.full((6, 3), -4.0, np.float32)
    for t, c in enumerate([0, 2, 0, 2, 1, 1]):
        x[t, c] = 4.0
    plain, merged = run(x[None], [6], 4, 2), run(x[None], [6], 4, 2, merge=True)
    assert plain[0][0, 0, :4].tolist() == [0, 0, 1, -1] and merged[0][0, 0, :3].tolist() == [0, 1, -1]
    assert plain[1][0, 0] == 3 and merged[1][0, 0] == 2 and np.array_equal(plain[2], merged[2])
    xs = case(3, (48, 6, 5, 5))[0]
    for l_max in (1, 3):                                        # 3 is shorter than the best path of this input
        assert len(M.beam_search(xs, None, 5, 5)["paths"][0]) > 3
        r64, bound, decided = judge(xs, 5, 5, l_max=l_max)
        got = run(xs[None], [48], 5, 5, l_max=l_max)
        assert got[0].shape == (1, 5, l_max) and got[1].max() <= l_max
        check(xs, tuple(g[0] for g in got), r64, bound, decided, l_max=l_max)
    one = M.make_logits(0, 1, 3, 4)                             # one frame, two labels: three prefixes exist, rank 3 does not
    paths, lens, lp = run(one[None], [1], 4, 4)
    assert np.isfinite(lp[0, :3]).all() and lp[0, 3] == -np.inf and lens[0, 3] == 0 and (paths[0, 3] == -1).all()
    assert sorted(lens[0, :3].tolist()) == [0, 1, 1]


def test_non_default_stream():
    x = case(0, (48, 8, 16, 16))[0]
    want = run(x[None], [48], 16, 16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = run(x[None], [48], 16, 16, stream=side)
    assert all(np.array_equal(a, g) for a, g in zip(want, got))


def test_through_the_model_and_the_python_entry_points():
    """DeployModel.forward's logits at the reference shape, decoded by ctc_beam_search_decode, against the restatement on the same logits;
    the top path through decode_best into ctc_predict, evaluate and WERCalculator"""
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd import prediction as P
    from keyword_spotting_amd.rnn_ctc import DeployModel
    from keyword_spotting_amd.wer import WERCalculator
    from oracle import gru_oracle as G
    cfg = get_config()
    model = DeployModel(cfg, weights.init_weights(cfg, seed=0))
    mel = G.synthetic_mel(16, 48, cfg.n_mel, seed=3)
    logits = model.forward(torch.from_numpy(mel), model.zero_state(16))["logits"]
    model.close()
    dense, log_probs = P.ctc_beam_search_decode(logits, top_paths=3, merge_repeated=False)
    assert tuple(dense.shape) == (16, 3, 64) and tuple(log_probs.shape) == (16, 3) and dense.dtype == torch.int32
    host = logits.cpu().numpy()
    c = cfg.num_classes
    for i in range(16):
        r64, bound, decided = judge(host[i], c - 1, 3)                                  # beam_width None: config.beam_size
        d = dense[i].cpu().numpy()
        check(host[i], (d, (d >= 0).sum(1).astype(np.int32), log_probs[i].cpu().numpy()), r64, bound, decided)
    one, one_lp = P.ctc_beam_search_decode(logits[2], top_paths=2)
    assert tuple(one.shape) == (2, 64) and tuple(one_lp.shape) == (2,)
    assert torch.equal(one_lp, P.ctc_beam_search_decode(logits, top_paths=2)[1][2])
    # peaked rows that spell 1 2 3 3 with the space class between the words: the top path, the keyword decision, the WER
    spell = [5, 0, 1, 1, 5, 0, 2, 0, 5, 3, 5, 0, 5, 3, 3, 0, 5, 5]
    x = np.full((2, len(spell), c), -5.0, np.float32)
    x[0, np.arange(len(spell)), spell] = 5.0
    x[1, :, 5] = 5.0
    best = P.decode_best(x)
    assert best[0].tolist() == P.ctc_label([1, 2, 3, 3]).tolist() and best[1].tolist() == [0]
    assert P.decode_best(x[0]).tolist() == best[0].tolist()
    row = P.ctc_beam_search_decode(x[0])[0][0]
    assert P.ctc_predict(row.cpu().numpy(), "1233") == 1 and P.ctc_predict(best[0], "1233") == 1 and P.ctc_predict(best[1], "1233") == 0
    assert P.evaluate([P.ctc_predict(b, "1233") for b in best], [1, 0]) == (0, 1, 0)
    assert WERCalculator([0, -1]).cal_batch_wer([P.ctc_label([1, 2, 3, 3]), P.ctc_label([1, 2])], best).tolist() == [0.0, 1.0]
