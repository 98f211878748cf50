"""Training of the self-attention CTC model, everything that needs no GPU: the restatement (tests/attention_train_model.py) against
torch autograd and finite differences, its forward against the serving contract, the dropout hash against the library's host entry,
the schedules, the optimisers, every refusal kws_attention_train_check decides from host memory, and the tie conditions the GPU tests
(tests/test_gpu_attention_train.py) lean on."""
import ctypes

import numpy as np
import pytest
import torch

import attention_model as A
import attention_train_model as M

GENERIC = [n for n, c in M.CASES.items() if c[4] == "generic"]
DECIDED = [n for n, c in M.CASES.items() if c[4] == "decided"]


@pytest.mark.parametrize("name,keep", [("c2", 1.0), ("c2", 0.6), ("head32", 0.9), ("c1", 1.0), ("c4", 0.9), ("tiles", 0.9)])
def test_restatement_is_torch_fp64_autograd(name, keep):
    p = M.make_problem(name)
    loss, grads, logits = M.loss_and_grad(p["config"], p["w"], p["x"], p["seq_len"], p["labels"], seed=11, keep_prob=keep)
    r = M.torch_reference(p["config"], p["w"], p["x"], p["seq_len"], p["labels"], torch.float64, seed=11, keep_prob=keep)
    fin = np.isfinite(loss)
    assert np.abs(loss[fin] - r["loss"][fin]).max() <= 1e-10
    assert (r["loss"][~fin] == 0).all()
    assert np.abs(logits - r["logits"]).max() <= 1e-10
    for (key, g), (_, t) in zip(M.flat(grads), M.flat(r["grads"])):
        assert np.abs(g - t).max() <= 1e-10, key


def test_finite_differences_on_a_tiny_case():
    cfg = M.config_of(n_mel=3, combine_frame=2, hidden_size=64, multi_head_num=4, feed_forward_inner_size=64, num_layers=1, num_classes=4)
    from keyword_spotting_amd import attention_weights
    w = M.as_dtype(attention_weights.init(cfg, seed=3), np.float64)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 5, 3))
    seq, labels = np.array([5, 3]), [[0, 1], [2]]

    def total(wv):
        return M.loss_and_grad(cfg, wv, x, seq, labels, seed=5, keep_prob=0.8)[0].sum() / 2

    _, grads, _ = M.loss_and_grad(cfg, w, x, seq, labels, seed=5, keep_prob=0.8)
    names = [k for k, _ in M.flat(w)]
    for key in names:
        arr = dict(M.flat(w))[key]
        g = dict(M.flat(grads))[key]
        for idx in [tuple(rng.integers(0, s) for s in arr.shape) for _ in range(3)]:
            keep = arr[idx]
            arr[idx] = keep + 1e-6
            up = total(w)
            arr[idx] = keep - 1e-6
            dn = total(w)
            arr[idx] = keep
            assert abs((up - dn) / 2e-6 - g[idx]) <= 1e-6 * max(1.0, abs(g[idx])), (key, idx)


@pytest.mark.parametrize("name", ["c1", "c2", "c3", "c4", "head32"])
def test_forward_at_keep_prob_one_is_the_serving_contract(name):
    p = M.make_problem(name)
    _, _, logits = M.loss_and_grad(p["config"], p["w"], p["x"], p["seq_len"], p["labels"])
    for b, n in enumerate(p["seq_len"]):
        if A.frames_out(int(n), p["config"].combine_frame) == 0:          # an empty slot: no rows
            assert (logits[b] == 0).all()
            continue
        want, _ = A.forward(p["config"], p["w"], p["x"][b, :n])
        np.testing.assert_allclose(logits[b, :want.shape[0]], want, rtol=0, atol=1e-12)
        assert (logits[b, want.shape[0]:] == 0).all()


def test_the_float32_restatement_is_float32_throughout():
    """The tie yardstick (_pre_deviation) is forward_utt on float32 weights: every tensor of its tape is float32, so its deviation
    from the fp64 run is that of float32 arithmetic from the first product to the logits."""
    p = M.make_problem("c2")
    w32 = M.as_dtype(p["w"], np.float32)
    logits, tape = M.forward_utt(p["config"], w32, np.asarray(p["x"][0, :int(p["seq_len"][0])], np.float32), 0, 3, 0.9)
    assert logits.dtype == np.float32 and tape["xs"].dtype == np.float32
    assert tape["top"].dtype == np.float32 and tape["pre_out"].dtype == np.float32
    for lay in tape["layers"]:
        for key, v in lay.items():
            for a in (v if isinstance(v, list) else [v]):
                assert a.dtype == np.float32, key
    _, tape64 = M.forward_utt(p["config"], M.as_dtype(p["w"], np.float64), np.asarray(p["x"][0, :int(p["seq_len"][0])], np.float64), 0, 3, 0.9)
    assert tape64["pre_out"].dtype == np.float64 and tape64["layers"][-1]["pre1"].dtype == np.float64


def test_the_bench_tools_eager_graph_is_the_restatements_torch_graph():
    """tools/bench_attention_train.py times torch eager on a batched form of torch_forward (full-length utterances, the block layer
    norm as a mean over dims (1, 2)): at keep_prob 1 and in float64 the two graphs give the same logits."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_attention_train", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                         "tools", "bench_attention_train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    for name, B, T in (("c2", 3, 12), ("c2", 2, 7), ("c1", 2, 9), ("c3", 2, 9)):          # c2: T mod c = 0 and T mod c = 1
        p = M.make_problem(name)
        cfg = p["config"]
        x = np.asarray(p["x"][:B, :T], np.float64)
        tw = M.torch_params(p["w"], torch.float64)
        want = torch.stack([M.torch_forward(cfg, tw, x[b], b, 0, 1.0, torch.float64) for b in range(B)])
        t1 = A.frames_out(T, cfg.combine_frame)
        got, rows = tool.eager_logits(cfg, tw, tw["layers"], torch.tensor(x), torch.tensor(A.pe_table(t1, cfg.hidden_size)), 0.0)
        assert rows == t1 and got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12, name


# ---- the dropout hash ----------------------------------------------------------------------------------------------------------------

def test_numpy_hash_is_the_librarys():
    from keyword_spotting_amd import attention_training as T
    rng = np.random.default_rng(1)
    total = 0
    for seed, keep, site, layer, b, head in [(0, 0.9, 0, 0, 0, 0), (2 ** 64 - 1, 0.6, 1, 7, 65535, 0), (123456789012345, 0.5, 2, 3, 17, 0),
                                             (7, 0.9, 0, 5, 300, 15), (2 ** 63 + 5, 0.25, 0, 1, 2, 7)]:
        rows, cols = rng.integers(0, 16384, 30000), rng.integers(0, 16384, 30000)
        got = T.drop_keep(seed, keep, site, layer, b, head, rows, cols)
        np.testing.assert_array_equal(got != 0, M.drop_keep(seed, keep, site, layer, b, head, rows, cols))
        total += rows.size
    assert total >= 10 ** 5
    assert T.drop_keep(5, 1.0, 0, 0, 0, 0, rows, cols).all() and M.drop_keep(5, 1.0, 0, 0, 0, 0, rows, cols).all()


@pytest.mark.parametrize("site", [0, 1, 2])
@pytest.mark.parametrize("keep", [0.9, 0.6])
def test_keep_fraction(site, keep):
    n = 1024
    m = M._mask(42, keep, site, 1, 3, 2 if site == 0 else 0, n, n)
    kp = float(np.float32(keep))
    sigma = np.sqrt(kp * (1 - kp) / m.size)
    assert m.size >= 10 ** 6 and abs(m.mean() - kp) <= 4 * sigma, (m.mean(), kp, sigma)


def test_masks_differ_between_sites_layers_utterances_heads_and_seeds():
    base = M._mask(1, 0.6, 0, 0, 0, 0, 64, 64)
    others = [M._mask(1, 0.6, 1, 0, 0, 0, 64, 64), M._mask(1, 0.6, 2, 0, 0, 0, 64, 64), M._mask(1, 0.6, 0, 1, 0, 0, 64, 64),
              M._mask(1, 0.6, 0, 0, 1, 0, 64, 64), M._mask(1, 0.6, 0, 0, 0, 1, 64, 64), M._mask(2, 0.6, 0, 0, 0, 0, 64, 64)]
    for i, o in enumerate(others):
        assert 0.3 < (o != base).mean() < 0.7, i          # independent masks at keep 0.6 differ on 48 % of the entries
    for i in range(len(others)):
        for j in range(i):
            assert (others[i] != others[j]).any()


# ---- schedules, optimisers -----------------------------------------------------------------------------------------------------------

def test_both_schedules_by_hand():
    from keyword_spotting_amd.attention_training import learning_rate_at
    assert learning_rate_at(0) == 1e-3
    assert abs(learning_rate_at(40000) - 9e-4) < 1e-18
    assert abs(learning_rate_at(10000) - 1e-3 * 0.9 ** 0.25) < 1e-18
    # warm-up: min(polynomial_decay(5e-3, step, 40000, 1.35e-3, 0.5), exponential_decay(1.5e-3, step, 40000, 0.9))
    assert learning_rate_at(0, warmup=True) == 1.5e-3                                     # min(5e-3, 1.5e-3)
    assert abs(learning_rate_at(30000, warmup=True) - 1.5e-3 * 0.9 ** 0.75) < 1e-18       # the polynomial is 3.175e-3 there
    poly = (5e-3 - 1.35e-3) * (1 - 39999 / 40000) ** 0.5 + 1.35e-3
    assert abs(learning_rate_at(39999, warmup=True) - min(poly, 1.5e-3 * 0.9 ** (39999 / 40000))) < 1e-18
    assert abs(learning_rate_at(80000, warmup=True) - min(1.35e-3, 1.5e-3 * 0.81)) < 1e-18  # clamped polynomial: its end value
    assert learning_rate_at(80000, warmup=True) == pytest.approx(1.215e-3)
    assert M.polynomial_decay(5e-3, 10000, 40000, 1.35e-3, 0.5) == pytest.approx(1.35e-3 + 3.65e-3 * np.sqrt(0.75))


def test_optimisers_and_clip_by_hand():
    w = dict(W_in=np.array([[1.0, 2.0]]), b_in=np.array([0.5, -0.5]), layers=[], W_out=np.array([[3.0], [4.0]]), b_out=np.array([0.0]))
    g = dict(W_in=np.array([[3.0, 0.0]]), b_in=np.array([0.0, 4.0]), layers=[], W_out=np.array([[0.0], [0.0]]), b_out=np.array([12.0]))
    assert M.global_norm(g) == 13.0
    o = M.Optimizer(w, "nesterov")
    w1 = o.apply(w, g, 0.1, max_grad_norm=6.5)          # g / 2; a = g / 2; theta - lr g/2 - lr 0.9 g/2
    np.testing.assert_allclose(w1["W_in"], [[1.0 - 0.1 * 1.5 * 1.9, 2.0]])
    np.testing.assert_allclose(w1["b_out"], [-0.1 * 6.0 * 1.9])
    w2 = M.Optimizer(w, "nesterov").apply(w, g, 0.1, max_grad_norm=20.0)      # inactive clip
    np.testing.assert_allclose(w2["b_in"], [0.5, -0.5 - 0.1 * 4.0 * 1.9])
    a = M.Optimizer(w, "adam")
    w3 = a.apply(w, g, 0.01)          # first Adam step: theta - lr sign(g) up to epsilon
    np.testing.assert_allclose(w3["W_in"], [[1.0 - 0.01, 2.0]], atol=1e-8)
    np.testing.assert_allclose(a.m[0], [[0.3, 0.0]])
    np.testing.assert_allclose(a.v[0], [[0.009, 0.0]])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def _check(cfg_kw=None, shape=(2, 8), lengths=None, labels=([0], [1]), **kw):
    from keyword_spotting_amd import attention_training as T
    T.check_call(M.config_of(**(cfg_kw or {})), shape, lengths, list(labels), **kw)


def test_every_refusal_comes_before_the_device():
    from keyword_spotting_amd import _lib
    _check()
    for cfg_kw, field in [(dict(hidden_size=96), "hidden"), (dict(multi_head_num=1), "num_heads"), (dict(feed_forward_inner_size=100), "ffn_inner"),
                          (dict(num_layers=9), "num_layers"), (dict(combine_frame=5), "combine_frame"), (dict(num_classes=9), "num_classes"),
                          (dict(n_mel=300, combine_frame=2), "n_mel*combine_frame")]:
        with pytest.raises(_lib.UnsupportedError, match=field.replace("*", r"\*")):
            _check(cfg_kw)
    with pytest.raises(_lib.UnsupportedError, match="keep_prob"):
        _check(keep_prob=0.0)
    with pytest.raises(_lib.UnsupportedError, match="keep_prob"):
        _check(keep_prob=1.5)
    with pytest.raises(_lib.InvalidArgumentError, match="max_grad_norm"):
        _check(max_grad_norm=float("inf"))
    with pytest.raises(_lib.InvalidArgumentError, match="optimizer"):
        _check(optimizer="sgd")
    with pytest.raises(_lib.UnsupportedError, match="max_frames"):
        _check(dict(max_frames=4), shape=(2, 8))
    with pytest.raises(_lib.InvalidArgumentError, match=r"seq_len\[1\]=9"):
        _check(lengths=[8, 9])
    with pytest.raises(_lib.InvalidArgumentError, match=r"labels\[0\]\[0\]=5"):
        _check(labels=([5], [1]))          # the blank (class 5 of 6) is no label
    with pytest.raises(_lib.InvalidArgumentError, match="S_max=32"):
        _check(labels=([0] * 32, [1]))
    with pytest.raises(_lib.UnsupportedError, match="LDS"):
        _check(dict(combine_frame=1, max_frames=8192), shape=(1, 8000), labels=([0] * 20,))
    lib = _lib.load()
    assert lib.kws_attention_train_check(None, None, None, None, None, 1, 1, 0, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    h = ctypes.c_void_p()
    assert lib.kws_attention_train_create(None, ctypes.byref(h)) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_train_grad(None, None, None, None, None, 1, 1, 0, 0, None, None, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_train_step(None, None, None, None, None, 1, 1, 0, 0, 0.1, None, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_attention_train_destroy(None) == _lib.KWS_OK
    assert lib.kws_attention_drop_keep(0, 0.5, 3, 0, 0, 0, None, None, 0, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert b"site=3" in lib.kws_last_error()


# ---- the tie conditions of the GPU tests ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GENERIC)
def test_generic_cases_keep_every_relu_unit_16_deviations_from_its_tie(name):
    """attention_weights.init unchanged; the seed is the first at which |pre| >= 16 x the float32 restatement's worst deviation."""
    p = M.make_problem(name)
    np.testing.assert_array_equal(M.flat(p["w"])[0][1], M.flat(M.raw_problem(name, p["seed"])["w"])[0][1])
    (ffn, out), (dev_ffn, dev_out) = p["margins"], p["deviation"]
    cfg = p["config"]
    units = sum(A.frames_out(int(n), cfg.combine_frame) for n in p["seq_len"]) * (cfg.feed_forward_inner_size * cfg.num_layers + cfg.num_classes)
    print("TIE %s: seed %d, %d relu units, min |pre| ffn %.3e (deviation %.3e) logits %.3e (deviation %.3e)" %
          (name, p["seed"], units, ffn, dev_ffn, out, dev_out))
    assert units <= 12000
    assert ffn >= 16 * dev_ffn and out >= 16 * dev_out


@pytest.mark.parametrize("keep", [0.9, 0.6])
def test_generic_dropout_case_keeps_its_tie_condition_under_the_masks(keep):
    seed, (ffn, out), (dev_ffn, dev_out) = M.drop_seed_for("c2", keep)
    print("TIE c2 keep %.1f: dropout seed %d, min |pre| ffn %.3e (deviation %.3e) logits %.3e (deviation %.3e)" % (keep, seed, ffn, dev_ffn, out, dev_out))
    assert ffn >= 16 * dev_ffn and out >= 16 * dev_out


@pytest.mark.parametrize("name", DECIDED)
def test_decided_cases_keep_every_relu_unit_half_a_unit_from_its_tie(name):
    p = M.make_problem(name)
    for seed, keep in ((0, 1.0), (3, 0.9), (3, 0.6)) if name in ("reference",) else ((0, 1.0),):
        _, _, _, tapes = M.loss_and_grad(p["config"], p["w"], p["x"], p["seq_len"], p["labels"], seed=seed, keep_prob=keep, want_tapes=True)
        ffn, out = M.relu_margins(p, tapes)
        print("TIE %s keep %.1f: min |pre| ffn %.3f logits %.3f" % (name, keep, ffn, out))
        assert ffn >= 0.5 and out >= 0.5


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_trajectory_case_stays_decided_along_all_twenty_steps(kind):
    _, _, margins = M.trajectory("traj", kind, 20, M.TRAJECTORY_LR[kind])
    assert len(margins) == 20
    for step, (ffn, out) in enumerate(margins):
        assert ffn >= 0.5 and out >= 0.5, (step, ffn, out)
