"""CPU checks of the training of the stack: the fp64 restatement tests/train_model.py against torch's autograd in float64 and central
finite differences, TensorFlow's Adam / Nesterov / global-norm clip / exponential decay by hand, every refusal the train entry points
raise before they touch a device, and the conditions the GPU tests lean on (established here, on the references alone)."""
import ctypes

import numpy as np
import pytest

import train_model as M
from conftest import have_gpu


def _scale(a):
    return max(float(np.abs(a).max()), 1e-300)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_restatement_matches_torch_fp64(name):
    import torch
    p = M.make_problem(name)
    drop = M.drop_masks(p, 0.6) if name in ("odd_mel", "t2") else None
    loss, grads, logits = M.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], drop, 0.6)
    want = M.torch_reference(p["w"], p["x"], p["seq_len"], p["labels"], torch.float64, drop, 0.6)
    finite = np.isfinite(loss)
    assert np.abs(logits - want["logits"]).max() <= 1e-10 * _scale(want["logits"])
    assert np.abs(np.where(finite, loss, 0.0) - want["loss"]).max() <= 1e-10 * _scale(want["loss"])
    for (key, got), (_, ref) in zip(M.flat(grads), M.flat(want["grads"])):
        assert np.abs(got - ref).max() <= 1e-10 * _scale(ref), key
    assert (loss[p["seq_len"] == 0] == 0).all()
    if name == "no_path":
        assert list(finite) == [True, False, True] and loss[1] == np.inf
        # ... whose contribution is exactly 0: the batch without it (its slot emptied, B unchanged) has the same gradient
        seq = p["seq_len"].copy()
        seq[1] = 0
        _, without, _ = M.loss_and_grad(p["w"], p["x"], seq, p["labels"])
        for (key, got), (_, ref) in zip(M.flat(grads), M.flat(without)):
            assert np.array_equal(got, ref), key
    else:
        assert finite.all()


def _cut_down(name, b, t):
    """The first b utterances and t frames of a case, labels cut to one: its model at a size finite differences can afford."""
    p = dict(M.make_problem(name))
    p.update(x=p["x"][:b, :t], seq_len=np.minimum(p["seq_len"][:b], t), labels=[s[:1] for s in p["labels"][:b]], B=b, T=t)
    assert (p["seq_len"] > 0).all()
    return p


@pytest.mark.parametrize("name", ["t2", "odd_mel", "h256"])
def test_restatement_matches_central_finite_differences(name):
    p = _cut_down(name, 2, 4) if name == "h256" else M.make_problem(name)          # the yardstick itself at hidden 256: B 2, T 4
    w = M.as_dtype(p["w"], np.float64)
    _, grads, _ = M.loss_and_grad(w, p["x"], p["seq_len"], p["labels"])

    def total(wd):
        return M.loss_and_grad(wd, p["x"], p["seq_len"], p["labels"])[0].sum() / p["B"]
    rng = np.random.default_rng(3)
    eps = 1e-6
    probes = [("Wfc", None), ("bfc", None)] + [(k, l) for l in range(len(w["layers"])) for k in ("Wg", "bg", "Wc", "bc")]
    for key, l in probes:
        arr = w[key] if l is None else w["layers"][l][key]
        g = grads[key] if l is None else grads["layers"][l][key]
        for _ in range(2):
            idx = tuple(int(rng.integers(0, n)) for n in arr.shape)
            keep = arr[idx]
            arr[idx] = keep + eps
            up = total(w)
            arr[idx] = keep - eps
            down = total(w)
            arr[idx] = keep
            assert abs((up - down) / (2 * eps) - g[idx]) <= 1e-6 * max(1.0, _scale(g)), (key, l, idx)


def test_adam_and_nesterov_by_hand():
    """Two parameters (1, -2), lr 0.1, gradients (0.5, -1), (-0.25, 0.5), (0.125, 0.25), each step by the formulas of the header."""
    w = dict(layers=[], Wfc=np.array([[1.0, -2.0]]), bfc=np.zeros(2))
    gs = [np.array([[0.5, -1.0]]), np.array([[-0.25, 0.5]]), np.array([[0.125, 0.25]])]
    # Nesterov: a <- 0.9 a + g; theta <- theta - lr g - lr 0.9 a
    opt, cur = M.Optimizer(w, "nesterov"), w
    a, theta = np.zeros((1, 2)), w["Wfc"].copy()
    for g in gs:
        cur = opt.apply(cur, dict(layers=[], Wfc=g, bfc=np.zeros(2)), 0.1)
        a = 0.9 * a + g
        theta = theta - 0.1 * g - 0.1 * 0.9 * a
        assert np.abs(cur["Wfc"] - theta).max() < 1e-15
    # a: 0.5, 0.2, 0.305 -> theta0: 1 - 0.05 - 0.045 = 0.905; + 0.025 - 0.018 = 0.912; - 0.0125 - 0.02745 = 0.87205
    assert abs(cur["Wfc"][0, 0] - 0.87205) < 1e-12
    theta_one, a_one = M.nesterov_step(1.0, 0.0, 0.5, 0.1)
    assert abs(theta_one - 0.905) < 1e-15 and a_one == 0.5
    # Adam: enroll_model.adam_step is the hand-checked one (tests/test_enroll_host.py); three steps of the same thing
    opt, cur = M.Optimizer(w, "adam"), w
    theta, m, v = w["Wfc"].copy(), np.zeros((1, 2)), np.zeros((1, 2))
    for t, g in enumerate(gs, 1):
        cur = opt.apply(cur, dict(layers=[], Wfc=g, bfc=np.zeros(2)), 0.1)
        theta, m, v = M.E.adam_step(theta, m, v, g, t, 0.1)
        assert np.abs(cur["Wfc"] - theta).max() < 1e-15
    # t=3 from theta 0.8733663743517929 (t=1,2 as tests/test_enroll_host.py works them): m = 0.0305, v = 0.00032756275,
    # lr_t = 0.1 sqrt(1 - 0.999^3) / (1 - 0.9^3) = 0.0202010597 -> theta -= 0.0202010597 * 0.0305 / (0.0180987 + 1e-8)
    assert abs(cur["Wfc"][0, 0] - 0.8393234783404581) < 1e-12
    assert np.array_equal(cur["bfc"], np.zeros(2))          # a zero gradient moves nothing (0 / (0 + 1e-8))


def test_global_norm_clip_active_and_inactive():
    g = dict(layers=[dict(Wg=np.array([[3.0]]), bg=np.array([0.0]), Wc=np.array([[0.0]]), bc=np.array([4.0]))], Wfc=np.array([[12.0]]), bfc=np.array([0.0]))
    assert M.global_norm(g) == 13.0
    c = M.clip_by_global_norm(g, 6.5)                     # active: every tensor halves
    assert c["layers"][0]["Wg"][0, 0] == 1.5 and c["layers"][0]["bc"][0] == 2.0 and c["Wfc"][0, 0] == 6.0
    assert abs(M.global_norm(c) - 6.5) < 1e-15
    for clip in (13.0, 20.0):                             # inactive: clip / max(norm, clip) = 1 exactly
        c = M.clip_by_global_norm(g, clip)
        assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(M.flat(c), M.flat(g)))
    assert M.clip_by_global_norm(g, -1) is g              # max_grad_norm <= 0: no clipping (config/rnn_config.py:77)


def test_learning_rate_schedule():
    from keyword_spotting_amd.training import learning_rate_at
    assert learning_rate_at(0) == 1.5e-3
    assert abs(learning_rate_at(20000) - 1.2e-3) < 1e-18
    assert abs(learning_rate_at(10000) - 1.5e-3 * np.sqrt(0.8)) < 1e-18          # not a staircase
    assert abs(learning_rate_at(5, 0.1, 0.5, 10) - M.exponential_decay(0.1, 5, 10, 0.5)) < 1e-18
    assert abs(learning_rate_at(30, 0.1, 0.5, 10) - 0.0125) < 1e-18


# ---- refusals that need no device ------------------------------------------------------------------------------------------------

_KEEP = []


def _i32(*v):
    a = np.array(v, np.int32)
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def _cfg(n_mel=40, hidden=128, layers=2, classes=6, use_relu=0, value_clip=-1.0, precision=0, ln=0, res=0, var=0, opt=0, clip=-1.0, keep=1.0):
    from keyword_spotting_amd import _lib
    return _lib.KwsTrainConfig(_lib.KwsConfig(n_mel, hidden, layers, classes, use_relu, value_clip, precision), _lib.KwsCellWrappers(ln, res), var,
                               opt, clip, keep)


def test_create_refusals_name_the_field():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()

    def create(**kw):
        cfg = _cfg(**kw)
        rc = lib.kws_train_create(ctypes.byref(cfg), ctypes.byref(h))
        return rc, lib.kws_last_error()
    uns, bad = _lib.KWS_ERR_UNSUPPORTED, _lib.KWS_ERR_INVALID_ARGUMENT
    for kw, code, word in ((dict(use_relu=1), uns, b"use_relu"), (dict(value_clip=20.0), uns, b"value_clip"),
                           (dict(ln=1), uns, b"use_layer_norm"), (dict(res=1), uns, b"use_residual"),
                           (dict(var=1), uns, b"variational_recurrent"),
                           (dict(precision=_lib.BF16), uns, b"precision"), (dict(precision=_lib.INT8), uns, b"precision"),
                           (dict(precision=_lib.F16X3), uns, b"precision"),
                           (dict(keep=0.0), uns, b"keep_prob"), (dict(keep=1.5), uns, b"keep_prob"), (dict(keep=float("nan")), uns, b"keep_prob"),
                           (dict(opt=2), bad, b"optimizer"), (dict(hidden=100), bad, b"hidden=100"), (dict(layers=0), bad, b"num_layers"),
                           (dict(layers=9), bad, b"num_layers"), (dict(n_mel=0), bad, b"n_mel"), (dict(n_mel=1025), bad, b"n_mel"),
                           (dict(classes=2), bad, b"num_classes"), (dict(classes=9), bad, b"num_classes")):
        rc, msg = create(**kw)
        assert rc == code and word in msg and not h.value, (kw, rc, msg)
    assert lib.kws_train_create(None, ctypes.byref(h)) == bad
    assert lib.kws_train_create(ctypes.byref(_cfg()), None) == bad
    if not have_gpu():
        for kw in (dict(), dict(hidden=64, layers=1, n_mel=1, classes=3), dict(hidden=256, layers=8, n_mel=1024, classes=8, opt=1, clip=5.0, keep=0.6)):
            assert create(**kw)[0] == _lib.KWS_ERR_NO_DEVICE, kw
    assert lib.kws_sizeof_train_config() == ctypes.sizeof(_lib.KwsTrainConfig)


def test_call_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    x = ctypes.c_void_p(256)            # a non-null, aligned address that is never read
    sl, ll, lab = _i32(4, 4), _i32(2, 1), _i32(1, 4, 0, 0)
    cfg = _cfg()

    def check(cfg=cfg, x=x, seq=sl, labels=lab, lens=ll, b=2, t=4, s_max=2, loss=x):
        rc = lib.kws_train_check(ctypes.byref(cfg), x, seq, labels, lens, b, t, s_max, loss)
        return rc, lib.kws_last_error()
    bad, uns = _lib.KWS_ERR_INVALID_ARGUMENT, _lib.KWS_ERR_UNSUPPORTED
    assert check()[0] == _lib.KWS_OK
    assert check(cfg=_cfg(keep=0.0)) [0] == uns and b"keep_prob" in lib.kws_last_error()
    assert check(b=0)[0] == bad and b"B=0" in lib.kws_last_error()
    assert check(t=0)[0] == bad
    assert check(s_max=32)[0] == bad and b"S_max=32" in lib.kws_last_error()
    for kw in (dict(x=None), dict(seq=None), dict(labels=None), dict(lens=None), dict(loss=None)):
        assert check(**kw)[0] == bad and b"null pointer" in lib.kws_last_error(), kw
    assert check(x=ctypes.c_void_p(258))[0] == bad and b"aligned" in lib.kws_last_error()
    assert check(cfg=_cfg(classes=5))[0] == bad and b"labels[0][1]=4" in lib.kws_last_error()          # 4 is the blank of 5 classes
    assert check(labels=_i32(1, -1, 0, 0))[0] == bad
    assert check(seq=_i32(4, 5))[0] == bad and b"seq_len[1]=5" in lib.kws_last_error()
    assert check(lens=_i32(3, 1))[0] == bad and b"label_len[0]=3" in lib.kws_last_error()
    assert check(labels=_i32(9, 9, 0, 0), seq=_i32(0, 4))[0] == _lib.KWS_OK                              # an empty slot's label is ignored
    # the CTC kernel's LDS: 4 T (8 + 2 S_max + 1) bytes, 700 x 71 floats = 198800 > 163840
    rc, msg = check(b=1, t=700, s_max=31, seq=_i32(700), lens=_i32(0), labels=_i32(*([0] * 31)))
    assert rc == uns and b"198800 bytes exceed the 163840" in msg
    # the entry points themselves: a null handle is refused before anything else
    assert lib.kws_train_grad(None, x, sl, lab, ll, 2, 4, 2, None, x, x, None, None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_train_step(None, x, sl, lab, ll, 2, 4, 2, None, 0.01, x, None, None) == bad
    assert lib.kws_train_set_weights(None, x, 4, None) == bad and lib.kws_train_get_weights(None, x, 4, None) == bad
    assert lib.kws_train_moments(None, x, x, None) == bad and lib.kws_train_reserve(None, 1, 1, 1) == bad
    assert lib.kws_train_stats(None, None, None, None, None, None) == bad
    assert lib.kws_train_destroy(None) == _lib.KWS_OK


def test_trainer_refuses_unknown_optimizers_on_the_host():
    from keyword_spotting_amd import _lib, get_config
    from keyword_spotting_amd.training import train_config
    with pytest.raises(_lib.InvalidArgumentError, match="optimizer"):
        train_config(get_config(), optimizer="sgd")
    c = train_config(get_config(use_relu=True, precision="bf16"), "nesterov", 5.0, 0.6)
    assert (c.model.use_relu, c.model.precision, c.optimizer, c.max_grad_norm, round(c.keep_prob, 6)) == (1, _lib.BF16, _lib.OPT_NESTEROV, 5.0, 0.6)


# ---- conditions the GPU tests lean on ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["adam", "nesterov"])
@pytest.mark.parametrize("name", ["t2", "ref_shape", "c8_s_long", "h256"])
def test_float32_trajectory_stays_close_to_fp64(name, kind):
    """Twenty steps: float32 arithmetic alone stays within 1e-3 of the parameter scale, so a bound of 4 x its drift has teeth."""
    steps, lr = 20, M.TRAJECTORY_LR[kind]
    _, path64 = M.trajectory(name, kind, steps, lr)
    _, path32 = M.trajectory(name, kind, steps, lr, float32=True)
    start = M.blob_of(M.make_problem(name)["w"])
    moved = float(np.abs(path64[-1] - start).max())
    drift = max(float(np.abs(a - b).max()) for a, b in zip(path32, path64))
    assert drift <= 1e-3 * _scale(path64[-1]), (drift, _scale(path64[-1]))
    assert moved >= 100 * drift, (moved, drift)              # ... and the parameters really move


@pytest.mark.parametrize("hidden", [64, 128])
def test_toy_task_trains_on_the_restatement(hidden):
    from oracle import decode_oracle as D
    losses, _, logits = M.toy_trained(0, hidden)
    assert losses[-1] < 0.1 * losses[0] / 10, (losses[0], losses[-1])          # a margin of ten on the GPU test's 0.1
    sm = np.exp(M.E.log_softmax(logits))
    for i in range(M.TOY["B"]):
        assert D.ctc_predict(D.ctc_decode2(sm[i], M.TOY["C"]), M.TOY["label"]) == 1, i
