"""CPU checks of the training of the wrapped stack (layer norm, residual, variational dropout): the fp64 restatement
tests/train_wrapped_model.py against torch's autograd in float64, central finite differences and the serving restatement
tests/wrapped_cell_model.py; every refusal kws_train_create_wrapped raises before it touches a device; and the condition the GPU
test of the toy task leans on."""
import ctypes

import numpy as np
import pytest

import train_model as M
import train_wrapped_model as TW
import wrapped_cell_model as W
from conftest import have_gpu


def _scale(a):
    return max(float(np.abs(a).max()), 1e-300)


def _run(p, **kw):
    return TW.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], p["ln"], p["res"], **kw)


@pytest.mark.parametrize("name", sorted(TW.CASES))
def test_restatement_matches_torch_fp64(name):
    import torch
    p = TW.make_problem(name)
    drop = TW.drop_masks(p, 0.6) if name in ("ln_odd_mel", "res_l2", "both_l8") else None
    loss, grads, logits = _run(p, drop=drop, keep_prob=0.6)
    want = TW.torch_reference(p["w"], p["x"], p["seq_len"], p["labels"], torch.float64, p["ln"], p["res"], drop, 0.6)
    finite = np.isfinite(loss)
    assert np.abs(logits - want["logits"]).max() <= 1e-10 * _scale(want["logits"])
    assert np.abs(np.where(finite, loss, 0.0) - want["loss"]).max() <= 1e-10 * _scale(want["loss"])
    keys = [k for k, _ in TW.flat(grads)]
    assert ("l0_ibeta" in keys and "l%d_igamma" % (p["config"].num_layers - 1) in keys) == p["ln"]
    for (key, got), (_, ref) in zip(TW.flat(grads), TW.flat(want["grads"])):
        assert np.shape(got) == np.shape(ref) and np.abs(got - ref).max() <= 1e-10 * _scale(ref), key
    assert (loss[p["seq_len"] == 0] == 0).all()
    if name == "both_no_path":          # ... whose contribution is exactly 0: the batch with its slot emptied has the same gradient
        assert list(finite) == [True, False, True] and loss[1] == np.inf
        seq = p["seq_len"].copy()
        seq[1] = 0
        _, without, _ = TW.loss_and_grad(p["w"], p["x"], seq, p["labels"], p["ln"], p["res"])
        for (key, got), (_, ref) in zip(TW.flat(grads), TW.flat(without)):
            assert np.array_equal(got, ref), key
    else:
        assert finite.all()
    if name == "ln_mel1":          # one feature: xn = 0 exactly, so the layer norm's scale has no gradient and its input none either
        assert grads["layers"][0]["ibeta"] == 0.0 and np.abs(grads["layers"][0]["igamma"]).max() > 0


@pytest.mark.parametrize("name", ["ln_odd_mel", "res_l2", "both_no_path"])
def test_restatement_matches_central_finite_differences(name):
    p = TW.make_problem(name)
    w = TW.as_dtype(p["w"], np.float64)
    _, grads, _ = _run(dict(p, w=w))

    def total(wd):
        loss = _run(dict(p, w=wd))[0]
        return loss[np.isfinite(loss)].sum() / p["B"]
    rng = np.random.default_rng(3)
    eps = 1e-6
    flat_w, flat_g = dict(TW.flat(w)), dict(TW.flat(grads))
    for key, arr in flat_w.items():
        g = flat_g[key]
        for _ in range(2):
            idx = tuple(int(rng.integers(0, n)) for n in arr.shape)
            keep = arr[idx].copy()
            arr[idx] = keep + eps
            up = total(w)
            arr[idx] = keep - eps
            down = total(w)
            arr[idx] = keep
            assert abs((up - down) / (2 * eps) - g[idx]) <= 1e-6 * max(1.0, _scale(g)), (key, idx)


@pytest.mark.parametrize("name", sorted(set(TW.CASES) - {"ln_rows_chunk512"}))
def test_forward_is_the_serving_restatement(name):
    """At full length, without dropout: the logits of wrapped_cell_model.wrapped_forward, to 1e-12."""
    p = TW.make_problem(name)
    got = TW.forward(p["w"], p["x"], np.full(p["B"], p["T"]), p["ln"], p["res"])[0]
    want = W.wrapped_forward(TW.as_dtype(p["w"], np.float64), p["x"], p["ln"], p["res"])[0]
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, _scale(want))


def test_one_layer_residual_and_switches_off_are_the_plain_restatement_exactly():
    p = TW.make_problem("res_l1")
    assert p["res"] and not p["ln"] and p["config"].num_layers == 1
    drop = TW.drop_masks(p, 0.6)
    for kw in (dict(), dict(drop=drop, keep_prob=0.6)):
        want = M.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], **kw)
        for ln_res in ((False, True), (False, False)):
            got = TW.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], *ln_res, **kw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
            for (key, a), (_, b) in zip(TW.flat(got[1]), M.flat(want[1])):
                assert np.array_equal(a, b), key
    # ... and on two layers with the switches off
    q = M.make_problem("odd_mel")
    want = M.loss_and_grad(q["w"], q["x"], q["seq_len"], q["labels"])
    got = TW.loss_and_grad(q["w"], q["x"], q["seq_len"], q["labels"])
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(TW.flat(got[1]), M.flat(want[1])))


def test_variational_mask_is_the_mask_broadcast_over_the_frames():
    import torch
    p = TW.make_problem("both_l8")
    var = TW.drop_masks(p, 0.6, variational=True)
    assert var.shape == (8, p["B"], 64) and 0.3 < var.mean() < 0.9
    wide = np.ascontiguousarray(np.broadcast_to(var[:, :, None, :], (8, p["B"], p["T"], 64)))
    a, b = _run(p, drop=var, keep_prob=0.6), _run(p, drop=wide, keep_prob=0.6)
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(u, v) for (_, u), (_, v) in zip(TW.flat(a[1]), TW.flat(b[1])))
    plain = _run(p)
    assert not np.array_equal(a[0], plain[0])
    ref = TW.torch_reference(p["w"], p["x"], p["seq_len"], p["labels"], torch.float64, p["ln"], p["res"], var, 0.6)
    for (key, got), (_, want) in zip(TW.flat(a[1]), TW.flat(ref["grads"])):
        assert np.abs(got - want).max() <= 1e-10 * _scale(want), key


def test_optimizer_over_the_extended_set_is_train_models_on_the_plain_tensors():
    """Adam and Nesterov with an active clip: the plain tensors take train_model.Optimizer's numbers when the layer norm's
    gradients are zero (they then add nothing to the norm), and ibeta / igamma take the same update rule."""
    p = TW.make_problem("ln_odd_mel")
    _, grads, _ = _run(p)
    plain_w = dict(layers=[{k: lay[k] for k in TW.LAYER_KEYS} for lay in p["w"]["layers"]], Wfc=p["w"]["Wfc"], bfc=p["w"]["bfc"])
    plain_g = dict(layers=[{k: lay[k] for k in TW.LAYER_KEYS} for lay in grads["layers"]], Wfc=grads["Wfc"], bfc=grads["bfc"])
    zeroed = TW.unflat(grads, [g if "_i" not in k else np.zeros_like(g) for k, g in TW.flat(grads)])
    assert TW.global_norm(grads) > TW.global_norm(zeroed) == M.global_norm(plain_g)
    for kind in ("adam", "nesterov"):
        clip = 0.5 * M.global_norm(plain_g)
        want = M.Optimizer(plain_w, kind).apply(plain_w, plain_g, 0.01, clip)
        got = TW.Optimizer(p["w"], kind).apply(p["w"], zeroed, 0.01, clip)
        for (key, a), (_, b) in zip(M.flat(got), M.flat(want)):
            assert np.array_equal(a, b), (kind, key)
        full = TW.Optimizer(p["w"], kind).apply(p["w"], grads, 0.01, clip)
        s = clip / TW.global_norm(grads)
        g, theta = grads["layers"][1]["igamma"] * s, np.asarray(p["w"]["layers"][1]["igamma"], np.float64)
        # the first step of either rule from zero slots: Adam's m = 0.1 g, v = 0.001 g^2, lr_1 = lr sqrt(0.001) / 0.1; Nesterov's a = g
        lr_1 = 0.01 * np.sqrt(1.0 - 0.999) / (1.0 - 0.9)
        step = lr_1 * 0.1 * g / (np.sqrt(0.001 * g * g) + 1e-8) if kind == "adam" else 0.01 * g + 0.01 * 0.9 * g
        assert np.abs(full["layers"][1]["igamma"] - (theta - step)).max() <= 1e-12


# ---- the C entry points, no device ---------------------------------------------------------------------------------------------------

_KEEP = []


def _i32(*v):
    a = np.array(v, np.int32)
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def _cfg(n_mel=40, hidden=128, layers=2, classes=6, use_relu=0, value_clip=-1.0, precision=0, ln=0, res=0, var=0, opt=0, clip=-1.0, keep=1.0):
    from keyword_spotting_amd import _lib
    return _lib.KwsTrainConfig(_lib.KwsConfig(n_mel, hidden, layers, classes, use_relu, value_clip, precision), _lib.KwsCellWrappers(ln, res), var,
                               opt, clip, keep)


SWITCHES = [dict(ln=a, res=b, var=c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


def test_new_entry_points_exist():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_train_create_wrapped", "kws_train_check_wrapped"):
        assert hasattr(lib, sym), sym


def test_wrapped_create_takes_every_switch_combination_and_keeps_the_other_refusals():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()

    def create(**kw):
        cfg = _cfg(**kw)
        rc = lib.kws_train_create_wrapped(ctypes.byref(cfg), ctypes.byref(h))
        return rc, lib.kws_last_error()
    uns, bad = _lib.KWS_ERR_UNSUPPORTED, _lib.KWS_ERR_INVALID_ARGUMENT
    for sw in SWITCHES:
        for kw, code, word in ((dict(use_relu=1), uns, b"use_relu"), (dict(value_clip=20.0), uns, b"value_clip"),
                               (dict(precision=_lib.BF16), uns, b"precision"), (dict(precision=_lib.INT8), uns, b"precision"),
                               (dict(precision=_lib.F16X3), uns, b"precision"),
                               (dict(keep=0.0), uns, b"keep_prob"), (dict(keep=1.5), uns, b"keep_prob"), (dict(keep=float("nan")), uns, b"keep_prob"),
                               (dict(opt=2), bad, b"optimizer"), (dict(clip=float("inf")), bad, b"max_grad_norm"), (dict(hidden=100), bad, b"hidden=100"),
                               (dict(layers=0), bad, b"num_layers"), (dict(layers=9), bad, b"num_layers"), (dict(n_mel=0), bad, b"n_mel"),
                               (dict(n_mel=1025), bad, b"n_mel"), (dict(classes=2), bad, b"num_classes"), (dict(classes=9), bad, b"num_classes")):
            rc, msg = create(**dict(sw, **kw))
            assert rc == code and word in msg and not h.value, (sw, kw, rc, msg)
    for kw, word in ((dict(ln=2), b"wrappers.use_layer_norm=2"), (dict(ln=-1), b"wrappers.use_layer_norm=-1"), (dict(res=2), b"wrappers.use_residual=2"),
                     (dict(res=1, var=3), b"variational_recurrent=3"), (dict(var=-1), b"variational_recurrent=-1")):
        rc, msg = create(**kw)
        assert rc == bad and word in msg and not h.value, (kw, rc, msg)
    assert lib.kws_train_create_wrapped(None, ctypes.byref(h)) == bad
    assert lib.kws_train_create_wrapped(ctypes.byref(_cfg(ln=1)), None) == bad
    if not have_gpu():          # every valid combination goes on to the device
        for sw in SWITCHES:
            for shape in (dict(), dict(hidden=64, layers=1, n_mel=1, classes=3), dict(hidden=256, layers=8, n_mel=1024, classes=8, opt=1, clip=5.0, keep=0.6)):
                assert create(**dict(sw, **shape))[0] == _lib.KWS_ERR_NO_DEVICE, (sw, shape)


def test_plain_create_still_refuses_the_switches_and_points_to_the_wrapped_entry():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    for kw, word in ((dict(ln=1), b"use_layer_norm"), (dict(res=1), b"use_residual"), (dict(var=1), b"variational_recurrent")):
        cfg = _cfg(**kw)
        assert lib.kws_train_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.KWS_ERR_UNSUPPORTED
        msg = lib.kws_last_error()
        assert word in msg and b"kws_train_create_wrapped" in msg and not h.value, msg


def test_wrapped_check_is_ok_on_a_valid_call_and_refuses_as_the_plain_one():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    x = ctypes.c_void_p(256)            # a non-null, aligned address that is never read
    sl, ll, lab = _i32(4, 4), _i32(2, 1), _i32(1, 4, 0, 0)

    def check(cfg, b=2, s_max=2, x=x):
        rc = lib.kws_train_check_wrapped(ctypes.byref(cfg), x, sl, lab, ll, b, 4, s_max, x)
        return rc, lib.kws_last_error()
    for sw in SWITCHES:
        assert check(_cfg(**sw))[0] == _lib.KWS_OK, sw
    bad, uns = _lib.KWS_ERR_INVALID_ARGUMENT, _lib.KWS_ERR_UNSUPPORTED
    rc, msg = check(_cfg(ln=1, res=1, var=1, keep=0.0))
    assert rc == uns and b"keep_prob" in msg
    rc, msg = check(_cfg(ln=1, var=2))
    assert rc == bad and b"variational_recurrent=2" in msg
    rc, msg = check(_cfg(ln=1), b=0)
    assert rc == bad and b"B=0" in msg
    rc, msg = check(_cfg(res=1), s_max=32)
    assert rc == bad and b"S_max=32" in msg
    rc, msg = check(_cfg(ln=1), x=ctypes.c_void_p(258))
    assert rc == bad and b"aligned" in msg
    assert lib.kws_train_check_wrapped(None, x, sl, lab, ll, 2, 4, 2, x) == bad
    # the plain check keeps refusing the switches
    assert lib.kws_train_check(ctypes.byref(_cfg(ln=1)), x, sl, lab, ll, 2, 4, 2, x) == uns


def test_train_config_reads_the_three_switches():
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.training import train_config
    c = train_config(get_config())
    assert (c.wrappers.use_layer_norm, c.wrappers.use_residual, c.variational_recurrent) == (0, 0, 0)
    cfg = TW.config_of(64, 2, 8, 4, ln=True, res=True, var=True)
    c = train_config(cfg, "nesterov", 5.0, 0.6)
    assert (c.wrappers.use_layer_norm, c.wrappers.use_residual, c.variational_recurrent) == (1, 1, 1)
    c = train_config(TW.config_of(64, 2, 8, 4, res=True))
    assert (c.wrappers.use_layer_norm, c.wrappers.use_residual, c.variational_recurrent) == (0, 1, 0)


# ---- the condition the GPU test of the toy task leans on -----------------------------------------------------------------------------

def test_toy_task_trains_on_the_restatement_with_all_three_switches():
    from oracle import decode_oracle as D
    assert TW.TOY["L"] == 2 and TW.TOY["keep_prob"] < 1
    losses, w, logits = TW.toy_trained(0)
    assert losses[-1] < 0.1 * losses[0] / 10, (losses[0], losses[-1])          # a margin of ten on the GPU test's 0.1
    # the layer norms' scales left TF's initial 0: layer 0's is the input's only way into the stack
    assert abs(float(w["layers"][0]["ibeta"])) > 0.1 and all(float(lay["ibeta"]) != 0 for lay in w["layers"])
    sm = np.exp(M.E.log_softmax(logits))
    for i in range(TW.TOY["B"]):
        assert D.ctc_predict(D.ctc_decode2(sm[i], TW.TOY["C"]), TW.TOY["label"]) == 1, i
