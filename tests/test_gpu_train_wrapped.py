"""Training of the wrapped stack on the device (kws_train_create_wrapped, training.Trainer with config.use_layer_norm / use_residual /
variational_recurrent) against the fp64 restatement tests/train_wrapped_model.py.  The yardstick is tests/test_gpu_train.py's: per
tensor, bound = max(4 x the deviation of the identical torch graph in float32 on the CPU, 16 * 2^-23 * max|reference|), every
comparison printing its TRAIN-RATIO line before it asserts.  What has to hold to the bit is compared as uint32.

Launches of one gradient call, L layers, n = layer norm, r = residual (0 / 1), whatever T and the variational switch:
    4 L + 6 + n (2 L + 1) + r (L - 1) (3 - n)          (a step: two more)"""
import numpy as np
import pytest
import torch

import train_model as M
import train_wrapped_model as TW
from test_gpu_train import FLOOR, _check_trajectory, _report

pytestmark = pytest.mark.gpu


def grad_launches(layers, ln, res):
    return 4 * layers + 6 + int(ln) * (2 * layers + 1) + int(res) * (layers - 1) * (3 - int(ln))


def _trainer(p, **kw):
    from keyword_spotting_amd.training import Trainer
    return Trainer(p["config"], p["w"], **kw)


def _check_grads(what, name, got, ref64, ref32):
    worst = []
    for (key, g), (_, r64), (_, r32) in zip(TW.flat(got), TW.flat(ref64), TW.flat(ref32)):
        assert np.shape(g) == np.shape(r64), key
        err, bound = _report(what + " " + key, name, g, r64, r32)
        if err > bound:
            worst.append((key, err, bound))
    assert not worst, worst


def _bits(t, x, seq_len, labels, drop=None):
    """One loss_and_grad -> [(name, array)]: the per-utterance losses, the logits and every gradient tensor."""
    _, g, loss, logits = t.loss_and_grad(x, seq_len, labels, drop=drop, want_logits=True)
    return [("loss", loss), ("logits", logits.cpu().numpy())] + [(k, np.asarray(v)) for k, v in TW.flat(g)]


def _assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for (key, u), (_, v) in zip(a, b):
        assert u.shape == v.shape and np.array_equal(u.view(np.uint32), v.view(np.uint32)), (what, key)


@pytest.mark.parametrize("name", sorted(TW.CASES))
def test_taped_forward_logits(name):
    """No dropout: logits against the restatement (1e-4, the wrapped serving bound of tests/test_gpu_wrapped.py), rows t >= seq_len are
    bfc bitwise, and at full length the logits of kws_step on a kws_create_wrapped handle of the same weights (2e-4: both sides' 1e-4)."""
    from keyword_spotting_amd.rnn_ctc import DeployModel
    p = TW.make_problem(name)
    t = _trainer(p)
    try:
        logits = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], want_logits=True)[3].cpu().numpy()
        full = t.loss_and_grad(p["x"], None, [[]] * p["B"], want_logits=True)[3].cpu().numpy()
    finally:
        t.close()
    want = TW.reference(name)[0][2]
    err = float(np.abs(logits - want).max())
    print("TRAIN-RATIO wrapped forward logits %s: kernel %.3e  bound 1.000e-04" % (name, err))
    assert err <= 1e-4
    for b in range(p["B"]):
        dead = logits[b, p["seq_len"][b]:]
        assert np.array_equal(dead, np.broadcast_to(p["w"]["bfc"], dead.shape)), b
    m = DeployModel(p["config"], p["w"])
    try:
        served = m.forward(torch.from_numpy(p["x"]), m.zero_state(p["B"]), want_softmax=False)["logits"].cpu().numpy()
    finally:
        m.close()
    err = float(np.abs(full - served).max())
    print("TRAIN-RATIO wrapped forward vs kws_step %s: %.3e  bound 2.000e-04" % (name, err))
    assert err <= 2e-4


@pytest.mark.parametrize("name", sorted(TW.CASES))
def test_gradients_against_the_restatement(name):
    p = TW.make_problem(name)
    (loss64, grads64, _), r32 = TW.reference(name)
    t = _trainer(p)
    try:
        total, grads, loss = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
        stats = t.stats()
        if name == "both_no_path":          # the utterance without a path contributes exactly 0: the same batch with its slot emptied
            seq = p["seq_len"].copy()
            seq[1] = 0
            _, without, loss_without = t.loss_and_grad(p["x"], seq, p["labels"])
    finally:
        t.close()
    inf = np.isinf(loss64)
    assert np.array_equal(np.isinf(loss), inf) and (loss[inf] > 0).all()
    assert np.isinf(total) == inf.any()
    assert (loss[p["seq_len"] == 0] == 0).all()
    err, bound = _report("wrapped loss", name, np.where(inf, 0.0, loss), np.where(inf, 0.0, loss64), r32["loss"])
    assert err <= bound
    assert ("ibeta" in grads["layers"][0]) == p["ln"]
    _check_grads("wrapped grad", name, grads, grads64, r32["grads"])
    assert stats["launches"] == grad_launches(p["config"].num_layers, p["ln"], p["res"])
    if name == "both_no_path":
        assert list(inf) == [False, True, False] and loss_without[1] == 0
        for (key, a), (_, b) in zip(TW.flat(grads), TW.flat(without)):
            assert np.array_equal(a, b), key
    if name == "ln_mel1":          # one feature: xn is exactly 0, and so is the gradient of the scale
        assert grads["layers"][0]["ibeta"] == 0 and np.abs(grads["layers"][0]["igamma"]).max() > 0
    if name == "ln_odd_mel":
        assert (p["seq_len"] == 0).sum() == 1
    if name == "both_split_rows":
        rows, chunk = p["B"] * p["T"], stats["chunk_rows"]
        assert rows >= 2.5 * chunk and rows % chunk != 0, (rows, chunk)
    if name == "ln_rows_chunk512":
        rows = p["B"] * p["T"]
        assert stats["chunk_rows"] == 512 and rows % 512 != 0, (rows, stats["chunk_rows"])


@pytest.mark.parametrize("name", ["both_ref_shape", "both_l8"])
def test_dropout_masks(name):
    p = TW.make_problem(name)
    drop = TW.drop_masks(p, 0.6)
    (loss64, grads64, _), r32 = TW.reference(name, 0.6)
    t = _trainer(p, keep_prob=0.6)
    try:
        _, grads, loss = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=drop)
    finally:
        t.close()
    err, bound = _report("wrapped dropout loss", name, loss, loss64, r32["loss"])
    assert err <= bound
    _check_grads("wrapped dropout grad", name, grads, grads64, r32["grads"])


# ---- bitwise properties --------------------------------------------------------------------------------------------------------------

def test_all_switches_off_through_the_wrapped_entry_is_the_plain_handle():
    """Loss, logits, gradient, launches and one step (masks at keep 0.6) of kws_train_create_wrapped with the three fields 0: the bits of
    kws_train_create."""
    p = M.make_problem("ref_shape")
    drop = M.drop_masks(p, 0.6)
    out = {}
    for wrapped in (False, True):
        t = _trainer(p, keep_prob=0.6, wrapped=wrapped)
        try:
            bits = _bits(t, p["x"], p["seq_len"], p["labels"], drop=drop)
            launches = t.stats()["launches"]
            loss = t.step_raw(p["x"], p["seq_len"], p["labels"], 0.01, drop=drop).cpu().numpy()
            out[wrapped] = (bits, launches, loss, t.weights_blob(), t.stats()["launches"])
        finally:
            t.close()
    _assert_same_bits(out[False][0], out[True][0], "switches off")
    assert out[False][1] == out[True][1] == grad_launches(2, 0, 0) and out[False][4] == out[True][4] == grad_launches(2, 0, 0) + 2
    assert np.array_equal(out[False][2].view(np.uint32), out[True][2].view(np.uint32))
    assert np.array_equal(out[False][3].view(np.uint32), out[True][3].view(np.uint32))
    assert not np.array_equal(out[True][3], M.blob_of(p["w"]).astype(np.float32))


def test_one_layer_residual_is_the_plain_handle():
    p = TW.make_problem("res_l1")
    plain = dict(p, config=TW.config_of(p["config"].hidden_size, 1, p["config"].n_mel, p["config"].num_classes))
    out = []
    for q in (plain, p):
        t = _trainer(q)
        try:
            assert (t._cfg.wrappers.use_residual == 1) == (q is p)
            out.append((_bits(t, p["x"], p["seq_len"], p["labels"]), t.stats()["launches"]))
        finally:
            t.close()
    _assert_same_bits(out[0][0], out[1][0], "res_l1")
    assert out[0][1] == out[1][1] == grad_launches(1, 0, 1) == grad_launches(1, 0, 0)


@pytest.mark.parametrize("name", ["both_ref_shape", "res_l2"])
def test_variational_mask_is_the_broadcast_mask_on_a_per_frame_handle(name):
    p, pv = TW.make_problem(name), TW.make_problem(name, var=True)
    layers, hidden = p["config"].num_layers, p["config"].hidden_size
    var = TW.drop_masks(p, 0.6, variational=True)
    wide = np.ascontiguousarray(np.broadcast_to(var[:, :, None, :], (layers, p["B"], p["T"], hidden)))
    a, b = _trainer(pv, keep_prob=0.6), _trainer(p, keep_prob=0.6)
    try:
        assert a._cfg.variational_recurrent == 1 and b._cfg.variational_recurrent == 0
        got, want = _bits(a, p["x"], p["seq_len"], p["labels"], drop=var), _bits(b, p["x"], p["seq_len"], p["labels"], drop=wide)
        none = _bits(b, p["x"], p["seq_len"], p["labels"])
        assert a.stats()["launches"] == b.stats()["launches"]
    finally:
        a.close()
        b.close()
    _assert_same_bits(got, want, "variational " + name)
    assert not np.array_equal(got[0][1], none[0][1])          # ... and the masks do something


def test_nan_padding_gives_the_bits_of_zero_padding_and_calls_repeat_bitwise():
    p = TW.make_problem("both_ref_shape")
    live = np.arange(p["T"])[None, :] < p["seq_len"][:, None]
    zero = np.where(live[:, :, None], p["x"], np.float32(0))
    nan = np.where(live[:, :, None], p["x"], np.float32(np.nan))
    t = _trainer(p)
    try:
        z, n, n2 = (_bits(t, x, p["seq_len"], p["labels"]) for x in (zero, nan, nan))
    finally:
        t.close()
    assert all(np.isfinite(v).all() for _, v in n)
    _assert_same_bits(z, n, "nan padding")
    _assert_same_bits(n, n2, "the same call twice")


# ---- the optimiser over the extended parameter set -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_one_step_is_the_fp64_update_of_the_devices_own_gradient(kind):
    """... within the bound's floor per tensor, ibeta / igamma and their kws_train_moments entries included; the clip active (grad_norm
    against fp64, over all tensors: the layer norm's gradients count) and inactive (the bits of no clipping)."""
    p = TW.make_problem("both_ref_shape")
    lr = 0.01
    after = {}
    for clip in ("none", "active", "inactive"):
        t = _trainer(p, optimizer=kind)
        try:
            _, g, _ = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
            norm64 = TW.global_norm(g)
            assert norm64 > M.global_norm(g) * (1 + 1e-6)          # M.global_norm: the plain tensors alone
            max_norm = {"none": -1.0, "active": 0.5 * norm64, "inactive": 2.0 * norm64}[clip]
            t.close()
            t = _trainer(p, optimizer=kind, max_grad_norm=max_norm)
            _, norm = t.step_raw(p["x"], p["seq_len"], p["labels"], lr, want_norm=True)
            after[clip] = t.weights()
            m, v = t.moments()
            assert t.stats()["steps"] == 1
        finally:
            t.close()
        assert abs(float(norm.item()) - norm64) <= FLOOR * norm64, (clip, float(norm.item()), norm64)
        opt = TW.Optimizer(p["w"], kind)
        want = opt.apply(p["w"], g, lr, max_norm)
        for (key, a), (_, r) in zip(TW.flat(after[clip]), TW.flat(want)):
            err, floor = float(np.abs(a - r).max()), FLOOR * float(np.abs(r).max())
            print("TRAIN-RATIO wrapped one step %s clip %s %s: kernel %.3e  floor %.3e" % (kind, clip, key, err, floor))
            assert np.shape(a) == np.shape(r) and err <= floor, (clip, key, err, floor)
        for i, ((key, got_m), (_, got_v)) in enumerate(zip(TW.flat(m), TW.flat(v))):
            for what, got, ref in (("m", got_m, opt.m[i]), ("v", got_v, opt.v[i])):
                err, floor = float(np.abs(got - ref).max()), FLOOR * float(np.abs(ref).max())
                assert np.shape(got) == np.shape(ref) and err <= floor, (clip, what, key, err, floor)
            if "_i" in key:          # the layer norm's slots are live
                assert np.abs(got_m).max() > 0 and (kind == "nesterov" or np.abs(got_v).max() > 0), key
    flat = {c: TW.flat(after[c]) for c in after}
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(flat["none"], flat["inactive"]))
    assert not all(np.array_equal(a, b) for (_, a), (_, b) in zip(flat["none"], flat["active"]))
    moved = dict((k, not np.array_equal(a, b)) for (k, a), (_, b) in zip(flat["none"], TW.flat(p["w"])))
    assert moved["l0_ibeta"] and moved["l1_igamma"]


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
@pytest.mark.parametrize("name", ["both_ref_shape", "both_h256"])
def test_twenty_steps_follow_the_restatement(name, kind):
    steps, lr = 20, M.TRAJECTORY_LR[kind]
    p = TW.make_problem(name)
    loss64, path64 = TW.trajectory(name, kind, steps, lr)
    loss32, path32 = TW.trajectory(name, kind, steps, lr, float32=True)
    t = _trainer(p, optimizer=kind)
    got_loss, got_path = [], []
    try:
        for _ in range(steps):
            got_loss.append(t.step_raw(p["x"], p["seq_len"], p["labels"], lr).cpu().numpy())
            got_path.append(t.weights_blob())
    finally:
        t.close()
    assert got_path[0].size == path64[0].size
    _check_trajectory("wrapped twenty steps %s %s" % (name, kind), got_loss, got_path, loss64, path64, loss32, path32)


# ---- steady state, end to end, refusals -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln,res,var", [(1, 1, 1), (1, 0, 0), (0, 1, 0)])
def test_steady_state_allocates_nothing_and_the_launch_count_is_the_documented_one(ln, res, var):
    p = dict(TW.make_problem("both_l8"))
    cfg = p["config"]
    layers = cfg.num_layers
    p["config"] = TW.config_of(cfg.hidden_size, layers, cfg.n_mel, cfg.num_classes, ln, res, var)
    if not ln:
        p["w"] = dict(layers=[{k: lay[k] for k in TW.LAYER_KEYS} for lay in p["w"]["layers"]], Wfc=p["w"]["Wfc"], bfc=p["w"]["bfc"])
    t = _trainer(p)
    try:
        assert t.stats()["allocs"] == 0
        t.reserve(p["B"], p["T"])
        reserved = t.stats()
        t.step_raw(p["x"], p["seq_len"], p["labels"], 0.01)
        first = t.stats()
        for _ in range(2):
            t.step_raw(p["x"], p["seq_len"], p["labels"], 0.01)
        t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
        grad_count = t.stats()["launches"]
        short = t.step_raw(p["x"][:, :3], np.minimum(p["seq_len"], 3), [[1]] * p["B"], 0.01)          # another T in the same tape
        last = t.stats()
        assert np.isfinite(short.cpu().numpy()).all()
    finally:
        t.close()
    assert reserved["allocs"] == first["allocs"] == last["allocs"] == 1 and last["device_bytes"] == reserved["device_bytes"]
    assert grad_count == grad_launches(layers, ln, res) and first["launches"] == last["launches"] == grad_count + 2
    assert last["steps"] == 4


def test_toy_task_end_to_end_with_all_three_switches():
    """Trainer.step on the L = 2 toy task with layer norm, residual and variational masks at keep_prob 0.9, for the steps the host test
    established; deploy() serves the result through kws_create_wrapped and ctc_predict recognises every utterance."""
    from keyword_spotting_amd.prediction import ctc_decode2, ctc_predict
    from keyword_spotting_amd.training import Trainer
    p = TW.toy_task(0)
    t = Trainer(p["config"], p["w"], learning_rate=TW.TOY["lr"], lr_decay=1.0, keep_prob=TW.TOY["keep_prob"])
    try:
        assert t.variational and t._drop_shape(p["B"], p["T"]) == (2, p["B"], TW.TOY["H"])
        losses = [t.step(p["x"], p["seq_len"], p["labels"]) for _ in range(TW.TOY["steps"])]
        final = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])[0]
        w = t.weights()
        model = t.deploy()
    finally:
        t.close()
    try:
        print("TRAIN-RATIO wrapped toy task: loss %.4f -> %.4f in %d steps, ibeta %s" % (losses[0], final, TW.TOY["steps"], [float(lay["ibeta"]) for lay in w["layers"]]))
        assert model.wrappers == (True, True)
        assert final < 0.1 * losses[0]
        assert float(w["layers"][0]["ibeta"]) != 0
        sm = model.forward(torch.from_numpy(p["x"]), model.zero_state(p["B"]), want_logits=False)["softmax"]
        assert [ctc_predict(ctc_decode2(sm[i], TW.TOY["C"]), TW.TOY["label"]) for i in range(p["B"])] == [1] * p["B"]
    finally:
        model.close()


def test_a_drop_of_the_wrong_shape_for_the_handle_is_refused():
    from keyword_spotting_amd import _lib
    p, pv = TW.make_problem("res_l2"), TW.make_problem("res_l2", var=True)
    per_frame, per_stream = TW.drop_masks(p, 0.6), TW.drop_masks(p, 0.6, variational=True)
    a, b = _trainer(pv, keep_prob=0.6), _trainer(p, keep_prob=0.6)
    try:
        with pytest.raises(_lib.InvalidArgumentError, match=r"drop must be \[2,3,64\] \(variational_recurrent"):
            a.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=per_frame)
        with pytest.raises(_lib.InvalidArgumentError, match=r"drop must be \[2,3,8,64\], got"):
            b.step_raw(p["x"], p["seq_len"], p["labels"], 0.01, drop=per_stream)
        assert a.stats()["allocs"] == 0 and b.stats()["steps"] == 0          # nothing ran
        assert np.isfinite(a.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=per_stream)[0])
    finally:
        a.close()
        b.close()
