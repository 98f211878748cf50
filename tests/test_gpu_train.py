"""Training of the stack on the device (kws_train_*, keyword_spotting_amd.training.Trainer) against the fp64 restatement
tests/train_model.py, with the deviation of the identical torch graph in float32 (CPU) as the yardstick: per tensor, bound = max(4 x
that deviation, 16 * 2^-23 * max|reference|) -- the project's bound for this kind of comparison (tests/test_gpu_enroll.py).  Every
comparison prints a TRAIN-RATIO line (kernel / float32-CPU / bound) before it asserts."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import train_model as M

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -23


def _bound(ref64, ref32):
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    return max(4.0 * dev, FLOOR * (float(np.abs(ref64).max()) if np.size(ref64) else 0.0)), dev


def _report(what, name, got, ref64, ref32):
    bound, dev = _bound(ref64, ref32)
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    print("TRAIN-RATIO %s %s: kernel %.3e  float32-CPU %.3e  bound %.3e  kernel/bound %.3f" % (what, name, err, dev, bound, err / bound if bound > 0 else 0.0))
    return err, bound


def _trainer(p, **kw):
    from keyword_spotting_amd.training import Trainer
    return Trainer(p["config"], p["w"], **kw)


@pytest.fixture(scope="module")
def refs():
    """name -> (fp64 restatement, float32 torch) of the plain gradient call, computed once per case."""
    cache = {}

    def get(name):
        if name not in cache:
            p = M.make_problem(name)
            cache[name] = (M.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"]),
                           M.torch_reference(p["w"], p["x"], p["seq_len"], p["labels"], torch.float32))
        return cache[name]
    return get


def _check_grads(what, name, got, ref64, ref32):
    worst = []
    for (key, g), (_, r64), (_, r32) in zip(M.flat(got), M.flat(ref64), M.flat(ref32)):
        err, bound = _report(what + " " + key, name, g, r64, r32)
        if err > bound:
            worst.append((key, err, bound))
    assert not worst, worst


def test_new_entry_points_exist():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_train_create", "kws_train_destroy", "kws_train_set_weights", "kws_train_get_weights", "kws_train_grad", "kws_train_step",
                "kws_train_moments", "kws_train_stats", "kws_train_reserve", "kws_train_check"):
        assert hasattr(lib, sym), sym


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_taped_forward_logits(name, refs):
    """No dropout: logits against the restatement (1e-4), rows t >= seq_len are bfc bitwise, and at full length the logits of
    kws_step on the same weights (2e-5)."""
    from keyword_spotting_amd.rnn_ctc import DeployModel
    p = M.make_problem(name)
    t = _trainer(p)
    try:
        logits = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], want_logits=True)[3].cpu().numpy()
        full = t.loss_and_grad(p["x"], None, [[]] * p["B"], want_logits=True)[3].cpu().numpy()
    finally:
        t.close()
    want = refs(name)[0][2]
    err = float(np.abs(logits - want).max())
    print("TRAIN-RATIO forward logits %s: kernel %.3e  bound 1.000e-04" % (name, err))
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
    print("TRAIN-RATIO forward vs kws_step %s: %.3e  bound 2.000e-05" % (name, err))
    assert err <= 2e-5


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_gradients_against_the_restatement(name, refs):
    p = M.make_problem(name)
    (loss64, grads64, _), r32 = refs(name)
    t = _trainer(p)
    try:
        total, grads, loss = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
        stats = t.stats()
        if name == "no_path":          # the utterance without a path contributes exactly 0: the same batch with its slot emptied
            seq = p["seq_len"].copy()
            seq[1] = 0
            _, without, loss_without = t.loss_and_grad(p["x"], seq, p["labels"])
    finally:
        t.close()
    inf = np.isinf(loss64)
    assert np.array_equal(np.isinf(loss), inf) and (loss[inf] > 0).all()
    assert np.isinf(total) == inf.any()
    assert (loss[p["seq_len"] == 0] == 0).all()
    err, bound = _report("loss", name, np.where(inf, 0.0, loss), np.where(inf, 0.0, loss64), r32["loss"])
    assert err <= bound
    _check_grads("grad", name, grads, grads64, r32["grads"])
    if name == "no_path":
        assert list(inf) == [False, True, False] and loss_without[1] == 0
        for (key, a), (_, b) in zip(M.flat(grads), M.flat(without)):
            assert np.array_equal(a, b), key
    if name == "split_rows":
        rows, chunk = p["B"] * p["T"], stats["chunk_rows"]
        assert rows >= 2.5 * chunk and rows % chunk != 0, (rows, chunk)


@pytest.mark.parametrize("name", ["odd_mel", "ref_shape"])
def test_dropout_masks(name):
    p = M.make_problem(name)
    drop = M.drop_masks(p, 0.6)
    loss64, grads64, _ = M.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], drop, 0.6)
    r32 = M.torch_reference(p["w"], p["x"], p["seq_len"], p["labels"], torch.float32, drop, 0.6)
    t = _trainer(p, keep_prob=0.6)
    try:
        _, grads, loss = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=drop)
    finally:
        t.close()
    err, bound = _report("dropout loss", name, loss, loss64, r32["loss"])
    assert err <= bound
    _check_grads("dropout grad", name, grads, grads64, r32["grads"])


def test_all_ones_mask_at_keep_prob_one_is_no_mask_bitwise():
    p = M.make_problem("ref_shape")
    ones = np.ones((p["config"].num_layers, p["B"], p["T"], p["config"].hidden_size), np.uint8)
    t = _trainer(p)
    try:
        _, g0, l0 = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
        _, g1, l1 = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=ones)
    finally:
        t.close()
    assert np.array_equal(l0, l1) and all(np.array_equal(a, b) for (_, a), (_, b) in zip(M.flat(g0), M.flat(g1)))


def test_nan_padding_gives_the_bits_of_zero_padding_and_calls_repeat_bitwise():
    p = M.make_problem("ref_shape")
    live = np.arange(p["T"])[None, :] < p["seq_len"][:, None]
    zero = np.where(live[:, :, None], p["x"], np.float32(0))
    nan = np.where(live[:, :, None], p["x"], np.float32(np.nan))
    t = _trainer(p)
    try:
        _, gz, lz, logz = t.loss_and_grad(zero, p["seq_len"], p["labels"], want_logits=True)
        _, gn, ln, logn = t.loss_and_grad(nan, p["seq_len"], p["labels"], want_logits=True)
        _, gn2, ln2 = t.loss_and_grad(nan, p["seq_len"], p["labels"])
    finally:
        t.close()
    assert np.isfinite(ln).all() and torch.equal(logz, logn)
    for (key, a), (_, b), (_, c) in zip(M.flat(gz), M.flat(gn), M.flat(gn2)):
        assert np.isfinite(b).all() and np.array_equal(a, b) and np.array_equal(b, c), key
    assert np.array_equal(lz, ln) and np.array_equal(ln, ln2)


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_one_step_is_the_fp64_update_of_the_devices_own_gradient(kind):
    """... within the bound's floor per tensor; the clip active (grad_norm against fp64) and inactive (the bits of no clipping)."""
    p = M.make_problem("ref_shape")
    lr = 0.01
    after = {}
    for clip in ("none", "active", "inactive"):
        t = _trainer(p, optimizer=kind)
        try:
            _, g, _ = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
            norm64 = M.global_norm(g)
            max_norm = {"none": -1.0, "active": 0.5 * norm64, "inactive": 2.0 * norm64}[clip]
            t.close()
            t = _trainer(p, optimizer=kind, max_grad_norm=max_norm)
            _, norm = t.step_raw(p["x"], p["seq_len"], p["labels"], lr, want_norm=True)
            after[clip] = t.weights()
            assert t.stats()["steps"] == 1
        finally:
            t.close()
        assert abs(float(norm.item()) - norm64) <= FLOOR * norm64, (clip, float(norm.item()), norm64)
        want = M.Optimizer(p["w"], kind).apply(p["w"], g, lr, max_norm)
        for (key, a), (_, r) in zip(M.flat(after[clip]), M.flat(want)):
            err, floor = float(np.abs(a - r).max()), FLOOR * float(np.abs(r).max())
            print("TRAIN-RATIO one step %s clip %s %s: kernel %.3e  floor %.3e" % (kind, clip, key, err, floor))
            assert err <= floor, (clip, key, err, floor)
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(M.flat(after["none"]), M.flat(after["inactive"])))
    assert not all(np.array_equal(a, b) for (_, a), (_, b) in zip(M.flat(after["none"]), M.flat(after["active"])))


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
@pytest.mark.parametrize("name", ["t2", "ref_shape", "c8_s_long"])
def test_twenty_steps_follow_the_restatement(name, kind):
    """Losses and parameters after every step against the fp64 restatement, one call per step, weights read back each step.  The
    yardstick at step s is the largest deviation the float32 torch trajectory has shown from the fp64 one up to s; bound_s = max(4 x
    that, s x floor) -- test_twenty_step_fit_follows_the_restatement's."""
    steps, lr = 20, M.TRAJECTORY_LR[kind]
    p = M.make_problem(name)
    loss64, path64 = M.trajectory(name, kind, steps, lr)
    loss32, path32 = M.trajectory(name, kind, steps, lr, float32=True)
    t = _trainer(p, optimizer=kind)
    got_loss, got_path = [], []
    try:
        for _ in range(steps):
            got_loss.append(t.step_raw(p["x"], p["seq_len"], p["labels"], lr).cpu().numpy())
            got_path.append(t.weights_blob())
    finally:
        t.close()
    dev_l = dev_w = worst = 0.0
    for s in range(steps):
        dev_l = max(dev_l, float(np.abs(loss32[s] - loss64[s]).max()))
        dev_w = max(dev_w, float(np.abs(path32[s] - path64[s]).max()))
        b_l = max(4 * dev_l, (s + 1) * FLOOR * float(np.abs(loss64[s]).max()))
        b_w = max(4 * dev_w, (s + 1) * FLOOR * float(np.abs(path64[s]).max()))
        e_l = float(np.abs(got_loss[s] - loss64[s]).max())
        e_w = float(np.abs(got_path[s] - path64[s]).max())
        worst = max(worst, e_l / b_l, e_w / b_w)
        assert e_l <= b_l and e_w <= b_w, (s, e_l, b_l, e_w, b_w)
    print("TRAIN-RATIO twenty steps %s %s: worst kernel/bound %.3f (float32-CPU drift: loss %.3e, parameters %.3e)" % (name, kind, worst, dev_l, dev_w))


def _train_toy(hidden):
    """Trainer.step on the toy task for the steps the host test established -> (first loss, final loss, the trainer)."""
    from keyword_spotting_amd.training import Trainer
    p = M.toy_task(0, hidden)
    t = Trainer(p["config"], p["w"], learning_rate=M.TOY["lr"], lr_decay=1.0)
    try:
        losses = [t.step(p["x"], p["seq_len"], p["labels"]) for _ in range(M.TOY["steps"])]
        final = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])[0]
    except Exception:
        t.close()
        raise
    print("TRAIN-RATIO toy task H=%d: loss %.4f -> %.4f in %d steps" % (p["config"].hidden_size, losses[0], final, M.TOY["steps"]))
    return p, losses[0], final, t


def _recognised(model, p):
    from keyword_spotting_amd.prediction import ctc_decode2, ctc_predict
    sm = model.forward(torch.from_numpy(p["x"]), model.zero_state(p["B"]), want_logits=False)["softmax"]
    return [ctc_predict(ctc_decode2(sm[i], M.TOY["C"]), M.TOY["label"]) for i in range(p["B"])]


def test_toy_task_end_to_end():
    """Trainer.step on the toy task of tests/test_train_host.py (H 64), then deploy(): the loss falls below a tenth and every training
    utterance is recognised through DeployModel and ctc_predict."""
    p, first, final, t = _train_toy(None)
    try:
        model = t.deploy()
    finally:
        t.close()
    try:
        assert final < 0.1 * first
        assert _recognised(model, p) == [1] * p["B"]
    finally:
        model.close()


def test_trained_weights_serve_on_the_fast_path():
    """deploy(precision="f16x3") against the fp32 deploy, 1e-4 on logits.  The f16x3 kernels take hidden 128 / 256 only, so the toy task
    is trained at H = 128 (the host test establishes that the restatement trains there too): the same steps, the same loss bound, and
    every utterance recognised through BOTH deploys."""
    p, first, final, t = _train_toy(128)
    try:
        fp32, fast = t.deploy(), t.deploy(precision="f16x3")
    finally:
        t.close()
    try:
        assert final < 0.1 * first
        x = torch.from_numpy(p["x"])
        a = fp32.forward(x, fp32.zero_state(p["B"]), want_softmax=False)["logits"]
        b = fast.forward(x, fast.zero_state(p["B"]), want_softmax=False)["logits"]
        err = float((a - b).abs().max().item())
        print("TRAIN-RATIO trained weights on f16x3: %.3e  bound 1.000e-04" % err)
        assert err <= 1e-4
        assert _recognised(fp32, p) == [1] * p["B"] and _recognised(fast, p) == [1] * p["B"]
    finally:
        fp32.close()
        fast.close()


def test_steady_state_allocates_nothing_and_the_launch_count_does_not_depend_on_t():
    p = M.make_problem("ref_shape")
    layers = p["config"].num_layers
    t = _trainer(p)
    try:
        assert t.stats()["allocs"] == 0
        t.step_raw(p["x"], p["seq_len"], p["labels"], 0.01)
        first = t.stats()
        for _ in range(3):
            t.step_raw(p["x"], p["seq_len"], p["labels"], 0.01)
        t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
        grad_launches = t.stats()["launches"]
        short = t.step_raw(p["x"][:, :5], np.minimum(p["seq_len"], 5), [[1]] * p["B"], 0.01)          # a smaller shape fits the same tape
        last = t.stats()
        assert np.isfinite(short.cpu().numpy()).all()
    finally:
        t.close()
    assert first["allocs"] == 1 and last["allocs"] == 1 and last["device_bytes"] == first["device_bytes"]
    assert first["launches"] == last["launches"] == 4 * layers + 8 and grad_launches == 4 * layers + 6
    assert last["steps"] == 5


def test_refusals_behind_the_device_check():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.training import Trainer
    p = M.make_problem("t2")
    t = _trainer(p)
    try:
        with pytest.raises(_lib.KwsError, match=r"takes \d+ bytes: the device has \d+ free") as e:
            t.reserve(65536, 2000)                    # 131 M frames x 64 units x 9 blocks x 4 bytes and more
        assert e.value.code == _lib.KWS_ERR_OUT_OF_MEMORY and t.stats()["allocs"] == 0
        with pytest.raises(_lib.UnsupportedError, match="198800 bytes exceed the 163840"):
            t.loss_and_grad(np.zeros((1, 700, 4), np.float32), [700], [[0] * 31])
        with pytest.raises(_lib.InvalidArgumentError, match=r"labels\[0\]\[1\]=2"):
            t.loss_and_grad(p["x"], p["seq_len"], [[0, 2]])
        with pytest.raises(_lib.InvalidArgumentError, match="lr="):
            t.step_raw(p["x"], p["seq_len"], p["labels"], 0.0)
        # the masks are read four units at a time: a drop pointer off a 4-byte boundary is refused, not read
        cfg = p["config"]
        masks = torch.ones(cfg.num_layers * p["B"] * p["T"] * cfg.hidden_size + 4, dtype=torch.uint8, device="cuda")
        xd, loss = torch.from_numpy(p["x"]).cuda(), torch.empty(p["B"], device="cuda")
        ints = [np.ascontiguousarray(a, np.int32) for a in (p["seq_len"], [[0, 1]], [2])]
        rc = t._lib.kws_train_step(t._handle, _lib.ptr(xd), *[a.ctypes.data_as(ctypes.c_void_p) for a in ints], p["B"], p["T"], 2,
                                   ctypes.c_void_p(masks.data_ptr() + 1), 0.01, _lib.ptr(loss), None, None)
        assert rc == _lib.KWS_ERR_INVALID_ARGUMENT and b"drop" in t._lib.kws_last_error()
        assert t.stats()["allocs"] == 0 and t.stats()["steps"] == 0          # nothing ran, nothing was allocated
        # hidden 256 is served, not refused
        big = M.config_of(256, 1, 4, 3)
        from keyword_spotting_amd import weights
        t256 = Trainer(big, weights.init_weights(big, seed=1))
        try:
            loss = t256.loss_and_grad(p["x"], p["seq_len"], p["labels"])[0]
            assert np.isfinite(loss)
        finally:
            t256.close()
        # a second host thread inside the handle: KWS_ERR_BUSY, nothing launched; afterwards the handle works
        stop, blob = threading.Event(), t.weights_blob()

        def hold():
            n = 0
            while not stop.is_set() and n < 100000:
                try:
                    t.set_weights(blob)          # waits for its stream inside the call
                except _lib.BusyError:
                    pass
                n += 1
        th = threading.Thread(target=hold)
        th.start()
        seen = False
        try:
            for _ in range(1000000):
                try:
                    t.reserve(1, 2, 2)
                except _lib.BusyError:
                    seen = True
                    break
                if not th.is_alive():
                    break
        finally:
            stop.set()
            th.join(60)
        assert seen
        assert np.isfinite(t.loss_and_grad(p["x"], p["seq_len"], p["labels"])[0])
    finally:
        t.close()
