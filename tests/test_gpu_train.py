"""Training of the stack on the device (kws_train_*, keyword_spotting_amd.training.Trainer) against the fp64 restatement
tests/train_model.py, with the deviation of the identical torch graph in float32 (CPU) as the yardstick: per tensor, bound = max(4 x
that deviation, 16 * 2^-23 * max|reference|) -- the project's bound for this kind of comparison (tests/test_gpu_enroll.py).  Every
comparison prints a TRAIN-RATIO line (kernel / float32-CPU / bound) before it asserts.  What has to hold to the bit -- inputs off a
16-byte boundary, a re-carved arena against a fresh handle, calls from two streams, Trainer.step against a twin fed the same draws -- is
compared as uint32."""
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
    kws_step on the same weights (2e-5) for the first nine cases.  The later cases go where the serving kernels' own distance from fp64
    (bound 1e-4, tests/test_gpu_config_space.py; 1.5e-5 measured at n_mel 1024) leaves no room for 2e-5 between the two: there each
    side is held against the restatement's full-length logits at 1e-4 and the difference between them is printed."""
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
    if name == "dead_group":          # the workgroup that never enters its frame loops: bfc at EVERY frame
        assert (p["seq_len"][16:32] == 0).all() and (p["seq_len"][:16] > 0).any() and p["seq_len"][32] == p["T"]
        assert np.array_equal(logits[16:32], np.broadcast_to(p["w"]["bfc"], logits[16:32].shape))
    m = DeployModel(p["config"], p["w"])
    try:
        served = m.forward(torch.from_numpy(p["x"]), m.zero_state(p["B"]), want_softmax=False)["logits"].cpu().numpy()
    finally:
        m.close()
    err = float(np.abs(full - served).max())
    if name in M.FIRST_CASES:
        print("TRAIN-RATIO forward vs kws_step %s: %.3e  bound 2.000e-05" % (name, err))
        assert err <= 2e-5
        return
    want_full = M.forward(p["w"], p["x"], np.full(p["B"], p["T"]))[0]
    e_train, e_served = float(np.abs(full - want_full).max()), float(np.abs(served - want_full).max())
    print("TRAIN-RATIO forward at full length %s: kernel %.3e  kws_step %.3e  bound 1.000e-04  (kernel vs kws_step %.3e, not asserted)"
          % (name, e_train, e_served, err))
    assert e_train <= 1e-4 and e_served <= 1e-4


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
    if name == "rows_chunk512":          # the chunk has grown past its unit of 256 rows, and the last chunk is partial
        rows = p["B"] * p["T"]
        assert stats["chunk_rows"] == 512 and rows % 512 != 0, (rows, stats["chunk_rows"])
    if name == "dead_group":
        assert (p["seq_len"][16:32] == 0).all() and (loss[16:32] == 0).all() and (loss[:16] > 0).all() and loss[32] > 0


@pytest.mark.parametrize("name", ["odd_mel", "ref_shape", "h256", "l8"])
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


def _check_trajectory(what, got_loss, got_path, loss64, path64, loss32, path32):
    """Losses and parameter blobs after every step against the fp64 trajectory.  The yardstick at step s is the largest deviation the
    float32 torch trajectory has shown from the fp64 one up to s; bound_s = max(4 x that, s x floor) --
    test_twenty_step_fit_follows_the_restatement's."""
    dev_l = dev_w = worst = 0.0
    for s in range(len(got_path)):
        dev_l = max(dev_l, float(np.abs(loss32[s] - loss64[s]).max()))
        dev_w = max(dev_w, float(np.abs(path32[s] - path64[s]).max()))
        b_l = max(4 * dev_l, (s + 1) * FLOOR * float(np.abs(loss64[s]).max()))
        b_w = max(4 * dev_w, (s + 1) * FLOOR * float(np.abs(path64[s]).max()))
        e_l = float(np.abs(got_loss[s] - loss64[s]).max())
        e_w = float(np.abs(got_path[s] - path64[s]).max())
        worst = max(worst, e_l / b_l, e_w / b_w)
        assert e_l <= b_l and e_w <= b_w, (s, e_l, b_l, e_w, b_w)
    print("TRAIN-RATIO %s: worst kernel/bound %.3f (float32-CPU drift: loss %.3e, parameters %.3e)" % (what, worst, dev_l, dev_w))


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
@pytest.mark.parametrize("name", ["t2", "ref_shape", "c8_s_long", "h256"])
def test_twenty_steps_follow_the_restatement(name, kind):
    """Losses and parameters after every step against the fp64 restatement, one call per step, weights read back each step, under
    _check_trajectory's bound."""
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
    _check_trajectory("twenty steps %s %s" % (name, kind), got_loss, got_path, loss64, path64, loss32, path32)


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_trainer_step_draws_masks_and_follows_the_schedule(kind):
    """Trainer.step as main.py runs it (keep_prob 0.6, the rate halving every two steps), three steps on odd_mel.  A twin trainer gets
    the same draws made here -- a generator of the same seed, per step the x mask then the [L,B,T,H] masks -- through step_raw: equal
    losses, the same weights bitwise after every step; and those weights follow the restatement run with these masks and rates under
    _check_trajectory's bound."""
    from keyword_spotting_amd.training import learning_rate_at
    p = M.make_problem("odd_mel")
    cfg, seed, keep_prob, steps = p["config"], 11, 0.6, 3
    kw = dict(keep_prob=keep_prob, learning_rate=0.1, lr_decay=0.5, decay_step=2, optimizer=kind)
    t, twin = _trainer(p, seed=seed, **kw), _trainer(p, seed=seed + 1, **kw)          # the twin's own generator is never drawn from
    xs, drops, lrs, got_loss, got_path = [], [], [], [], []
    try:
        gen = torch.Generator(device=t.device)
        gen.manual_seed(seed)
        x = torch.from_numpy(p["x"]).to(t.device)
        for s in range(steps):
            keep = torch.floor(keep_prob + torch.rand(x.shape, generator=gen, device=t.device))
            xd = x / keep_prob * keep
            drop = torch.floor(keep_prob + torch.rand((cfg.num_layers, p["B"], p["T"], cfg.hidden_size), generator=gen, device=t.device)).to(torch.uint8)
            lr = learning_rate_at(s, 0.1, 0.5, 2)
            assert lr == t.learning_rate_at(t.global_step)
            total = t.step(p["x"], p["seq_len"], p["labels"])
            per = twin.step_raw(xd, p["seq_len"], p["labels"], lr, drop=drop).cpu().numpy()
            assert total == float(per.astype(np.float64).sum() / p["B"]), s
            mine, theirs = t.weights_blob(), twin.weights_blob()
            assert np.array_equal(mine.view(np.uint32), theirs.view(np.uint32)), s
            xs.append(xd.cpu().numpy()); drops.append(drop.cpu().numpy()); lrs.append(lr); got_loss.append(per); got_path.append(mine)
        assert t.global_step == steps and t.stats()["steps"] == steps
    finally:
        t.close()
        twin.close()
    assert lrs == [0.1, 0.1 * 0.5 ** 0.5, 0.05]
    for d, xd in zip(drops, xs):          # both kinds of dropout are live, and no two steps share a draw
        assert 0.3 < d.mean() < 0.9 and 0.3 < (xd != 0).mean() < 0.9
    assert not np.array_equal(drops[0], drops[1]) and not np.array_equal(xs[0], xs[1])

    def run(float32):
        w = p["w"] if float32 else M.as_dtype(p["w"], np.float64)
        opt = M.Optimizer(w, kind, np.float32 if float32 else np.float64)
        losses, path = [], []
        for s in range(steps):
            if float32:
                r = M.torch_reference(w, xs[s], p["seq_len"], p["labels"], torch.float32, drops[s], keep_prob)
                loss, grads = r["loss"], r["grads"]
            else:
                loss, grads, _ = M.loss_and_grad(w, xs[s], p["seq_len"], p["labels"], drops[s], keep_prob)
            w = opt.apply(w, grads, lrs[s])
            losses.append(np.asarray(loss, np.float64))
            path.append(M.blob_of(w))
        return losses, path
    loss64, path64 = run(False)
    loss32, path32 = run(True)
    _check_trajectory("Trainer.step odd_mel %s" % kind, got_loss, got_path, loss64, path64, loss32, path32)


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_moments_after_three_steps(kind):
    """kws_train_moments: Adam's m and v (Nesterov: the accumulator, and zeros) against the fp64 optimiser fed the device's own
    gradients, within the bound's floor per tensor as the one-step test; set_weights zeroes them and the step count.

    The regression test of Adam's 1 - beta2: formed as 1.0f - 0.999f = 0.00099998713 it left v 1.29e-5 below the fp64 optimiser's on
    every tensor (l0_Wg: 2.296e-10 against a floor of 3.392e-11), which no comparison of the parameters is fine enough to see."""
    p = M.make_problem("t2")
    lr = M.TRAJECTORY_LR[kind]
    opt, opt32 = M.Optimizer(p["w"], kind), M.Optimizer(p["w"], kind, np.float32)
    t = _trainer(p, optimizer=kind)
    try:
        for _ in range(3):
            _, g, _ = t.loss_and_grad(p["x"], p["seq_len"], p["labels"])          # the gradient the step below takes: the parameters stay
            opt.apply(t.weights(), g, lr)
            opt32.apply(t.weights(), g, lr)
            t.step_raw(p["x"], p["seq_len"], p["labels"], lr)
        m, v = t.moments()
        assert t.stats()["steps"] == 3
        t.set_weights(p["w"])
        m0, v0 = t.moments()
        assert t.stats()["steps"] == 0
    finally:
        t.close()
    assert all(not a.any() and not b.any() for (_, a), (_, b) in zip(M.flat(m0), M.flat(v0)))
    over = []
    for i, ((key, got_m), (_, got_v)) in enumerate(zip(M.flat(m), M.flat(v))):
        for what, got, ref, ref32 in (("m", got_m, opt.m[i], opt32.m[i]), ("v", got_v, opt.v[i], opt32.v[i])):
            assert got.shape == ref.shape
            err, floor = float(np.abs(got - ref).max()), FLOOR * float(np.abs(ref).max())
            print("TRAIN-RATIO moments %s %s %s: kernel %.3e  floor %.3e  (against the float32 optimiser %.3e, not asserted)"
                  % (kind, what, key, err, floor, float(np.abs(got - ref32.astype(np.float64)).max())))
            if err > floor:
                over.append((what, key, err, floor))
        assert np.abs(opt.m[i]).max() > 0, key
        if kind == "nesterov":
            assert not got_v.any(), key
        else:
            assert np.abs(opt.v[i]).max() > 0, key
    assert not over, over


# ---- bitwise properties: alignment of the inputs, reuse of the arena, calls from two streams ---------------------------------------

def _bits(t, x, seq_len, labels, drop=None):
    """One loss_and_grad -> [(name, array)]: the per-utterance losses, the logits and every gradient tensor."""
    _, g, loss, logits = t.loss_and_grad(x, seq_len, labels, drop=drop, want_logits=True)
    return [("loss", loss), ("logits", logits.cpu().numpy())] + M.flat(g)


def _assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for (key, u), (_, v) in zip(a, b):
        assert u.shape == v.shape and np.array_equal(u.view(np.uint32), v.view(np.uint32)), (what, key)


@pytest.mark.parametrize("name", ["mel72", "ref_shape"])
def test_x_one_float_past_a_16_byte_boundary_gives_the_same_bits(name):
    """The x-part GEMM takes 16-byte loads only from a 16-byte aligned base; the ABI asks for 4 bytes.  The scalar loads fetch the same
    floats into the same products in the same order, so nothing may move by a bit (mel72: behind the first pass of the K loop too)."""
    p = M.make_problem(name)
    aligned = torch.from_numpy(p["x"]).cuda()
    store = torch.empty(1 + p["x"].size, dtype=torch.float32, device="cuda")
    store[1:] = aligned.reshape(-1)
    shifted = store[1:].view(p["x"].shape)
    t = _trainer(p)
    try:
        for x, off in ((aligned, 0), (shifted, 4)):          # the pointer the C entry gets is the tensor's own
            assert t._inputs(x, p["seq_len"], p["labels"], None)[0].data_ptr() == x.data_ptr() and x.data_ptr() % 16 == off
        want = _bits(t, aligned, p["seq_len"], p["labels"])
        got = _bits(t, shifted, p["seq_len"], p["labels"])
    finally:
        t.close()
    _assert_same_bits(want, got, name)


def test_drop_masks_four_bytes_past_a_16_byte_boundary_give_the_same_bits():
    """The masks are read four units at a time from a pointer that has to be 4-byte aligned and no more: through the C entry."""
    from keyword_spotting_amd import _lib, weights
    p = M.make_problem("ref_shape")
    drop = M.drop_masks(p, 0.6)
    store = torch.zeros(4 + drop.size, dtype=torch.uint8, device="cuda")
    store[4:] = torch.from_numpy(drop.reshape(-1)).cuda()
    assert store.data_ptr() % 16 == 0
    t = _trainer(p, keep_prob=0.6)
    try:
        want = _bits(t, p["x"], p["seq_len"], p["labels"], drop=drop)
        x, b, frames, (_, sl_p), (lab, lab_p), (_, ll_p), _ = t._inputs(p["x"], p["seq_len"], p["labels"], None)
        loss = torch.empty(b, device="cuda")
        grad = torch.empty(t.weights_blob().size, device="cuda")
        logits = torch.empty(b, frames, p["config"].num_classes, device="cuda")
        masks = ctypes.c_void_p(store.data_ptr() + 4)
        assert masks.value % 4 == 0 and masks.value % 16 != 0
        _lib.check(t._lib.kws_train_grad(t._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, frames, int(lab.shape[1]), masks, _lib.ptr(loss),
                                         _lib.ptr(grad), _lib.ptr(logits), _lib.current_stream_ptr()))
        got = [("loss", loss.cpu().numpy()), ("logits", logits.cpu().numpy())] + M.flat(weights.from_blob(p["config"], grad.cpu().numpy()))
    finally:
        t.close()
    _assert_same_bits(want, got, "drop")


def test_a_recarved_arena_gives_the_bits_of_a_fresh_handle():
    """One handle through ref_shape, t2's shape, mel60_l3's shape (smaller and larger B x T, another S_max), ref_shape again, then
    reserve() for something larger and ref_shape once more: every call the bits of a fresh handle at that shape, and the arena is
    allocated anew exactly when a shape needs more bytes than any before it."""
    p = M.make_problem("ref_shape")
    rng = np.random.default_rng(5)

    def shaped(b, frames, seq_len, labels):
        return rng.standard_normal((b, frames, p["config"].n_mel)).astype(np.float32), np.array(seq_len, np.int32), labels
    calls = {"ref_shape": (p["x"], p["seq_len"], p["labels"]), "t2": shaped(*M.CASES["t2"][4:]), "mel60_l3": shaped(*M.CASES["mel60_l3"][4:])}
    fresh, need = {}, {}
    for key, args in calls.items():
        t = _trainer(p)
        try:
            fresh[key] = _bits(t, *args)
            need[key] = t.stats()["device_bytes"]          # the handle's fixed state + the arena of this one shape
            assert t.stats()["allocs"] == 1
        finally:
            t.close()
    assert need["t2"] < need["ref_shape"] < need["mel60_l3"]
    t = _trainer(p)
    try:
        high = 0
        for key in ("ref_shape", "t2", "mel60_l3", "ref_shape"):
            before = t.stats()["allocs"]
            _assert_same_bits(fresh[key], _bits(t, *calls[key]), key)
            after = t.stats()
            assert after["allocs"] == before + (1 if need[key] > high else 0), (key, before, after)
            high = max(high, need[key])
            assert after["device_bytes"] == high, (key, after, high)
        assert t.stats()["allocs"] == 2
        t.reserve(40, 30)
        grown = t.stats()
        assert grown["allocs"] == 3 and grown["device_bytes"] > high
        _assert_same_bits(fresh["ref_shape"], _bits(t, *calls["ref_shape"]), "after reserve")
        assert t.stats()["allocs"] == 3 and t.stats()["device_bytes"] == grown["device_bytes"]
    finally:
        t.close()


def test_calls_from_two_streams_are_ordered_by_the_handle():
    """A step on one stream, a step on a second stream without synchronising in between, a gradient call on the default stream: the
    handle orders them by an event wait, so weights and gradient are the bits of the same three calls made on one stream."""
    p = M.make_problem("ref_shape")
    args = (p["x"], p["seq_len"], p["labels"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    one, two = _trainer(p), _trainer(p)
    try:
        want_loss = [one.step_raw(*args, 0.01), one.step_raw(*args, 0.01)]
        want = _bits(one, *args)
        want_w = one.weights_blob()
        with torch.cuda.stream(s1):
            l1 = two.step_raw(*args, 0.01)
        with torch.cuda.stream(s2):
            l2 = two.step_raw(*args, 0.01)
        got = _bits(two, *args)
        got_w = two.weights_blob()
        torch.cuda.synchronize()
        assert two.stats()["steps"] == 2
        for a, b in zip(want_loss, (l1, l2)):
            assert torch.equal(a, b)
    finally:
        one.close()
        two.close()
    _assert_same_bits(want, got, "two streams")
    assert np.array_equal(want_w.view(np.uint32), got_w.view(np.uint32))
    assert not np.array_equal(want_w, M.blob_of(p["w"]).astype(np.float32))          # ... and the two steps did move the weights


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
