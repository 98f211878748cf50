"""Training from and to carried states on the device (kws_train_grad_state / _step_state / kws_train_apply and the Trainer arguments
over them) against the fp64 restatement tests/train_state_model.py under the rule of tests/test_gpu_train.py: per tensor, bound =
max(4 x the deviation of the float32-CPU torch graph from fp64, 16 * 2^-23 * max|reference|).  Every comparison prints a
TRAIN-STATE-RATIO line before it asserts.  What has to hold to the bit -- the plain calls, streams that run no frame, a forward cut
into two calls, aliased and shifted state tensors, apply() behind loss_and_grad against step_raw -- is compared as uint32."""
import ctypes

import numpy as np
import pytest
import torch

import train_model as M
import train_state_model as S
import train_wrapped_model as WM
from test_gpu_train import FLOOR, _bound, _check_trajectory

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7.25)


def _report(what, name, got, ref64, ref32):
    bound, dev = _bound(ref64, ref32)
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    print("TRAIN-STATE-RATIO %s %s: kernel %.3e  float32-CPU %.3e  bound %.3e  kernel/bound %.3f" % (what, name, err, dev, bound, err / bound if bound > 0 else 0.0))
    return err, bound


def _check_all(what, name, pairs):
    """pairs: [(tensor name, got, ref64, ref32)] -> every ratio printed, then one assert."""
    over = []
    for key, got, r64, r32 in pairs:
        err, bound = _report(what + " " + key, name, got, r64, r32)
        if err > bound:
            over.append((key, err, bound))
    assert not over, over


def _grad_pairs(got, ref64, ref32):
    return [(key, g, r64, r32) for (key, g), (_, r64), (_, r32) in zip(WM.flat(got), WM.flat(ref64), WM.flat(ref32))]


def _trainer(p, **kw):
    from keyword_spotting_amd.training import Trainer
    return Trainer(p["config"], p["w"], **kw)


def _u32(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what):
    assert len(a) == len(b), what
    for (key, u), (_, v) in zip(a, b):
        assert np.array_equal(_u32(u).ravel(), _u32(v).ravel()), (what, key)


def _bits(t, p, **kw):
    """One loss_and_grad on the problem -> [(name, array)]: losses, logits, every gradient tensor [, state_out, dstate_in]."""
    args = dict(x=p["x"], lengths=p["seq_len"], labels=p["labels"], drop=p.get("drop"), want_logits=True)
    args.update(kw)
    out = t.loss_and_grad(args.pop("x"), args.pop("lengths"), args.pop("labels"), **args)
    bits = [("loss", out[2]), ("logits", out[3])] + WM.flat(out[1])
    if args.get("want_state"):
        bits += [("state_out", out[4][0]), ("dstate_in", out[4][1])]
    return bits


def _grad_state_c(t, p, io, seq_len=None):
    """kws_train_grad_state through the C entry with the kws_train_state_io given (or None) -> [(name, array)] as _bits."""
    from keyword_spotting_amd import _lib, weights
    x, b, frames, (_, sl_p), (lab, lab_p), (_, ll_p), drop = t._inputs(p["x"], p["seq_len"] if seq_len is None else seq_len, p["labels"], p.get("drop"))
    loss = torch.empty(b, device="cuda")
    grad = torch.empty(t.weights_blob().size, device="cuda")
    logits = torch.empty(b, frames, p["config"].num_classes, device="cuda")
    _lib.check(t._lib.kws_train_grad_state(t._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, frames, int(lab.shape[1]), _lib.ptr(drop), _lib.ptr(loss),
                                           _lib.ptr(grad), _lib.ptr(logits), None if io is None else ctypes.byref(io), _lib.current_stream_ptr()))
    return [("loss", loss.cpu().numpy()), ("logits", logits.cpu().numpy())] + WM.flat(weights.from_blob(p["config"], grad.cpu().numpy()))


# ---- the case table ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(S.TABLE))
def test_case_table(key):
    """Loss, logits (1e-4 as the plain calls'), every gradient tensor, state_out and dstate_in of one kws_train_grad_state."""
    p = S.make_problem(key)
    (loss64, grads64, logits64, state64, dstate64), r32 = S.reference(key)
    t = _trainer(p, keep_prob=p["keep_prob"])
    try:
        total, grads, loss, logits, (state_out, dstate_in) = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=p["drop"], want_logits=True,
                                                                            state=p["state_in"], dstate_out=p["dstate_out"], want_state=True)
        launches = t.stats()["launches"]
        t.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=p["drop"])
        assert t.stats()["launches"] == launches          # a call with state launches exactly the kernels of a call without
    finally:
        t.close()
    inf = np.isinf(loss64)
    assert np.array_equal(np.isinf(loss), inf) and inf.any() == (key == "no_path") and np.isinf(total) == inf.any()
    err = float(np.abs(logits.cpu().numpy() - logits64).max())
    print("TRAIN-STATE-RATIO logits %s: kernel %.3e  bound 1.000e-04" % (key, err))
    assert err <= 1e-4
    pairs = [("loss", np.where(inf, 0.0, loss), np.where(inf, 0.0, loss64), r32["loss"])] + _grad_pairs(grads, grads64, r32["grads"])
    pairs += [("state_out", state_out.cpu().numpy(), state64, r32["state_out"]), ("dstate_in", dstate_in.cpu().numpy(), dstate64, r32["dstate_in"])]
    _check_all("case", key, pairs)


def test_dropout_per_frame_masks():
    p = dict(S.make_problem("ref_shape"))
    p.update(drop=M.drop_masks(p, 0.6), keep_prob=0.6)
    r64, r32 = S.of_problem(p), S.torch_of_problem(p, torch.float32)
    t = _trainer(p, keep_prob=0.6)
    try:
        _, grads, loss, (state_out, dstate_in) = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], drop=p["drop"], state=p["state_in"],
                                                                 dstate_out=p["dstate_out"], want_state=True)
    finally:
        t.close()
    pairs = [("loss", loss, r64[0], r32["loss"])] + _grad_pairs(grads, r64[1], r32["grads"])
    pairs += [("state_out", state_out.cpu().numpy(), r64[3], r32["state_out"]), ("dstate_in", dstate_in.cpu().numpy(), r64[4], r32["dstate_in"])]
    _check_all("dropout", "ref_shape", pairs)


# ---- bitwise against the plain calls ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["ref_shape", "both_ref_shape"])
def test_no_state_is_the_plain_call_bitwise(key):
    from keyword_spotting_amd import _lib
    p = S.make_problem(key)
    zeros = np.zeros_like(p["state_in"])
    t = _trainer(p)
    try:
        want = _bits(t, p)
        plain_launches = t.stats()["launches"]
        _same_bits(want, _grad_state_c(t, p, None), "io = NULL")
        _same_bits(want, _grad_state_c(t, p, _lib.KwsTrainStateIo()), "all four fields NULL")
        assert t.stats()["launches"] == plain_launches
        got = _bits(t, p, state=zeros, dstate_out=zeros, want_state=True)
        assert t.stats()["launches"] == plain_launches
        _same_bits(want, got[:len(want)], "zeros given as tensors")
        only_out = _bits(t, p, want_state=True)          # state_in and dstate_out NULL, the outputs asked for
        _same_bits(got, only_out, "NULL inputs against zeros")
        assert np.abs(only_out[-2][1].cpu().numpy()).max() > 0 and np.abs(only_out[-1][1].cpu().numpy()).max() > 0
    finally:
        t.close()


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_three_state_steps_from_zeros_are_three_plain_steps_bitwise(kind):
    p = S.make_problem("ref_shape")
    one, two = _trainer(p, optimizer=kind), _trainer(p, optimizer=kind)
    try:
        zeros = one.zero_state(p["B"])
        for s in range(3):
            want = one.step_raw(p["x"], p["seq_len"], p["labels"], 0.01)
            got, (state_out, _) = two.step_raw(p["x"], p["seq_len"], p["labels"], 0.01, state=zeros, dstate_out=zeros, want_state=True)
            assert torch.equal(want, got), s
            assert np.array_equal(_u32(one.weights_blob()), _u32(two.weights_blob())), s
            assert one.stats()["launches"] == two.stats()["launches"]
        assert two.stats()["steps"] == 3 and state_out.abs().max().item() > 0
    finally:
        one.close()
        two.close()


# ---- streams and workgroups that run no frame; rows b >= B -------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["dead_group", "ref_shape", "h256"])
def test_pass_through_is_bitwise_and_nothing_is_written_behind_the_batch(key):
    """Empty slots and the workgroup without a frame copy state_in to state_out and dstate_out to dstate_in bit for bit.  All four
    tensors end in a guard row (a stream b = B of the last layer would land there) that keeps its sentinel; the outputs start as
    sentinels, so every row of a valid stream is shown to be written."""
    from keyword_spotting_amd import _lib
    p = S.make_problem(key)
    n = p["state_in"].size
    hid = p["config"].hidden_size

    def guarded(values=None):
        buf = torch.full((n + hid,), float(SENTINEL), dtype=torch.float32, device="cuda")
        if values is not None:
            buf[:n] = torch.from_numpy(values.reshape(-1)).cuda()
        return buf
    s_in, s_out, d_out, d_in = guarded(p["state_in"]), guarded(), guarded(p["dstate_out"]), guarded()
    t = _trainer(p)
    try:
        _grad_state_c(t, p, _lib.KwsTrainStateIo(s_in.data_ptr(), s_out.data_ptr(), d_out.data_ptr(), d_in.data_ptr()))
    finally:
        t.close()
    torch.cuda.synchronize()
    for name, buf in (("state_in", s_in), ("state_out", s_out), ("dstate_out", d_out), ("dstate_in", d_in)):
        assert (buf[n:].cpu().numpy() == SENTINEL).all(), name
    empty = p["seq_len"] == 0
    assert empty.any()
    if key == "dead_group":
        assert empty[16:32].all() and not empty[:16].any() and not empty[32]
    state_out, dstate_in = s_out[:n].cpu().numpy().reshape(p["state_in"].shape), d_in[:n].cpu().numpy().reshape(p["state_in"].shape)
    assert np.array_equal(_u32(state_out[:, empty]), _u32(p["state_in"][:, empty]))
    assert np.array_equal(_u32(dstate_in[:, empty]), _u32(p["dstate_out"][:, empty]))
    assert np.array_equal(_u32(s_in[:n]), _u32(p["state_in"].reshape(-1))) and np.array_equal(_u32(d_out[:n]), _u32(p["dstate_out"].reshape(-1)))
    live = ~empty
    assert (state_out[:, live] != p["state_in"][:, live]).any(axis=2).all() and (dstate_in[:, live] != p["dstate_out"][:, live]).any(axis=2).all()
    assert (state_out != SENTINEL).all() and (dstate_in != SENTINEL).all()


# ---- a forward cut into two calls ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["ref_shape", "h256"])
def test_forward_chain_is_one_call_bitwise(key):
    """Frames [0, T1) then [T1, T) from the carried state: concatenated logits and the final state are those of one call as uint32 --
    no frame's arithmetic depends on the call's T.  Streams shorter than T1 run the second call at seq_len = 0."""
    from keyword_spotting_amd.training import segment_lengths
    p = S.make_problem(key)
    none = [[]] * p["B"]
    t = _trainer(p)
    try:
        _, _, _, one_logits, (one_state, _) = t.loss_and_grad(p["x"], p["seq_len"], none, want_logits=True, state=p["state_in"], want_state=True)
        for cut in (1, 7, p["T"] - 1):
            la, lb = segment_lengths(p["seq_len"], 0, cut), segment_lengths(p["seq_len"], cut, p["T"] - cut)
            assert ((lb == 0) & (p["seq_len"] > 0)).any() or cut == 1
            _, _, _, logits_a, (sa, _) = t.loss_and_grad(p["x"][:, :cut], la, none, want_logits=True, state=p["state_in"], want_state=True)
            _, _, _, logits_b, (sb, _) = t.loss_and_grad(p["x"][:, cut:], lb, none, want_logits=True, state=sa, want_state=True)
            assert np.array_equal(_u32(torch.cat([logits_a, logits_b], dim=1)), _u32(one_logits)), cut
            assert np.array_equal(_u32(sb), _u32(one_state)), cut
    finally:
        t.close()


# ---- chained back-propagation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(S.CHAIN_CUT))
def test_chained_back_propagation(key):
    """A, then B from A's state_out (B's own state_out weighted with the case's dstate_out), then A again with dstate_out = B's
    dstate_in: grad(A) + grad(B) and A's dstate_in against the fp64 two-segment graph; the float32-CPU yardstick is the same
    two-segment torch graph.  Streams that end inside A carry their part of dstate_out through B's seq_len = 0 and A's dead frames."""
    p, (seg_a, seg_b) = S.chain_problem(key)
    r64, r32 = S.chain_reference(key)
    t = _trainer(p)
    try:
        _, _, _, (sa, _) = t.loss_and_grad(*seg_a, state=p["state_in"], want_state=True)
        _, gb, loss_b, (sb, da) = t.loss_and_grad(*seg_b, state=sa, dstate_out=p["dstate_out"], want_state=True)
        _, ga, loss_a, (_, d0) = t.loss_and_grad(*seg_a, state=p["state_in"], dstate_out=da, want_state=True)
    finally:
        t.close()
    pairs = [("loss", np.array([loss_a, loss_b]), r64["loss"], r32["loss"])] + _grad_pairs(S.add_grads(p["w"], ga, gb), r64["grads"], r32["grads"])
    pairs += [("state_out", sb.cpu().numpy(), r64["state_out"], r32["state_out"]), ("dstate_in", d0.cpu().numpy(), r64["dstate_in"], r32["dstate_in"])]
    _check_all("chain", key, pairs)
    assert da.abs().max().item() > 0


# ---- against serving ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["t2", "odd_mel", "ref_shape", "mel60_l3"])
def test_forward_against_serving_from_the_same_state(name):
    """At full length from the same random state: logits and state_out against DeployModel.forward's at the 2e-5 the two forwards are
    held to from the zero state (tests/test_gpu_train.py)."""
    from keyword_spotting_amd.rnn_ctc import DeployModel
    p = M.make_problem(name)
    cfg = p["config"]
    state = np.random.default_rng(9).uniform(-0.9, 0.9, (cfg.num_layers, p["B"], cfg.hidden_size)).astype(np.float32)
    t = _trainer(p)
    try:
        _, _, _, logits, (state_out, _) = t.loss_and_grad(p["x"], None, [[]] * p["B"], want_logits=True, state=state, want_state=True)
    finally:
        t.close()
    m = DeployModel(cfg, p["w"])
    try:
        served = m.forward(torch.from_numpy(p["x"]), torch.from_numpy(state), want_softmax=False)
        e_logits = float((served["logits"] - logits).abs().max().item())
        e_state = float((served["state"] - state_out).abs().max().item())
    finally:
        m.close()
    print("TRAIN-STATE-RATIO vs kws_step %s: logits %.3e  state %.3e  bound 2.000e-05" % (name, e_logits, e_state))
    assert e_logits <= 2e-5 and e_state <= 2e-5


# ---- apply ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip", ["active", "inactive"])
@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_apply_behind_loss_and_grad_is_step_raw_bitwise(kind, clip):
    p = S.make_problem("ref_shape")
    probe = _trainer(p)
    try:
        norm64 = M.global_norm(probe.loss_and_grad(p["x"], p["seq_len"], p["labels"])[1])
    finally:
        probe.close()
    kw = dict(optimizer=kind, max_grad_norm={"active": 0.5, "inactive": 4.0}[clip] * norm64)
    one, two = _trainer(p, **kw), _trainer(p, **kw)
    try:
        for s in range(3):
            _, want_norm = one.step_raw(p["x"], p["seq_len"], p["labels"], 0.01, want_norm=True)
            _, grads, _ = two.loss_and_grad(p["x"], p["seq_len"], p["labels"])
            norm = two.apply(grads, lr=0.01)
            assert two.stats()["launches"] == 3
            assert torch.equal(norm, want_norm), s
            assert s > 0 or abs(float(norm.item()) - norm64) <= FLOOR * norm64
            assert np.array_equal(_u32(one.weights_blob()), _u32(two.weights_blob())), s
        assert one.stats()["steps"] == two.stats()["steps"] == 3 and two.global_step == 0
        for mine, theirs in zip(one.moments(), two.moments()):
            for (key, a), (_, b) in zip(M.flat(mine), M.flat(theirs)):
                assert (a == b).all(), key
    finally:
        one.close()
        two.close()


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_apply_of_a_chains_summed_gradient_is_the_fp64_update(kind):
    """... of that device gradient, within the floor test_one_step_is_the_fp64_update_of_the_devices_own_gradient uses; apply() with the
    schedule advances global_step and takes a device blob as well as the dict."""
    p, (seg_a, seg_b) = S.chain_problem("ref_shape")
    t = _trainer(p, optimizer=kind, learning_rate=0.01, lr_decay=0.5, decay_step=1)
    try:
        _, _, _, (sa, _) = t.loss_and_grad(*seg_a, state=p["state_in"], want_state=True)
        _, gb, _, (_, da) = t.loss_and_grad(*seg_b, state=sa, want_state=True)
        _, ga, _, _ = t.loss_and_grad(*seg_a, state=p["state_in"], dstate_out=da, want_state=True)
        from keyword_spotting_amd import weights
        summed = weights.to_blob(p["config"], ga) + weights.to_blob(p["config"], gb)          # float32, as a caller on the device would add
        g = weights.from_blob(p["config"], summed)
        opt, w = M.Optimizer(p["w"], kind), p["w"]
        for s, form in enumerate((g, torch.from_numpy(summed).cuda())):
            t.apply(form)
            w = opt.apply(w, g, 0.01 * 0.5 ** s)
            for (key, a), (_, r) in zip(M.flat(t.weights()), M.flat(w)):
                err, floor = float(np.abs(a - r).max()), (s + 1) * FLOOR * float(np.abs(r).max())
                print("TRAIN-STATE-RATIO apply %s step %d %s: kernel %.3e  floor %.3e" % (kind, s, key, err, floor))
                assert err <= floor, (s, key, err, floor)
        assert t.global_step == 2 and t.stats()["steps"] == 2
    finally:
        t.close()


# ---- trajectories ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_twenty_carried_steps_follow_the_restatement(kind):
    """step(..., state = the previous step's state_out) twenty times against the restatement run the same way, under _check_trajectory."""
    steps, lr = 20, M.TRAJECTORY_LR[kind]
    p = S.make_problem("ref_shape")
    loss64, path64 = S.trajectory("ref_shape", kind, steps, lr)
    loss32, path32 = S.trajectory("ref_shape", kind, steps, lr, float32=True)
    t = _trainer(p, optimizer=kind, learning_rate=lr, lr_decay=1.0)
    got_loss, got_path, state = [], [], None
    try:
        for _ in range(steps):
            total, state = t.step(p["x"], p["seq_len"], p["labels"], state=state, want_state=True)
            got_path.append(t.weights_blob())
            got_loss.append(None)
        # step() returns the mean; the per-utterance losses of the same trajectory through step_raw on a twin
        twin = _trainer(p, optimizer=kind)
        try:
            state = None
            for s in range(steps):
                got_loss[s], (state, _) = twin.step_raw(p["x"], p["seq_len"], p["labels"], lr, state=state, want_state=True)
                got_loss[s] = got_loss[s].cpu().numpy()
                assert np.array_equal(_u32(twin.weights_blob()), _u32(got_path[s])), s
        finally:
            twin.close()
        assert t.global_step == steps
    finally:
        t.close()
    _check_trajectory("carried twenty steps ref_shape %s" % kind, got_loss, got_path, loss64, path64, loss32, path32)


def test_state_noise_draws_after_the_dropout_draws():
    """Trainer(state_noise=0.3, keep_prob=0.6): a twin of the same seed gives the same bits; a third trainer fed the draws made here in
    the documented order (x mask, output masks, then randn [L,B,H]) through step_raw does too; and the noise is live."""
    p = S.make_problem("ref_shape")
    cfg, seed, keep = p["config"], 5, 0.6
    kw = dict(keep_prob=keep, learning_rate=0.01, lr_decay=1.0)
    a, b, c, quiet = (_trainer(p, seed=seed, state_noise=0.3, **kw), _trainer(p, seed=seed, state_noise=0.3, **kw), _trainer(p, seed=seed + 1, **kw),
                      _trainer(p, seed=seed, **kw))
    try:
        gen = torch.Generator(device=a.device)
        gen.manual_seed(seed)
        x = torch.from_numpy(p["x"]).to(a.device)
        for s in range(2):
            la, lb, lq = a.step(p["x"], p["seq_len"], p["labels"]), b.step(p["x"], p["seq_len"], p["labels"]), quiet.step(p["x"], p["seq_len"], p["labels"])
            mask = torch.floor(keep + torch.rand(x.shape, generator=gen, device=a.device))
            drop = torch.floor(keep + torch.rand((cfg.num_layers, p["B"], p["T"], cfg.hidden_size), generator=gen, device=a.device)).to(torch.uint8)
            h0 = 0.3 * torch.randn((cfg.num_layers, p["B"], cfg.hidden_size), generator=gen, device=a.device)
            c.step_raw(x / keep * mask, p["seq_len"], p["labels"], 0.01, drop=drop, state=h0)
            assert la == lb and la != lq, s
            wa = a.weights_blob()
            assert np.array_equal(_u32(wa), _u32(b.weights_blob())) and np.array_equal(_u32(wa), _u32(c.weights_blob())), s
            assert h0.abs().max().item() > 0.3 and not np.array_equal(wa, quiet.weights_blob())
    finally:
        for t in (a, b, c, quiet):
            t.close()


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------

def test_shifted_and_aliased_state_tensors_give_the_same_bits():
    """State tensors 16 bytes past a 256-byte boundary; state_out in state_in's memory and dstate_in in dstate_out's."""
    from keyword_spotting_amd import _lib
    p = S.make_problem("ref_shape")
    n = p["state_in"].size

    def shifted(values=None):
        store = torch.zeros(4 + n, dtype=torch.float32, device="cuda")
        view = store[4:]
        assert store.data_ptr() % 256 == 0 and view.data_ptr() % 256 == 16
        if values is not None:
            view.copy_(torch.from_numpy(values.reshape(-1)))
        return view
    t = _trainer(p)
    try:
        want = _bits(t, p, state=p["state_in"], dstate_out=p["dstate_out"], want_state=True)
        s_in, s_out, d_out, d_in = shifted(p["state_in"]), shifted(), shifted(p["dstate_out"]), shifted()
        got = _grad_state_c(t, p, _lib.KwsTrainStateIo(s_in.data_ptr(), s_out.data_ptr(), d_out.data_ptr(), d_in.data_ptr()))
        _same_bits(want, got + [("state_out", s_out), ("dstate_in", d_in)], "16 bytes past a 256-byte boundary")
        a, d = torch.from_numpy(p["state_in"]).cuda(), torch.from_numpy(p["dstate_out"]).cuda()
        got = _grad_state_c(t, p, _lib.KwsTrainStateIo(a.data_ptr(), a.data_ptr(), d.data_ptr(), d.data_ptr()))
        _same_bits(want, got + [("state_out", a), ("dstate_in", d)], "aliased")
    finally:
        t.close()


def test_steady_state_allocates_nothing():
    p = S.make_problem("ref_shape")
    t = _trainer(p)
    try:
        assert t.stats()["allocs"] == 0
        _, state = t.step(p["x"], p["seq_len"], p["labels"], want_state=True)
        first = t.stats()
        for _ in range(3):
            _, state = t.step(p["x"], p["seq_len"], p["labels"], state=state, want_state=True)
        _, grads, _, (_, d) = t.loss_and_grad(p["x"], p["seq_len"], p["labels"], state=state, want_state=True)
        t.loss_and_grad(p["x"], p["seq_len"], p["labels"], dstate_out=d)
        t.apply(grads, lr=0.01)
        last = t.stats()
    finally:
        t.close()
    assert first["allocs"] == 1 and last["allocs"] == 1 and last["device_bytes"] == first["device_bytes"] and last["steps"] == 5


def test_refusals():
    from keyword_spotting_amd import _lib
    p = S.make_problem("t2")
    cfg = p["config"]
    t = _trainer(p)
    try:
        store = torch.zeros(p["state_in"].size + 4, dtype=torch.float32, device="cuda")
        for i, field in enumerate(("state_in", "state_out", "dstate_out", "dstate_in")):
            ptrs = [None] * 4
            ptrs[i] = store.data_ptr() + 4
            with pytest.raises(_lib.InvalidArgumentError, match="io->%s must be 16-byte aligned" % field):
                _grad_state_c(t, p, _lib.KwsTrainStateIo(*ptrs))
        with pytest.raises(_lib.InvalidArgumentError, match=r"state must be \[1,1,64\]"):
            t.loss_and_grad(p["x"], p["seq_len"], p["labels"], state=np.zeros((1, 2, 64), np.float32))
        with pytest.raises(_lib.InvalidArgumentError, match=r"dstate_out must be \[1,1,64\]"):
            t.step_raw(p["x"], p["seq_len"], p["labels"], 0.01, dstate_out=np.zeros((1, 1, 32), np.float32))
        with pytest.raises(_lib.InvalidArgumentError, match=r"labels\[0\]\[1\]=2"):
            t.loss_and_grad(p["x"], p["seq_len"], [[0, 2]], state=p["state_in"])
        with pytest.raises(_lib.InvalidArgumentError, match="lr="):
            t.step_raw(p["x"], p["seq_len"], p["labels"], 0.0, state=p["state_in"])
        with pytest.raises(_lib.InvalidArgumentError, match="lr="):
            t.apply(t.weights(), lr=float("inf"))
        with pytest.raises(_lib.InvalidArgumentError, match="the gradient has 3 floats"):
            t.apply(np.zeros(3, np.float32), lr=0.01)
        assert t._lib.kws_train_apply(t._handle, None, 0.01, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT and b"null pointer" in t._lib.kws_last_error()
        assert t.stats()["allocs"] == 0 and t.stats()["steps"] == 0 and t.global_step == 0          # nothing ran
        assert tuple(t.zero_state(3).shape) == (cfg.num_layers, 3, cfg.hidden_size) and not t.zero_state(3).any()
        assert np.isfinite(t.loss_and_grad(p["x"], p["seq_len"], p["labels"], state=p["state_in"])[0])
    finally:
        t.close()
