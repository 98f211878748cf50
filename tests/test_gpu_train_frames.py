"""Both trainers on frame-wise targets (kws_train_*_frames, kws_attention_train_*_frames; loss_and_grad_frames, step_frames and
step_raw(targets=) of Trainer and AttentionTrainer) against the torch graphs of tests/frame_loss_model.py in float64, with the same graph in float32 on the CPU as the yardstick: per
tensor, bound = max(4 x that deviation, 16 * 2^-23 * max|reference|), as tests/test_gpu_train.py and tests/test_gpu_attention_train.py.
Every comparison prints a FRAMES-RATIO line (kernel / float32-CPU / bound) before it asserts.  What has to hold to the bit -- the new
calls at frame_weight 0 against the plain ones, the frame term added onto a CTC gradient of zeros against the frame term written -- is
compared as uint32."""
import ctypes

import numpy as np
import pytest
import torch

import attention_train_model as AM
import frame_loss_model as F
import train_model as M
import train_state_model as SM
import train_wrapped_model as WM

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -23


def _report(what, name, got, ref64, ref32):
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    bound = max(4.0 * dev, FLOOR * (float(np.abs(ref64).max()) if np.size(ref64) else 0.0))
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max()) if np.size(ref64) else 0.0
    print("FRAMES-RATIO %s %s: kernel %.3e  float32-CPU %.3e  bound %.3e  kernel/bound %.3f" % (what, name, err, dev, bound, err / bound if bound > 0 else 0.0))
    return err, bound


def _check(what, name, pairs):
    """pairs: [(key, got, ref64, ref32)] -> every one reported, then all asserted."""
    worst = []
    for key, got, r64, r32 in pairs:
        err, bound = _report(what + " " + key, name, got, r64, r32)
        if not err <= bound:
            worst.append((key, err, bound))
    assert not worst, worst


def _grad_pairs(flat, got, r64, r32):
    return [(k, g, a, b) for (k, g), (_, a), (_, b) in zip(flat(got), flat(r64), flat(r32))]


def _trainer(p, objective="mixed", weight=None, **kw):
    from keyword_spotting_amd.training import Trainer
    cw, fw, _ = F.OBJECTIVES[objective]
    return Trainer(p["config"], p["w"], ctc_weight=cw, frame_weight=fw, class_weight=weight, **kw)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bits(t, p, **kw):
    """One loss_and_grad -> [(name, array)]: the per-utterance losses, the logits and every gradient tensor."""
    _, g, loss, logits = t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], kw.pop("targets", None), want_logits=True, **kw)[:4]
    return [("loss", loss), ("logits", logits.cpu().numpy())] + WM.flat(g)


def _assert_same_bits(a, b, what):
    assert len(a) == len(b)
    for (key, u), (_, v) in zip(a, b):
        assert u.shape == v.shape and np.array_equal(_u32(u), _u32(v)), (what, key)


def test_new_entry_points_exist():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_frame_loss", "kws_sizeof_frame_targets", "kws_train_grad_frames", "kws_train_step_frames", "kws_train_check_frames",
                "kws_attention_train_grad_frames", "kws_attention_train_step_frames", "kws_attention_train_check_frames"):
        assert hasattr(lib, sym), sym


# ---- the GRU trainer -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("objective", sorted(F.OBJECTIVES))
@pytest.mark.parametrize("name", F.GRU_CASES)
def test_gru_gradients_against_the_torch_graph(name, objective):
    """Random targets with runs of -1; frames only (labels None), the CTC loss alone through the new call, and ctc + 0.5 ce with class
    weights: loss, ce, logits and every gradient tensor."""
    p = M.make_problem(name)
    r64, r32, targets, weight = F.gru_reference(name, objective)
    t = _trainer(p, objective, weight)
    try:
        labels = None if objective == "frames" else p["labels"]
        total, grads, loss, logits, ce = t.loss_and_grad_frames(p["x"], p["seq_len"], labels, targets, want_logits=True,
                                                         want_frame_loss=objective != "ctc")[:5] + ((None,) if objective == "ctc" else ())
    finally:
        t.close()
    assert np.isfinite(loss).all() and total == float(loss.astype(np.float64).sum() / p["B"])
    pairs = [("loss", loss, r64["loss"], r32["loss"]), ("logits", logits.cpu().numpy(), r64["logits"], r32["logits"])]
    if ce is not None:
        pairs.append(("ce", ce.cpu().numpy(), r64["ce"], r32["ce"]))
    _check("gru %s" % objective, name, pairs + _grad_pairs(M.flat, grads, r64["grads"], r32["grads"]))
    assert (loss[p["seq_len"] == 0] == 0).all()


@pytest.mark.parametrize("name", ["odd_mel", "ref_shape"])
def test_frame_weight_zero_is_the_plain_call_bitwise(name):
    """ctc_weight 1, frame_weight 0 through kws_train_grad_frames / kws_train_step_frames: the plain calls' launches and bits -- loss,
    logits, every gradient tensor; after one step the weights and both moments.  A trainer built with a mixed objective that is
    given no targets makes the plain call too."""
    p = M.make_problem(name)
    targets = F.gru_targets(p)
    plain, framed, mixed = _trainer(p, "ctc"), _trainer(p, "ctc"), _trainer(p, "mixed", F.class_weights(p["config"].num_classes))
    try:
        want = _bits(plain, p)
        launches = plain.stats()["launches"]
        got = _bits(framed, p, targets=targets)
        assert framed.stats()["launches"] == launches
        _assert_same_bits(want, got, "grad")
        _assert_same_bits(want, _bits(mixed, p), "no targets")
        assert mixed.stats()["launches"] == launches
        l0 = plain.step_raw(p["x"], p["seq_len"], p["labels"], 0.01)
        l1 = framed.step_raw(p["x"], p["seq_len"], p["labels"], 0.01, targets=targets)
        l2 = mixed.step_raw(p["x"], p["seq_len"], p["labels"], 0.01)
        assert torch.equal(l0, l1) and torch.equal(l0, l2)
        w0 = plain.weights_blob()
        assert np.array_equal(_u32(w0), _u32(framed.weights_blob())) and np.array_equal(_u32(w0), _u32(mixed.weights_blob()))
        for a, b in zip(plain.moments(), framed.moments()):
            for (key, u), (_, v) in zip(M.flat(a), M.flat(b)):
                assert np.array_equal(_u32(u), _u32(v)), key
    finally:
        plain.close(); framed.close(); mixed.close()


def test_the_frame_term_added_onto_zeros_is_the_frame_term_written():
    """Accumulate mode against write mode.  Every utterance gets a transcript with no valid path (seven repeats in at most nine frames):
    the CTC term leaves a gradient of exactly 0 and a loss of +inf, so ctc + ce adds the frame rows onto zeros and has to give the
    gradient bits of ce alone, which writes them."""
    p = M.make_problem("odd_mel")
    targets = F.gru_targets(p)
    weight = F.class_weights(p["config"].num_classes)
    no_path = [[1] * 7] * p["B"]
    from keyword_spotting_amd.training import Trainer
    mixed = Trainer(p["config"], p["w"], ctc_weight=1.0, frame_weight=1.0, class_weight=weight)
    frames = Trainer(p["config"], p["w"], ctc_weight=0.0, frame_weight=1.0, class_weight=weight)
    try:
        _, g_mixed, loss_mixed, ce_mixed = mixed.loss_and_grad_frames(p["x"], p["seq_len"], no_path, targets, want_frame_loss=True)
        _, g_frames, loss_frames, ce_frames = frames.loss_and_grad_frames(p["x"], p["seq_len"], None, targets, want_frame_loss=True)
    finally:
        mixed.close(); frames.close()
    assert np.isposinf(loss_mixed).all() and np.isfinite(loss_frames).all() and torch.equal(ce_mixed, ce_frames)
    assert np.array_equal(_u32(loss_frames), _u32(ce_frames.cpu().numpy()))
    for (key, a), (_, b) in zip(M.flat(g_mixed), M.flat(g_frames)):
        assert np.abs(b).max() > 0 and np.array_equal(_u32(a), _u32(b)), key


def test_a_target_out_of_range_on_the_device_gives_a_nan_loss_and_no_poisoned_gradient():
    p = M.make_problem("odd_mel")
    targets = F.gru_targets(p)
    bad, none = targets.copy(), targets.copy()
    bad[1, 2], none[1, 2] = p["config"].num_classes, -1
    t = _trainer(p, "mixed")
    try:
        _, g_want, loss_want = t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], none)
        _, g_got, loss_got = t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], torch.from_numpy(bad).cuda())
    finally:
        t.close()
    assert np.isnan(loss_got[1]) and np.array_equal(_u32(np.delete(loss_got, 1)), _u32(np.delete(loss_want, 1)))
    for (key, a), (_, b) in zip(M.flat(g_got), M.flat(g_want)):
        assert np.isfinite(a).all() and np.array_equal(_u32(a), _u32(b)), key


def test_wrapped_handle_against_the_torch_graph():
    """Layer norm and residual (kws_train_create_wrapped), the mixed objective with class weights."""
    p = WM.make_problem("both_ref_shape")
    cw, fw, _ = F.OBJECTIVES["mixed"]
    targets, weight = F.gru_targets(p), F.class_weights(p["config"].num_classes)
    args = (p["w"], p["x"], p["seq_len"], p["labels"], targets)
    kw = dict(ctc_weight=cw, frame_weight=fw, class_weight=weight, ln=p["ln"], res=p["res"])
    r64, r32 = F.gru_torch(*args, torch.float64, **kw), F.gru_torch(*args, torch.float32, **kw)
    t = _trainer(p, "mixed", weight)
    try:
        _, grads, loss, logits, ce = t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], targets, want_logits=True, want_frame_loss=True)
    finally:
        t.close()
    assert p["ln"] and p["res"]
    pairs = [("loss", loss, r64["loss"], r32["loss"]), ("ce", ce.cpu().numpy(), r64["ce"], r32["ce"]),
             ("logits", logits.cpu().numpy(), r64["logits"], r32["logits"])]
    _check("wrapped mixed", "both_ref_shape", pairs + _grad_pairs(WM.flat, grads, r64["grads"], r32["grads"]))


@pytest.mark.parametrize("objective", ["frames", "mixed"])
def test_carried_state_handle_against_the_torch_graph(objective):
    """state, dstate_out and want_state through kws_train_grad_frames: J = sum_b loss_b / B + <dstate_out, state_out>."""
    p = SM.make_problem("ref_shape")
    cw, fw, weighted = F.OBJECTIVES[objective]
    targets, weight = F.gru_targets(p), F.class_weights(p["config"].num_classes, weighted)
    args = (p["w"], p["x"], p["seq_len"], p["labels"], targets)
    kw = dict(ctc_weight=cw, frame_weight=fw, class_weight=weight, state_in=p["state_in"], dstate_out=p["dstate_out"])
    r64, r32 = F.gru_torch(*args, torch.float64, **kw), F.gru_torch(*args, torch.float32, **kw)
    t = _trainer(p, objective, weight)
    try:
        _, grads, loss, (state_out, dstate_in), ce = t.loss_and_grad_frames(p["x"], p["seq_len"], None if cw == 0 else p["labels"], targets,
                                                                     state=p["state_in"], dstate_out=p["dstate_out"], want_state=True,
                                                                     want_frame_loss=True)
    finally:
        t.close()
    pairs = [("loss", loss, r64["loss"], r32["loss"]), ("ce", ce.cpu().numpy(), r64["ce"], r32["ce"]),
             ("state_out", state_out.cpu().numpy(), r64["state_out"], r32["state_out"]),
             ("dstate_in", dstate_in.cpu().numpy(), r64["dstate_in"], r32["dstate_in"])]
    _check("state %s" % objective, "ref_shape", pairs + _grad_pairs(M.flat, grads, r64["grads"], r32["grads"]))


def test_launch_counts_and_a_steady_state_that_allocates_nothing():
    """stats()["launches"]: frames only = plain - 1, mixed = plain + 1, at two T; repeated calls at a shape the arena has seen allocate
    nothing, whichever objective."""
    p = M.make_problem("ref_shape")
    targets = F.gru_targets(p)
    counts = {}
    for frames in (p["T"], 7):
        x, seq, tg = p["x"][:, :frames], np.minimum(p["seq_len"], frames), targets[:, :frames]
        for objective in ("ctc", "frames", "mixed"):
            t = _trainer(p, objective)
            try:
                t.loss_and_grad(x, seq, p["labels"])
                plain = t.stats()["launches"]
                t.loss_and_grad_frames(x, seq, p["labels"], tg)
                allocs = t.stats()["allocs"]
                for _ in range(3):
                    t.loss_and_grad_frames(x, seq, p["labels"], tg)
                    t.step_raw(x, seq, p["labels"], 1e-3, targets=tg)
                assert t.stats()["allocs"] == allocs, (objective, frames)
                t.loss_and_grad_frames(x, seq, p["labels"], tg)
                counts[objective, frames] = (plain, t.stats()["launches"])
            finally:
                t.close()
    for frames in (p["T"], 7):
        plain = counts["ctc", frames][0]
        assert counts["ctc", frames] == (plain, plain) and counts["frames", frames] == (plain, plain - 1) and counts["mixed", frames] == (plain, plain + 1), counts
    assert counts["ctc", 7] == counts["ctc", p["T"]]          # independent of T


def test_long_utterances_train_on_frames_where_the_ctc_kernel_has_no_room():
    """T = 2000 at hidden 64: the plain call refuses a seven-label transcript on the CTC kernel's LDS (4 x 2000 x (8 + 15) bytes), the
    frames-only call has no such limit.  ce against the restatement: the forward's logits are held to 1e-4 (tests/test_gpu_train.py), and
    ce moves by at most twice the largest change of a logit, so 2e-4 plus the bound's floor."""
    from keyword_spotting_amd import _lib, weights
    from keyword_spotting_amd.training import Trainer
    cfg = M.config_of(64, 1, 8, 6)
    rng = np.random.default_rng(21)
    b, frames = 2, 2000
    x = rng.standard_normal((b, frames, 8)).astype(np.float32)
    seq_len = np.array([frames, 1501], np.int32)
    targets = F.random_targets(rng, seq_len, frames, 6)
    w = weights.init_weights(cfg, seed=2)
    t = Trainer(cfg, w, ctc_weight=0.0, frame_weight=1.0)
    try:
        with pytest.raises(_lib.UnsupportedError, match="LDS"):
            t.loss_and_grad(x, seq_len, [[0, 1, 2, 3, 4, 0, 1]] * b)
        total, grads, loss, ce = t.loss_and_grad_frames(x, seq_len, None, targets, want_frame_loss=True)
    finally:
        t.close()
    want = F.gru_loss_and_grad(w, x, seq_len, None, targets, 0.0, 1.0)
    err = float(np.abs(ce.cpu().numpy() - want["ce"]).max())
    bound = 2e-4 + FLOOR * float(np.abs(want["ce"]).max())
    print("FRAMES-RATIO long ce: kernel %.3e  bound %.3e" % (err, bound))
    assert err <= bound and np.array_equal(_u32(loss), _u32(ce.cpu().numpy()))
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for _, g in M.flat(grads))


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_one_step_is_the_fp64_update_of_the_devices_own_gradient(kind):
    """... of the mixed objective, within the bound's floor per tensor, as tests/test_gpu_train.py does it for the plain step."""
    p = M.make_problem("ref_shape")
    targets, weight = F.gru_targets(p), F.class_weights(p["config"].num_classes)
    lr = 0.01
    t = _trainer(p, "mixed", weight, optimizer=kind)
    try:
        _, g, _ = t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], targets)
        _, norm = t.step_raw(p["x"], p["seq_len"], p["labels"], lr, want_norm=True, targets=targets)
        after = t.weights()
        assert t.stats()["steps"] == 1
    finally:
        t.close()
    norm64 = M.global_norm(g)
    assert abs(float(norm.item()) - norm64) <= FLOOR * norm64
    want = M.Optimizer(p["w"], kind).apply(p["w"], g, lr)
    for (key, a), (_, r) in zip(M.flat(after), M.flat(want)):
        err, floor = float(np.abs(a - r).max()), FLOOR * float(np.abs(r).max())
        print("FRAMES-RATIO one step %s %s: kernel %.3e  floor %.3e" % (kind, key, err, floor))
        assert err <= floor, (key, err, floor)


def test_twenty_mixed_steps_follow_the_restatement():
    """Losses and parameters after every step of frame_loss_model.TRAJECTORY against the fp64 restatement.  The yardstick at step s is the
    largest deviation the float32 torch trajectory has shown up to s; bound_s = max(4 x that, s x floor), as tests/test_gpu_train.py."""
    tr = F.TRAJECTORY
    p = M.make_problem(tr["name"])
    targets, weight = F.gru_targets(p), F.class_weights(p["config"].num_classes)
    (loss64, path64), (loss32, path32) = F.gru_trajectory(), F.gru_trajectory(float32=True)
    t = _trainer(p, tr["objective"], weight, optimizer=tr["kind"])
    got_loss, got_path = [], []
    try:
        for _ in range(tr["steps"]):
            got_loss.append(t.step_raw(p["x"], p["seq_len"], p["labels"], tr["lr"], targets=targets).cpu().numpy())
            got_path.append(t.weights_blob())
    finally:
        t.close()
    dev_l = dev_w = worst = 0.0
    for s in range(tr["steps"]):
        dev_l = max(dev_l, float(np.abs(loss32[s] - loss64[s]).max()))
        dev_w = max(dev_w, float(np.abs(path32[s] - path64[s]).max()))
        b_l = max(4 * dev_l, (s + 1) * FLOOR * float(np.abs(loss64[s]).max()))
        b_w = max(4 * dev_w, (s + 1) * FLOOR * float(np.abs(path64[s]).max()))
        e_l, e_w = float(np.abs(got_loss[s] - loss64[s]).max()), float(np.abs(got_path[s] - path64[s]).max())
        worst = max(worst, e_l / b_l, e_w / b_w)
        assert e_l <= b_l and e_w <= b_w, (s, e_l, b_l, e_w, b_w)
    print("FRAMES-RATIO twenty mixed steps: worst kernel/bound %.3f (float32-CPU drift: loss %.3e, parameters %.3e)" % (worst, dev_l, dev_w))


# ---- the attention trainer -------------------------------------------------------------------------------------------------------------

def _attention_trainer(p, objective, weight, **kw):
    from keyword_spotting_amd.attention_training import AttentionTrainer
    cw, fw, _ = F.OBJECTIVES[objective]
    return AttentionTrainer(p["config"], p["w"], ctc_weight=cw, frame_weight=fw, class_weight=weight, **kw)


@pytest.mark.parametrize("name", sorted(F.ATTENTION_CASES))
def test_attention_gradients_against_the_torch_graph(name):
    """Targets [B,T'] with runs of -1: frames only on c2 (an empty slot, relu on the logits), mixed with class weights on c4 (C = 8) and,
    with dropout at keep 0.9 on all three sites, on head32."""
    objective, keep = F.ATTENTION_CASES[name]
    p = AM.make_problem(name)
    seed = AM.drop_seed_for(name, keep)[0] if keep < 1.0 else 0
    cw, fw, weighted = F.OBJECTIVES[objective]
    cfg = p["config"]
    targets, weight = F.attention_targets(p), F.class_weights(cfg.num_classes, weighted)
    args = (cfg, p["w"], p["x"], p["seq_len"], p["labels"], targets)
    kw = dict(ctc_weight=cw, frame_weight=fw, class_weight=weight, seed=seed, keep_prob=keep)
    r64, r32 = F.attention_torch(*args, torch.float64, **kw), F.attention_torch(*args, torch.float32, **kw)
    t = _attention_trainer(p, objective, weight, keep_prob=keep)
    try:
        plain_launches = None
        if cw > 0:
            t.loss_and_grad(p["x"], p["seq_len"], p["labels"], seed=seed)
            plain_launches = t.stats()["launches"]
        _, grads, loss, logits, ce = t.loss_and_grad_frames(p["x"], p["seq_len"], None if cw == 0 else p["labels"], targets, seed=seed,
                                                            want_logits=True, want_frame_loss=True)
        launches = t.stats()["launches"]
    finally:
        t.close()
    assert plain_launches is None or launches == plain_launches + 1
    pairs = [("loss", loss, r64["loss"], r32["loss"]), ("ce", ce.cpu().numpy(), r64["ce"], r32["ce"]),
             ("logits", logits.cpu().numpy(), r64["logits"], r32["logits"])]
    _check("attention %s" % objective, name, pairs + _grad_pairs(AM.flat, grads, r64["grads"], r32["grads"]))


def test_attention_frame_weight_zero_is_the_plain_call_bitwise():
    p = AM.make_problem("c2")
    targets = F.attention_targets(p)
    plain, framed = _attention_trainer(p, "ctc", None), _attention_trainer(p, "ctc", None)
    try:
        _, g0, l0, lg0 = plain.loss_and_grad(p["x"], p["seq_len"], p["labels"], want_logits=True)
        _, g1, l1, lg1 = framed.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], targets, want_logits=True)
        assert plain.stats()["launches"] == framed.stats()["launches"]
        s0 = plain.step_raw(p["x"], p["seq_len"], p["labels"], 1e-3)
        s1 = framed.step_raw(p["x"], p["seq_len"], p["labels"], 1e-3, targets=targets)
        w0, w1 = plain.weights_blob(), framed.weights_blob()
    finally:
        plain.close(); framed.close()
    assert np.array_equal(_u32(l0), _u32(l1)) and torch.equal(lg0, lg1) and torch.equal(s0, s1) and np.array_equal(_u32(w0), _u32(w1))
    for (key, a), (_, b) in zip(AM.flat(g0), AM.flat(g1)):
        assert np.array_equal(_u32(a), _u32(b)), key


def test_attention_frames_only_is_one_launch_fewer():
    p = AM.make_problem("c2")
    t = _attention_trainer(p, "frames", None)
    try:
        t.loss_and_grad(p["x"], p["seq_len"], p["labels"])
        plain = t.stats()["launches"]
        t.loss_and_grad_frames(p["x"], p["seq_len"], None, F.attention_targets(p))
        assert t.stats()["launches"] == plain - 1
    finally:
        t.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------

def test_align_then_train_on_the_frame_labels_end_to_end():
    """A CTC-trained toy model's logits -> ctc_align on the device -> frame_labels -> a fresh Trainer(frame_weight=1, ctc_weight=0) trained
    on those targets alone with the settings tests/test_frame_loss_host.py established -> deploy() -> ctc_predict finds "12" in all 16."""
    from keyword_spotting_amd.custom_keyword import ctc_align, frame_labels
    from keyword_spotting_amd.prediction import ctc_decode2, ctc_predict
    from keyword_spotting_amd.training import Trainer
    p = M.toy_task(0)
    c = M.TOY["C"]
    teacher = Trainer(p["config"], p["w"], learning_rate=M.TOY["lr"], lr_decay=1.0)
    try:
        for _ in range(M.TOY["steps"]):
            teacher.step(p["x"], p["seq_len"], p["labels"])
        logits = teacher.loss_and_grad(p["x"], p["seq_len"], p["labels"], want_logits=True)[3]
    finally:
        teacher.close()
    targets = frame_labels(ctc_align(logits, p["seq_len"], p["labels"]).states, p["labels"], c - 1)
    assert targets.shape == (p["B"], p["T"]) and ((targets >= 0) & (targets < c)).all()
    student = Trainer(p["config"], p["w"], learning_rate=F.TOY_FRAMES["lr"], lr_decay=1.0, frame_weight=1.0, ctc_weight=0.0,
                      class_weight=F.TOY_FRAMES["class_weight"])
    try:
        losses = [student.step_frames(p["x"], p["seq_len"], None, targets) for _ in range(F.TOY_FRAMES["steps"])]
        model = student.deploy()
    finally:
        student.close()
    try:
        sm = model.forward(torch.from_numpy(p["x"]), model.zero_state(p["B"]), want_logits=False)["softmax"]
        hits = [ctc_predict(ctc_decode2(sm[i], c), M.TOY["label"]) for i in range(p["B"])]
    finally:
        model.close()
    print("FRAMES-RATIO toy task on frame labels: loss %.4f -> %.4f in %d steps, %d of %d recognised"
          % (losses[0], losses[-1], len(losses), sum(hits), len(hits)))
    assert losses[-1] < 0.1 * losses[0] and all(h == 1 for h in hits), hits


# ---- refusals behind the device check --------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_handle():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.training import Trainer
    p = M.make_problem("odd_mel")
    targets = F.gru_targets(p)
    t = _trainer(p, "mixed")
    try:
        with pytest.raises(_lib.InvalidArgumentError, match="labels may be None only"):
            t.loss_and_grad_frames(p["x"], p["seq_len"], None, targets)
        with pytest.raises(_lib.InvalidArgumentError, match="want_frame_loss needs targets"):
            t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], None, want_frame_loss=True)
        with pytest.raises(_lib.InvalidArgumentError, match=r"targets must be \[5,9\]"):
            t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], targets[:, :8])
        with pytest.raises(_lib.InvalidArgumentError, match="targets outside"):
            t.loss_and_grad_frames(p["x"], p["seq_len"], p["labels"], np.where(targets == 0, 6, targets))
        # through the C entry with the live handle: a null ft, null targets, a bad class weight, a null gradient blob
        x, b, frames, (_, sl_p), (lab, lab_p), (_, ll_p), _ = t._inputs(p["x"], p["seq_len"], p["labels"], None)
        loss = torch.empty(b, device="cuda")
        grad = torch.empty(t.weights_blob().size, device="cuda")
        tg = torch.from_numpy(targets).cuda()
        weight = np.array([1, 1, -1, 1, 1, 1], np.float32)

        def call(ft, grad_ptr=_lib.ptr(grad)):
            return t._lib.kws_train_grad_frames(t._handle, _lib.ptr(x), sl_p, lab_p, ll_p, b, frames, int(lab.shape[1]), None, _lib.ptr(loss),
                                                grad_ptr, None, None, ft, _lib.current_stream_ptr())
        bad = _lib.KWS_ERR_INVALID_ARGUMENT
        assert call(None) == bad and b"frame targets are null" in t._lib.kws_last_error()
        assert call(ctypes.byref(_lib.KwsFrameTargets(None, None, 1.0, 1.0, None))) == bad and b"ft->targets is null" in t._lib.kws_last_error()
        assert call(ctypes.byref(_lib.KwsFrameTargets(tg.data_ptr(), weight.ctypes.data, 1.0, 1.0, None))) == bad
        assert b"class_weight[2]=-1" in t._lib.kws_last_error()
        ok = _lib.KwsFrameTargets(tg.data_ptr(), None, 1.0, 1.0, None)
        assert call(ctypes.byref(ok), None) == bad and b"null pointer" in t._lib.kws_last_error()
        assert call(ctypes.byref(ok)) == _lib.KWS_OK
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all()
    finally:
        t.close()
    with pytest.raises(_lib.InvalidArgumentError, match="class_weight"):
        Trainer(p["config"], p["w"], frame_weight=1.0, class_weight=[1.0, 2.0])
