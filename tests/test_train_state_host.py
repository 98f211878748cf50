"""CPU checks of training from carried states: the fp64 restatement tests/train_state_model.py against torch's autograd in float64 and
central finite differences with respect to state_in, the chain identity that chained calls rest on, segment_lengths, and every refusal
kws_train_check_state and kws_train_apply raise before they touch a device."""
import ctypes

import numpy as np
import pytest

import train_model as M
import train_state_model as S
import train_wrapped_model as WM


def _scale(a):
    return max(float(np.abs(a).max()), 1e-300)


def _close(got, ref, tol, what):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
    assert err <= tol * _scale(ref), (what, err, tol * _scale(ref))


@pytest.mark.parametrize("key", sorted(S.TABLE))
def test_restatement_matches_torch_fp64(key):
    import torch
    p = S.make_problem(key)
    loss, grads, logits, state_out, dstate_in = S.of_problem(p)
    want = S.torch_of_problem(p, torch.float64)
    finite = np.isfinite(loss)
    _close(logits, want["logits"], 1e-10, "logits")
    _close(np.where(finite, loss, 0.0), want["loss"], 1e-10, "loss")
    _close(state_out, want["state_out"], 1e-10, "state_out")
    _close(dstate_in, want["dstate_in"], 1e-10, "dstate_in")
    for (name, got), (_, ref) in zip(WM.flat(grads), WM.flat(want["grads"])):
        _close(got, ref, 1e-10, name)
    assert finite.all() != (key == "no_path")
    # streams that run no frame: the state and its gradient pass through untouched
    empty = p["seq_len"] == 0
    assert np.array_equal(state_out[:, empty], p["state_in"][:, empty].astype(np.float64))
    assert np.array_equal(dstate_in[:, empty], p["dstate_out"][:, empty].astype(np.float64))
    assert np.abs(dstate_in).max() > 0 and np.abs(state_out - p["state_in"])[:, ~empty].max() > 0


@pytest.mark.parametrize("key", ["t2", "no_path", "res_l2_var"])
def test_dstate_in_matches_central_finite_differences(key):
    """J(state_in) = sum_b ctc_b / B (finite losses only: the others add exactly 0) + <dstate_out, state_out> along random directions."""
    p = S.make_problem(key)
    s0 = p["state_in"].astype(np.float64)
    dstate_in = S.of_problem(p)[4]

    def objective(state):
        loss, _, _, state_out, _ = S.of_problem(p, state_in=state)
        return np.where(np.isfinite(loss), loss, 0.0).sum() / p["B"] + (p["dstate_out"].astype(np.float64) * state_out).sum()
    rng = np.random.default_rng(3)
    eps = 1e-6
    for _ in range(4):
        v = rng.standard_normal(s0.shape)
        fd = (objective(s0 + eps * v) - objective(s0 - eps * v)) / (2 * eps)
        an = float((dstate_in * v).sum())
        assert abs(fd - an) <= 1e-7 * max(abs(an), 1.0), (key, fd, an)


@pytest.mark.parametrize("name", ["ref_shape", "no_path", "l8"])
def test_without_states_it_is_train_model_exactly(name):
    p = M.make_problem(name)
    loss, grads, logits = M.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"])
    loss_s, grads_s, logits_s, state_out, dstate_in = S.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"])
    assert np.array_equal(loss, loss_s) and np.array_equal(logits, logits_s)
    for (key, a), (_, b) in zip(M.flat(grads), M.flat(grads_s)):
        assert np.array_equal(a, b), key
    assert not state_out[:, p["seq_len"] == 0].any() and state_out.any()
    # ... and zeros given explicitly are the same numbers
    zeros = np.zeros_like(state_out)
    again = S.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], zeros, zeros)
    assert np.array_equal(again[0], loss) and np.array_equal(again[3], state_out) and np.array_equal(again[4], dstate_in)
    for (key, a), (_, b) in zip(M.flat(grads), M.flat(again[1])):
        assert np.array_equal(a, b), key


def test_without_states_it_is_train_wrapped_model_exactly():
    p = WM.make_problem("both_ref_shape")
    loss, grads, logits = WM.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], True, True)
    loss_s, grads_s, logits_s, _, _ = S.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], ln=True, res=True)
    assert np.array_equal(loss, loss_s) and np.array_equal(logits, logits_s)
    for (key, a), (_, b) in zip(WM.flat(grads), WM.flat(grads_s)):
        assert np.array_equal(a, b), key


@pytest.mark.parametrize("key", sorted(S.CHAIN_CUT))
def test_chain_identity(key):
    """Two segments whose state flows through, in one graph (B's state_out weighted with the case's dstate_out, so that streams which
    ended in A have a gradient to carry back too): the parameter gradient is grad(A with dstate_out = B's dstate_in) + grad(B), and
    its dstate_in is A's.  The identity itself is held at 1e-12 where both sides are the same arithmetic (torch float64:
    three single-segment graphs against the two-segment graph); the restatement chained the same way is held against the two-segment
    graph at the 1e-10 of test_restatement_matches_torch_fp64."""
    import torch
    p, (seg_a, seg_b) = S.chain_problem(key)
    whole = S.chain_reference(key)[0]
    kw = dict(ln=p["ln"], res=p["res"])
    # torch, segment by segment
    a1 = S.torch_reference(p["w"], *seg_a, torch.float64, state_in=p["state_in"], **kw)
    b1 = S.torch_reference(p["w"], *seg_b, torch.float64, state_in=a1["state_out"], dstate_out=p["dstate_out"], **kw)
    a2 = S.torch_reference(p["w"], *seg_a, torch.float64, state_in=p["state_in"], dstate_out=b1["dstate_in"], **kw)
    _close(b1["state_out"], whole["state_out"], 1e-12, "state_out")
    _close(a2["dstate_in"], whole["dstate_in"], 1e-12, "dstate_in")
    _close(np.array([a1["loss"], b1["loss"]]), whole["loss"], 1e-12, "loss")
    for (name, got), (_, ref) in zip(WM.flat(S.add_grads(p["w"], a2["grads"], b1["grads"])), WM.flat(whole["grads"])):
        _close(got, ref, 1e-12, name)
    # the restatement, segment by segment
    _, _, _, sa, _ = S.loss_and_grad(p["w"], *seg_a, state_in=p["state_in"], **kw)
    loss_b, gb, _, sb, da = S.loss_and_grad(p["w"], *seg_b, state_in=sa, dstate_out=p["dstate_out"], **kw)
    loss_a, ga, _, _, d0 = S.loss_and_grad(p["w"], *seg_a, state_in=p["state_in"], dstate_out=da, **kw)
    _close(sb, whole["state_out"], 1e-10, "state_out")
    _close(d0, whole["dstate_in"], 1e-10, "dstate_in")
    _close(np.array([loss_a, loss_b]), whole["loss"], 1e-10, "loss")
    for (name, got), (_, ref) in zip(WM.flat(S.add_grads(p["w"], ga, gb)), WM.flat(whole["grads"])):
        _close(got, ref, 1e-10, name)
    # the cut leaves work on both sides, streams that end inside A, and B's gradient does reach A
    assert (seg_a[1] > 0).sum() > (seg_b[1] > 0).sum() > 0 and np.abs(da).max() > 0
    ended = (seg_a[1] > 0) & (seg_a[1] < seg_a[1].max())          # live in A, shorter than A, absent from B: dstate_out passes B and A's dead frames
    assert ended.any() and (seg_b[1][ended] == 0).all() and np.array_equal(da[:, ended], p["dstate_out"][:, ended].astype(np.float64))
    assert any(len(s) for s in seg_a[2]) and any(len(s) for s in seg_b[2])


def test_forward_chain_is_one_call_in_the_restatement():
    """Frames [0, T1) then [T1, T) from the carried state give the logits and the final state of one call, streams shorter than T1
    running the second call at seq_len 0 (fp64: to rounding, the operations are the same)."""
    from keyword_spotting_amd.training import segment_lengths
    p = S.make_problem("ref_shape")
    one_logits, _, one_state = S.forward(p["w"], p["x"], p["seq_len"], p["state_in"])
    for cut in (1, 7, p["T"] - 1):
        la, lb = segment_lengths(p["seq_len"], 0, cut), segment_lengths(p["seq_len"], cut, p["T"] - cut)
        assert (la + lb == p["seq_len"]).all() and (lb == 0).sum() >= (p["seq_len"] <= cut).sum()
        logits_a, _, sa = S.forward(p["w"], p["x"][:, :cut], la, p["state_in"])
        logits_b, _, sb = S.forward(p["w"], p["x"][:, cut:], lb, sa)
        _close(np.concatenate([logits_a, logits_b], axis=1), one_logits, 1e-13, cut)
        _close(sb, one_state, 1e-13, cut)


def test_segment_lengths():
    from keyword_spotting_amd.training import segment_lengths
    lengths = [0, 3, 7, 10, 23]
    assert segment_lengths(lengths, 0, 7).tolist() == [0, 3, 7, 7, 7]
    assert segment_lengths(lengths, 7, 7).tolist() == [0, 0, 0, 3, 7]
    assert segment_lengths(lengths, 14, 9).tolist() == [0, 0, 0, 0, 9]
    assert segment_lengths(lengths, 30, 5).tolist() == [0] * 5
    out = segment_lengths(np.array(lengths, np.int32), 2, 4)
    assert out.dtype == np.int32 and out.tolist() == [0, 1, 4, 4, 4]
    total = sum(segment_lengths(lengths, s, 5) for s in range(0, 25, 5))
    assert total.tolist() == lengths


def _i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _cfg(hidden=64, layers=1, n_mel=4, classes=6, ln=0, res=0, var=0, keep=1.0):
    from keyword_spotting_amd import _lib
    return _lib.KwsTrainConfig(_lib.KwsConfig(n_mel, hidden, layers, classes, 0, -1.0, _lib.FP32), _lib.KwsCellWrappers(ln, res), var, _lib.OPT_ADAM,
                               -1.0, keep)


def test_state_call_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    assert lib.kws_sizeof_train_state_io() == 32 == ctypes.sizeof(_lib.KwsTrainStateIo)
    x = ctypes.c_void_p(256)            # a non-null, aligned address that is never read
    sl, ll, lab = _i32(4, 4), _i32(2, 1), _i32(1, 4, 0, 0)
    good = _lib.KwsTrainStateIo(256, 512, 1024, 2048)

    def check(cfg=None, wrapped=0, x=x, seq=sl, labels=lab, lens=ll, b=2, t=4, s_max=2, loss=x, io=good):
        rc = lib.kws_train_check_state(ctypes.byref(cfg or _cfg()), wrapped, x, seq, labels, lens, b, t, s_max, loss,
                                       None if io is None else ctypes.byref(io))
        return rc, lib.kws_last_error()
    bad, uns = _lib.KWS_ERR_INVALID_ARGUMENT, _lib.KWS_ERR_UNSUPPORTED
    assert check()[0] == _lib.KWS_OK and check(io=None)[0] == _lib.KWS_OK and check(io=_lib.KwsTrainStateIo())[0] == _lib.KWS_OK
    assert check(io=_lib.KwsTrainStateIo(256, 256, 512, 512))[0] == _lib.KWS_OK          # the two allowed aliases
    # a state pointer off a 16-byte boundary, named
    for i, field in enumerate(("state_in", "state_out", "dstate_out", "dstate_in")):
        for off in (4, 8, 12, 1):
            ptrs = [256, 512, 1024, 2048]
            ptrs[i] += off
            rc, msg = check(io=_lib.KwsTrainStateIo(*ptrs))
            assert rc == bad and ("io->%s must be 16-byte aligned" % field).encode() in msg, (field, off, msg)
    # every refusal of the plain calls
    assert check(cfg=_cfg(keep=0.0))[0] == uns and b"keep_prob" in lib.kws_last_error()
    assert check(cfg=_cfg(ln=1))[0] == uns and b"kws_train_create_wrapped" in lib.kws_last_error()
    assert check(cfg=_cfg(ln=1, res=1, var=1), wrapped=1)[0] == _lib.KWS_OK
    assert check(cfg=_cfg(ln=2), wrapped=1)[0] == bad and b"wrappers.use_layer_norm=2" in lib.kws_last_error()
    assert check(cfg=_cfg(hidden=100))[0] == bad and b"hidden=100" in lib.kws_last_error()
    assert check(b=0)[0] == bad and b"B=0" in lib.kws_last_error()
    assert check(t=0)[0] == bad
    assert check(s_max=32)[0] == bad and b"S_max=32" in lib.kws_last_error()
    for kw in (dict(x=None), dict(seq=None), dict(labels=None), dict(lens=None), dict(loss=None)):
        assert check(**kw)[0] == bad and b"null pointer" in lib.kws_last_error(), kw
    assert check(x=ctypes.c_void_p(258))[0] == bad and b"aligned" in lib.kws_last_error()
    assert check(cfg=_cfg(classes=5))[0] == bad and b"labels[0][1]=4" in lib.kws_last_error()
    assert check(seq=_i32(4, 5))[0] == bad and b"seq_len[1]=5" in lib.kws_last_error()
    assert check(lens=_i32(3, 1))[0] == bad and b"label_len[0]=3" in lib.kws_last_error()
    rc, msg = check(b=1, t=700, s_max=31, seq=_i32(700), lens=_i32(0), labels=_i32(*([0] * 31)))
    assert rc == uns and b"198800 bytes exceed the 163840" in msg
    assert lib.kws_train_check_state(None, 0, x, sl, lab, ll, 2, 4, 2, x, None) == bad and b"config is null" in lib.kws_last_error()
    # the entry points themselves: a null handle is refused before anything else
    io = ctypes.byref(good)
    assert lib.kws_train_grad_state(None, x, sl, lab, ll, 2, 4, 2, None, x, x, None, io, None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_train_step_state(None, x, sl, lab, ll, 2, 4, 2, None, 0.01, x, None, io, None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_train_apply(None, x, 0.01, None, None) == bad and b"handle is null" in lib.kws_last_error()


def test_the_binding_declares_the_new_entry_points():
    from keyword_spotting_amd import _lib, training
    for sym in ("kws_sizeof_train_state_io", "kws_train_grad_state", "kws_train_step_state", "kws_train_check_state", "kws_train_apply"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym), sym
    import inspect
    assert list(inspect.signature(training.Trainer.loss_and_grad).parameters)[1:] == ["x", "lengths", "labels", "drop", "want_logits", "state",
                                                                                    "dstate_out", "want_state"]
    assert list(inspect.signature(training.Trainer.step).parameters)[1:] == ["x", "lengths", "labels", "state", "want_state"]
    assert inspect.signature(training.Trainer.__init__).parameters["state_noise"].default == 0.0
