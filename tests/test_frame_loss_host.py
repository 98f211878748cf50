"""CPU checks of frame-wise targets: the restatement tests/frame_loss_model.py against torch's F.cross_entropy in float64 and against
central finite differences through the GRU graph, the alignment round trip that makes the targets, every refusal the new entry
points raise before they touch a device, Python's host range check, and the conditions the GPU tests lean on (the toy task trains on
its frame-wise targets alone; the float32 trajectory of the mixed objective stays close to fp64)."""
import ctypes

import numpy as np
import pytest

import align_model as AL
import frame_loss_model as F
import train_model as M
import train_state_model as SM
from conftest import have_gpu


def _scale(a):
    return max(float(np.abs(a).max()), 1e-300)


# ---- the restatement against torch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,weight", [(3, None), (6, [0.5, 1.0, 0.0, 2.0, 1.0, 1.5]), (8, [50.0, 1.0, 1.0, 2.0, 5.0, 1.0, 10.0, 0.0])])
def test_restatement_matches_torch_cross_entropy_fp64(c, weight):
    """Per utterance F.cross_entropy(weight=, ignore_index=-1, reduction='mean') and its autograd gradient: ragged lengths, runs of -1,
    weights of zero; an empty slot, an utterance without a target and one whose targets all weigh 0 give 0 / 0."""
    import torch
    import torch.nn.functional as TF
    rng = np.random.default_rng(10 + c)
    b, t = 7, 19
    seq_len = np.array([19, 0, 11, 7, 19, 5, 13])
    logits = 3.0 * rng.standard_normal((b, t, c))
    targets = F.random_targets(rng, seq_len, t, c, garbage=True)
    targets[3, :] = -1
    if weight is not None:
        targets[5, :5] = int(np.flatnonzero(np.asarray(weight) == 0)[0])
    logits[np.arange(t)[None, :] >= seq_len[:, None]] = np.nan          # never read
    ce, grad = F.frame_loss(logits, seq_len, targets, weight)
    assert (targets[0, :19] == -1).any() and (targets[0, :19] >= 0).any()
    empty = [1, 3] + ([5] if weight is not None else [])
    for i in range(b):
        n = seq_len[i]
        assert not grad[i, n:].any() and not grad[i, :n][targets[i, :n] < 0].any()
        if i in empty:
            assert ce[i] == 0 and not grad[i].any(), i
            continue
        z = torch.tensor(logits[i, :n], dtype=torch.float64, requires_grad=True)
        w = None if weight is None else torch.tensor(weight, dtype=torch.float64)
        want = TF.cross_entropy(z, torch.tensor(targets[i, :n].astype(np.int64)), weight=w, ignore_index=-1, reduction="mean")
        want.backward()
        assert abs(ce[i] - float(want.detach())) <= 1e-10 * max(1.0, abs(float(want.detach()))), i
        assert np.abs(grad[i, :n] - z.grad.numpy()).max() <= 1e-10, i


def test_a_target_out_of_range_counts_as_none_and_poisons_its_utterance_only():
    rng = np.random.default_rng(2)
    seq_len = np.array([9, 6, 9])
    logits = rng.standard_normal((3, 9, 4))
    targets = F.random_targets(rng, seq_len, 9, 4)
    targets[1, 2] = 1
    ce, grad = F.frame_loss(logits, seq_len, targets)
    bad, none = targets.copy(), targets.copy()
    bad[1, 2], none[1, 2] = 4, -1
    ce_bad, grad_bad = F.frame_loss(logits, seq_len, bad)
    ce_none, grad_none = F.frame_loss(logits, seq_len, none)
    assert np.isnan(ce_bad[1]) and np.array_equal(ce_bad[[0, 2]], ce[[0, 2]])
    assert np.array_equal(grad_bad, grad_none) and not np.array_equal(grad_bad[1], grad[1])
    bad[1, 8] = 99                                                      # past seq_len: never read
    assert np.array_equal(F.frame_loss(logits, seq_len, bad)[1], grad_bad)


def test_float32_evaluation_is_close_and_not_equal():
    """The yardstick of the GPU test is the restatement with every operation in float32: a real float32 evaluation (not the fp64 one
    rounded), within 1e-5 of the fp64 values."""
    p = F.kernel_problem("t300_c3_b17")
    (ce64, g64), (ce32, g32) = p["ref64"], p["ref32"]
    assert ce32.dtype == np.float32 and g32.dtype == np.float32
    assert 0 < np.abs(ce32 - ce64).max() <= 1e-5 * _scale(ce64) and 0 < np.abs(g32 - g64).max() <= 1e-5


def test_kernel_case_table_covers_what_it_says():
    seen_t, seen_c, seen_b = set(), set(), set()
    for name in F.KERNEL_CASES:
        p = F.kernel_problem(name)
        seen_t.add(p["T"]); seen_c.add(p["C"]); seen_b.add(p["B"])
        assert p["seq_len"].max() == p["T"]
        if p["B"] == 17:
            assert p["seq_len"][3] == 0 and p["seq_len"][16] == p["T"] and (p["targets"][5] == -1).all()
            n7 = p["seq_len"][7]
            assert (p["targets"][7, :n7] == p["C"] - 1).all()
            assert p["targets"][16, 0] == -1 and p["targets"][16, p["T"] - 1] == -1
    assert seen_t >= {1, 2, 63, 64, 65, 255, 256, 257, 300, 4000} and seen_c == {3, 5, 6, 8} and seen_b >= {1, 17}
    weights = [F.kernel_problem(n)["weight"] for n in F.KERNEL_CASES]
    assert any(w is None for w in weights) and any(w is not None and (w == 0).any() for w in weights)
    assert any(w is not None and w.max() / w[w > 0].min() == 50 for w in weights)


# ---- the mixed objective through the GRU graph ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["t2", "both_ref_shape"])
def test_ctc_only_is_the_state_restatement_to_the_last_bit(key):
    """frame_loss_model's backward restates train_state_model.loss_and_grad's: at frame_weight 0 the numbers are equal, not close."""
    p = SM.make_problem(key)
    kw = dict(state_in=p["state_in"], dstate_out=p["dstate_out"], ln=p["ln"], res=p["res"], drop=p["drop"], keep_prob=p["keep_prob"])
    loss, grads, logits, state_out, dstate_in = SM.loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], **kw)
    r = F.gru_loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], None, 1.0, 0.0, **kw)
    assert np.array_equal(loss, r["loss"]) and np.array_equal(logits, r["logits"]) and np.array_equal(dstate_in, r["dstate_in"])
    for (k, a), (_, b) in zip(SM.WM.flat(grads), SM.WM.flat(r["grads"])):
        assert np.array_equal(a, b), k


@pytest.mark.parametrize("key,objective", [("t2", "frames"), ("ref_shape", "mixed"), ("both_ref_shape", "mixed"), ("t1", "mixed")])
def test_mixed_restatement_matches_the_torch_graph_fp64(key, objective):
    import torch
    p = SM.make_problem(key)
    cw, fw, weighted = F.OBJECTIVES[objective]
    targets, weight = F.gru_targets(p), F.class_weights(p["config"].num_classes, weighted)
    kw = dict(ctc_weight=cw, frame_weight=fw, class_weight=weight, state_in=p["state_in"], dstate_out=p["dstate_out"], ln=p["ln"], res=p["res"])
    got = F.gru_loss_and_grad(p["w"], p["x"], p["seq_len"], p["labels"], targets, **kw)
    want = F.gru_torch(p["w"], p["x"], p["seq_len"], p["labels"], targets, torch.float64, **kw)
    for k in ("loss", "ce", "logits", "state_out", "dstate_in"):
        assert np.abs(got[k] - want[k]).max() <= 1e-10 * max(1.0, _scale(want[k])), k
    for (k, a), (_, b) in zip(SM.WM.flat(got["grads"]), SM.WM.flat(want["grads"])):
        assert np.abs(a - b).max() <= 1e-10 * max(1.0, _scale(b)), k


@pytest.mark.parametrize("key,with_state", [("t2", False), ("odd_mel", False), ("t2", True)])
def test_mixed_objective_matches_central_finite_differences(key, with_state):
    """J = sum_b (ctc_b + 0.5 ce_b) / B [+ <dstate_out, state_out> from a carried state] against (J(w + e) - J(w - e)) / 2e, two probes per
    parameter tensor and, with the state, two of state_in."""
    p = SM.make_problem(key) if with_state else M.make_problem(key)
    cw, fw, weighted = F.OBJECTIVES["mixed"]
    targets, weight = F.gru_targets(p), F.class_weights(p["config"].num_classes, weighted)
    w = M.as_dtype(p["w"], np.float64)
    s0 = np.asarray(p["state_in"], np.float64).copy() if with_state else None
    d_out = np.asarray(p["dstate_out"], np.float64) if with_state else None

    def run(wd):
        return F.gru_loss_and_grad(wd, p["x"], p["seq_len"], p["labels"], targets, cw, fw, weight, state_in=s0, dstate_out=d_out)

    def total(wd):
        r = run(wd)
        return r["loss"].sum() / p["B"] + (float((d_out * r["state_out"]).sum()) if with_state else 0.0)
    r = run(w)
    rng = np.random.default_rng(3)
    eps = 1e-6
    probes = [("Wfc", None), ("bfc", None)] + [(k, l) for l in range(len(w["layers"])) for k in ("Wg", "bg", "Wc", "bc")]
    pairs = [(w[k] if l is None else w["layers"][l][k], r["grads"][k] if l is None else r["grads"]["layers"][l][k], (k, l)) for k, l in probes]
    if with_state:
        pairs.append((s0, r["dstate_in"], "state_in"))
    for arr, g, what in pairs:
        for _ in range(2):
            idx = tuple(int(rng.integers(0, n)) for n in arr.shape)
            keep = arr[idx]
            arr[idx] = keep + eps
            up = total(w)
            arr[idx] = keep - eps
            down = total(w)
            arr[idx] = keep
            assert abs((up - down) / (2 * eps) - g[idx]) <= 1e-6 * max(1.0, _scale(g)), (what, idx)


# ---- the alignment round trip --------------------------------------------------------------------------------------------------------

def test_frame_labels_of_a_viterbi_path_are_targets_that_spell_the_transcript():
    from keyword_spotting_amd.custom_keyword import frame_labels
    c, t = 6, 30
    seq_len = [30, 17, 0, 24]
    labels = [AL.make_label(s, 12, c, 4) for s in range(4)]
    logits = np.stack([AL.make_logits(s, t, c) for s in range(4)])
    states = np.stack([AL.align(logits[i], seq_len[i], labels[i])["states"] for i in range(4)])
    targets = frame_labels(states, labels, c - 1)
    assert targets.dtype == np.int32 and targets.shape == (4, t)
    for i in range(4):
        n = seq_len[i]
        assert (targets[i, n:] == -1).all() and ((targets[i, :n] >= 0) & (targets[i, :n] < c)).all()
        assert np.array_equal(targets[i], AL.frame_classes(states[i], labels[i], c - 1))
        if n:
            assert list(AL.collapse(targets[i, :n], c - 1)) == list(labels[i]), i
    ce, grad = F.frame_loss(logits, seq_len, targets)
    assert np.isfinite(ce).all() and ce[2] == 0 and (ce[[0, 1, 3]] > 0).all() and not grad[2].any()


# ---- refusals that need no device ------------------------------------------------------------------------------------------------------

_KEEP = []


def _i32(*v):
    a = np.array(v, np.int32)
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def _f32(*v):
    a = np.array(v, np.float32)
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def _ft(targets=ctypes.c_void_p(512), weight=None, ctc=1.0, frame=1.0, out=None):
    from keyword_spotting_amd import _lib
    ft = _lib.KwsFrameTargets(targets, weight, ctc, frame, out)
    _KEEP.append(ft)
    return ctypes.byref(ft)


def test_new_entry_points_exist_and_the_struct_has_the_headers_size():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_frame_loss", "kws_sizeof_frame_targets", "kws_train_grad_frames", "kws_train_step_frames", "kws_train_check_frames",
                "kws_attention_train_grad_frames", "kws_attention_train_step_frames", "kws_attention_train_check_frames"):
        assert hasattr(lib, sym), sym
    assert lib.kws_sizeof_frame_targets() == ctypes.sizeof(_lib.KwsFrameTargets) == 32


def test_frame_loss_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    x = ctypes.c_void_p(256)
    sl = _i32(4, 3)

    def call(logits=x, seq=sl, targets=x, weight=None, b=2, t=4, c=6, loss=x, grad=None):
        rc = lib.kws_frame_loss(logits, seq, targets, weight, b, t, c, loss, grad, None)
        return rc, lib.kws_last_error()
    bad, uns = _lib.KWS_ERR_INVALID_ARGUMENT, _lib.KWS_ERR_UNSUPPORTED
    assert call(b=-1)[0] == bad and b"bad shape B=-1" in lib.kws_last_error()
    assert call(t=0)[0] == bad and b"T=0" in lib.kws_last_error()
    for c in (2, 9):
        rc, msg = call(c=c)
        assert rc == bad and b"out of range [3,8]" in msg
    rc, msg = call(b=1 << 20, t=1 << 12)
    assert rc == uns and b"2^31 - 1 frames" in msg
    assert call(b=0, logits=None, seq=None, targets=None, loss=None)[0] == _lib.KWS_OK          # nothing to do, as kws_ctc_loss
    for kw in (dict(logits=None), dict(seq=None), dict(targets=None), dict(loss=None)):
        assert call(**kw)[0] == bad and b"null pointer" in lib.kws_last_error(), kw
    for kw in (dict(logits=ctypes.c_void_p(258)), dict(targets=ctypes.c_void_p(257)), dict(loss=ctypes.c_void_p(259)), dict(grad=ctypes.c_void_p(262))):
        assert call(**kw)[0] == bad and b"4-byte aligned" in lib.kws_last_error(), kw
    assert call(seq=_i32(4, 5))[0] == bad and b"seq_len[1]=5 outside [0,4]" in lib.kws_last_error()
    assert call(seq=_i32(-1, 4))[0] == bad and b"seq_len[0]=-1" in lib.kws_last_error()
    for w, word in (((1, 1, -0.5, 1, 1, 1), b"class_weight[2]=-0.5"), ((1, float("inf"), 1, 1, 1, 1), b"class_weight[1]=inf"),
                    ((float("nan"), 1, 1, 1, 1, 1), b"class_weight[0]=nan")):
        rc, msg = call(weight=_f32(*w))
        assert rc == bad and word in msg, (w, msg)
    if not have_gpu():
        assert call(weight=_f32(1, 0, 2, 1, 1, 50))[0] == _lib.KWS_ERR_NO_DEVICE          # everything above came first


def _train_cfg(n_mel=40, hidden=128, layers=2, classes=6, ln=0, res=0, keep=1.0):
    from keyword_spotting_amd import _lib
    return _lib.KwsTrainConfig(_lib.KwsConfig(n_mel, hidden, layers, classes, 0, -1.0, _lib.FP32), _lib.KwsCellWrappers(ln, res), 0, _lib.OPT_ADAM,
                               -1.0, keep)


def test_train_frames_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    x = ctypes.c_void_p(256)
    sl, ll, lab = _i32(4, 4), _i32(2, 1), _i32(1, 4, 0, 0)
    cfg = _train_cfg()

    def check(ft, cfg=cfg, wrapped=0, x=x, seq=sl, labels=lab, lens=ll, b=2, t=4, s_max=2, loss=x, io=None):
        rc = lib.kws_train_check_frames(ctypes.byref(cfg), wrapped, x, seq, labels, lens, b, t, s_max, loss, io, ft)
        return rc, lib.kws_last_error()
    bad, uns = _lib.KWS_ERR_INVALID_ARGUMENT, _lib.KWS_ERR_UNSUPPORTED
    assert check(_ft())[0] == _lib.KWS_OK
    assert check(_ft(weight=_f32(1, 0, 2, 1, 1, 50), out=ctypes.c_void_p(1024)))[0] == _lib.KWS_OK
    assert check(None)[0] == bad and b"frame targets are null" in lib.kws_last_error()
    assert check(_ft(targets=None))[0] == bad and b"ft->targets is null" in lib.kws_last_error()
    for kw, word in ((dict(ctc=-1.0), b"ft->ctc_weight=-1"), (dict(ctc=float("nan")), b"ft->ctc_weight=nan"), (dict(frame=-0.5), b"ft->frame_weight=-0.5"),
                     (dict(frame=float("inf")), b"ft->frame_weight=inf"), (dict(ctc=0.0, frame=0.0), b"both 0"),
                     (dict(ctc=2.0, frame=0.0), b"ft->frame_weight=0 is the plain call"),
                     (dict(targets=ctypes.c_void_p(514)), b"4-byte aligned"), (dict(out=ctypes.c_void_p(1026)), b"4-byte aligned"),
                     (dict(weight=_f32(1, 1, 1, -2, 1, 1)), b"class_weight[3]=-2"), (dict(weight=_f32(1, 1, 1, 1, 1, float("nan"))), b"class_weight[5]=nan")):
        rc, msg = check(_ft(**kw))
        assert rc == bad and word in msg, (kw, msg)
    # everything the state call refuses
    assert check(_ft(), cfg=_train_cfg(keep=0.0))[0] == uns and b"keep_prob" in lib.kws_last_error()
    assert check(_ft(), cfg=_train_cfg(ln=1))[0] == uns and check(_ft(), cfg=_train_cfg(ln=1), wrapped=1)[0] == _lib.KWS_OK
    assert check(_ft(), b=0)[0] == bad and check(_ft(), s_max=32)[0] == bad and b"S_max=32" in lib.kws_last_error()
    for kw in (dict(x=None), dict(seq=None), dict(labels=None), dict(lens=None), dict(loss=None)):
        assert check(_ft(), **kw)[0] == bad and b"null pointer" in lib.kws_last_error(), kw
    assert check(_ft(), seq=_i32(4, 5))[0] == bad and b"seq_len[1]=5" in lib.kws_last_error()
    assert check(_ft(), labels=_i32(1, 5, 0, 0))[0] == bad and b"labels[0][1]=5" in lib.kws_last_error()
    io = _lib.KwsTrainStateIo(ctypes.c_void_p(264), None, None, None)
    assert check(_ft(), io=ctypes.byref(io))[0] == bad and b"io->state_in must be 16-byte aligned" in lib.kws_last_error()
    rc, msg = check(_ft(), b=1, t=700, s_max=31, seq=_i32(700), lens=_i32(0), labels=_i32(*([0] * 31)))
    assert rc == uns and b"198800 bytes exceed the 163840" in msg
    # ctc_weight 0: nothing about the labels, S_max or the CTC kernel's LDS -- the lengths are still checked
    frames = dict(ctc=0.0, frame=1.0)
    assert check(_ft(**frames), labels=None, lens=None, s_max=0)[0] == _lib.KWS_OK
    assert check(_ft(**frames), labels=None, lens=None, s_max=0, b=1, t=4000, seq=_i32(4000))[0] == _lib.KWS_OK
    assert check(_ft(**frames), labels=_i32(9, 9, 9, 9), s_max=77)[0] == _lib.KWS_OK
    assert check(_ft(**frames), seq=_i32(4, 5), labels=None, lens=None)[0] == bad and b"seq_len[1]=5 outside [0,4]" in lib.kws_last_error()
    assert check(_ft(**frames), x=None)[0] == bad
    # the entry points themselves: a null handle first, then -- the handle is never looked at on this path -- nothing else to tell without one
    assert lib.kws_train_grad_frames(None, x, sl, lab, ll, 2, 4, 2, None, x, x, None, None, _ft(), None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_train_step_frames(None, x, sl, lab, ll, 2, 4, 2, None, 0.01, x, None, None, _ft(), None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_train_check_frames(None, 0, x, sl, lab, ll, 2, 4, 2, x, None, _ft()) == bad and b"config is null" in lib.kws_last_error()


def test_attention_train_frames_refusals_come_before_the_device():
    import attention_train_model as AM
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.attention_training import train_config
    lib = _lib.load()
    p = AM.raw_problem("c2", 0)          # combine_frame 2: T = 12 -> T' = 7
    cfg = train_config(p["config"])
    x = ctypes.c_void_p(256)
    sl, ll, lab = _i32(12, 7), _i32(2, 1), _i32(1, 4, 0, 0)

    def check(ft, cfg=cfg, x=x, seq=sl, labels=lab, lens=ll, b=2, t=12, s_max=2, loss=x):
        rc = lib.kws_attention_train_check_frames(ctypes.byref(cfg), x, seq, labels, lens, b, t, s_max, loss, ft)
        return rc, lib.kws_last_error()
    bad, uns = _lib.KWS_ERR_INVALID_ARGUMENT, _lib.KWS_ERR_UNSUPPORTED
    assert check(_ft())[0] == _lib.KWS_OK
    assert check(None)[0] == bad and b"frame targets are null" in lib.kws_last_error()
    assert check(_ft(targets=None))[0] == bad and b"ft->targets is null" in lib.kws_last_error()
    for kw, word in ((dict(ctc=-1.0), b"ft->ctc_weight=-1"), (dict(frame=float("nan")), b"ft->frame_weight=nan"), (dict(ctc=0.0, frame=0.0), b"both 0"),
                     (dict(ctc=0.5, frame=0.0), b"plain call"), (dict(targets=ctypes.c_void_p(513)), b"4-byte aligned"),
                     (dict(weight=_f32(1, 1, float("inf"), 1, 1, 1)), b"class_weight[2]=inf")):
        rc, msg = check(_ft(**kw))
        assert rc == bad and word in msg, (kw, msg)
    assert check(_ft(), cfg=train_config(p["config"], keep_prob=0.0))[0] == uns and b"keep_prob" in lib.kws_last_error()
    assert check(_ft(), t=5000, seq=_i32(5000, 1))[0] == uns and b"max_frames" in lib.kws_last_error()
    assert check(_ft(), s_max=32)[0] == bad and check(_ft(), labels=None)[0] == bad and check(_ft(), lens=None)[0] == bad
    assert check(_ft(), seq=_i32(12, 13))[0] == bad and b"seq_len[1]=13" in lib.kws_last_error()
    assert check(_ft(), labels=_i32(1, 5, 0, 0))[0] == bad
    frames = dict(ctc=0.0, frame=1.0)
    assert check(_ft(**frames), labels=None, lens=None, s_max=0)[0] == _lib.KWS_OK
    assert check(_ft(**frames), labels=None, lens=None, s_max=0, seq=_i32(12, 13))[0] == bad
    # T' = 2049 rows x (8 + 63) floats of CTC LDS is refused for the CTC term and not for the frame term alone
    long_seq, long_ll, long_lab = _i32(4096), _i32(0), _i32(*([0] * 31))
    rc, msg = check(_ft(), b=1, t=4096, s_max=31, seq=long_seq, lens=long_ll, labels=long_lab)
    assert rc == uns and b"bytes exceed" in msg
    assert check(_ft(**frames), b=1, t=4096, s_max=31, seq=long_seq, lens=long_ll, labels=long_lab)[0] == _lib.KWS_OK
    assert lib.kws_attention_train_grad_frames(None, x, sl, lab, ll, 2, 12, 2, 0, x, x, None, _ft(), None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_attention_train_step_frames(None, x, sl, lab, ll, 2, 12, 2, 0, 0.01, x, None, _ft(), None) == bad and b"handle is null" in lib.kws_last_error()
    assert lib.kws_attention_train_check_frames(None, x, sl, lab, ll, 2, 12, 2, x, _ft()) == bad and b"config is null" in lib.kws_last_error()


def test_python_checks_host_targets_before_anything_is_uploaded():
    """custom_keyword._frame_targets (frame_loss and both trainers go through it): a host array outside [-1, C) is refused with the
    range; the shape is checked on both paths.  No device is needed for the refusals."""
    import torch
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.custom_keyword import _class_weight, _frame_targets
    ok = np.array([[0, -1, 5], [5, 5, -1]])
    for bad_value in (6, -2, 2 ** 31 - 1):
        t = ok.copy()
        t[1, 1] = bad_value
        for form in (t, t.astype(np.int32), torch.from_numpy(t)):
            with pytest.raises(_lib.InvalidArgumentError, match=r"targets outside \[-1,5\]"):
                _frame_targets(form, (2, 3), 6, "cpu")
    with pytest.raises(_lib.InvalidArgumentError, match=r"targets must be \[2,4\]"):
        _frame_targets(ok, (2, 4), 6, "cpu")
    got = _frame_targets(ok, (2, 3), 6, "cpu")
    assert got.dtype == torch.int32 and got.is_contiguous() and np.array_equal(got.numpy(), ok)
    assert _class_weight(None, 6) == (None, None)
    w, p = _class_weight([1, 2, 0, 1, 1, 50], 6)
    assert w.dtype == np.float32 and p.value == w.ctypes.data
    with pytest.raises(_lib.InvalidArgumentError, match="class_weight"):
        _class_weight([1, 2, 3], 6)


# ---- conditions the GPU tests lean on --------------------------------------------------------------------------------------------------

def test_toy_task_trains_on_its_frame_wise_targets_alone():
    """The targets: align_model's best paths on the CTC-trained restatement's logits.  The restatement trained on them alone, from the
    toy task's initial weights with TOY_FRAMES' settings (train_model.TOY's 150 steps at 0.02, unit weights), recognises all 16
    utterances through ctc_decode2 / ctc_predict; every frame's argmax is its target, and the smallest margin between a frame's target
    logit and the next one is above 1 -- room to spare for a float32 run of the same steps (tests/test_gpu_train_frames.py)."""
    from oracle import decode_oracle as D
    p = M.toy_task(0)
    losses, logits, targets = F.toy_frames_trained(0)
    c = M.TOY["C"]
    assert ((targets >= 0) & (targets < c)).all()
    for i in range(p["B"]):
        assert list(AL.collapse(targets[i], c - 1)) == p["labels"][i], i
    assert losses[-1] < 0.05 * losses[0], (losses[0], losses[-1])
    sm = np.exp(M.E.log_softmax(logits))
    for i in range(p["B"]):
        assert D.ctc_predict(D.ctc_decode2(sm[i], c), M.TOY["label"]) == 1, i
    top = np.take_along_axis(logits, targets[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    rest = np.where(np.arange(c)[None, None, :] == targets[:, :, None], -np.inf, logits).max(axis=2)
    print("toy task on frame-wise targets: loss %.4f -> %.4f, smallest target margin %.3f" % (losses[0], losses[-1], float((top - rest).min())))
    assert (top - rest).min() > 1.0


def test_float32_trajectory_of_the_mixed_objective_stays_close_to_fp64():
    """Twenty Adam steps of ctc + 0.5 ce with class weights on ref_shape: float32 arithmetic alone stays within 1e-3 of the parameter
    scale and the parameters really move, so the GPU test's bound of 4 x that drift has teeth."""
    _, path64 = F.gru_trajectory()
    _, path32 = F.gru_trajectory(float32=True)
    start = M.blob_of(M.make_problem(F.TRAJECTORY["name"])["w"])
    moved = float(np.abs(path64[-1] - start).max())
    drift = max(float(np.abs(a - b).max()) for a, b in zip(path32, path64))
    assert drift <= 1e-3 * _scale(path64[-1]), (drift, _scale(path64[-1]))
    assert moved >= 100 * drift, (moved, drift)
