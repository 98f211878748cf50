"""CPU checks of the enrolment fit on frame-wise targets: the fp64 restatement tests/enroll_frames_model.py against the torch fp64 graph
(F.ctc_loss + F.cross_entropy on the spliced logits, autograd with respect to the new columns and their bias only) and against central
differences; frame_weight 0 is tests/enroll_model.py's step to the last bit; every refusal of kws_enroll_check_frames by code and
message; extend_targets and the frame_targets round trip; and the two end-to-end claims tests/test_gpu_enroll_frames.py makes on the
device, established here on the restatement with the seeds, steps and weights recorded in enroll_frames_model.FLOW_A / FLOW_B."""
import ctypes
import functools

import numpy as np
import pytest

import align_model as AL
import enroll_frames_model as EF
import enroll_model as M


@pytest.mark.parametrize("objective", sorted(EF.OBJECTIVES))
@pytest.mark.parametrize("name", sorted(EF.CASES))
def test_restatement_matches_torch_fp64(name, objective):
    import torch
    p = EF.make_problem(name)
    got, want = EF.step64(p, objective), EF.torch_reference(p, torch.float64, *EF.OBJECTIVES[objective])
    finite = np.isfinite(got["loss"])
    assert np.abs(np.where(finite, got["loss"], 0.0) - np.where(finite, want["loss"], 0.0)).max() <= 1e-10
    assert np.abs(got["ce"] - want["ce"]).max() <= 1e-10
    assert np.abs(got["gW"] - want["gW"]).max() <= 1e-10 and np.abs(got["gb"] - want["gb"]).max() <= 1e-10
    if objective == "ce":
        assert finite.all()
    if name == "t2_k3_no_path" and objective != "ce":
        assert list(finite) == [True, False, True] and got["loss"][1] == np.inf
        # ... and the slot without a path still contributes its frame term: alone, its gradient is the frame loss's
        q = dict(p, seq_len=np.array([0, 2, 0], np.int32))
        cw, fw = EF.OBJECTIVES[objective]
        alone, ce_only = EF.step64(q, objective), EF.step64(q, "ce")
        assert np.abs(alone["gW"] - fw * ce_only["gW"]).max() <= 1e-15 and np.abs(alone["gW"]).max() > 1e-3
        assert np.abs(alone["gW"] - EF.torch_reference(q, torch.float64, cw, fw)["gW"]).max() <= 1e-10
    if name == "t33_k3_all_none":
        assert got["ce"][2] == 0.0          # W_b == 0: loss 0 (and no NaN anywhere)
        assert np.isfinite(got["gW"]).all()
    if name == "t9_k4_empty_slot":
        assert got["loss"][2] == 0.0 and got["ce"][2] == 0.0


def test_restatement_matches_central_differences():
    p = EF.make_problem("t9_k4_empty_slot")
    cw, fw = EF.OBJECTIVES["mixed_03_2"]
    _, lab_len = M.padded_labels(p["labels"])

    def objective(wn, bn):
        return EF.loss_grad(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, p["targets"], p["weight"], wn, bn, cw, fw)[0].sum() / p["K"]
    r = EF.step64(p, "mixed_03_2")
    wn, bn, eps = p["wn"].astype(np.float64), p["bn"].astype(np.float64), 1e-6
    for (i, j) in ((0, 0), (17, 3), (63, 4), (30, 1)):
        d = np.zeros_like(wn)
        d[i, j] = eps
        fd = (objective(wn + d, bn) - objective(wn - d, bn)) / (2 * eps)
        assert abs(fd - r["gW"][i, j]) <= 1e-7 * max(1.0, abs(fd)), (i, j, fd, r["gW"][i, j])
    for j in range(p["n"]):
        d = np.zeros_like(bn)
        d[j] = eps
        fd = (objective(wn, bn + d) - objective(wn, bn - d)) / (2 * eps)
        assert abs(fd - r["gb"][j]) <= 1e-7 * max(1.0, abs(fd)), (j, fd, r["gb"][j])


def test_trajectory_matches_torch_fp64():
    p = EF.make_problem("t33_k3_all_none")
    cw, fw = EF.OBJECTIVES["mixed"]
    _, lab_len = M.padded_labels(p["labels"])
    _, _, trace, ce, path = EF.fit(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, p["targets"], p["weight"], p["wn"], p["bn"], 5,
                                   0.01, cw, fw)
    want_trace, want_path = EF.torch_fit(p, 5, 0.01, cw, fw, np.float64)
    assert np.abs(trace - want_trace).max() <= 1e-9
    for (w, b), (ww, wb) in zip(path, want_path):
        assert np.abs(w - ww).max() <= 1e-9 and np.abs(b - wb).max() <= 1e-9
    assert (ce[-1][:2] < ce[0][:2]).all()          # the frame term falls on the slots that have targets


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_frame_weight_zero_is_the_ctc_step_to_the_last_bit(name):
    p = M.make_problem(name)
    _, lab_len = M.padded_labels(p["labels"])
    targets = np.zeros((p["K"], p["T"]), np.int32)          # never read
    want = M.enroll_loss_grad(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, p["wn"], p["bn"])
    loss, ce, gw, gb = EF.loss_grad(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, targets, None, p["wn"], p["bn"], 1.0, 0.0)
    assert np.array_equal(loss, want[0]) and np.array_equal(gw, want[1]) and np.array_equal(gb, want[2]) and not ce.any()
    if name == "repeats_k4":
        a = M.fit(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, p["wn"], p["bn"], 3, 0.01)
        b = EF.fit(p["nn"], p["logits1"], p["seq_len"], p["labels"], lab_len, targets, None, p["wn"], p["bn"], 3, 0.01, 1.0, 0.0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---- kws_enroll_check_frames ---------------------------------------------------------------------------------------------------------

_KEEP = []


def _i32(*v):
    a = np.array(v, np.int32)
    _KEEP.append(a)
    return a.ctypes.data_as(ctypes.c_void_p)


def test_every_refusal_of_check_frames_by_code_and_message():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    bad, unsupported, ok = _lib.KWS_ERR_INVALID_ARGUMENT, _lib.KWS_ERR_UNSUPPORTED, _lib.KWS_OK
    x = 256                                   # a non-null, aligned address that is never read
    seq, lens, labels = _i32(4, 4, 3), _i32(2, 1, 0), _i32(1, 6, 0, 0, 0, 0)

    def targets(tg=x, cw=1.0, fw=1.0, class_weight=None, frame_loss=None):
        w = None
        if class_weight is not None:
            w = np.asarray(class_weight, np.float32)
            _KEEP.append(w)
        return _lib.KwsFrameTargets(tg, None if w is None else w.ctypes.data, cw, fw, frame_loss)

    def call(h=128, c=6, n=2, e=1, k=3, seq=seq, labels=labels, lens=lens, t=4, s_max=2, ft=None, lr=0.01, iterations=1, **kw):
        ft = targets(**kw) if ft is None else ft
        return lib.kws_enroll_check_frames(h, c, n, e, k, seq, labels, lens, t, s_max, ctypes.byref(ft) if ft != "null" else None, lr, iterations)

    def refused(code, text, **kw):
        assert call(**kw) == code, kw
        assert text.encode() in lib.kws_last_error(), (kw, lib.kws_last_error())

    assert call() == ok and call(cw=0.0) == ok and call(cw=1.0, fw=0.0) == ok and call(cw=0.3, fw=2.0) == ok
    # the shape, as kws_enroll_create
    refused(unsupported, "hidden=100", h=100)
    for c, n in ((6, 3), (2, 1), (6, 0), (8, 1)):
        refused(bad, "C=%d n_new=%d" % (c, n), c=c, n=n)
    refused(bad, "E=0", e=0)
    refused(bad, "K=5", k=5)
    refused(bad, "K=0", k=0)
    # the frame targets
    refused(bad, "frame targets are null", ft="null")
    refused(bad, "ft->targets is null", tg=None)
    refused(bad, "ft->ctc_weight=-1", cw=-1.0)
    refused(bad, "ft->ctc_weight=nan", cw=float("nan"))
    refused(bad, "ft->frame_weight=inf", fw=float("inf"))
    refused(bad, "ft->frame_weight=-0.5", fw=-0.5)
    refused(bad, "both 0", cw=0.0, fw=0.0)
    refused(bad, "takes ft->ctc_weight=1, not 0.5", cw=0.5, fw=0.0)
    refused(bad, "4-byte aligned", tg=258)
    refused(bad, "4-byte aligned", frame_loss=257)
    refused(bad, "class_weight[1]=-1", class_weight=[1, -1, 1, 1, 1, 1, 1, 1])
    refused(bad, "class_weight[7]=inf", class_weight=[1, 1, 1, 1, 1, 1, 1, np.inf])
    assert call(class_weight=[1, 0, 1, 1, 2, 1, 1, 1]) == ok
    # the call, as kws_enroll_fit
    refused(bad, "bad shape T=0", t=0)
    refused(bad, "bad shape", s_max=-1)
    refused(bad, "S_max=32", s_max=32)
    refused(bad, "iterations=0", iterations=0)
    refused(bad, "lr=0", lr=0.0)
    refused(bad, "lr=", lr=float("inf"))
    refused(bad, "null pointer", seq=None)
    refused(bad, "null pointer", labels=None)
    refused(bad, "null pointer", lens=None)
    refused(bad, "seq_len[1]=5", seq=_i32(4, 5, 3))
    refused(bad, "seq_len[1]=5", seq=_i32(4, 5, 3), cw=0.0)
    refused(bad, "label_len[0]=3", lens=_i32(3, 1, 0))
    refused(bad, "labels[0][1]=7 outside [0,6]", labels=_i32(1, 7, 0, 0, 0, 0))          # 7 is the blank of the extended head
    # 4 x 300 x 71 floats next to 7 x 129 x 2 of parameters: refused with the CTC term, with the byte counts ...
    big = dict(k=4, t=300, s_max=31, seq=_i32(300, 300, 300, 300), lens=_i32(0, 0, 0, 0), labels=_i32(*([0] * 124)))
    refused(unsupported, "348024 bytes exceed the 163840", **big)
    refused(unsupported, "348024 bytes exceed the 163840", cw=0.3, fw=2.0, **big)
    # ... and at ctc_weight 0 nothing about T, S_max or the labels is: the parameter block alone, whatever T is
    assert call(cw=0.0, **big) == ok
    assert call(cw=0.0, k=1, t=4000, seq=_i32(4000)) == ok
    assert call(k=1, t=4000, seq=_i32(4000), lens=_i32(0), labels=_i32(0, 0)) == unsupported
    assert call(cw=0.0, labels=None, lens=None, s_max=0) == ok and call(cw=0.0, labels=None, lens=None, s_max=32) == ok
    assert call(cw=0.0, labels=_i32(9, 9, 9, 9, 9, 9), lens=_i32(7, 7, 7)) == ok
    refused(unsupported, "2^31", e=1 << 20, k=4, t=1024, cw=0.0)           # decided before seq_len is read
    # the entry point itself, before a device is needed
    assert lib.kws_enroll_fit_frames(None, None, None, None, None, None, 4, 2, None, 0.01, 1, None, None) == bad
    assert b"handle is null" in lib.kws_last_error()


# ---- extend_targets, frame_targets --------------------------------------------------------------------------------------------------

def test_extend_targets_renumbers_the_blank_only():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.custom_keyword import extend_targets
    t = np.array([[-1, 0, 1, 4, 5, 5, -1], [5, 2, 3, -1, -1, 0, 5]], np.int32)
    got = extend_targets(t, 6, 2)
    assert got.dtype == np.int32 and got.tolist() == [[-1, 0, 1, 4, 7, 7, -1], [7, 2, 3, -1, -1, 0, 7]]
    assert np.array_equal(got, EF.extend_targets(t, 6, 2))
    assert extend_targets(np.array([[2, 0, -1]]), 3, 5).tolist() == [[7, 0, -1]]
    for wrong in (np.array([[6]]), np.array([[-2]]), np.array([[0.5]])):
        with pytest.raises(_lib.InvalidArgumentError, match="targets outside"):
            extend_targets(wrong, 6, 2)
    with pytest.raises(_lib.InvalidArgumentError, match="C=6 n_new=3"):
        extend_targets(t, 6, 3)


def test_frame_targets_round_trip_on_the_restatement():
    """frame_targets of a fitted head collapse back to the labels they were aligned with, use the extended head's blank, and are what
    custom_keyword.frame_labels makes of the same states."""
    from keyword_spotting_amd.custom_keyword import frame_labels
    p = M.make_problem("repeats_k4")
    c2 = p["C"] + p["n"]
    tg = EF.frame_targets(p["nn"], p["logits1"], p["seq_len"], p["labels"], p["wn"].astype(np.float64), p["bn"].astype(np.float64))
    z = M.splice(p["logits1"].astype(np.float64), p["nn"].astype(np.float64) @ p["wn"] + p["bn"])
    states = np.stack([AL.align(z[i], p["seq_len"][i], p["labels"][i])["states"] for i in range(p["K"])])
    assert np.array_equal(tg, frame_labels(states, p["labels"], c2 - 1))
    for i in range(p["K"]):
        n = p["seq_len"][i]
        assert (tg[i, n:] == -1).all() and (tg[i, :n] >= 0).all() and (tg[i, :n] < c2).all()
        assert [int(v) for v in AL.collapse(tg[i, :n], c2 - 1)] == p["labels"][i]


# ---- the end-to-end claims, on the restatement -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _flow_a(seed):
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.custom_keyword import truncated_normal
    from keyword_spotting_amd.prediction import ctc_label
    from oracle import decode_oracle as D
    from oracle import gru_oracle as G
    a = EF.FLOW_A
    cfg = get_config(label_dict=a["label_dict"])
    w = weights.init_weights(cfg, seed=seed)
    mel = G.synthetic_mel(3, a["frames"], cfg.n_mel, seed=seed + 10)
    nn, l1 = EF.features(w, mel)
    c, n = cfg.num_classes, a["n_new"]
    labels, seq_len = [list(ctc_label(a["words"]))] * 3, np.full(3, a["frames"])
    lab_len = np.full(3, len(labels[0]))
    init = truncated_normal((1, cfg.hidden_size, n), seed)[0]
    wn, bn, _, _ = M.fit(nn, l1, seq_len, labels, lab_len, init, np.zeros(n), a["ctc_steps"], a["lr"])
    targets = EF.frame_targets(nn, l1, seq_len, labels, wn, bn)
    wn, bn, _, ce, _ = EF.fit(nn, l1, seq_len, None, None, targets, None, init, np.zeros(n), a["frame_steps"], a["lr"], 0.0, 1.0)
    sm = np.exp(M.log_softmax(M.splice(l1, nn @ wn + bn)))
    # predict_ctc's head 2: ctc_decode called with the class count in lockout's place (server_demo.py:104-130)
    return c, targets, ce, [D.ctc_predict(D.ctc_decode(sm[i], c + n), a["keyword"]) for i in range(3)]


@pytest.mark.parametrize("seed", EF.FLOW_A["seeds"])
def test_flow_a_frames_only_from_a_fresh_start_finds_the_keyword(seed):
    c, targets, ce, hits = _flow_a(seed)
    assert c == 4 and set(np.unique(targets)) <= {0, 3, 4, 5} and {3, 4} <= set(np.unique(targets))
    assert (ce[-1] < 0.5 * ce[0]).all()
    assert hits == [1, 1, 1]


@functools.lru_cache(maxsize=None)
def _flow_b(seed):
    from keyword_spotting_amd import get_config, weights
    from keyword_spotting_amd.custom_keyword import truncated_normal
    from keyword_spotting_amd.prediction import ctc_label
    from oracle import gru_oracle as G
    b = EF.FLOW_B
    cfg = get_config()
    w = weights.init_weights(cfg, seed=seed)
    mel = np.concatenate([G.synthetic_mel(3, b["frames"], cfg.n_mel, seed=seed + 10), G.synthetic_mel(1, b["frames"], cfg.n_mel, seed=seed + 20)])
    nn, l1 = EF.features(w, mel)
    c, n = cfg.num_classes, b["n_new"]
    labels, seq_len = [list(ctc_label(b["words"]))] * 3, np.full(4, b["frames"])
    init = truncated_normal((1, cfg.hidden_size, n), seed)[0]
    wn, bn, _, _ = M.fit(nn[:3], l1[:3], seq_len[:3], labels, np.full(3, len(labels[0])), init, np.zeros(n), b["steps"], b["lr"])
    before = EF.new_mass(nn, l1, seq_len, wn, bn)
    pos = EF.frame_targets(nn[:3], l1[:3], seq_len[:3], labels, wn, bn)
    states = AL.align(l1[3], seq_len[3], b["negative_label"])["states"]
    neg = EF.extend_targets(AL.frame_classes(states, b["negative_label"], c - 1)[None], c, n)
    labels = labels + [b["negative_label"]]
    wn, bn, _, _, _ = EF.fit(nn, l1, seq_len, labels, np.array([len(l) for l in labels]), np.concatenate([pos, neg]), None, wn, bn,
                             b["refit_steps"], b["lr"], 1.0, 1.0)
    return before, EF.new_mass(nn, l1, seq_len, wn, bn), neg


@pytest.mark.parametrize("seed", EF.FLOW_B["seeds"])
def test_flow_b_a_negative_in_a_spare_slot_lowers_the_new_classes_mass_on_it(seed):
    before, after, neg = _flow_b(seed)
    assert set(np.unique(neg)) <= {0, 4, 7}          # head 1's transcript 0 4 0 and the extended head's blank: no new class anywhere
    assert after[3] < before[3], (before, after)
