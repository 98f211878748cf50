"""CPU checks of the bank of enrolled heads (kws_bank): the fp64 restatement tests/bank_model.py against tests/heads_model.py on
weights.extend_head weights, a stream without a slot, every refusal that needs no live handle -- by code and message, none reaching the
device probe --, KeywordBank's refusals, and the bound symbols.  (Refusals that need live handles: tests/test_gpu_bank_stream.py.)"""
import ctypes
import types

import numpy as np
import pytest

import bank_model as BM
import heads_model as HM
from oracle import gru_oracle as G


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.parametrize("c,n_new", [(6, 2), (6, 1), (3, 5)])
def test_one_slot_for_all_equals_heads_model_on_extend_head_weights(c, n_new):
    from keyword_spotting_amd import weights
    hidden, b, t = 64, 5, 9
    w = G.random_weights(13, hidden, 2, c, seed=3)
    cols, bias = BM.random_bank(hidden, n_new, 3, seed=4)
    mel = G.synthetic_mel(b, t, 13, seed=5)
    st = (0.3 * np.random.default_rng(6).standard_normal((2, b, hidden))).astype(np.float32)
    lens = np.array([0, 1, t - 1, t, t], np.int64)
    for relu, clip in ((False, -1.0), (True, 20.0)):
        for u in range(3):
            got = BM.bank_forward(w, cols, bias, np.full(b, u), mel, st, lens, use_relu=relu, value_clip=clip)
            w2 = dict(w)
            w2["Wfc2"], w2["bfc2"] = weights.extend_head(w["Wfc"], w["bfc"], cols[u], bias[u])
            want = HM.heads_forward(w2, mel, st, lens, use_relu=relu, value_clip=clip)
            for k in ("top", "state", "logits1", "softmax1", "logits2", "softmax2"):
                assert np.abs(got[k] - want[k]).max() <= 1e-12, (k, u, relu)
    # rows past seq_len: head 2's new classes are exactly bn[u]
    got = BM.bank_forward(w, cols, bias, np.full(b, 1), mel, st, lens)
    assert np.array_equal(got["logits2"][0, :, c - 1:c - 1 + n_new], np.broadcast_to(bias[1].astype(np.float64), (t, n_new)))


def test_a_stream_without_a_slot_is_a_plain_one_head_stream():
    hidden, b, t, c, n_new = 64, 4, 30, 6, 2
    w = G.random_weights(13, hidden, 1, c, seed=7)
    w["Wfc"] = (w["Wfc"] * 3).astype(np.float32)
    cols, bias = BM.random_bank(hidden, n_new, 2, seed=8, scale=3.0)
    mel = G.synthetic_mel(b, t, 13, seed=9)
    users = np.array([0, -1, 2, 1])                   # 2: out of range, reads as -1
    r = BM.bank_forward(w, cols, bias, users, mel)
    ref = G.softmax(G.gru_forward(w, mel, dtype=np.float64)[0])
    assert np.abs(r["softmax1"] - ref).max() <= 1e-12
    for s in (1, 2):
        assert not r["logits2"][s].any() and not r["softmax2"][s].any()
        assert not HM.frame_tokens(r["softmax2"][s], c + n_new, 0.0)[0].any()          # no word at any threshold
    assert r["softmax2"][0].any() and r["softmax2"][3].any()
    # the policy loop: such a stream never reports head 2, and its head 1 is what a stream with a slot and the same audio reports
    # until one of them fires
    chunks = [10, 0, 10, 10]
    pol = BM.policy_loop(w, cols, bias, np.array([-1, 5, 0, 1]), mel, chunks, np.ones((4, b), bool), ("1", "5"), (0.4, 0.4), 2)
    assert not (pol["mask"][:, :2] & 2).any()


def test_refusals_come_before_the_device():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_bank_create", "kws_bank_destroy", "kws_bank_set", "kws_bank_get", "kws_step_bank", "kws_stream_create_bank",
                "kws_step_bank_window"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTED_SYMBOLS
    bad, h = _lib.KWS_ERR_INVALID_ARGUMENT, ctypes.c_void_p()
    err = lambda: lib.kws_last_error().decode()
    assert lib.kws_bank_create(128, 6, 2, 4, None) == bad
    assert lib.kws_bank_create(100, 6, 2, 4, ctypes.byref(h)) == _lib.KWS_ERR_UNSUPPORTED and "hidden=100" in err()
    for c, n in ((6, 3), (2, 1), (6, 0), (8, 1), (3, 6)):
        assert lib.kws_bank_create(128, c, n, 4, ctypes.byref(h)) == bad and "C=%d n_new=%d" % (c, n) in err(), (c, n)
    assert lib.kws_bank_create(128, 6, 2, 0, ctypes.byref(h)) == bad and "capacity=0" in err()
    assert not h.value
    if not have_gpu():
        assert lib.kws_bank_create(128, 6, 2, 4, ctypes.byref(h)) == _lib.KWS_ERR_NO_DEVICE
    assert lib.kws_bank_destroy(None) == _lib.KWS_OK
    dummy = ctypes.c_void_p(256)                      # a non-null address that is no live handle and is never read
    for fn in (lib.kws_bank_set, lib.kws_bank_get):
        assert fn(None, 0, 1, dummy, dummy, None) == bad and "bank is null" in err()
        assert fn(dummy, 0, 1, dummy, dummy, None) == bad and "not alive" in err()
    # kws_step_bank: null model / bank / user; handles that are not alive
    def step(model=dummy, bank=dummy, user=dummy):
        return lib.kws_step_bank(model, bank, user, dummy, dummy, dummy, None, None, None, None, None, 1, 1, None)
    assert step(model=None) == bad and step(bank=None) == bad and "bank or user is null" in err() and step(user=None) == bad
    assert step() == bad and "not alive" in err()
    # kws_stream_create_bank: no out pointer; null arguments (out is cleared); handles that are not alive
    def create(out, model=dummy, fe=dummy, w1=dummy, w2=dummy, bank=dummy, user=dummy, l1=b"12", l2=b"5", state=dummy, restart=dummy):
        return lib.kws_stream_create_bank(model, fe, w1, w2, bank, user, 1, 3600, 30.0, l1, l2, state, restart, out)
    assert create(None) == bad
    for hole in ("model", "fe", "w1", "w2", "bank", "user", "l1", "l2", "state", "restart"):
        out = ctypes.c_void_p(7)
        assert create(ctypes.byref(out), **{hole: None}) == bad, hole
        assert out.value is None
    out = ctypes.c_void_p(7)
    assert create(ctypes.byref(out)) == bad and "not alive" in err() and out.value is None
    # kws_step_bank_window: null model; null bank / user / windows / labels / hit / state / mel; bad shapes; handles that are not alive
    def window(model=dummy, b=1, t=1, **kw):
        a = dict(bank=dummy, user=dummy, mel=dummy, si=dummy, so=dummy, w1=dummy, w2=dummy, l1=b"12", l2=b"5", hit=dummy)
        a.update(kw)
        return lib.kws_step_bank_window(model, a["bank"], a["user"], a["mel"], a["si"], a["so"], None, b, t, a["w1"], a["w2"], a["l1"], a["l2"],
                                        None, None, None, a["hit"], None, None)
    assert window(model=None) == bad and "handle is null" in err()
    for hole in ("bank", "user", "mel", "si", "so", "w1", "w2", "l1", "l2", "hit"):
        assert window(**{hole: None}) == bad and "null pointer" in err(), hole
    assert window(b=0) == bad and "bad shape" in err() and window(t=-1) == bad
    assert window() == bad and "not alive" in err()


def _fake_model(**kw):
    from keyword_spotting_amd import get_config
    num_classes2 = kw.pop("num_classes2", 0)
    return types.SimpleNamespace(config=get_config(**kw), num_classes2=num_classes2, wrappers=(False, False), device="cuda:0")


def test_keyword_bank_refuses_what_the_enroller_refuses():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.custom_keyword import KeywordBank
    with pytest.raises(_lib.UnsupportedError, match="use_relu"):
        KeywordBank(_fake_model(use_relu=True), 2, 4)
    with pytest.raises(_lib.InvalidArgumentError, match="second head"):
        KeywordBank(_fake_model(num_classes2=8), 2, 4)
    for precision in ("bf16", "int8", "f16x3"):
        with pytest.raises(_lib.UnsupportedError, match="fp32"):
            KeywordBank(_fake_model(precision=precision), 2, 4)
    wrapped = _fake_model()
    wrapped.wrappers = (True, False)
    with pytest.raises(_lib.UnsupportedError, match="wrapped"):
        KeywordBank(wrapped, 2, 4)
    with pytest.raises(_lib.InvalidArgumentError, match="n_new=3"):
        KeywordBank(_fake_model(), 3, 4)              # 6 + 3 classes
    with pytest.raises(_lib.InvalidArgumentError, match="capacity=0"):
        KeywordBank(_fake_model(), 2, 0)


def test_bank_and_users_go_together_before_any_device_call():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.detector import _bank_model
    model = object()
    assert _bank_model(model, None, None, None, 4) == (model, None)
    with pytest.raises(_lib.InvalidArgumentError, match="users needs bank"):
        _bank_model(model, None, [0, 1, 2, 3], "5", 4)
    bank = types.SimpleNamespace(stack=object(), device="cpu", model=model)
    with pytest.raises(_lib.InvalidArgumentError, match="bank needs users"):
        _bank_model(model, bank, None, "5", 4)
    with pytest.raises(_lib.InvalidArgumentError, match="bank needs users"):
        _bank_model(model, bank, [0, 1, 2, 3], None, 4)
    with pytest.raises(_lib.InvalidArgumentError, match=r"users must be \[4\]"):
        _bank_model(model, bank, [0, 1, 2], "5", 4)
    stack, users = _bank_model(model, bank, [0, -1, 2, 3], "5", 4)
    assert stack is bank.stack and users.tolist() == [0, -1, 2, 3]
    assert _bank_model(None, bank, [0, -1, 2, 3], "5", 4)[0] is bank.stack              # None: the bank's own model
    with pytest.raises(_lib.InvalidArgumentError, match="not the model this bank was built on"):
        _bank_model(object(), bank, [0, -1, 2, 3], "5", 4)


def test_stream_server_passes_bank_and_users_through(monkeypatch):
    from keyword_spotting_amd import serving

    class Stub(object):
        def __init__(self, *a, **kw):
            self.args, self.kw = a, kw

        def close(self):
            pass
    for name in ("DeployModel", "MelFrontend", "StreamManager"):
        monkeypatch.setattr(serving, name, Stub)
    monkeypatch.setattr(serving.torch.cuda, "Stream", lambda device=None: None)
    bank = object()
    srv = serving.StreamServer(object(), weights={}, handles=1, label="12", label2="5", bank=bank, users=lambda k: [k] * 4)
    assert srv._banks == [bank] and srv._users(3) == [3] * 4 and srv._mgr_args["label2"] == "5"
    with pytest.raises(ValueError):
        serving.StreamServer(object(), weights={}, handles=1, label="12", label2="5", bank=bank)
    with pytest.raises(ValueError):
        serving.StreamServer(object(), weights={}, handles=2, label="12", label2="5", bank=[bank], users=lambda k: [0])
