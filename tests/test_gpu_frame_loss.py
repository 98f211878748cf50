"""kws_frame_loss (custom_keyword.frame_loss) on the device against the fp64 restatement tests/frame_loss_model.py, with the deviation of
the same restatement evaluated in float32 on the CPU as the yardstick: per tensor, bound = max(4 x that deviation, 16 * 2^-23 *
max|reference|) -- the project's bound (tests/test_gpu_train.py).  Every comparison prints a FRAME-RATIO line (kernel / float32-CPU /
bound) before it asserts.  What has to hold to the bit is compared as uint32."""
import numpy as np
import pytest
import torch

import frame_loss_model as F

pytestmark = pytest.mark.gpu
FLOOR = 16 * 2.0 ** -23


def _report(what, name, got, ref64, ref32):
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    bound = max(4.0 * dev, FLOOR * float(np.abs(ref64).max()))
    err = float(np.abs(np.asarray(got, np.float64) - ref64).max())
    print("FRAME-RATIO %s %s: kernel %.3e  float32-CPU %.3e  bound %.3e  kernel/bound %.3f" % (what, name, err, dev, bound, err / bound if bound > 0 else 0.0))
    return err, bound


def _run(p, logits=None, targets=None, seq_len=None, want_grad=True):
    from keyword_spotting_amd.custom_keyword import frame_loss
    loss, grad = frame_loss(p["logits"] if logits is None else logits, p["seq_len"] if seq_len is None else seq_len,
                            p["targets"] if targets is None else targets, p["weight"], want_grad=want_grad)
    return loss.cpu().numpy(), (grad.cpu().numpy() if want_grad else None)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_new_entry_points_exist():
    from keyword_spotting_amd import _lib, custom_keyword
    lib = _lib.load()
    for sym in ("kws_frame_loss", "kws_sizeof_frame_targets"):
        assert hasattr(lib, sym), sym
    assert callable(custom_keyword.frame_loss)


@pytest.mark.parametrize("name", sorted(F.KERNEL_CASES))
def test_kernel_against_the_restatement(name):
    p = F.kernel_problem(name)
    (ce64, g64), (ce32, g32) = p["ref64"], p["ref32"]
    loss, grad = _run(p)
    loss_only, none = _run(p, want_grad=False)
    assert none is None and _same(loss, loss_only)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    err, bound = _report("loss", name, loss, ce64, ce32)
    assert err <= bound
    err, bound = _report("grad", name, grad, g64, g32)
    assert err <= bound
    live = np.arange(p["T"])[None, :] < p["seq_len"][:, None]
    assert not grad[~live].any()                                         # rows at t >= seq_len: exactly 0
    assert not grad[live & (p["targets"] < 0)].any()                     # ... and the unlabelled rows
    if p["weight"] is not None and (p["weight"] == 0).any():             # a class of weight 0 has a gradient of exactly 0 too
        zero = live & (p["targets"] >= 0) & (p["weight"][np.clip(p["targets"], 0, None)] == 0)
        assert zero.any() and not grad[zero].any()
    if p["B"] == 17:
        assert loss[3] == 0 and loss[5] == 0 and not grad[3].any() and not grad[5].any() and loss[7] > 0


@pytest.mark.parametrize("name", ["t65_c3_b17", "t300_c3_b17", "t33_c3_b17"])
def test_an_utterance_alone_has_the_bits_it_has_inside_a_batch(name):
    p = F.kernel_problem(name)
    loss, grad = _run(p)
    for i in (0, 3, 7, 16):
        one_loss, one_grad = _run(p, p["logits"][i:i + 1], p["targets"][i:i + 1], p["seq_len"][i:i + 1])
        assert _same(one_loss, loss[i:i + 1]) and _same(one_grad, grad[i:i + 1]), i


def test_nan_and_garbage_past_seq_len_give_the_bits_of_zero_padding_and_calls_repeat_bitwise():
    p = F.kernel_problem("t257_c8_b17")
    live = np.arange(p["T"])[None, :] < p["seq_len"][:, None]
    rng = np.random.default_rng(0)
    zero_logits = np.where(live[:, :, None], p["logits"], np.float32(0))
    nan_logits = np.where(live[:, :, None], p["logits"], np.float32(np.nan))
    junk = np.where(live, p["targets"], rng.integers(-2 ** 31, 2 ** 31 - 1, size=live.shape)).astype(np.int32)
    clean = np.where(live, p["targets"], -1).astype(np.int32)
    want = _run(p, zero_logits, clean)
    got = _run(p, nan_logits, torch.from_numpy(junk).cuda())             # a device tensor: nothing on the host looks at it
    again = _run(p, nan_logits, torch.from_numpy(junk).cuda())
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert _same(want[0], got[0]) and _same(want[1], got[1]) and _same(got[0], again[0]) and _same(got[1], again[1])


@pytest.mark.parametrize("name", ["t65_c3_b17", "t40_c8_b17", "t33_c3_b17"])
def test_logits_and_targets_one_element_past_a_16_byte_boundary_give_the_same_bits(name):
    """Rows of C floats are 4-byte aligned and no more: the same values from a base 4 bytes past a 16-byte boundary."""
    from keyword_spotting_amd.custom_keyword import frame_loss
    p = F.kernel_problem(name)
    lg = torch.from_numpy(p["logits"]).cuda()
    tg = torch.from_numpy(p["targets"]).cuda()
    lg_store = torch.empty(1 + lg.numel(), dtype=torch.float32, device="cuda")
    tg_store = torch.empty(1 + tg.numel(), dtype=torch.int32, device="cuda")
    lg_store[1:], tg_store[1:] = lg.reshape(-1), tg.reshape(-1)
    lg_off, tg_off = lg_store[1:].view(lg.shape), tg_store[1:].view(tg.shape)
    assert lg.data_ptr() % 16 == 0 and tg.data_ptr() % 16 == 0 and lg_off.data_ptr() % 16 == 4 and tg_off.data_ptr() % 16 == 4
    want = frame_loss(lg, p["seq_len"], tg, p["weight"])
    got = frame_loss(lg_off, p["seq_len"], tg_off, p["weight"])
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert _same(want[1].cpu().numpy(), got[1].cpu().numpy())


def test_a_target_out_of_range_on_the_device_is_loud_and_harmless():
    """A device tensor cannot be checked on the host.  A value outside [-1, C) at a live frame: that utterance's loss is NaN, its gradient
    rows are those of the same targets with -1 there, and the other utterances keep their bits."""
    p = F.kernel_problem("t65_c3_b17")
    b, t = 16, 40                                                        # the full-length utterance; utterance 9 has 21 frames at least
    assert p["seq_len"][b] > t and p["seq_len"][9] > 0
    bad, none = p["targets"].copy(), p["targets"].copy()
    bad[b, t], none[b, t] = p["C"], -1
    bad[9, 0], none[9, 0] = -2, -1
    want_loss, want_grad = _run(p, targets=none)
    loss, grad = _run(p, targets=torch.from_numpy(bad).cuda())
    assert np.isnan(loss[[b, 9]]).all() and np.isfinite(np.delete(loss, [b, 9])).all()
    assert _same(np.delete(loss, [b, 9]), np.delete(want_loss, [b, 9]))
    assert np.isfinite(grad).all() and _same(grad, want_grad)
    from keyword_spotting_amd import _lib
    with pytest.raises(_lib.InvalidArgumentError, match="targets outside"):          # the same array from the host is refused
        _run(p, targets=bad)
