"""kws_step across the configuration space kws_create accepts, against the fp64 oracle (tests/config_space_grid.py holds
the grid and restates the launch-layout choice).  Each row runs one kernel family in one launch layout, asserted through
kernel_names(), at a class count, input width, depth and relu / clip setting the rest of the suite does not reach:

  fp32 / f16x3  logits and state within 1e-4 of gru_forward(float64), softmax within 2e-5, the C oracle likewise, the
                fused ctc_decode2 tokens and their carried word against the oracle's softmax
  bf16          gru_forward_bf16, the tolerances of test_gpu_bf16.py
  int8          gru_forward_octbit, the tolerances of test_gpu_octbit_gru.py
  relu rows     the same tolerances x 20 (the projection is scaled by 20 so that logits cross the clip at 20)

plus rows past seq_len == bfc bit for bit, chunked == one call bit for bit, and the overlapped / pipelined layouts bit for
bit against the sequential launches on shared streams."""
import numpy as np
import pytest
import torch

from oracle import decode_oracle as D
from oracle import gru_oracle as G
from tests import config_space_grid as S

pytestmark = pytest.mark.gpu
TOL = 1e-4
THRES = 0.4


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def weights_of(row):
    w = G.random_weights(row.n_mel, row.hidden, row.layers, row.classes, seed=S.seed_of(row))
    w["Wfc"] = (w["Wfc"] * np.float32(row.wfc)).astype(np.float32)
    return w


_models = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def _model(row):
    """One model per row: the row's own call, its chunked calls and its twin batch share it."""
    from keyword_spotting_amd import get_config
    from keyword_spotting_amd.rnn_ctc import DeployModel
    key = row.name
    if key not in _models:
        cfg = get_config(n_mel=row.n_mel, hidden_size=row.hidden, num_layers=row.layers, precision=row.prec,
                         use_relu=bool(row.relu), value_clip=row.clip)
        cfg.label_dict = {str(k): k for k in range(1, row.classes - 2)}
        assert cfg.num_classes == row.classes
        _models[key] = DeployModel(cfg, weights_of(row), kernel=row.kernel)
    return _models[key]


def inputs(row, batch=None, frames=None):
    b, t = batch or row.batch, frames or row.frames
    rng = np.random.default_rng(S.seed_of(row) + 1)
    mel = G.synthetic_mel(b, t, row.n_mel, seed=S.seed_of(row) + 2)
    st0 = (0.5 * rng.standard_normal((row.layers, b, row.hidden))).astype(np.float32)
    lens = reset = None
    if row.masks:
        lens = rng.integers(0, t + 1, b).astype(np.int32)
        lens[:3] = [0, t, 1][:b]
        reset = (rng.random(b) < 0.4).astype(np.uint8)
    return mel, st0, lens, reset


def _relu(logits, row):
    if not row.relu:
        return logits
    out = np.maximum(logits, 0.0)
    return np.minimum(out, 20.0) if row.clip > 0 else out


def reference(row, mel, st0, lens, reset):
    """(logits, state) of the row's precision on these inputs, in float64 where the precision allows."""
    st = st0 if reset is None else st0 * (1 - reset)[None, :, None].astype(np.float32)
    w = weights_of(row)
    if row.prec in ("fp32", "f16x3"):
        return G.gru_forward(w, mel, st, seq_len=lens, dtype=np.float64, use_relu=bool(row.relu), value_clip=row.clip)
    fwd = G.gru_forward_bf16 if row.prec == "bf16" else G.gru_forward_octbit
    want_l, want_s = fwd(w, mel, st, seq_len=lens)
    return _relu(np.asarray(want_l, np.float64), row), want_s


def margin_ok(sm_row, classes, thres=THRES, eps=1e-4):
    """ctc_decode2's frame word (first maximum of classes 1..C-2, strictly above thres) is decided with room to spare:
    the maximum is not within eps of the threshold, and where it clears it, not within eps of the runner-up."""
    p = np.asarray(sm_row)[1:classes - 1]
    srt = np.sort(p)
    return abs(srt[-1] - thres) > eps and (srt[-1] < thres or len(p) < 2 or srt[-1] - srt[-2] > eps)


def check_decode(toks, pw, sm, classes, margin=1e-4):
    """Fused tokens == ctc_decode2 of the softmax `sm` on the streams no frame of which sits on the threshold or a tie;
    the carried word == the last frame's word.  Returns (streams checked, words they hold)."""
    from keyword_spotting_amd.prediction import tokens_to_seq
    b = sm.shape[0]
    checked = words = 0
    for k in range(b):
        if not all(margin_ok(f, classes, eps=margin) for f in sm[k]):
            continue
        want = D.ctc_decode2(sm[k], classes)
        np.testing.assert_array_equal(tokens_to_seq(toks[k]), want, err_msg="stream %d" % k)
        checked += 1
        words += int((want > 0).sum())
    last = D.frame_words(sm[:, -1, :], 1, classes - 1, THRES)
    ok = [k for k in range(b) if margin_ok(sm[k, -1], classes, eps=margin)]
    np.testing.assert_array_equal(pw[ok], last[ok])
    return checked, words


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _forward(m, mel, st0, lens=None, reset=None, prev_word=None):
    return m.forward(_t(mel), _t(st0), seq_len=_t(lens), reset_mask=_t(reset), prev_word=prev_word)


def _check_values(row, got_l, got_s, got_sm, want_l, want_s, oracle_c=None, mel=None, st_eff=None, lens=None):
    """The row's tolerances; returns (max |dlogit|, max |dstate|)."""
    el, es = np.abs(got_l - want_l), np.abs(got_s - want_s)
    scale = 20.0 if row.relu else 1.0
    np.testing.assert_allclose(got_sm.sum(-1), 1.0, atol=1e-6)
    if row.prec in ("fp32", "f16x3"):
        assert el.max() < TOL * scale, el.max()
        assert es.max() < TOL, es.max()
        if row.relu:       # the softmax of relu'd logits: consistent with the logits the call returned
            np.testing.assert_allclose(got_sm, G.softmax(got_l.astype(np.float64)), atol=2e-6)
        else:
            assert np.abs(got_sm - G.softmax(want_l)).max() < 2e-5
        if oracle_c is not None:
            c_l, _, c_s = oracle_c.gru_forward((row.n_mel, row.hidden, row.layers, row.classes, row.relu, row.clip),
                                               G.weights_to_blob(weights_of(row)), mel, st_eff, seq_len=lens)
            assert np.abs(got_l - c_l).max() < TOL * scale and np.abs(got_s - c_s).max() < TOL
    elif row.prec == "bf16":
        assert el.max() < 6e-2 * scale and el.mean() < 6e-3 * scale, (el.max(), el.mean())
        assert es.max() < 2e-2 and es.mean() < 1e-3, (es.max(), es.mean())
        np.testing.assert_allclose(got_sm, G.softmax(got_l.astype(np.float64)), atol=2e-6)
    else:
        assert el.max() < 0.1 * scale and el.mean() < 2e-3 * scale, (el.max(), el.mean())
        assert es.max() < 2e-2 and es.mean() < 2e-4, (es.max(), es.mean())
        np.testing.assert_allclose(got_sm, G.softmax(got_l.astype(np.float64)), atol=2e-6)
    return float(el.max()), float(es.max())


@pytest.mark.parametrize("row", S.ROWS, ids=[r.name for r in S.ROWS])
def test_row_matches_the_oracle(row, oracle_c):
    cus = _cus()
    assert S.layout_of(row, row.batch, row.frames, cus) == row.layout, "this row no longer takes the layout it was written for"
    m = _model(row)
    b, t, C = row.batch, row.frames, row.classes
    mel, st0, lens, reset = inputs(row)
    want_l, want_s = reference(row, mel, st0, lens, reset)
    pw = m.fresh_prev_word(b)
    r = _forward(m, mel, st0, lens, reset, prev_word=pw)
    assert m.kernel_names() == S.expected_names(row, b, t, cus)
    got_l, got_s, got_sm = (r[k].cpu().numpy() for k in ("logits", "state", "softmax"))
    toks, pw = r["tokens"].cpu().numpy(), pw.cpu().numpy()
    st_eff = st0 if reset is None else st0 * (1 - reset)[None, :, None].astype(np.float32)
    el, es = _check_values(row, got_l, got_s, got_sm, want_l, want_s, oracle_c, mel, st_eff, lens)
    if lens is not None:
        bias_row = _relu(weights_of(row)["bfc"], row).astype(np.float32)
        for k in range(b):           # dynamic_rnn's zero output past seq_len: the projection's bias, bit for bit
            np.testing.assert_array_equal(got_l[k, lens[k]:], np.broadcast_to(bias_row, (t - lens[k], C)))
        if row.prec == "int8":       # stream 0 never ran: its state is the (reset) initial state, bit for bit
            np.testing.assert_array_equal(got_s[:, 0], st_eff[:, 0])
    if row.relu:
        assert got_l.min() == 0.0
        assert got_l.max() == 20.0 if row.clip > 0 else got_l.max() > 20.0
    elif row.prec in ("fp32", "f16x3"):
        checked, words = check_decode(toks, pw, G.softmax(want_l), C)
        assert 2 * checked >= b and words > 0, (checked, words, b)       # at least half the streams, not vacuous
    else:
        # bf16 / int8: the fused decode against the call's own softmax (the epilogues are the ones under test here)
        checked, words = check_decode(toks, pw, got_sm.astype(np.float64), C, margin=1e-5)
        assert 2 * checked >= b and words > 0, (checked, words, b)
    print("config-space %-26s %-62s max|dlogit| %.2e max|dstate| %.2e" % (row.name, " | ".join(n for n in m.kernel_names() if n), el, es))


CHUNKS = [r for r in S.ROWS if r.chunk]


@pytest.mark.parametrize("row", CHUNKS, ids=[r.name for r in CHUNKS])
def test_chunked_equals_one_shot_bitwise(row):
    """State and the decode carry across calls of 1..n frames == one call, bit for bit (in every layout a chunk takes)."""
    m = _model(row)
    b, t = row.batch, row.frames
    mel, st0, _, _ = inputs(row)
    x, s0 = _t(mel).cuda(), _t(st0).cuda()
    pw = m.fresh_prev_word(b)
    whole = m.forward(x, s0, prev_word=pw)
    cuts = sorted({0, t, 1, t // 2, t // 2 + 1, t - 3})
    pw2, st, parts = m.fresh_prev_word(b), s0, []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        rr = m.forward(x[:, lo:hi].contiguous(), st, prev_word=pw2)
        parts.append(rr)
        st = rr["state"]
    for k in ("logits", "softmax", "tokens"):
        assert torch.equal(torch.cat([p[k] for p in parts], 1), whole[k]), k
    assert torch.equal(st, whole["state"]) and torch.equal(pw2, pw)


TWINS = [r for r in S.ROWS if r.twin]


@pytest.mark.parametrize("row", TWINS, ids=[r.name for r in TWINS])
def test_layout_twin_on_shared_streams(row, oracle_c):
    """The row's streams inside a batch too large for its layout (16 * (CUs // L + 1) + 1 streams: L x groups > CUs):
    overlapped rows -> sequential launches, bitwise equal; pipelined rows -> one launch per layer, a sample of at least
    32 streams (first and last group, group seams, the partial last group) against the oracle, and bitwise equal to the
    pipelined launch on the streams both calls hold."""
    cus = _cus()
    m = _model(row)
    big_b = S.sequential_batch(row.layers, cus)
    t = row.frames if row.layout == "ovl" else row.twin
    assert S.layout_of(row, big_b, t, cus) == "seq"
    mel, st0, lens, reset = inputs(row, big_b, t)
    b = row.batch
    if row.layout == "ovl":
        small_mel, small_st0, small_lens, small_reset = inputs(row)
        mel[:b], st0[:, :b] = small_mel, small_st0
        if lens is not None:
            lens[:b], reset[:b] = small_lens, small_reset
    big = _forward(m, mel, st0, lens, reset)
    assert m.kernel_names() == S.expected_names(row, big_b, t, cus)
    small = _forward(m, mel[:b], st0[:, :b], None if lens is None else lens[:b], None if reset is None else reset[:b])
    assert m.kernel_names() == S.expected_names(row, b, t, cus)
    assert S.layout_of(row, b, t, cus) == row.layout
    for k in ("logits", "softmax"):
        assert torch.equal(small[k], big[k][:b]), k
    assert torch.equal(small["state"], big["state"][:, :b])
    if row.layout == "ovl":
        return
    g = S.STREAMS_PER_GROUP
    pick = sorted({0, 1, g - 1, g, g + 1, 2 * g - 1, 2 * g, big_b // 2 - 1, big_b // 2, big_b - g - 1, big_b - g, big_b - 2, big_b - 1}
                  | set(range(3 * g + 5, big_b - g, max(1, (big_b - 4 * g) // 20))))
    assert len(pick) >= 32
    want_l, want_s = reference(row, mel[pick], st0[:, pick], None, None)
    got = {k: big[k].cpu().numpy() for k in ("logits", "state", "softmax")}
    _check_values(row, got["logits"][pick], got["state"][:, pick], got["softmax"][pick], want_l, want_s, oracle_c,
                  np.ascontiguousarray(mel[pick]), np.ascontiguousarray(st0[:, pick]))


def test_profiling_plans_sequential_launches_and_zero_frames_keep_the_names():
    """Two rules of plan_step that no row pins, at the smallest overlap-eligible shape (one group, T == KWS_OVERLAP_MIN_T):
    kws_set_profiling turns the overlapped call into one launch per layer -- same bits, inside what kws_reserve sized for
    either answer -- and a zero-frame call launches no GRU kernel, so kernel_names() keeps the step before."""
    row = S.R("fp32_res_n40_L2_ovl_min", "fp32", "auto", 40, 128, 2, 4, 16, S.OVERLAP_MIN_T, "ovl", wfc=2.0)
    cus = _cus()
    b, t = row.batch, row.frames
    assert S.layout_of(row, b, t, cus) == "ovl" and S.layout_of(row, b, t - 1, cus) == "seq"
    m = _model(row)
    mel, st0, _, _ = inputs(row)
    m.reserve(b, t)
    stats = m.scratch_stats()
    ovl = _forward(m, mel, st0)
    assert m.kernel_names() == S.expected_names(row, b, t, cus)
    assert m.scratch_stats() == stats
    m.set_profiling(True)
    seq = _forward(m, mel, st0)
    seq_names = S.expected_names(row, b, t - 1, cus)      # the row's names with the layout forced to sequential
    assert m.kernel_names() == seq_names
    assert [n for _, n in m.kernel_times()] == [1] * row.layers      # one timed launch per layer: not the time blocks
    for k in ("logits", "softmax", "state"):
        assert torch.equal(seq[k], ovl[k]), k
    assert m.scratch_stats() == stats
    none = _forward(m, mel[:, :0], st0)
    assert none["logits"].shape[1] == 0 and torch.equal(none["state"].cpu(), _t(st0))
    assert m.kernel_names() == seq_names
