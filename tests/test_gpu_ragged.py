"""Per-stream arrival (kws_stream_feed_ragged / StreamManager.feed_pcm(lengths=...)) and slot recycling (kws_stream_recycle).

The reference runs one loop per microphone (detector.py:158-209): each reads whatever its ring buffer holds, skips the
iteration when that is nothing, and keeps its own carry.  So stream b of a ragged manager must get, bit for bit, what a
lock-step manager gets when it is fed stream b's chunks alone -- on the periods where stream b had data, and not at all on the
others.  Triggers (reset-on-trigger, a restart held over a skipped period) are inside these runs: the weights and label emit
on noise."""
import numpy as np
import pytest
import torch

from oracle import decode_oracle as D
from oracle import gru_oracle as G

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "f16x3", "bf16"]
N_MAX = 5000


def _emitting(cfg, fe, rng):
    """Random weights whose model says something on noise, and its most frequent word as a one-digit label."""
    from keyword_spotting_amd.rnn_ctc import DeployModel
    b = 48
    noise = torch.from_numpy((rng.standard_normal((b, 16000)) * 0.2).astype(np.float32))
    for seed in range(7200, 7260):
        w = G.random_weights(40, 128, 2, 6, seed=seed)
        w["Wfc"] = (w["Wfc"] * 4.0).astype(np.float32)
        probe = DeployModel(cfg, w)
        sm = probe.forward(fe.forward(noise), probe.zero_state(b), want_logits=False)["softmax"].cpu().numpy()
        probe.close()
        words = np.concatenate([D.ctc_decode2(sm[k], 6)[1::2] for k in range(b)])
        if words.size >= 2 * b:
            return w, str(int(np.bincount(words).argmax()))
    raise AssertionError("no seed gives a model that emits words")


_SETUP = {}


def _setup(precision):
    """(config, front-end, model, label) per precision, shared by the tests of this module."""
    if precision not in _SETUP:
        from keyword_spotting_amd import get_config
        from keyword_spotting_amd.frontend import MelFrontend
        from keyword_spotting_amd.rnn_ctc import DeployModel
        cfg = get_config(precision=precision)
        fe = MelFrontend(cfg)
        w, label = _emitting(cfg, fe, np.random.default_rng(8100))
        _SETUP[precision] = (cfg, fe, DeployModel(cfg, w), label)
    return _SETUP[precision]


def _manager(precision, batch):
    from keyword_spotting_amd.detector import StreamManager
    cfg, fe, model, label = _setup(precision)
    return StreamManager(model, batch, label=label)


def _schedules(rng, n_streams, periods):
    """[n_streams, periods] lengths from {0, 150, 1800, 3600, 5000}; some streams open with runs of 150 (sub-frame chunks)."""
    lens = rng.choice([0, 150, 1800, 3600, 5000], size=(n_streams, periods), p=[0.15, 0.15, 0.2, 0.35, 0.15])
    opening = rng.random(n_streams) < 0.3
    lens[opening, 0] = 150
    lens[opening, 1] = 150
    return lens.astype(np.int32)


def _pcm(rng, n_streams, lens):
    """[n_streams, N_MAX] int16: the first lens[b] samples are stream b's chunk (about 5 % of chunks quiet: below vad(data, 30)),
    the padding past them loud noise that must never reach a result."""
    pcm = rng.integers(-32768, 32767, (n_streams, N_MAX)).astype(np.int16)
    speech = rng.integers(-6000, 6000, (n_streams, N_MAX)).astype(np.int16)
    quiet = rng.random(n_streams) < 0.05
    speech[quiet] //= 4096
    cols = np.arange(N_MAX)[None, :] < lens[:, None]
    return np.where(cols, speech, pcm).astype(np.int16)


def _snap(mgr):
    torch.cuda.synchronize()
    return mgr.state.clone(), mgr.restart.clone()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                       b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_arrival_equals_per_stream_lockstep_replay(precision):
    cfg, fe, model, label = _setup(precision)
    rng = np.random.default_rng(9100 + PRECISIONS.index(precision))
    B, periods = 256, 20
    lens = _schedules(rng, B, periods)
    chunks = [_pcm(rng, B, lens[:, p]) for p in range(periods)]
    rag = _manager(precision, B)
    hits = np.zeros((B, periods), np.int32)
    for p in range(periods):
        h = rag.feed_pcm(torch.from_numpy(chunks[p]).cuda(), fe, lengths=torch.from_numpy(lens[:, p]))
        hits[:, p] = h.cpu().numpy()
    state, restart = _snap(rag)
    assert hits.sum() > 0, "no trigger: the run does not cover reset-on-trigger"
    assert (lens == 0).any() and ((lens[:, 0] == 150) & (lens[:, 1] == 150)).any()
    for b in range(B):
        oracle = _manager(precision, B)
        for p in range(periods):
            n = int(lens[b, p])
            if n == 0:
                assert hits[b, p] == 0, (b, p)
                continue
            row = torch.from_numpy(np.repeat(chunks[p][b:b + 1, :n], B, 0)).cuda()
            want = int(oracle.feed_pcm(row, fe)[0].item())
            assert hits[b, p] == want, (precision, b, p, n)
        torch.cuda.synchronize()
        assert _bits_equal(state[:, b], oracle.state[:, 0]), (precision, b)
        assert int(restart[b]) == int(oracle.restart[0]), (precision, b)
        oracle.close()
    rag.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_groups_past_16_per_cu(precision):
    """B = 4100 (more 16-stream groups than CUs: persistent workgroups), 5 length groups, one lock-step oracle per group."""
    cfg, fe, model, label = _setup(precision)
    rng = np.random.default_rng(9200 + PRECISIONS.index(precision))
    B, periods, groups = 4100, 12, 5
    group = rng.integers(0, groups, B)
    sched = _schedules(rng, groups, periods)
    lens = sched[group]                                   # [B, periods]
    chunks = [_pcm(rng, B, lens[:, p]) for p in range(periods)]
    rag = _manager(precision, B)
    hits = np.zeros((B, periods), np.int32)
    for p in range(periods):
        hits[:, p] = rag.feed_pcm(torch.from_numpy(chunks[p]).cuda(), fe, lengths=torch.from_numpy(lens[:, p])).cpu().numpy()
    state, restart = _snap(rag)
    for g in range(groups):
        sel = torch.from_numpy(np.nonzero(group == g)[0]).cuda()
        oracle = _manager(precision, B)
        for p in range(periods):
            n = int(sched[g, p])
            if n == 0:
                assert (hits[group == g, p] == 0).all()
                continue
            want = oracle.feed_pcm(torch.from_numpy(chunks[p][:, :n].copy()).cuda(), fe).cpu().numpy()
            assert np.array_equal(hits[group == g, p], want[group == g]), (precision, g, p)
        torch.cuda.synchronize()
        assert _bits_equal(state[:, sel], oracle.state[:, sel]), (precision, g)
        assert torch.equal(restart[sel], oracle.restart[sel])
        oracle.close()
    rag.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_lengths_mixing_and_reset_match_lockstep(precision):
    cfg, fe, model, label = _setup(precision)
    rng = np.random.default_rng(9300 + PRECISIONS.index(precision))
    B = 96
    ns = [3600, 150, 150, 1800, 5000, 3600, 200, 3600, 3600, 1800]
    chunks = [torch.from_numpy(_pcm(rng, B, np.full(B, n))[:, :n].copy()).cuda() for n in ns]
    lock, rag, mixed = (_manager(precision, B) for _ in range(3))
    res = np.zeros((B, 0), np.float32)              # detector.py:179-183 on the host: the samples every stream must carry
    for p, c in enumerate(chunks):
        full = torch.full((B,), c.shape[1], dtype=torch.int32)
        h_lock = lock.feed_pcm(c, fe).clone()
        h_rag = rag.feed_pcm(c, fe, lengths=full).clone()
        # `mixed` opens lock-step (a carry of 240 samples) and switches at p = 1: the switch reads the lock-step layout
        h_mix = (mixed.feed_pcm(c, fe) if p % 2 == 0 else mixed.feed_pcm(c, fe, lengths=full)).clone()
        assert torch.equal(h_lock, h_rag) and torch.equal(h_rag, h_mix), (precision, p)
        data = np.concatenate([res, c.cpu().numpy().astype(np.float32) / np.float32(32768.0)], 1)
        n = data.shape[1]
        res = data[:, n - (n if n < 400 else (n - 400) % 160 + 240):]
        for m in (lock, rag, mixed):
            samples, lengths = m.carry()
            assert (lengths.cpu().numpy() == res.shape[1]).all(), (precision, p)
            assert np.array_equal(samples[:, :res.shape[1]].cpu().numpy().view(np.int32), res.view(np.int32)), (precision, p)
    torch.cuda.synchronize()
    for m in (rag, mixed):
        assert _bits_equal(lock.state, m.state) and torch.equal(lock.restart, m.restart), precision
    # kws_stream_reset returns a ragged handle to lock-step mode with no carry: the same bits as a handle that never went ragged
    for m in (lock, rag):
        assert m._lib.kws_stream_reset(m._stream) == 0
        assert (m.carry()[1] == 0).all()
    for p, c in enumerate(chunks[:5]):
        assert torch.equal(lock.feed_pcm(c, fe), rag.feed_pcm(c, fe)), (precision, p)
        (s_l, n_l), (s_r, n_r) = lock.carry(), rag.carry()
        k = int(n_l[0])
        assert torch.equal(n_l, n_r) and _bits_equal(s_l[:, :k], s_r[:, :k]), (precision, p)
    torch.cuda.synchronize()
    assert _bits_equal(lock.state, rag.state) and torch.equal(lock.restart, rag.restart)
    for m in (lock, rag, mixed):
        m.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_skips_subframe_silence_clamping_padding_and_launches(precision):
    cfg, fe, model, label = _setup(precision)
    rng = np.random.default_rng(9400 + PRECISIONS.index(precision))
    B = 64
    warm = [torch.from_numpy(_pcm(rng, B, np.full(B, 3600))[:, :3600].copy()).cuda() for _ in range(3)]
    a, b = _manager(precision, B), _manager(precision, B)
    for c in warm:
        a.feed_pcm(c, fe)
        b.feed_pcm(c, fe)
    # n_b == 0: state and restart bitwise unchanged, hit 0; out-of-range lengths clamp to [0, n_max]
    lens = rng.choice([0, 3600, 5000], B).astype(np.int32)
    lens[:4] = 0
    lens[4:8] = N_MAX
    wild = lens.copy()
    wild[:4] = -7
    wild[4:8] = N_MAX + 999
    pcm = _pcm(rng, B, lens)
    s0, r0 = _snap(a)
    ha = a.feed_pcm(torch.from_numpy(pcm).cuda(), fe, lengths=torch.from_numpy(lens)).clone()
    # padding past n_b changes nothing
    pcm2 = pcm.copy()
    pad = np.arange(N_MAX)[None, :] >= lens[:, None]
    pcm2[pad] = rng.integers(-32768, 32767, int(pad.sum())).astype(np.int16)
    hb = b.feed_pcm(torch.from_numpy(pcm2).cuda(), fe, lengths=torch.from_numpy(wild).cuda()).clone()
    s1, r1 = _snap(a)
    skipped = torch.from_numpy(np.nonzero(lens == 0)[0]).cuda()
    assert _bits_equal(s1[:, skipped], s0[:, skipped]) and torch.equal(r1[skipped], r0[skipped])
    assert (ha[skipped] == 0).all()
    assert torch.equal(ha, hb) and _bits_equal(a.state, b.state) and torch.equal(a.restart, b.restart)
    # launches: front-end + gate, the GRU launches (no window tail: they take lengths), window_inc_kernel
    names = model.kernel_names()
    assert not any("window tail" in nm for nm in names)
    gru = sum(1 for nm in names if nm)
    assert 1 + gru + 1 == (3 if precision == "bf16" else 4), names
    a.close(); b.close()
    # a sub-frame chunk (no carry yet: 150 < 400 samples) that is silent zeroes the state of its stream, and only its
    c = _manager(precision, B)
    c.state.copy_(torch.from_numpy(rng.standard_normal(tuple(c.state.shape)).astype(np.float32)).cuda())
    sub = np.zeros(B, np.int32)
    sub[:8] = 150
    quiet = np.zeros((B, 160), np.int16)
    s2, _ = _snap(c)
    c.feed_pcm(torch.from_numpy(quiet).cuda(), fe, lengths=torch.from_numpy(sub))
    s3, _ = _snap(c)
    assert (s3[:, :8] == 0).all()
    assert _bits_equal(s3[:, 8:], s2[:, 8:])
    c.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B", [256, 4100])
def test_gru_over_zero_frames_with_lengths(precision, B):
    """The assumption the ragged path rests on, in its configuration (state stepped in place, the manager's B, T = the frames
    of a full carry plus max_chunk_samples): seq_len = 0 with reset hands back a zero state, without reset the state bitwise."""
    cfg, fe, model, label = _setup(precision)
    T = fe.num_frames(32 * cfg.hop_size + cfg.fft_size - 1)          # StreamManager's default max_frames = 32
    rng = np.random.default_rng(9500)
    mel = torch.from_numpy(rng.standard_normal((B, T, cfg.n_mel)).astype(np.float32)).cuda()
    state = torch.from_numpy(rng.standard_normal((cfg.num_layers, B, cfg.hidden_size)).astype(np.float32)).cuda()
    before = state.clone()
    seq = torch.from_numpy(rng.choice([0, 3, T], B).astype(np.int32))
    seq[:8] = 0
    reset = torch.zeros(B, dtype=torch.uint8)
    reset[:4] = 1
    model.forward(mel, state, seq_len=seq, reset_mask=reset, want_logits=False, state_out=state)
    torch.cuda.synchronize()
    assert (state[:, :4] == 0).all()
    assert _bits_equal(state[:, 4:8], before[:, 4:8])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", ["lockstep", "ragged"])
def test_recycled_slots_equal_fresh_streams(precision, mode):
    cfg, fe, model, label = _setup(precision)
    rng = np.random.default_rng(9600 + PRECISIONS.index(precision))
    B, before, after = 80, 6, 8
    lens = np.full((B, before + after), 3600, np.int32)
    if mode == "ragged":
        lens[:, :before] = _schedules(rng, B, before)
    chunks = [_pcm(rng, B, lens[:, p]) for p in range(before + after)]
    rec, plain, fresh = _manager(precision, B), _manager(precision, B), _manager(precision, B)

    def feed(m, p):
        c = torch.from_numpy(chunks[p]).cuda()
        if mode == "ragged":
            return m.feed_pcm(c, fe, lengths=torch.from_numpy(lens[:, p])).clone()
        return m.feed_pcm(c[:, :3600].contiguous(), fe).clone()

    for p in range(before):
        feed(rec, p)
        feed(plain, p)
    slots = torch.zeros(B, dtype=torch.bool)
    slots[rng.choice(B, 20, replace=False)] = True
    rec.recycle(slots)
    s_r, r_r = _snap(rec)
    assert (s_r[:, slots.cuda()] == 0).all() and (r_r[slots.cuda()] == 0).all()
    keep = (~slots).cuda()
    for p in range(before, before + after):
        h_rec, h_plain, h_fresh = feed(rec, p), feed(plain, p), feed(fresh, p)
        assert torch.equal(h_rec[slots.cuda()], h_fresh[slots.cuda()]), (precision, mode, p)
        assert torch.equal(h_rec[keep], h_plain[keep]), (precision, mode, p)
    torch.cuda.synchronize()
    assert _bits_equal(rec.state[:, slots.cuda()], fresh.state[:, slots.cuda()])
    assert torch.equal(rec.restart[slots.cuda()], fresh.restart[slots.cuda()])
    assert _bits_equal(rec.state[:, keep], plain.state[:, keep]) and torch.equal(rec.restart[keep], plain.restart[keep])
    for m in (rec, plain, fresh):
        m.close()
