"""The self-attention model's sliding-window stream manager on the GPU (kws_attention_stream_*, attention_stream.AttentionStreamManager)
against its host mirror (AttentionHotwordDetector: exact), against the public decoders on the softmax it returns, and against the float64
policy loop (tests/attention_stream_model.py) up to each stream's first decision edge.  The cases, their weights, labels and seeds are
attention_stream_model.CASES; what they lean on is asserted on the CPU in test_attention_stream_host.py."""
import functools

import numpy as np
import pytest
import torch

import attention_stream_model as SM

pytestmark = pytest.mark.gpu


def _model(case, precision="fp32"):
    from keyword_spotting_amd.attention_ctc import DeployModel
    return DeployModel(SM.case_config(case), SM.case_weights(case), precision=precision)


def _pair(case, model):
    from keyword_spotting_amd.attention_stream import AttentionHotwordDetector, AttentionStreamManager
    k = SM.CASES[case]
    kw = dict(window_chunks=k["nq"], max_chunk_samples=SM.MAX_CHUNK, vad_thres=SM.VAD_THRES, label=k["label"], decode_thres=k["thres"])
    return AttentionStreamManager(model, k["B"], **kw), AttentionHotwordDetector(model, k["B"], **kw)


def _feeds(case):
    """The case's chunks as the GPU is fed them: (pcm tensor [B, n] float32 or int16, lengths or None)."""
    k = SM.CASES[case]
    pcms, lens = SM.case_inputs(case)
    out = []
    for x, n in zip(pcms, lens):
        t = torch.from_numpy(np.round(x * 32768.0).astype(np.int16)) if k["int16"] else torch.from_numpy(x)
        out.append((t, torch.from_numpy(n) if k["ragged"] else None))
    return out


def _snapshot(mgr, hit, softmax):
    mel, frames, chunks = mgr.window()
    samples, clen = mgr.carry()
    return dict(hit=hit.cpu().numpy().copy(), softmax=softmax.cpu().numpy().copy(), mel=mel.cpu().numpy(), frames=frames.cpu().numpy(),
                chunks=chunks.cpu().numpy(), carry=samples.cpu().numpy(), carry_len=clen.cpu().numpy(),
                launches=mgr.stats()["launches_last_feed"])


def _mirror_snapshot(mir, hit, softmax):
    B = mir.batch
    return dict(hit=np.asarray(hit).copy(), softmax=None if softmax is None else softmax.cpu().numpy().copy(), rows=mir.rows.copy(),
                window=[mir.window_of(b).cpu().numpy() for b in range(B)], chunks=np.array([q.len for q in mir.queue]),
                carry=[mir.res[b].cpu().numpy() for b in range(B)])


@functools.lru_cache(maxsize=None)
def _run(case, precision="fp32", chunks=SM.CHUNKS):
    """Manager and mirror side by side over the case's chunks, once per process: what each gave after every chunk."""
    model = _model(case, precision)
    mgr, mir = _pair(case, model)
    got, want = [], []
    for pcm, lens in _feeds(case)[:chunks]:
        hit, sm = mgr.feed_pcm(pcm, lens, want_softmax=True)
        got.append(_snapshot(mgr, hit, sm))
        want.append(_mirror_snapshot(mir, *mir.feed_pcm(pcm, lens, want_softmax=True)))
    device_bytes = mgr.stats()["device_bytes"]
    mgr.close()
    model.close()
    return got, want, device_bytes


def _assert_equals_mirror(case, got, want):
    k = SM.CASES[case]
    cfg = SM.case_config(case)
    for t, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g["hit"], w["hit"], err_msg="chunk %d" % t)
        np.testing.assert_array_equal(g["chunks"], w["chunks"], err_msg="chunk %d" % t)
        for b in range(k["B"]):
            n = w["window"][b].shape[0]
            assert g["frames"][b] == n, (t, b)
            np.testing.assert_array_equal(g["mel"][b, :n], w["window"][b], err_msg="window, chunk %d stream %d" % (t, b))
            nc = w["carry"][b].shape[0]
            assert g["carry_len"][b] == nc, (t, b)
            np.testing.assert_array_equal(g["carry"][b, :nc], w["carry"][b], err_msg="carry, chunk %d stream %d" % (t, b))
            rows = int(w["rows"][b])
            if rows:                       # the rows the decision was taken on, bitwise what DeployModel.forward gives; zeros past them
                np.testing.assert_array_equal(g["softmax"][b, :rows], w["softmax"][b, :rows], err_msg="softmax, chunk %d stream %d" % (t, b))
                assert not g["softmax"][b, rows:].any(), (t, b)
            else:                          # no row is decoded (with combine_frame > 1 the model still writes its one all-pad row)
                assert not g["softmax"][b, 1 if cfg.combine_frame > 1 else 0:].any() and g["hit"][b] == 0, (t, b)


@pytest.mark.parametrize("case", sorted(SM.CASES))
def test_manager_equals_the_host_mirror(case):
    """hit, the window (frames, chunk count, mel bitwise), the carry and the returned softmax after every chunk; float and int16 PCM,
    lock-step and ragged (CASES); 5 + 3 L launches per feed; the owned bytes are the documented ones."""
    got, want, device_bytes = _run(case)
    _assert_equals_mirror(case, got, want)
    k = SM.CASES[case]
    assert all(g["launches"] == 5 + 3 * k["L"] for g in got), [g["launches"] for g in got]
    W, pad = k["nq"] * 32, lambda n: (n + 255) // 256 * 256
    assert device_bytes == 2 * pad(k["B"] * 399 * 4) + 2 * pad(k["B"] * 4) + pad(k["B"] * W * k["n_mel"] * 4) + pad(k["B"] * k["nq"] * 4) + 2 * pad(k["B"] * 4)
    assert sum(int(g["hit"].sum()) for g in got) >= 3          # (the conditions themselves: test_attention_stream_host.py)
    if case == "w15_c1":
        assert max(int(w["rows"].max()) for w in want) > 256   # the decide kernel took more than four passes


def test_f16x3_handle():
    """The manager only borrows the handle: an f16x3 model is served unchanged, manager == mirror."""
    got, want, _ = _run("w3_c2", "f16x3", 12)
    _assert_equals_mirror("w3_c2", got, want)
    assert sum(int(g["hit"].sum()) for g in got) >= 3


def test_softmax_is_forward_on_the_inspected_window():
    """Where a stream did not fire, the window inspected after the feed is the one the decision was taken on: the returned softmax is
    DeployModel.forward on it, bitwise -- padded to W as the manager runs it, or to the longest window alone."""
    case = "w15_c1"
    got, want, _ = _run(case)
    model = _model(case)
    for t in (3, 14, 22, 29):
        g = got[t]
        lens = np.where((g["hit"] == 0) & (want[t]["rows"] > 0), g["frames"], 0).astype(np.int32)
        for pad_to in (g["mel"].shape[1], max(int(lens.max()), 1)):
            sm = model.forward(torch.from_numpy(g["mel"][:, :pad_to].copy()), torch.from_numpy(lens), want_logits=False)["softmax"].cpu().numpy()
            for b in np.nonzero(lens)[0]:
                rows = int(want[t]["rows"][b])
                np.testing.assert_array_equal(sm[b, :rows], g["softmax"][b, :rows], err_msg="chunk %d stream %d" % (t, b))
    model.close()


@pytest.mark.parametrize("case", sorted(SM.CASES))
def test_decide_kernel_against_the_public_decoders(case):
    """hit == prediction.ctc_decode2 + ctc_predict on the softmax the manager returned, for every stream and chunk (a stream without
    rows decodes nothing)."""
    from keyword_spotting_amd import prediction
    got, want, _ = _run(case)
    k = SM.CASES[case]
    C = SM.case_config(case).num_classes
    for t, (g, w) in enumerate(zip(got, want)):
        sm = g["softmax"].copy()
        sm[w["rows"] == 0] = 0.0
        decoded = prediction.ctc_decode2(torch.from_numpy(sm).cuda(), C, k["thres"], raw=True)
        hits = prediction.ctc_predict(decoded, k["label"]).cpu().numpy()
        np.testing.assert_array_equal(g["hit"], np.where(w["rows"] > 0, hits, 0), err_msg="chunk %d" % t)


@pytest.mark.parametrize("case", sorted(SM.CASES))
def test_manager_against_the_float64_policy_loop(case):
    """Each stream up to its first decision edge (a VAD sum within 1e-5 of its threshold, a candidate softmax entry within 2e-4 of
    decode_thres, an argmax gap below 2e-4 on a row that emits): hit, frames and chunks held, carry length, and the softmax rows."""
    got, _, _ = _run(case)
    recs = SM.case_records(case)
    B = SM.CASES[case]["B"]
    compared, worst = 0, 0.0
    for b in range(B):
        for t in range(SM.CHUNKS):
            r, g = recs[t][b], got[t]
            if r["edge"]:
                break
            compared += 1
            assert g["hit"][b] == r["hit"], (t, b)
            assert (g["frames"][b], g["chunks"][b], g["carry_len"][b]) == (r["len_after"], r["chunks_after"], r["carry"]), (t, b)
            if r["rows"]:
                worst = max(worst, float(np.abs(g["softmax"][b, :r["rows"]] - r["softmax"]).max()))
    print("%s: %d of %d (stream, chunk) pairs compared, softmax within %.3g of float64" % (case, compared, B * SM.CHUNKS, worst))
    assert 2 * compared >= B * SM.CHUNKS


@pytest.mark.parametrize("case", ["w15_c1", "w3_c2"])
def test_a_skipped_stream_is_bitwise_untouched(case):
    got, _, _ = _run(case)
    lens = SM.case_inputs(case)[1]
    seen = 0
    for t in range(1, SM.CHUNKS):
        for b in np.nonzero(lens[t] == 0)[0]:
            g, p = got[t], got[t - 1]
            seen += 1
            assert g["hit"][b] == 0 and g["frames"][b] == p["frames"][b] and g["chunks"][b] == p["chunks"][b]
            np.testing.assert_array_equal(g["mel"][b], p["mel"][b])
            n = p["carry_len"][b]
            assert g["carry_len"][b] == n
            np.testing.assert_array_equal(g["carry"][b, :n], p["carry"][b, :n])
            assert not g["softmax"][b, 1:].any()
    assert seen >= 10


def _alone(case, model, feeds, **kw):
    """A manager alone over `feeds` -> snapshots."""
    from keyword_spotting_amd.attention_stream import AttentionStreamManager
    k = SM.CASES[case]
    args = dict(window_chunks=k["nq"], max_chunk_samples=SM.MAX_CHUNK, vad_thres=SM.VAD_THRES, label=k["label"], decode_thres=k["thres"])
    args.update(kw)
    mgr = AttentionStreamManager(model, int(feeds[0][0].shape[0]), **args)
    out = [_snapshot(mgr, *mgr.feed_pcm(pcm, lens, want_softmax=True)) for pcm, lens in feeds]
    mgr.close()
    return out


def _same_stream(a, b, sa, sb=None):
    sb = sa if sb is None else sb
    assert a["hit"][sa] == b["hit"][sb] and a["frames"][sa] == b["frames"][sb] and a["chunks"][sa] == b["chunks"][sb]
    n = a["frames"][sa]
    np.testing.assert_array_equal(a["mel"][sa, :n], b["mel"][sb, :n])
    assert a["carry_len"][sa] == b["carry_len"][sb]
    np.testing.assert_array_equal(a["carry"][sa, :a["carry_len"][sa]], b["carry"][sb, :b["carry_len"][sb]])
    np.testing.assert_array_equal(a["softmax"][sa], b["softmax"][sb])


def test_recycled_slots_start_afresh_and_neighbours_stay():
    from keyword_spotting_amd.attention_stream import AttentionStreamManager
    case = "w3_c2"
    k = SM.CASES[case]
    whole, _, _ = _run(case)
    feeds = _feeds(case)
    model = _model(case)
    fresh = _alone(case, model, feeds[10:20])
    mgr = AttentionStreamManager(model, k["B"], window_chunks=k["nq"], max_chunk_samples=SM.MAX_CHUNK, vad_thres=SM.VAD_THRES, label=k["label"],
                                 decode_thres=k["thres"])
    for pcm, lens in feeds[:10]:
        mgr.feed_pcm(pcm, lens)
    before = _snapshot(mgr, mgr.hit, torch.zeros(1))
    slots = [1, 5, 32]
    mgr.recycle(slots)
    after = _snapshot(mgr, mgr.hit, torch.zeros(1))
    for b in range(k["B"]):
        if b in slots:
            assert after["frames"][b] == 0 and after["chunks"][b] == 0 and after["carry_len"][b] == 0
        else:
            assert after["frames"][b] == before["frames"][b] and after["chunks"][b] == before["chunks"][b]
            np.testing.assert_array_equal(after["mel"][b], before["mel"][b])
            np.testing.assert_array_equal(after["carry"][b], before["carry"][b])
            assert after["carry_len"][b] == before["carry_len"][b]
    for i, (pcm, lens) in enumerate(feeds[10:20]):
        g = _snapshot(mgr, *mgr.feed_pcm(pcm, lens, want_softmax=True))
        for b in range(k["B"]):
            _same_stream(g, fresh[i] if b in slots else whole[10 + i], b)
    mgr.close()
    model.close()


def test_two_managers_on_one_model_interleaved():
    """The chunk's intermediates are the model handle's and shared; what a manager owns is its own: two managers of different shapes fed
    in turn give what each gives alone."""
    from keyword_spotting_amd.attention_stream import AttentionStreamManager
    case = "w3_c2"
    k = SM.CASES[case]
    whole, _, _ = _run(case)
    feeds = _feeds(case)
    model = _model(case)
    other = [(pcm[:5].flip(0).contiguous(), None if lens is None else lens[:5].flip(0).contiguous()) for pcm, lens in feeds]
    alone = _alone(case, model, other[:15], window_chunks=2, label="1")
    a = AttentionStreamManager(model, k["B"], window_chunks=k["nq"], max_chunk_samples=SM.MAX_CHUNK, vad_thres=SM.VAD_THRES, label=k["label"],
                               decode_thres=k["thres"])
    b = AttentionStreamManager(model, 5, window_chunks=2, max_chunk_samples=SM.MAX_CHUNK, vad_thres=SM.VAD_THRES, label="1", decode_thres=k["thres"])
    for t in range(15):
        ga = _snapshot(a, *a.feed_pcm(*feeds[t], want_softmax=True))
        gb = _snapshot(b, *b.feed_pcm(*other[t], want_softmax=True))
        for s in range(k["B"]):
            _same_stream(ga, whole[t], s)
        for s in range(5):
            _same_stream(gb, alone[t], s)
    a.close(), b.close()
    model.close()


def test_refusals_with_live_handles():
    import attention_stream_refusals
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.attention_stream import AttentionStreamManager
    attention_stream_refusals.check()
    case = "w1_c2"
    model = _model(case)
    mgr = AttentionStreamManager(model, 2, window_chunks=2, max_chunk_samples=1000, label="12")
    with pytest.raises(_lib.InvalidArgumentError, match="n_max=1001"):
        mgr.feed_pcm(torch.zeros(2, 1001))
    with pytest.raises(_lib.InvalidArgumentError, match="expected PCM of shape"):
        mgr.feed_pcm(torch.zeros(3, 100))
    hit = mgr.feed_pcm(torch.zeros(2, 0))                       # every stream skipped: nothing launched
    assert not hit.cpu().numpy().any() and mgr.stats()["launches_last_feed"] == 0
    lib = _lib.load()
    assert lib.kws_attention_stream_feed(mgr._handle, None, 10, None, 0, _lib.ptr(mgr.hit), None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert b"pcm" in lib.kws_last_error()
    assert lib.kws_attention_stream_feed(mgr._handle, _lib.ptr(mgr.hit), 10, None, 0, None, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert b"hit" in lib.kws_last_error()
    assert lib.kws_attention_stream_recycle(mgr._handle, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT and b"slots" in lib.kws_last_error()
    model.close()                                               # the borrowed model is gone: every call fails cleanly
    with pytest.raises(_lib.InvalidArgumentError, match="has been destroyed"):
        mgr.feed_pcm(torch.zeros(2, 500))
    with pytest.raises(_lib.InvalidArgumentError, match="has been destroyed"):
        mgr.window()
    with pytest.raises(_lib.InvalidArgumentError, match="has been destroyed"):
        mgr.recycle([0])
    mgr.close()
