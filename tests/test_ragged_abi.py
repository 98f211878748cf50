"""Per-stream arrival and slot recycling of the stream manager (kws_stream_feed_ragged, kws_stream_recycle): the entry points
exist, refuse bad arguments before any device work, and the Python layer checks the lengths it is given before it touches
the device.  No GPU needed."""
import ctypes

import pytest
import torch


def test_ragged_and_recycle_symbols_are_exported_and_bound():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    for sym in ("kws_stream_feed_ragged", "kws_stream_recycle", "kws_stream_carry"):
        assert hasattr(lib, sym)
        assert sym in _lib.EXPORTED_SYMBOLS


def test_null_and_invalid_arguments_are_rejected():
    from keyword_spotting_amd import _lib
    lib = _lib.load()
    dummy = ctypes.c_void_p(1)
    assert lib.kws_stream_feed_ragged(None, None, 0, None, 0, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_stream_feed_ragged(None, dummy, 3600, dummy, 1, dummy, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_stream_recycle(None, None, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_stream_recycle(None, dummy, None) == _lib.KWS_ERR_INVALID_ARGUMENT
    assert lib.kws_stream_carry(None, dummy, dummy, None) == _lib.KWS_ERR_INVALID_ARGUMENT


class _NoDevice(object):
    """Stands in for the model: any attribute access means the manager went for the device."""
    def __getattr__(self, name):
        raise AssertionError("touched the model (%s) before the lengths were checked" % name)


def _manager(batch):
    from keyword_spotting_amd.detector import StreamManager
    m = StreamManager.__new__(StreamManager)
    m.batch, m.model, m._stream, m._win = batch, _NoDevice(), None, None
    return m


@pytest.mark.parametrize("lengths", [
    [3600] * 3,                                   # wrong length
    torch.full((4, 1), 3600, dtype=torch.int32),  # wrong shape
    torch.full((4,), 3600.0),                     # float
    torch.ones(4, dtype=torch.bool),              # bool
    [0.5, 1, 2, 3],                               # float sequence
])
def test_feed_pcm_rejects_bad_lengths_before_any_device_call(lengths):
    from keyword_spotting_amd import _lib
    m = _manager(4)
    pcm = torch.zeros(4, 3600, dtype=torch.int16)
    with pytest.raises(_lib.InvalidArgumentError):
        m.feed_pcm(pcm, None, lengths=lengths)


def test_recycle_slots_are_checked_before_any_device_call():
    from keyword_spotting_amd import _lib
    from keyword_spotting_amd.detector import _recycle_mask
    m = _manager(4)
    with pytest.raises(_lib.InvalidArgumentError):
        m.recycle([4])                               # out of range
    with pytest.raises(_lib.InvalidArgumentError):
        m.recycle(torch.zeros(3, dtype=torch.bool))  # wrong mask shape
    assert _recycle_mask([1, 3], 4).tolist() == [0, 1, 0, 1]
    assert _recycle_mask(torch.tensor([True, False, False, True]), 4).tolist() == [1, 0, 0, 1]
    assert _recycle_mask(torch.tensor([2]), 4).tolist() == [0, 0, 1, 0]
