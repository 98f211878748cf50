"""Greedy CTC collapse and keyword decision on the GPU -- same names and argument meaning as
utils/prediction.py.  Inputs are one stream's softmax [T,C] (the reference's form; the result is
then the reference's int32 [0,w1,0,w2,0,...] array) or a batch [B,T,C] (-> list of such arrays, or
raw device tensors with `raw=True`).  Everything runs in kws_ctc_decode / kws_ctc_predict."""
import numpy as np
import torch

from . import _lib


def _as_batch(softmax, device):
    sm = torch.as_tensor(softmax)
    if sm.dtype != torch.float32:
        sm = sm.to(torch.float32)
    single = sm.dim() == 2
    if single:
        sm = sm.unsqueeze(0)
    if sm.dim() != 3:
        raise _lib.InvalidArgumentError(-1, "softmax must be [T,C] or [B,T,C], got %s" % (tuple(sm.shape),))
    if not sm.is_cuda:
        sm = sm.to(device or "cuda:0")
    return sm.contiguous(), single


def decode_batch(kind, softmax, lengths=None, lockout=3, thres=0.5, loose_thres=0.2, max_words=None,
                 device=None):
    """-> (words [B,max_words] int32, counts [B] int32) device tensors."""
    lib = _lib.load()
    sm, _ = _as_batch(softmax, device)
    b, t, c = (int(v) for v in sm.shape)
    if max_words is None:
        max_words = max(t, 1)
    words = torch.zeros(b, max_words, dtype=torch.int32, device=sm.device)
    counts = torch.zeros(b, dtype=torch.int32, device=sm.device)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=sm.device, dtype=torch.int32).contiguous()
    with torch.cuda.device(sm.device):
        _lib.check(lib.kws_ctc_decode(kind, _lib.ptr(sm), _lib.ptr(lengths), b, t, c, int(lockout),
                                      float(thres), float(loose_thres), _lib.ptr(words), _lib.ptr(counts),
                                      int(max_words), _lib.current_stream_ptr()))
    return words, counts


def _format(words, counts, single):
    w = words.cpu().numpy()
    n = counts.cpu().numpy()
    outs = []
    for row, k in zip(w, n):
        k = min(int(k), w.shape[1])
        seq = np.zeros(2 * k + 1, np.int32)          # utils/prediction.py:58-62
        seq[1::2] = row[:k]
        outs.append(seq)
    return outs[0] if single else outs


def ctc_decode(softmax, lockout=3, thres=0.5, loose_thres=0.2, raw=False):
    """utils/prediction.py:18."""
    words, counts = decode_batch(_lib.DECODE, softmax, None, lockout, thres, loose_thres)
    return (words, counts) if raw else _format(words, counts, torch.as_tensor(softmax).dim() == 2)


def ctc_decode2(softmax, classnum, thres=0.4, raw=False):
    """utils/prediction.py:65."""
    _check_classnum(softmax, classnum)
    words, counts = decode_batch(_lib.DECODE2, softmax, None, 3, thres, 0.0)
    return (words, counts) if raw else _format(words, counts, torch.as_tensor(softmax).dim() == 2)


def ctc_decode_strict(softmax, classnum, lockout=3, thres=0.5, raw=False):
    """utils/prediction.py:89."""
    _check_classnum(softmax, classnum)
    words, counts = decode_batch(_lib.DECODE_STRICT, softmax, None, lockout, thres, 0.0)
    return (words, counts) if raw else _format(words, counts, torch.as_tensor(softmax).dim() == 2)


def _check_classnum(softmax, classnum):
    c = int(torch.as_tensor(softmax).shape[-1])
    if int(classnum) != c:
        raise _lib.InvalidArgumentError(-1, "classnum=%d but softmax has %d columns" % (classnum, c))


def ctc_predict(seq, label="1233"):
    """utils/prediction.py:111 -- seq is a decoded [0,w,0,...] array (or any int sequence; a
    negative entry terminates it).  Returns 0/1.  A (words, counts) pair of device tensors returns a
    device tensor of hits."""
    lib = _lib.load()
    if isinstance(seq, tuple):
        words, counts = seq
        b, mw = int(words.shape[0]), int(words.shape[1])
        hit = torch.zeros(b, dtype=torch.int32, device=words.device)
        with torch.cuda.device(words.device):
            _lib.check(lib.kws_ctc_predict(_lib.ptr(words), _lib.ptr(counts), b, mw, label.encode(),
                                           _lib.ptr(hit), _lib.current_stream_ptr()))
        return hit
    vals = []
    for v in np.asarray(seq).ravel().tolist():
        if v < 0:
            break
        if v > 0:
            vals.append(int(v))
    if any(v > 9 for v in vals):
        raise _lib.InvalidArgumentError(-1, "ctc_predict words must be single digits")
    words = torch.tensor([vals + [0]], dtype=torch.int32, device="cuda:0")
    counts = torch.tensor([len(vals)], dtype=torch.int32, device="cuda:0")
    return int(ctc_predict((words, counts), label)[0].item())


def ctc_beam_search_decode(inputs, lengths=None, beam_width=None, top_paths=1, merge_repeated=True, max_len=64, device=None):
    """tf.nn.ctc_beam_search_decoder as models/rnn_ctc.py:105-110 would call it (kws_ctc_beam_search, the exact-candidate form):
    inputs [B,T,C] logits or log(softmax) -- the kernel normalises each row itself --, the blank the last class.  beam_width None
    is C - 1, config.beam_size.  -> (dense [B,K,max_len] int32 padded with -1, log_probs [B,K]) device tensors, descending per
    utterance; a [T,C] input is one utterance and returns [K,max_len] and [K].  A row of `dense` goes straight into ctc_predict."""
    lib = _lib.load()
    x, single = _as_batch(inputs, device)
    if x.data_ptr() % 16:
        x = x.clone()
    b, t, c = (int(v) for v in x.shape)
    width = c - 1 if beam_width is None else int(beam_width)
    k, l_max = int(top_paths), int(max_len)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int32).contiguous()
        if tuple(lengths.shape) != (b,):
            raise _lib.InvalidArgumentError(-1, "lengths must be [%d], got %s" % (b, tuple(lengths.shape)))
    dense = torch.empty(b, max(k, 0), max(l_max, 0), dtype=torch.int32, device=x.device)
    lens = torch.empty(b, max(k, 0), dtype=torch.int32, device=x.device)
    log_probs = torch.empty(b, max(k, 0), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.kws_ctc_beam_search(_lib.ptr(x), _lib.ptr(lengths), b, t, c, width, k, l_max, 1 if merge_repeated else 0,
                                           _lib.ptr(dense), _lib.ptr(lens), _lib.ptr(log_probs), _lib.current_stream_ptr()))
    return (dense[0], log_probs[0]) if single else (dense, log_probs)


def decode_best(inputs, lengths=None, beam_width=None, merge_repeated=True, max_len=64, device=None):
    """The beam search's top path in the form of the other decoders: the words (labels above the space class 0) as the int32 array
    [0,w1,0,w2,0,...]; a batch gives a list of them.  What WERCalculator.cal_batch_wer and ctc_predict / evaluate take."""
    dense, _ = ctc_beam_search_decode(inputs, lengths, beam_width, 1, merge_repeated, max_len, device)
    single = dense.dim() == 2
    outs = [path_to_seq(row) for row in dense.reshape(-1, dense.shape[-1]).cpu().numpy()]
    return outs[0] if single else outs


def path_to_seq(path):
    """One row of ctc_beam_search_decode's dense output (labels, -1 past the end) -> the reference's [0,w,0,...] form."""
    row = np.asarray(path).ravel()
    end = np.flatnonzero(row < 0)
    row = row[:end[0] if len(end) else len(row)]
    w = row[row > 0].astype(np.int32)
    seq = np.zeros(2 * len(w) + 1, np.int32)
    seq[1::2] = w
    return seq


def evaluate(result, target):
    """utils/prediction.py:203 -- (miss, positives, false_accept)."""
    if len(result) != len(target):
        raise AssertionError("result and target differ in length")
    r = np.asarray(result, bool)
    t = np.asarray(target, bool)
    return int((t & ~r).sum()), int(t.sum()), int((r & ~t).sum())


def tokens_to_seq(tokens_row):
    """Fused kws_step token events of one stream ([T] int8) -> the reference's [0,w,0,...] form."""
    row = np.asarray(torch.as_tensor(tokens_row).cpu())
    w = row[row > 0].astype(np.int32)
    seq = np.zeros(2 * len(w) + 1, np.int32)
    seq[1::2] = w
    return seq


def ctc_label(words):
    """The dataset's label form (process_wav.py:57-66 convert_label): the word classes with the space class 0 around and between
    them, [0, w1, 0, w2, ..., 0] -- what tf.nn.ctc_loss is trained on, and what kws_ctc_loss / kws_enroll_fit take as `labels`."""
    words = [int(w) for w in words]
    if not words:
        raise _lib.InvalidArgumentError(-1, "ctc_label needs at least one word (convert_label asserts len(label) > 0)")
    if any(w < 1 for w in words):
        raise _lib.InvalidArgumentError(-1, "ctc_label words are classes >= 1 (0 is the space), got %s" % (words,))
    out = np.zeros(2 * len(words) + 1, np.int32)
    out[1::2] = words
    return out
