"""The configuration grid of tests/test_gpu_config_space.py and tests/test_config_space_refs.py: rows inside the space
kws_create accepts (api_model.hip:config_ok), the launch layout api_step.hip picks for each, and the rows just outside it.

`expected_names` restates the selection rules of api_step.hip (plan_step, the one place that holds them) and of
the packer (weight_pack.hip: resident_ok, f16_kx0, bf_kx0), so that a row's layout column is checked against the rules
and kernel_names() is checked against both."""
import zlib
from collections import namedtuple

STREAMS_PER_GROUP = 16
RESIDENT_MEL = (32, 40, 48, 60, 64)          # gru_resident_supported, first layer
OVERLAP_MIN_T = 64                           # KWS_OVERLAP_MIN_T

Row = namedtuple("Row", "name prec kernel n_mel hidden layers classes batch frames relu clip layout "
                        "masks chunk twin wfc")
# layout: "single" (one layer, one launch) | "seq" (one launch per layer) | "pipe" (all layers in one grid; XCD-affine
# when 8 % L == 0) | "ovl" (layers on streams, time-blocked) | "f16x3" (register-resident f16x3, one launch per layer)
# | "bf16" (one stack launch) | "int8" (fp32 layer 0, octbit layers, octbit projection)
# masks: random seq_len / reset mask.  chunk: chunked calls == one call, bitwise.
# twin: the same streams inside a batch too large for this row's layout -- "ovl" rows: bitwise equal;
# "pipe" rows: T of a sequential-sized batch (16 * (CUs // L + 1) + 1 streams), sampled against the oracle and bitwise
# equal to the pipelined launch on the shared streams.
# wfc: scale of the class projection (relu rows: 20, so that logits cross the clip at 20; others: words occur; int8 rows
# keep 1: a quantiser flip moves a logit by |w_q| * scale, which grows with the projection, and the tolerance does not).


def R(name, prec, kernel, n_mel, hidden, layers, classes, batch, frames, layout, relu=0, clip=-1.0, masks=False,
      chunk=False, twin=0, wfc=1.0):
    return Row(name, prec, kernel, n_mel, hidden, layers, classes, batch, frames, relu, clip, layout, masks, chunk, twin, wfc)


ROWS = [
    # fp32 generic, single layer (FIRST && LAST)
    R("fp32_single_n1", "fp32", "auto", 1, 64, 1, 3, 17, 33, "single", chunk=True, wfc=3.0),
    R("fp32_single_n13", "fp32", "auto", 13, 128, 1, 8, 1, 40, "single", wfc=3.0),
    # fp32 generic, layer-pipelined, XCD-affine (8 % L == 0)
    R("fp32_pipe_n13_L8", "fp32", "auto", 13, 64, 8, 8, 33, 20, "pipe", chunk=True, twin=8, wfc=3.0),
    R("fp32_pipe_n100_L2", "fp32", "generic", 100, 128, 2, 4, 16, 24, "pipe", masks=True, wfc=2.0),
    R("fp32_pipe_n1024_L2", "fp32", "auto", 1024, 256, 2, 8, 5, 12, "pipe", wfc=2.0),
    # fp32 generic, layer-pipelined, plain
    R("fp32_pipe_n257_L3", "fp32", "auto", 257, 256, 3, 7, 15, 16, "pipe", masks=True, wfc=2.0),
    R("fp32_pipe_n65_L7", "fp32", "auto", 65, 64, 7, 5, 16, 12, "pipe", wfc=3.0),
    R("fp32_pipe_n100_L5", "fp32", "generic", 100, 128, 5, 4, 31, 24, "pipe", twin=8, wfc=2.0),
    R("fp32_pipe_n63_L6", "fp32", "generic", 63, 128, 6, 3, 17, 12, "pipe", masks=True, wfc=2.0),
    # fp32 under auto, n_mel not resident: generic layer 0, resident layers 1..
    R("fp32_mixed_n100_L2", "fp32", "auto", 100, 128, 2, 4, 16, 24, "seq", wfc=2.0),
    R("fp32_mixed_n63_L6", "fp32", "auto", 63, 128, 6, 3, 17, 12, "seq", masks=True, wfc=2.0),
    R("fp32_mixed_n13_L3_ovl", "fp32", "auto", 13, 128, 3, 8, 5, 64, "ovl", twin=1, wfc=2.0),
    # fp32 resident, overlapped on streams
    R("fp32_res_n32_L5_ovl", "fp32", "auto", 32, 128, 5, 8, 19, 64, "ovl", chunk=True, twin=1, wfc=2.0),
    R("fp32_res_n48_L4_ovl", "fp32", "auto", 48, 128, 4, 3, 3, 65, "ovl", masks=True, twin=1, wfc=2.0),
    R("fp32_res_n64_L5_ovl", "fp32", "auto", 64, 128, 5, 7, 1, 127, "ovl", twin=1, wfc=2.0),
    # fp32 resident, sequential past the overlap limit (L > 5)
    R("fp32_res_n40_L6", "fp32", "auto", 40, 128, 6, 4, 17, 100, "seq", masks=True, wfc=2.0),
    R("fp32_res_n60_L8", "fp32", "auto", 60, 128, 8, 8, 33, 70, "seq", wfc=2.0),
    # f16x3, hidden 256: the L2-streaming kernels
    R("f16x3g_n4_L3", "f16x3", "auto", 4, 256, 3, 8, 17, 10, "pipe", chunk=True, wfc=1.0),
    R("f16x3g_n36_L8", "f16x3", "auto", 36, 256, 8, 3, 16, 8, "pipe", twin=8, wfc=1.0),
    R("f16x3g_n64_L5", "f16x3", "auto", 64, 256, 5, 4, 33, 8, "pipe", masks=True, wfc=1.0),
    # int8: layer 0 on the fp32 generic kernel (n_mel not resident), octbit layers 1.., octbit projection
    R("int8_n13_L2", "int8", "auto", 13, 128, 2, 3, 21, 20, "int8", masks=True),
    R("int8_n100_L5", "int8", "auto", 100, 128, 5, 8, 17, 12, "int8"),
]

# f16x3, hidden 128 (register-resident kernels; f16_kx0 = 1 up to n_mel 32, 2 above): every n_mel x C pairing
_F16_LAYERS, _F16_BATCH = (1, 2, 5, 8), (1, 15, 17, 33)
for _i, _n in enumerate((4, 8, 28, 36, 52, 56)):
    for _j, _c in enumerate((3, 4, 7, 8)):
        _b = _F16_BATCH[(_i + 2 * _j + 1) % 4]
        ROWS.append(R("f16x3_n%d_C%d" % (_n, _c), "f16x3", "auto", _n, 128, _F16_LAYERS[(_i + _j) % 4], _c, _b,
                      64 if _b == 1 else 16, "f16x3", masks=(_i + _j) % 3 == 0, wfc=3.0))
# bf16 (hidden 128, L <= 2; bf_kx0 = 1 up to n_mel 32, 2 above)
for _i, _n in enumerate((4, 16, 28, 36, 64)):
    for _l in (1, 2):
        ROWS.append(R("bf16_n%d_L%d" % (_n, _l), "bf16", "auto", _n, 128, _l, (3, 8)[(_i + _l) % 2], (9, 17)[_l - 1], 20,
                      "bf16", masks=_i % 2 == 0, wfc=3.0))
# relu with and without the clip at 20 (models/rnn_ctc.py:280-283: clipped to [0, 20] whenever value_clip > 0)
_RELU = [("fp32_res", "fp32", "auto", 40, 128, 2, 5, "seq"), ("fp32_pipe", "fp32", "auto", 13, 64, 4, 7, "pipe"),
         ("f16x3", "f16x3", "auto", 36, 128, 2, 8, "f16x3"), ("f16x3g", "f16x3", "auto", 20, 256, 2, 3, "pipe"),
         ("bf16", "bf16", "auto", 28, 128, 2, 4, "bf16"), ("int8", "int8", "auto", 13, 128, 2, 8, "int8")]
for _name, _p, _k, _n, _h, _l, _c, _lay in _RELU:
    for _clip in (-1.0, 0.0, 0.5):
        ROWS.append(R("relu_%s_clip%g" % (_name, _clip), _p, _k, _n, _h, _l, _c, 9, 16, _lay, relu=1, clip=_clip, wfc=20.0))

# just outside the accepted space: (precision, n_mel, hidden, layers, classes)
OUTSIDE = [("fp32", 0, 128, 2, 6), ("fp32", 1025, 128, 2, 6), ("fp32", 40, 128, 0, 6), ("fp32", 40, 128, 9, 6),
           ("fp32", 40, 128, 2, 2), ("fp32", 40, 128, 2, 9), ("fp32", 40, 32, 2, 6), ("fp32", 40, 512, 2, 6),
           ("f16x3", 2, 128, 2, 6), ("f16x3", 66, 128, 2, 6), ("f16x3", 68, 128, 2, 6), ("f16x3", 40, 64, 2, 6),
           ("bf16", 40, 128, 3, 6), ("bf16", 68, 128, 2, 6), ("int8", 40, 256, 2, 6)]

PRECISION = {"fp32": 0, "bf16": 1, "int8": 2, "f16x3": 3}


def seed_of(row):
    return zlib.crc32(row.name.encode()) & 0x7FFFFFFF


def groups(batch):
    return (batch + STREAMS_PER_GROUP - 1) // STREAMS_PER_GROUP


def sequential_batch(layers, cus):
    """The smallest batch whose L x groups workgroups no longer fit the chip at once."""
    return STREAMS_PER_GROUP * (cus // layers + 1) + 1


def _resident_ok(row, l):
    return row.hidden == 128 and (l > 0 or row.n_mel in RESIDENT_MEL)


def layout_of(row, batch, frames, cus):
    """api_step.hip's choice for a (batch, frames) call of this row's model."""
    L = row.layers
    fits = groups(batch) * L <= cus
    if row.prec == "bf16":
        return "bf16"
    if row.prec == "f16x3":
        if row.hidden == 128:
            return "f16x3"
        return "pipe" if L >= 2 and fits else ("single" if L == 1 else "seq")
    if row.prec == "int8":
        return "int8"
    any_res = row.kernel == "auto" and any(_resident_ok(row, l) for l in range(L))
    if L >= 2 and row.kernel != "resident" and not any_res and fits:
        return "pipe"
    if L == 1:
        return "single"
    if 2 <= L <= 5 and fits and frames >= OVERLAP_MIN_T:
        return "ovl"
    return "seq"


def _tf(b):
    return "true" if b else "false"


def expected_names(row, batch, frames, cus):
    """kernel_names() after a (batch, frames) call, one entry per profiling slot."""
    L, H = row.layers, row.hidden
    lay = layout_of(row, batch, frames, cus)
    if row.prec == "bf16":
        kx = (row.n_mel + 31) // 32
        name = ("gru_stack_bf16_ls<%d> (both layers, one launch, 8 waves)" % kx) if L == 2 else "gru_stack_bf16<%d, 1>" % kx
        return [name] + [""] * (L - 1)
    if row.prec == "f16x3" and H == 128:
        kx0 = (row.n_mel + 31) // 32
        return ["gru_layer_f16x3<%d, %s, %s>" % (kx0 if l == 0 else 4, _tf(l == 0), _tf(l == L - 1)) for l in range(L)]
    if row.prec == "f16x3":
        if lay == "pipe":
            return [""] * (L - 1) + ["gru_stack_f16x3_pipelined<%d> (all %d layers, one launch)" % (H // 64, L)]
        return ["gru_layer_f16x3_generic<%d, %s, %s>" % (H // 64, _tf(l == 0), _tf(l == L - 1)) for l in range(L)]
    if lay == "pipe":
        return [""] * (L - 1) + ["gru_stack_generic_pipelined<%d> (all %d layers, one launch)" % (H // 64, L)]
    out = []
    for l in range(L):
        first, last = l == 0, l == L - 1 and row.prec != "int8"
        if row.prec == "int8" and l > 0:
            out.append("gru_layer_octbit_kernel + octbit_fc_kernel" if l == L - 1 else "gru_layer_octbit_kernel")
        elif row.kernel == "resident" or (row.kernel == "auto" and _resident_ok(row, l)):
            out.append("gru_layer_resident<%d, %s, %s>" % ((row.n_mel + 3) // 4 if first else 32, _tf(first), _tf(last)))
        else:
            out.append("gru_layer_generic<%d, %s, %s>" % (H // 64, _tf(first), _tf(last)))
    return out
