#!/usr/bin/env python3
"""kws_attention_run (the self-attention CTC model, attention_ctc.DeployModel) at the reference shape (config/attention_config.py)
over B in {1, 16, 256, 4096} x T in {100, 300, 1000} mel frames, equal lengths and ragged lengths uniform in [T/2, T]:
ms per call (HIP events, median), utterances/s, mel-frames/s, algorithmic TFLOP/s and its fraction of the 157.3 TF fp32
matrix peak, and a torch-eager fp32 build of the same model on the same GPU (cuBLAS-class GEMMs, SDPA, masked layer norm),
timed the same way and checked against ours.  --precision fp32,f16x3: one row per precision and shape, both handles in the same
process, and on every row after the first precision's its speed-up over that one (`vs_<first>`); rows carry the spread
(min, max) of their repetitions.

    python tools/bench_attention.py [--shapes 4096x300,...] [--precision fp32,f16x3] [--reps 10] [--out bench_attention.json]

FLOPs per utterance (multiply-add = 2): 2 T' c F H + L (6 T' H^2 + 4 T'^2 H + 4 T' H Fi) + 2 T' H C, T' = T // c + 1.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from keyword_spotting_amd import attention_weights as AW                      # noqa: E402
from keyword_spotting_amd.attention_ctc import DeployModel, frames_out       # noqa: E402
from keyword_spotting_amd.config import get_attention_config                 # noqa: E402

PEAK_TF = 157.3
EAGER_SCORE_BYTES = 8 << 30            # the eager build materialises B x heads x T'^2 scores: skipped above this


def flops(cfg, t1):
    c, F, H, L, Fi, C = cfg.combine_frame, cfg.n_mel, cfg.hidden_size, cfg.num_layers, cfg.feed_forward_inner_size, cfg.num_classes
    t1 = np.asarray(t1, np.float64)
    return float((2 * t1 * c * F * H + L * (6 * t1 * H * H + 4 * t1 * t1 * H + 4 * t1 * H * Fi) + 2 * t1 * H * C).sum())


class Eager(object):
    """The contract in torch fp32 ops, batched with masks (keys past T'_b excluded, LN moments over each utterance's block)."""

    def __init__(self, cfg, w):
        self.cfg = cfg
        d = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda")
        self.w = {k: d(v) for k, v in w.items() if k != "layers"}
        self.layers = [{k: d(v) for k, v in lay.items()} for lay in w["layers"]]
        rows = cfg.max_frames // cfg.combine_frame + 1
        p = torch.arange(rows, dtype=torch.float64)[:, None]
        a = p / torch.pow(torch.tensor(10000.0, dtype=torch.float64),
                          2.0 * torch.arange(cfg.hidden_size // 2, dtype=torch.float64) / cfg.hidden_size)
        self.pe = torch.stack([torch.sin(a), torch.cos(a)], -1).reshape(rows, cfg.hidden_size).float().cuda()

    def _ln(self, x, m, cnt, g, b):
        mean = (x * m).sum((1, 2), keepdim=True) / cnt
        var = (((x - mean) * m) ** 2).sum((1, 2), keepdim=True) / cnt
        return (x - mean) / torch.sqrt(var + 1e-12) * g + b

    def __call__(self, mel, lengths):
        cfg, w = self.cfg, self.w
        c, H, heads = cfg.combine_frame, cfg.hidden_size, cfg.multi_head_num
        B, T, F = mel.shape
        T1 = frames_out(cfg, T)
        if c > 1:
            mel = Fn.pad(mel, (0, 0, 0, T1 * c - T))
        mel = mel * (torch.arange(T1 * c, device="cuda")[None, :] < lengths[:, None])[..., None]
        n = lengths // c + 1 if c > 1 else lengths
        rm = (torch.arange(T1, device="cuda")[None, :] < n[:, None])
        m = rm[..., None].float()
        cnt = (n.float() * H)[:, None, None]
        x = mel.reshape(B, T1, c * F) @ w["W_in"] + w["b_in"] + self.pe[:T1]
        mask = rm[:, None, None, :]
        for lay in self.layers:
            q, k, v = (x @ lay["W_qkv"] + lay["b_qkv"]).split(H, -1)
            sp = lambda a: a.reshape(B, T1, heads, H // heads).transpose(1, 2)
            att = Fn.scaled_dot_product_attention(sp(q), sp(k), sp(v), attn_mask=mask).transpose(1, 2).reshape(B, T1, H)
            y = self._ln(att + x, m, cnt, lay["ln_a_gamma"], lay["ln_a_beta"])
            z = torch.relu(y @ lay["W1"] + lay["b1"]) @ lay["W2"] + lay["b2"]
            x = self._ln(z + y, m, cnt, lay["ln_b_gamma"], lay["ln_b_beta"])
        logits = x @ w["W_out"] + w["b_out"]
        if cfg.use_relu:
            logits = torch.relu(logits)
        return logits * m, torch.softmax(logits, -1) * m


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x100,1x300,1x1000,16x100,16x300,16x1000,256x100,256x300,256x1000,4096x100,4096x300,4096x1000")
    ap.add_argument("--ragged", default="both", choices=("both", "equal", "ragged"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--precision", default="fp32", help="comma-separated: fp32, f16x3")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = get_attention_config()
    w = AW.init(cfg, 0)
    precisions = a.precision.split(",")
    models = {pr: DeployModel(cfg, w, precision=pr) for pr in precisions}
    eager = None if a.no_eager else Eager(cfg, w)
    rows = []
    for shape in a.shapes.split(","):
        B, T = (int(v) for v in shape.split("x"))
        for ragged in ((False, True) if a.ragged == "both" else (a.ragged == "ragged",)):
            g = torch.Generator(device="cpu").manual_seed(B * 7 + T)
            mel = torch.randn(B, T, cfg.n_mel, generator=g).cuda()
            lengths = (torch.randint(T // 2, T + 1, (B,), generator=g) if ragged else torch.full((B,), T)).to(torch.int32).cuda()
            t1 = [frames_out(cfg, int(v)) for v in lengths.cpu()]
            fl = flops(cfg, t1)
            base_ms = None
            for pr in precisions:
                model = models[pr]
                model.reserve(B, T)
                med, ms = timed(lambda: model.forward(mel, lengths, want_logits=False), a.reps)
                row = dict(B=B, T=T, ragged=ragged, precision=pr, ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                           utt_per_s=round(B / med * 1e3, 1), mel_frames_per_s=round(float(lengths.sum()) / med * 1e3, 1),
                           gflop=round(fl / 1e9, 3), tflops=round(fl / med / 1e9, 2), frac_peak=round(fl / med / 1e9 / PEAK_TF, 3))
                if base_ms is None:
                    base_ms = med
                else:
                    row["vs_" + precisions[0]] = round(base_ms / med, 3)
                t1max = frames_out(cfg, T)
                if eager is not None and B * cfg.multi_head_num * t1max * t1max * 4 <= EAGER_SCORE_BYTES:
                    with torch.no_grad():
                        e_med, _ = timed(lambda: eager(mel, lengths), max(3, a.reps // 2))
                        el, es = eager(mel, lengths)
                    r = model.forward(mel, lengths)
                    row.update(eager_ms=round(e_med, 4), speedup_vs_eager=round(e_med / med, 2),
                               eager_max_dlogit=float((el - r["logits"]).abs().max()), eager_max_dsoftmax=float((es - r["softmax"]).abs().max()))
                    del el, es, r
                else:
                    row.update(eager_ms=None)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del mel, lengths
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(dict(device=torch.cuda.get_device_name(0), config="reference (n_mel 60, c 2, H 128, 8 heads, Fi 512, L 3, C 6)",
                       peak_tf=PEAK_TF, rows=rows), open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
