"""How much headroom does a checkpoint leave in the 16-bit formats?  `python -m snrse.range_check`

Runs NCSNppHIP.range_report (one network evaluation with ops.range_stats on every tensor the executor stores) at
a few times t of the t_30 grid and prints, per tensor, the peak magnitude, the headroom to fp16's 65504 in bits
and the number of inf / NaN elements, the first tensor (in execution order) that fp16 cannot hold, and a
recommended format.  Run on a bf16 executor (--dtype bf16) the peaks above 65504 come out finite, so the table
shows where fp16 would overflow without producing NaN first.  Exit status 1 when fp16 does not hold.

    python -m snrse.range_check --ckpt model.ckpt --wav noisy.wav
    python -m snrse.range_check --synthetic --dtype fp16        # formula weights when no --ckpt is given
"""
from __future__ import annotations

import argparse
import math
import sys

import torch

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


def max_finite(dtype):
    return float(torch.finfo(dtype).max)


def headroom_bits(peak, dtype=torch.float16, nonfinite=0):
    """log2(max_finite(dtype) / peak): the factor, in bits, by which the peak could grow before `dtype` overflows
    (negative: it already would); -inf when the tensor holds an inf / NaN or the peak itself is not finite, +inf
    for an all-zero tensor."""
    peak = float(peak)
    if nonfinite or not math.isfinite(peak):
        return -math.inf
    if peak == 0.0:
        return math.inf
    return math.log2(max_finite(dtype) / peak)


def first_offender(report, dtype=torch.float16):
    """Name of the first tensor, in execution order, that is non-finite or whose peak exceeds max_finite(dtype);
    None when every tensor fits."""
    lim = max_finite(dtype)
    for name, peak, nonfinite in report:
        if int(torch.as_tensor(nonfinite).sum()) > 0 or float(torch.as_tensor(peak).max()) > lim:
            return name
    return None


def merge(reports):
    """Fold several range reports of the same network (other t, other inputs) into one: per tensor the largest peak
    and the total non-finite count over all rows."""
    out = {}
    for rep in reports:
        for name, peak, nonfinite in rep:
            p, n = float(torch.as_tensor(peak).max()), int(torch.as_tensor(nonfinite).sum())
            q = out.get(name)
            out[name] = (p, n) if q is None else (max(p, q[0]), n + q[1])
    return [(name, torch.tensor([p]), torch.tensor([n])) for name, (p, n) in out.items()]


def format_report(report, dtype=torch.float16, title=None):
    """The table: tensor, peak over the batch, headroom to `dtype` in bits, non-finite elements; then the first
    offending tensor (or that all fit) and the smallest headroom."""
    lines = [title] if title else []
    lines.append(f"{'tensor':<24}{'peak |v|':>14}{'headroom bits':>15}{'nonfinite':>11}")
    worst = (math.inf, None)
    for name, peak, nonfinite in report:
        p, n = float(torch.as_tensor(peak).max()), int(torch.as_tensor(nonfinite).sum())
        hb = headroom_bits(p, dtype, n)
        if hb < worst[0]:
            worst = (hb, name)
        lines.append(f"{name:<24}{p:>14.6g}{hb:>15.2f}{n:>11d}")
    bad = first_offender(report, dtype)
    lim = max_finite(dtype)
    if bad is not None:
        lines.append(f"first tensor outside the {dtype} range ({lim:g}): {bad}")
    else:
        lines.append(f"every tensor fits {dtype} ({lim:g}); least headroom {worst[0]:.2f} bits at {worst[1]}")
    return "\n".join(lines)


def recommend(report):
    """'fp16' when every stored tensor is finite and within 65504, else 'bf16' (fp32's exponent range; 'fp32x3'
    where bf16's accuracy is not enough)."""
    return "fp16" if first_offender(report, torch.float16) is None else "bf16"


def _load_sd(ckpt):
    if ckpt is None:
        import json
        import os

        from . import formula
        root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        with open(os.path.join(root, "tests", "golden", "state_dict_keys.json")) as f:
            shapes = {k: tuple(s) for k, s in json.load(f)["ncsnpp"]}
        return {k: torch.from_numpy(v) for k, v in formula.formula_state_dict(shapes).items()}, "formula weights"
    blob = torch.load(ckpt, map_location="cpu", weights_only=False)
    sd = blob.get("state_dict", blob)
    sd = {k[len("dnn."):]: v for k, v in sd.items() if k.startswith("dnn.")} or sd
    return sd, ckpt


def _inputs(args, dev):
    from . import enhance, formula
    if args.wav:
        from . import audio
        y = audio.load(args.wav)[0][:1].contiguous().to(dev)  # first channel, [1, L]
        return enhance.front_end(y, 1)[0]
    return (torch.from_numpy(formula.normal_tensor("range_check.y", (args.batch, 256, args.frames), True)) * 0.5).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description="range headroom of an NCSN++ checkpoint in the 16-bit formats")
    ap.add_argument("--ckpt", type=str, default=None, help="checkpoint (default: the formula weights)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--wav", type=str, help="noisy utterance to probe with")
    src.add_argument("--synthetic", action="store_true", help="formula-normal spectrogram of 0.5 standard deviation")
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="bf16",
                    help="format of the probed executor (bf16 shows peaks above 65504 as finite numbers)")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--sigma", type=float, default=0.5, help="x_t = y + sigma t z")
    args = ap.parse_args(argv)
    from . import enhance, formula, ncsnpp, ops
    dev = ops.current_device()
    sd, what = _load_sd(args.ckpt)
    net = ncsnpp.NCSNppHIP(sd, dtype=DTYPES[args.dtype], device=dev)
    Y = _inputs(args, dev).contiguous()
    B = Y.shape[0]
    Z = torch.from_numpy(formula.normal_tensor("range_check.z", tuple(Y.shape), True)).to(dev)
    reports = []
    for k in (29, 15, 0):  # t = 1, the middle and the low end of the t_30 grid
        t = float(enhance.T_30[k])
        x = (Y + args.sigma * t * Z).contiguous()
        reports.append(net.range_report(x, Y, torch.full((B,), t, device=dev)))
    rep = merge(reports)
    print(format_report(rep, torch.float16, title=f"range_check: {what}, {args.dtype} executor, input {tuple(Y.shape)}, "
                        f"t in {[round(float(enhance.T_30[k]), 4) for k in (29, 15, 0)]}"))
    rec = recommend(rep)
    print(f"recommended format: {rec}" + ("" if rec == "fp16" else " (fp16 does not hold this checkpoint; "
                                                                   "the default guard would recompute in bf16)"))
    return 0 if rec == "fp16" else 1


if __name__ == "__main__":
    sys.exit(main())
