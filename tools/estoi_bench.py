"""What ESTOI costs on the device, on the 64 clips of tools/eval_batch_bench.py (1-6 s at 16 kHz, seeded).

  kernel    snrse.ops.estoi(fs=16000) over the ragged batches of the evaluation plan (batch_size 32), the clips
            already on the device: both resampling launches and the five snrse_estoi launches per batch, between device
            events, `--reps` timed runs after `--warmup` untimed ones; and the same for the 10 kHz signals alone
            (fs=10000: snrse_estoi without the resampler).
  evaluate  the batched evaluation of the fp16 one-step SNR-aligned model at batch_size 32 (enhance_batch and the
            energy-ratio launch per batch, as tools/eval_batch_bench.py times it: no file I/O, no PESQ) without (A) and
            with (B) snrse.evaluate.estoi_batch per batch, alternated A B A B ... in one process, `--rounds` of each.
  host      tests/estoi_ref.py (fp64 numpy) on the same clips, one file after the other on the CPU.  It is the only
            CPU implementation at hand and it is NOT pystoi.

Writes profiles/estoi_bench.json.

    python tools/estoi_bench.py [--clips 64] [--batch-size 32] [--reps 20] [--warmup 3] [--rounds 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snr-aligned_diffse_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(v, nd=3):
    v = sorted(v)
    return {"median": round(float(np.median(v)), nd), "min": round(v[0], nd), "max": round(v[-1], nd), "n": len(v)}


def ragged(rows, dev):
    buf = np.zeros((len(rows), max(len(r) for r in rows)), np.float32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = r
    return torch.from_numpy(buf).to(dev)


def bench_kernel(data, plan, fs, args, dev):
    """ms for all clips: every batch of the plan through ops.estoi, between one pair of device events."""
    from snrse import ops
    if fs == 16000:
        bufs = [(ragged([data[i][0] for i in b], dev), ragged([data[i][1] for i in b], dev),
                 [len(data[i][0]) for i in b]) for b in plan]
    else:  # the 10 kHz signals, resampled once outside the timed region
        from snrse import audio
        taps = audio.stoi_resample_taps(5, 8)
        bufs = []
        for b in plan:
            lens = [len(data[i][0]) for i in b]
            x, ol = ops.resample_poly(ragged([data[i][0] for i in b], dev), 5, 8, lengths=lens, taps=taps)
            y, _ = ops.resample_poly(ragged([data[i][1] for i in b], dev), 5, 8, lengths=lens, taps=taps)
            bufs.append((x, y, ol.cpu().numpy()))
    ms = []
    for r in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for x, y, lens in bufs:
            ops.estoi(x, y, lengths=lens, fs=fs)
        e1.record()
        e1.synchronize()
        if r >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    return stats(ms)


def run_batched(model, data, kw, batch_size, max_frames, estoi):
    from snrse import batching, evaluate
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in data]
    vals = [None] * len(data)
    for b in batching.plan_batches([len(y) for _, y in data], batch_size, max_frames):
        hs = model.enhance_batch([data[i][1] for i in b], seeds=[seeds[i] for i in b], batch_size=len(b),
                                 max_frames=max_frames, **kw)
        evaluate.score_batch(hs, [data[i][0] for i in b], [data[i][1] for i in b])
        if estoi:
            for i, v in zip(b, evaluate.estoi_batch(hs, [data[i][0] for i in b])):
                vals[i] = float(v)
    return vals


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--max-frames", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-evaluate", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estoi_bench.json"))
    args = ap.parse_args(argv)
    import estoi_ref
    import eval_batch_bench as ebb
    from snrse import batching
    dev = torch.device("cuda", 0)
    data = ebb.clips(args.clips)
    secs = [len(y) / 16000.0 for _, y in data]
    plan = batching.plan_batches([len(y) for _, y in data], args.batch_size, args.max_frames)
    out = {"clips": args.clips, "seconds_total": round(sum(secs), 2), "batch_size": args.batch_size,
           "batches": len(plan), "device": torch.cuda.get_device_name(0),
           "launches_per_batch": {"resample": 2, "estoi": 5}, "readbacks_per_batch_added": 1}
    out["ops_estoi_fs16000_ms_all_clips"] = bench_kernel(data, plan, 16000, args, dev)
    out["ops_estoi_fs10000_ms_all_clips"] = bench_kernel(data, plan, 10000, args, dev)
    print(json.dumps(out), flush=True)
    if not args.no_evaluate:
        from sgmse.model import set_snr_model
        m, keys = ebb.formula_model("sebridge_v3", "true", "fp16", fixed_snr=0.17783)
        set_snr_model(ebb.formula_snr_estimator(keys))
        kw = dict(sampler_type="pc", N=30)
        torch.manual_seed(1)
        for flag in (False, True):  # warm-up: both variants, every batch shape of the timed runs
            run_batched(m, data, kw, args.batch_size, args.max_frames, flag)
        a, b = [], []
        for _ in range(args.rounds):  # A B A B ...
            for flag, acc in ((False, a), (True, b)):
                torch.manual_seed(7)
                t, _ = ebb.timed(lambda: run_batched(m, data, kw, args.batch_size, args.max_frames, flag))
                acc.append(t)
            print(f"evaluate batch_size {args.batch_size}: {a[-1]:.3f} s, with estoi {b[-1]:.3f} s", flush=True)
        out["evaluate_one_step_s"] = stats(a, 4)
        out["evaluate_one_step_estoi_s"] = stats(b, 4)
        out["evaluate_files_per_s"] = round(args.clips / float(np.median(a)), 1)
        out["evaluate_estoi_files_per_s"] = round(args.clips / float(np.median(b)), 1)
        out["estoi_share_of_evaluate"] = round(1.0 - float(np.median(a)) / float(np.median(b)), 4)
        out["difference_beyond_spread"] = bool(min(b) > max(a))
    if not args.no_host:
        t0 = time.perf_counter()
        for x, y in data:
            estoi_ref.estoi(x, y, 16000)
        out["host_reference_s_all_clips"] = round(time.perf_counter() - t0, 3)
        out["host_reference"] = "tests/estoi_ref.py, fp64 numpy + scipy resample_poly, one process; not pystoi"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
