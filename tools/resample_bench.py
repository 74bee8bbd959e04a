"""Cost of the sample-rate front end: the polyphase kernel alone, and an enhance_batch call with and without it.

For 32 rows x 4 s at 48 kHz -> 16 kHz and at 44.1 kHz -> 16 kHz:
  kernel   snrse_resample_poly (ops.resample_poly on a device-resident batch) between device events, `--reps`
           launches per timing, `--repeats` timings after a warm-up: median and spread of the time per launch, and
           the bytes the kernel has to move (the input read once, the output written once) over that time;
  call     one ScoreModel.enhance_batch call (formula weights, fp16 'bbed' PC sampler, N = 30) of the batch with
           sample_rates, against the plain call on 16 kHz clips of the same lengths: host clock around each call (it
           ends in the download of its results), alternated A B A B after one warm-up call each.  The cost bar: the
           resampled call takes at most 1 % more than the plain one.
Writes profiles/resample_bench.json.

    python tools/resample_bench.py [--rows 32] [--seconds 4] [--N 30] [--rounds 3] [--out profiles/resample_bench.json]
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
for p in (ROOT, os.path.join(ROOT, "snr-aligned_diffse_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def clips(rows, L, sr, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / float(sr)
    return [(0.2 * np.sin(2 * np.pi * rng.uniform(150.0, 900.0) * t) + 0.05 * rng.standard_normal(L)).astype(np.float32)
            for _ in range(rows)]


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": v[0], "max": v[-1], "n": len(v)}


def kernel_timing(x, up, down, reps, repeats):
    from snrse import _lib, audio, ops
    y, _ = ops.resample_poly(x, up, down)  # builds and caches the taps; y is the output buffer of the timed launches
    taps, half = ops.cached_taps(audio.resample_taps, up, down, x.device)
    B, L = x.shape
    ln = torch.full((B,), L, dtype=torch.int32, device=x.device)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        _lib.call("snrse_resample_poly", x.data_ptr(), ln.data_ptr(), B, L, up, down, half, taps.data_ptr(),
                  y.data_ptr(), y.shape[1], stream)

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / reps)
    nbytes = 4 * (x.numel() + y.numel())
    s = spread(us)
    return {"us_per_launch": s, "bytes_moved": nbytes, "gb_per_s_at_median": nbytes / s["median"] * 1e-3,
            "launches_per_timing": reps, "taps": 2 * half + 1}


def timed_call(model, ys, seeds, N, rates):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.enhance_batch(ys, seeds=seeds, batch_size=len(ys), N=N, sample_rates=rates)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtype", type=str, default="fp16")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: needs a HIP device; nothing is measured without one")
    from eval_batch_bench import formula_model
    from snrse import audio
    dev = torch.device("cuda", 0)
    model, _ = formula_model("bbed", "false", a.dtype)
    seeds = list(range(1000, 1000 + a.rows))
    res = {"rows": a.rows, "seconds": a.seconds, "N": a.N, "dtype": a.dtype, "device": torch.cuda.get_device_name(0),
           "rates": {}}
    for sr in (48000, 44100):
        L = int(round(a.seconds * sr))
        L16 = audio.resampled_length(L, sr, 16000)
        up, down = audio.rational(sr, 16000)
        ys = clips(a.rows, L, sr, sr)
        plain = clips(a.rows, L16, 16000, sr + 1)  # the plain call: 16 kHz clips of the same lengths
        entry = {"up": up, "down": down, "samples_in": L, "samples_16k": L16,
                 "kernel": kernel_timing(torch.from_numpy(np.stack(ys)).to(dev), up, down, a.reps, a.repeats)}
        timed_call(model, plain, seeds, a.N, None)  # warm-up of both shapes
        timed_call(model, ys, seeds, a.N, [sr] * a.rows)
        tp, tr = [], []
        for _ in range(a.rounds):
            tp.append(timed_call(model, plain, seeds, a.N, None)[0])
            t, out = timed_call(model, ys, seeds, a.N, [sr] * a.rows)
            tr.append(t)
        assert all(len(h) == L16 and np.isfinite(h).all() for h in out)
        sp, sr_ = spread(tp), spread(tr)
        entry["call"] = {"plain_s": sp, "resampled_s": sr_, "order": "plain, resampled, alternated",
                         "overhead_s_at_median": sr_["median"] - sp["median"],
                         "overhead_fraction_at_median": sr_["median"] / sp["median"] - 1.0,
                         "bar": "resampled <= 1.01 x plain"}
        print(json.dumps({sr: entry}), flush=True)
        res["rates"][str(sr)] = entry
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
