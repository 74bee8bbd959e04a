"""Cost of keeping the band above 8 kHz: the two high-band kernels alone, and an enhance_batch call with and without them.

For 32 rows x 4 s at 48 kHz and at 44.1 kHz:
  kernels  leg A, the step they replace: the plain 16 k -> R snrse_resample_poly launch on the enhanced rows; leg B:
           snrse_band_gain (two launches) + snrse_resample_mix on the same rows, and the mix alone.  Device-resident
           inputs, 3 warm-up runs and `--runs` timed runs per leg between device events (`--reps` launches per run),
           the legs alternated A B A B in one process: median and spread of the time per launch, the bytes each has to
           move (inputs read once, the output written once) and the rate that makes;
  call     one ScoreModel.enhance_batch(output_rate="input") call (formula weights, fp16 'bbed' PC sampler, N = 30)
           with highband="follow" against highband="drop": host clock around each call (it ends in the download of its
           results), `--warmup` warm-up calls and `--rounds` timed calls per leg, alternated A B A B.  The bar is the
           front end's: follow takes at most 1 % more than drop, on top of the spread of the drop runs.
Writes profiles/highband_bench.json.

    python tools/highband_bench.py [--rows 32] [--seconds 4] [--N 30] [--warmup 3] [--rounds 20]
        [--out profiles/highband_bench.json]
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

from resample_bench import clips, spread  # noqa: E402


def timed(launch, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernel_legs(y, rate, runs, reps):
    """y [B, L] on the device at `rate` -> the timings of the plain resampler and of the high-band kernels."""
    from snrse import _lib, audio, ops
    B, L = y.shape
    up, down = audio.rational(audio.MODEL_RATE, rate)
    u, _ = ops.resample_poly(y, down, up)  # the 16 kHz rows the enhancers would consume
    L16 = u.shape[1]
    x = (0.6 * u + 0.01 * torch.randn_like(u)).contiguous()  # a stand-in for their results
    taps, half = ops.cached_taps(audio.resample_taps, up, down, y.device)
    l16 = torch.full((B,), L16, dtype=torch.int32, device=y.device)
    lR = torch.full((B,), L, dtype=torch.int32, device=y.device)
    T = 1 + L16 // 128
    fr = torch.full((B,), T, dtype=torch.int32, device=y.device)
    energies = torch.empty(B, 2, T, dtype=torch.float64, device=y.device)
    gains = torch.empty(B, T, dtype=torch.float32, device=y.device)
    out = torch.empty(B, L, dtype=torch.float32, device=y.device)
    stream = torch.cuda.current_stream().cuda_stream

    def plain():
        _lib.call("snrse_resample_poly", x.data_ptr(), l16.data_ptr(), B, L16, up, down, half, taps.data_ptr(),
                  out.data_ptr(), L, stream)

    def gain():
        _lib.call("snrse_band_gain", u.data_ptr(), x.data_ptr(), l16.data_ptr(), B, L16, T, 10.0 ** -1.5,
                  energies.data_ptr(), gains.data_ptr(), stream)

    def mix():
        _lib.call("snrse_resample_mix", x.data_ptr(), u.data_ptr(), l16.data_ptr(), L16, y.data_ptr(), lR.data_ptr(),
                  L, B, up, down, half, taps.data_ptr(), gains.data_ptr(), fr.data_ptr(), T, 0.0, out.data_ptr(),
                  stream)

    def both():
        gain()
        mix()

    legs = {"resample_poly": plain, "band_gain": gain, "resample_mix": mix, "band_gain+resample_mix": both}
    us = {k: [] for k in legs}
    for _ in range(3):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    for _ in range(runs):  # A B A B
        for k, f in legs.items():
            us[k].append(timed(f, reps))
    nb = {"resample_poly": 4 * (x.numel() + out.numel()),
          "band_gain": 4 * (x.numel() + u.numel() + gains.numel()) + 2 * 8 * energies.numel(),
          "resample_mix": 4 * (x.numel() + u.numel() + y.numel() + out.numel() + gains.numel())}
    nb["band_gain+resample_mix"] = nb["band_gain"] + nb["resample_mix"]
    res = {}
    for k in legs:
        s = spread(us[k])
        res[k] = {"us_per_launch": s, "bytes_moved": nb[k], "gb_per_s_at_median": nb[k] / s["median"] * 1e-3}
    res["launches_per_timing"] = reps
    res["frames"] = T
    res["added_us_at_median"] = (res["band_gain+resample_mix"]["us_per_launch"]["median"]
                                 - res["resample_poly"]["us_per_launch"]["median"])
    return res


def timed_call(model, ys, seeds, N, rates, highband):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.enhance_batch(ys, seeds=seeds, batch_size=len(ys), N=N, sample_rates=rates, output_rate="input",
                              highband=highband)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", type=str, default="fp16")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "highband_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("highband_bench: needs a HIP device; nothing is measured without one")
    from eval_batch_bench import formula_model
    dev = torch.device("cuda", 0)
    model, _ = formula_model("bbed", "false", a.dtype)
    seeds = list(range(1000, 1000 + a.rows))
    res = {"rows": a.rows, "seconds": a.seconds, "N": a.N, "dtype": a.dtype, "device": torch.cuda.get_device_name(0),
           "rates": {}}
    for sr in (48000, 44100):
        L = int(round(a.seconds * sr))
        ys = clips(a.rows, L, sr, sr)
        entry = {"samples_in": L, "kernels": kernel_legs(torch.from_numpy(np.stack(ys)).to(dev), sr, a.runs, a.reps)}
        print(json.dumps({sr: entry}), flush=True)
        rates = [sr] * a.rows
        for _ in range(a.warmup):
            for hb in ("drop", "follow"):
                timed_call(model, ys, seeds, a.N, rates, hb)
        td, tf = [], []
        for _ in range(a.rounds):
            td.append(timed_call(model, ys, seeds, a.N, rates, "drop")[0])
            t, out = timed_call(model, ys, seeds, a.N, rates, "follow")
            tf.append(t)
        assert all(len(h) == L and np.isfinite(h).all() for h in out)
        sd, sf = spread(td), spread(tf)
        over = sf["median"] / sd["median"] - 1.0
        spread_d = (sd["max"] - sd["min"]) / sd["median"]
        entry["call"] = {"drop_s": sd, "follow_s": sf, "order": "drop, follow, alternated",
                         "warmup_calls_per_leg": a.warmup,
                         "overhead_s_at_median": sf["median"] - sd["median"], "overhead_fraction_at_median": over,
                         "drop_spread_fraction": spread_d, "bar": "follow <= 1.01 x drop, on top of the spread of the "
                         "drop runs", "within_bar": bool(over <= 0.01 + spread_d)}
        print(json.dumps({sr: entry["call"]}), flush=True)
        res["rates"][str(sr)] = entry
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
