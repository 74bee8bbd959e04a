"""Cost of the long-recording window layer: a 10-minute recording through ScoreModel.enhance_batch(window_frames=512,
overlap_frames=64) against the same windows given to the unwindowed enhance_batch as a list of separate utterances.

The recording is synthetic (a harmonic tone plus noise), at 16 kHz and the same at 48 kHz (resampled on the device
first); the routes are the fp16 one-step SNR-aligned model (C4; formula SNR estimator) and the fp16 'bbed' PC
sampler with N = 30.  Formula weights.  For each (rate, route):
  windowed   enhance_batch([y], sample_rates=[rate], window_frames=512, overlap_frames=64, batch_size=32): one
             upload, one gather, the windows in batches of 32, one merge, one download.
  list       enhance_batch(windows, seeds=window seeds, batch_size=32) with window_frames=None -- the code path of
             the commit before the window layer, which it leaves untouched -- on the windows of the 16 kHz signal cut
             on the host: what a caller had to do by hand, without the cross-fade (and for 48 kHz without the
             resampling, which only the windowed call pays here).
Host clock around each call (both end in the download of their results), alternated A B A B after one warm-up
call each.  The bar: windowed <= 1.01 x list on top of the spread between the list runs.  Also the
device time of the gather and of the merge at the recording's shapes, between device events.
Writes profiles/longform_bench.json.

    python tools/longform_bench.py [--minutes 10] [--rounds 2] [--N 30] [--out profiles/longform_bench.json]
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

WF, OF, BATCH = 512, 64, 32


def recording(L, sr, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / float(sr)
    x = sum(0.2 / h * np.sin(2 * np.pi * 180.0 * h * t * (1.0 + 0.02 * np.sin(2 * np.pi * 0.3 * t))) for h in (1, 2, 3))
    return (x * (0.6 + 0.4 * np.sin(2 * np.pi * 0.11 * t)) + 0.05 * rng.standard_normal(L)).astype(np.float32)


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": v[0], "max": v[-1], "n": len(v)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def device_us(fn, reps=10, repeats=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / reps)
    return spread(us)


def kernel_timing(L16, dev):
    """Gather and merge alone at the recording's shapes (the windows' contents do not matter to either)."""
    from snrse import longform, ops
    plan = longform.Plan([L16], WF, OF)
    src = torch.randn(1, L16, device=dev)
    table = torch.from_numpy(plan.table).to(dev)
    ln = torch.tensor([L16], dtype=torch.int32, device=dev)
    wins = ops.window_gather(src, ln, table, plan.W)
    st = torch.tensor(plan.starts, dtype=torch.int32, device=dev)
    fs = torch.tensor(plan.first, dtype=torch.int32, device=dev)
    sl = torch.zeros(len(plan), dtype=torch.uint8, device=dev)
    g = device_us(lambda: ops.window_gather(src, ln, table, plan.W))
    m = device_us(lambda: ops.window_merge(wins, st, fs, ln, plan.V, silent=sl, stride_out=L16))
    gb, mb = 4 * 2 * wins.numel(), 4 * (L16 + wins.numel())
    return {"windows": len(plan), "gather_us": g, "merge_us": m, "gather_bytes": gb, "merge_bytes_upper": mb,
            "gather_gb_per_s_at_median": gb / g["median"] * 1e-3, "merge_gb_per_s_at_median": mb / m["median"] * 1e-3,
            "note": "launches include the output allocation of ops.window_gather / ops.window_merge"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--dtype", type=str, default="fp16")
    ap.add_argument("--routes", type=str, default="c4,pc")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "longform_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("longform_bench: needs a HIP device; nothing is measured without one")
    import sgmse.model as sm
    from eval_batch_bench import formula_model, formula_snr_estimator
    from snrse import audio, longform, resample
    dev = torch.device("cuda", 0)
    models = {}
    if "c4" in a.routes:
        models["c4"], keys = formula_model("sebridge_v3", "true", a.dtype, fixed_snr=0.17783)
        sm.set_snr_model(formula_snr_estimator(keys))
    if "pc" in a.routes:
        models["pc"], _ = formula_model("bbed", "false", a.dtype)
    res = {"minutes": a.minutes, "N": a.N, "dtype": a.dtype, "window_frames": WF, "overlap_frames": OF,
           "batch_size": BATCH, "device": torch.cuda.get_device_name(0), "order": "list, windowed, alternated",
           "bar": "windowed <= 1.01 x list, on top of the spread of the list runs", "runs": {}}
    for sr in (16000, 48000):
        L = int(round(a.minutes * 60 * sr))
        y = recording(L, sr, sr)
        y16 = np.asarray(resample.convert([y], sr, audio.MODEL_RATE)[0], np.float32)
        plan = longform.Plan([len(y16)], WF, OF)
        windows = [y16[s:s + n].copy() for s, n in zip(plan.starts, plan.win_lengths)]
        wseeds = plan.seeds([4242])
        seconds = L / float(sr)
        if sr == 16000:
            res["kernels"] = kernel_timing(len(y16), dev)
            print(json.dumps({"kernels": res["kernels"]}), flush=True)
        for route, model in models.items():
            kw = dict(N=a.N) if route == "pc" else {}

            def run_list():
                return model.enhance_batch(windows, seeds=wseeds, batch_size=BATCH, **kw)

            def run_win():
                return model.enhance_batch([y], seeds=[4242], batch_size=BATCH, sample_rates=[sr], window_frames=WF,
                                           overlap_frames=OF, **kw)

            timed(run_list)
            timed(run_win)
            tl, tw = [], []
            for _ in range(a.rounds):
                tl.append(timed(run_list)[0])
                t, out = timed(run_win)
                tw.append(t)
            assert len(out) == 1 and len(out[0]) == len(y16) and np.isfinite(out[0]).all()
            sl, sw = spread(tl), spread(tw)
            over = sw["median"] / sl["median"] - 1.0
            spr = (sl["max"] - sl["min"]) / sl["median"]
            entry = {"samples_in": L, "samples_16k": len(y16), "windows": len(plan), "list_s": sl, "windowed_s": sw,
                     "real_time_factor_windowed": sw["median"] / seconds,
                     "windows_per_second_windowed": len(plan) / sw["median"],
                     "overhead_fraction_at_median": over, "list_spread_fraction": spr,
                     "within_bar": bool(over <= 0.01 + spr)}
            print(json.dumps({f"{sr}/{route}": entry}), flush=True)
            res["runs"][f"{sr}/{route}"] = entry
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
