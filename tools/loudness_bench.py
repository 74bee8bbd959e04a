"""What the loudness layer costs on the device.

  kernels   ops.loudness, ops.peak_oversampled and ops.gain_to_pcm16, each between device events, `--reps` timed runs
            after `--warmup` untimed ones, the data already on the device: (a) the noisy signals of the 64 clips of
            tools/eval_batch_bench.py (1-6 s at 16 kHz) as one ragged batch, every row a file; (b) one pair of rows of
            `--minutes` (30) minutes at 48 kHz measured as one stereo file.
  host      tests/loudness_ref.py (fp64, scipy.signal.lfilter) on the same data, one row after the other on the CPU:
            the only CPU implementation at hand.
  folder    snrse.enhance_files with the fp16 one-step SNR-aligned model (formula weights) on the 64 clips written
            as 16-bit files, without (A) and with (B) --loudness -23, alternated A B A B in one process, `--rounds`
            of each, host clock around each run, the code as it ships.  Then, in `--rounds` further B runs that
            are not part of that comparison, the host time spent in the loudness stage of each file
            (enhance_files.level_file: the second upload of the enhanced channels, the noisy file's upload, the
            launches, two read-backs) is summed between a device synchronise before and the stage's own last
            read-back, to set against the kernels' device time for the same 64 signals.

Writes profiles/loudness_bench.json.

    python tools/loudness_bench.py [--reps 20] [--warmup 3] [--rounds 3] [--minutes 30] [--no-folder] [--no-host]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snr-aligned_diffse_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(v, nd=4):
    v = sorted(v)
    return {"median": round(float(np.median(v)), nd), "min": round(v[0], nd), "max": round(v[-1], nd), "n": len(v)}


def device_ms(fn, args):
    ms = []
    for r in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    return stats(ms)


def bench_kernels(buf, lens, rate, groups, args):
    from snrse import ops
    gain = torch.full((buf.shape[0],), 0.5, device=buf.device, dtype=torch.float64)
    n = int(sum(lens))
    out = {"rows": int(buf.shape[0]), "samples": n,
           "loudness_ms": device_ms(lambda: ops.loudness(buf, lengths=lens, rate=rate, groups=groups), args),
           "peak_oversampled_ms": device_ms(lambda: ops.peak_oversampled(buf, lengths=lens), args),
           "gain_to_pcm16_ms": device_ms(lambda: ops.gain_to_pcm16(buf, gain, lengths=lens), args)}
    # the two passes over the samples read them once each; the states and partials add 48 B per 64-sample chunk
    out["loudness_gb_per_s_of_sample_reads_at_median"] = round(2 * 4 * n / out["loudness_ms"]["median"] * 1e-6, 1)
    out["loudness_samples_per_us_at_median"] = round(n / out["loudness_ms"]["median"] * 1e-3, 1)
    return out


def host_reference(rows, rate, groups):
    import loudness_ref as ref
    t0 = time.perf_counter()
    files = {}
    for x, g in zip(rows, groups):
        files.setdefault(g, []).append(x)
    vals = [ref.integrated(ch, rate)["lufs"] for _, ch in sorted(files.items())]
    return round(time.perf_counter() - t0, 3), vals


def bench_folder(data, args):
    import eval_batch_bench as ebb
    from sgmse.model import set_snr_model
    from snrse import audio, enhance_files
    m, keys = ebb.formula_model("sebridge_v3", "true", "fp16", fixed_snr=0.17783)
    set_snr_model(ebb.formula_snr_estimator(keys))
    stage = {"s": 0.0}
    inner = enhance_files.level_file

    def timed_level(*a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(*a, **kw)
        stage["s"] += time.perf_counter() - t0
        return r

    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        noisy = os.path.join(tmp, "noisy")
        os.makedirs(noisy)
        for k, (_, y) in enumerate(data):
            audio.write_wav(os.path.join(noisy, f"clip{k:03d}.wav"), y / max(1.0, float(np.abs(y).max()) / 0.99), 16000)

        def run(flag):
            torch.manual_seed(7)
            stage["s"] = 0.0
            return ebb.timed(lambda: enhance_files.enhance_files(
                m, noisy, os.path.join(tmp, "out_b" if flag else "out_a"), batch_size=32,
                loudness="-23" if flag else "off"))[0]

        for flag in (False, True):  # warm-up: both variants, every batch shape of the timed runs
            run(flag)
        a, b, st = [], [], []
        for _ in range(args.rounds):  # A B A B ...
            a.append(run(False))
            b.append(run(True))
            print(f"enhance_files: {a[-1]:.3f} s, with --loudness -23 {b[-1]:.3f} s", flush=True)
        enhance_files.level_file = timed_level  # the stage's share, in runs of their own: the wrapper synchronises
        try:
            for _ in range(args.rounds):
                run(True)
                st.append(stage["s"])
        finally:
            enhance_files.level_file = inner
        print(f"loudness stage, host: {st}", flush=True)
        with open(os.path.join(tmp, "out_b", "_enhanced.csv")) as f:
            rows = [r.split(",") for r in f.read().strip().split("\n")[1:]]
        res["limited_files"] = sum(r[-1] == "1" for r in rows)
    res.update(off_s=stats(a), loudness_s=stats(b), loudness_stage_host_s=stats(st),
               loudness_share_of_run=round(1.0 - float(np.median(a)) / float(np.median(b)), 4),
               difference_beyond_spread=bool(min(b) > max(a)), files=len(data))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--minutes", type=float, default=30.0)
    ap.add_argument("--no-folder", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("loudness_bench: needs a HIP device; nothing is measured without one")
    import eval_batch_bench as ebb
    from snrse import batching, ops
    dev = torch.device("cuda", 0)
    data = ebb.clips(args.clips)
    noisy = [y for _, y in data]
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "kweight_geometry": dict(zip(("chunk", "block", "group"), ops.kweight_geometry())),
           "launches": {"loudness": 7, "peak_oversampled": 1, "gain_to_pcm16": 1}}
    buf, lens = batching.pack_rows(noisy)
    out["clips"] = bench_kernels(buf.to(dev), lens, 16000, None, args)
    out["clips"]["seconds_total"] = round(sum(lens) / 16000.0, 2)
    print(json.dumps({"clips": out["clips"]}), flush=True)
    L = int(round(args.minutes * 60 * 48000))
    g = torch.Generator(device=dev).manual_seed(3)
    pair = torch.randn(2, L, device=dev, generator=g) * 0.1
    pair *= 0.6 + 0.4 * torch.sin(torch.arange(L, device=dev) * (2 * np.pi * 0.05 / 48000.0))  # a level that moves
    out["long_pair"] = bench_kernels(pair, [L, L], 48000, [0, 0], args)
    out["long_pair"]["minutes"] = args.minutes
    lufs_dev = float(ops.loudness(pair, rate=48000, groups=[0, 0])[0])
    out["long_pair"]["lufs"] = lufs_dev
    print(json.dumps({"long_pair": out["long_pair"]}), flush=True)
    if not args.no_host:
        t, vals = host_reference(noisy, 16000, list(range(len(noisy))))
        dv = ops.loudness(buf.to(dev), lengths=lens, rate=16000).cpu().numpy()
        out["host_reference_s_clips"] = t
        out["clips"]["worst_difference_from_host_lu"] = float(np.max(np.abs(dv - np.array(vals))))
        ph = pair.cpu().numpy()
        t, vals = host_reference([ph[0], ph[1]], 48000, [0, 0])
        out["host_reference_s_long_pair"] = t
        out["long_pair"]["difference_from_host_lu"] = abs(lufs_dev - vals[0])
        out["host_reference"] = "tests/loudness_ref.py, fp64 scipy.signal.lfilter, one process"
        del ph
    del pair
    if not args.no_folder:
        out["folder_one_step"] = bench_folder(data, args)
        k = out["clips"]
        out["folder_one_step"]["kernels_device_ms_same_signals"] = round(
            k["loudness_ms"]["median"] + k["peak_oversampled_ms"]["median"] + k["gain_to_pcm16_ms"]["median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
