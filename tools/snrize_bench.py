"""What the fixed-SNR dataset preparation costs, on `--clips` synthetic pairs of 2-6 s at 16 kHz (seeded; the noise
has silent and 60-dB-down windows) written as 16-bit PCM into a temporary folder.

  host      tests/snrize_ref.py (float64 numpy, vectorised: a generous baseline, not a quadratic Python loop) over
            the folder, one file after the other: read both files, remix, write the three outputs and active_rms.txt.
  device    snrse.snrize.remix_files on the same folder: the whole tool, file I/O included.
            host and device are alternated A B A B ... in one process, `--rounds` of each, after one untimed run of
            each.
  kernels   the four launches alone on the batches already resident on the device (batch_size 32), between device
            events, `--reps` timed passes over all batches after `--warmup` untimed ones: the analysis (two launches),
            the mix, the PCM pass, each with the bytes it moves by the model below, and a plain device copy of the
            same buffers timed in the same run.

Byte model (S = valid samples of all rows, P = B x stride elements of all batches; the elementwise kernels write their
whole rows, zeros past each length): analysis reads 8 S; mix reads 8 S and writes 8 P; PCM reads 12 S and writes 6 P;
copy reads 4 P and writes 4 P.  A batch is about 12 MB per signal, so all of this runs out of the Infinity Cache as
much as out of HBM: the copy's rate is the yardstick, not the HBM peak.

Writes profiles/snrize_bench.json.

    python tools/snrize_bench.py [--clips 512] [--batch-size 32] [--rounds 2] [--reps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snr-aligned_diffse_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(v, nd=4):
    v = sorted(v)
    return {"median": round(float(np.median(v)), nd), "min": round(v[0], nd), "max": round(v[-1], nd), "n": len(v)}


def make_corpus(root, clips):
    """-> [(name, samples)]; root/in/{clean,noise}/<name> as 16-bit PCM."""
    import snrize_ref as R
    from snrse import audio
    rng = np.random.default_rng(2024)
    lens = rng.integers(2 * 16000, 6 * 16000 + 1, clips)
    for sub in ("clean", "noise"):
        os.makedirs(os.path.join(root, "in", sub), exist_ok=True)

    def one(i):
        c, n = R.synth_pair(int(lens[i]), 1000 + i)
        cq, nq = R.quantise_pair(c, n)
        name = f"clip_{i:04d}.wav"
        audio.write_wav(os.path.join(root, "in", "clean", name), cq, 16000, bits=16)
        audio.write_wav(os.path.join(root, "in", "noise", name), nq, 16000, bits=16)
        return name, int(lens[i])

    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(one, range(clips)))


def host_leg(root, files, out):
    import snrize_ref as R
    from snrse import audio, snrize
    for sub in ("clean", "noise", "noisy"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    lines = []
    for name, _ in files:
        c = audio.read_wav(os.path.join(root, "in", "clean", name))[0][:, 0]
        n = audio.read_wav(os.path.join(root, "in", "noise", name))[0][:, 0]
        c1, n1, y, info = R.remix(c, n, 16000, -5.0)
        for sub, x in (("clean", c1), ("noise", n1), ("noisy", y)):
            audio.write_wav(os.path.join(out, sub, name), R.to_pcm16(x), 16000, bits=16)
        s = info["clip_scale"]
        lines.append(snrize.rms_line(name, info["clean_rms"] * s, info["noise_rms"] * info["gain"] * s))
    with open(os.path.join(out, "active_rms.txt"), "w") as f:
        f.writelines(lines)


def device_leg(root, out, batch_size):
    from snrse import snrize
    snrize.remix_files(os.path.join(root, "in", "clean"), out, noise_dir=os.path.join(root, "in", "noise"),
                       snr_db=-5.0, batch_size=batch_size)
    torch.cuda.synchronize()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def bench_kernels(root, files, args, dev):
    from snrse import audio, ops
    from snrse.batching import pack_rows
    batches = []
    for b0 in range(0, len(files), args.batch_size):
        part = files[b0:b0 + args.batch_size]
        c, lens = pack_rows([audio.read_wav(os.path.join(root, "in", "clean", k))[0][:, 0] for k, _ in part])
        n, _ = pack_rows([audio.read_wav(os.path.join(root, "in", "noise", k))[0][:, 0] for k, _ in part])
        c, n = c.to(dev), n.to(dev)
        ln = ops.as_lengths(lens, c.shape[0], c.shape[1], dev)
        fin, _ = ops._active_analysis(c, n, ln, 1600, -5.0)
        n1, y, peak = ops.snr_mix(c, n, fin[:, 4], lengths=ln)
        batches.append(dict(c=c, n=n, ln=ln, gain=fin[:, 4].contiguous(), n1=n1, y=y, peak=peak,
                            dst=torch.empty_like(c)))
    S = int(sum(int(b["ln"].host.sum()) for b in batches))
    P = int(sum(b["c"].numel() for b in batches))
    legs = {
        "analysis": (lambda b: ops._active_analysis(b["c"], b["n"], b["ln"], 1600, -5.0), 8 * S),
        "mix": (lambda b: ops.snr_mix(b["c"], b["n"], b["gain"], lengths=b["ln"]), 8 * S + 8 * P),
        "pcm16": (lambda b: ops.scale_to_pcm16(b["c"], b["n1"], b["y"], b["peak"], lengths=b["ln"], floats=False),
                  12 * S + 6 * P),
        "remix_all_four": (lambda b: ops.snr_remix(b["c"], b["n"], lengths=b["ln"], fs=16000, pcm16=True),
                           8 * S + 8 * S + 8 * P + 12 * S + 6 * P),
        "device_copy": (lambda b: b["dst"].copy_(b["c"]), 8 * P),
    }
    ms = {k: [] for k in legs}
    for r in range(args.warmup + args.reps):  # the legs alternate inside every pass
        for k, (fn, _) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for b in batches:
                fn(b)
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    out = {"valid_samples": S, "row_elements": P, "batches": len(batches),
           "note": "ms per pass over all batches, launch overheads and output allocations included"}
    for k, (_, nbytes) in legs.items():
        st = stats(ms[k])
        out[k] = {"ms": st, "model_bytes": nbytes, "GB_per_s_at_median": round(nbytes / st["median"] / 1e6, 1),
                  "files_per_s_at_median": round(len(files) / st["median"] * 1e3, 1)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snrize_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("snrize_bench: needs the MI355X (no CPU timing stands in for it)")
    dev = torch.device("cuda", 0)
    root = tempfile.mkdtemp(prefix="snrize_bench_")
    try:
        files = make_corpus(root, args.clips)
        secs = sum(L for _, L in files) / 16000.0
        out = {"clips": args.clips, "seconds_total": round(secs, 1), "batch_size": args.batch_size,
               "device": torch.cuda.get_device_name(0), "order": "host, device, alternated, after one untimed run of each",
               "io": "16-bit PCM in a temporary folder; 2 files read and 3 written per pair in both legs"}
        k = [0]

        def fresh():
            k[0] += 1
            return os.path.join(root, f"out{k[0]}")

        host_leg(root, files, fresh())
        device_leg(root, fresh(), args.batch_size)
        a, b = [], []
        for _ in range(args.rounds):
            a.append(timed(lambda: host_leg(root, files, fresh())))
            b.append(timed(lambda: device_leg(root, fresh(), args.batch_size)))
            print(f"host {a[-1]:.3f} s, device pipeline {b[-1]:.3f} s", flush=True)
        out["host_reference_s"] = stats(a)
        out["device_pipeline_s"] = stats(b)
        out["host_files_per_s"] = round(args.clips / float(np.median(a)), 1)
        out["device_pipeline_files_per_s"] = round(args.clips / float(np.median(b)), 1)
        out["device_pipeline_faster_beyond_spread"] = bool(max(b) < min(a))
        out["kernels"] = bench_kernels(root, files, args, dev)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
