"""Evaluation throughput on a set of clips of different lengths: the per-file loop against ragged batches.

A fixed seeded set of 64 synthetic clips with lengths uniform in 1-6 s is enhanced and scored (SI-SDR / SI-SIR /
SI-SAR; no file I/O, no PESQ) two ways, alternated A B A B in one process on one device:
  A  the per-file loop of snrse.evaluate (ScoreModel.enhance + score_files, B = 1 per call);
  B  batch_size = 32: snrse.batching.plan_batches, ScoreModel.enhance_batch and one ragged energy-ratio launch
     per batch (snrse.evaluate.score_batch).
Models (formula weights): the fp16 PC sampler at N = 30 (`bbed`) and the fp16 SNR-aligned one-step model
(`sebridge_v3`, SNRNet estimate).  Writes both times, the speed-up, the plan's batch-size histogram and the
largest per-file difference between the two modes' waveforms to profiles/eval_batch.json.

`--models ode` is the probability-flow ODE leg (fp16 `bbed`, rtol = atol = 1e-3): the per-file enhance() loop against
enhance_batch's per-row adaptive RK45, three runs each, interleaved; files/s of both with their spread, the batch
utilisation row_evals / (evals x B) and the per-file nfev range go to profiles/eval_batch_ode.json.

    python tools/eval_batch_bench.py [--clips 64] [--batch-size 32] [--N 30] [--rounds 2] [--out profiles/eval_batch.json]
    python tools/eval_batch_bench.py --models ode [--ode-tol 1e-3] [--ode-rounds 3] [--ode-out profiles/eval_batch_ode.json]
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snr-aligned_diffse_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def clips(n, seed=20240):
    """n (clean, noisy) pairs, lengths uniform in [1 s, 6 s] at 16 kHz, input SNR uniform in 0-20 dB."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = int(rng.integers(16000, 6 * 16000 + 1))
        t = np.arange(L) / 16000.0
        x = 0.2 * np.sin(2 * np.pi * rng.uniform(150.0, 900.0) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
        nz = rng.standard_normal(L)
        nz *= np.sqrt(np.mean(x ** 2) / np.mean(nz ** 2)) * 10 ** (-rng.uniform(0.0, 20.0) / 20)
        out.append((x.astype(np.float32), (x + nz).astype(np.float32)))
    return out


def formula_model(model_type, snr_conditioned, dtype, **kw):
    from sgmse.model import ScoreModel
    from snrse import formula
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        keys = json.load(f)
    hp = dict(backbone="ncsnpp", sde="ouve", model_type=model_type, snr_conditioned=snr_conditioned, theta=1.5,
              sigma_min=0.05, sigma_max=0.5, N=30, compute_dtype=dtype)
    hp.update(kw)
    m = ScoreModel(**hp)
    sd = formula.formula_state_dict({k: tuple(s) for k, s in keys["ncsnpp"]})
    m.dnn.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.cuda().eval(), keys


def formula_snr_estimator(keys):
    from sgmse.backbones import SNRNet
    from snrse import formula
    sd = formula.formula_state_dict({"snrnet." + k: tuple(s) for k, s in keys["snrnet"]})
    net = SNRNet()
    net.load_state_dict({k[len("snrnet."):]: torch.from_numpy(v) for k, v in sd.items()})

    class Est:
        def estimate_from_spec(self, spec):
            g = net.forward_complex(spec)[:, 0]
            return g / (1 - g)

    return Est()


def run_loop(model, data, kw):
    from snrse import evaluate
    outs, rows = [], []
    for x, y in data:
        yt = torch.from_numpy(y)[None]
        h = model.enhance(yt, yt, **kw)
        rows.append(evaluate.score_files(np.asarray(h, np.float32), x, y))
        outs.append(h)
    return outs, rows


def run_batched(model, data, kw, batch_size, max_frames):
    from snrse import batching, evaluate
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in data]
    plan = batching.plan_batches([len(y) for _, y in data], batch_size, max_frames)
    outs, rows = [None] * len(data), [None] * len(data)
    for b in plan:
        hs = model.enhance_batch([data[i][1] for i in b], seeds=[seeds[i] for i in b], batch_size=len(b),
                                 max_frames=max_frames, **kw)
        er, _ = evaluate.score_batch(hs, [data[i][0] for i in b], [data[i][1] for i in b])
        for r, i in enumerate(b):
            outs[i], rows[i] = hs[r], [float("nan"), *map(float, er[r])]
    return outs, rows, plan


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def bench_model(name, model, data, kw, args):
    res = {"model": name, "loop_s": [], "batched_s": []}
    warm = data[:2]
    torch.manual_seed(1)
    run_loop(model, warm, kw)
    run_batched(model, warm, kw, args.batch_size, args.max_frames)
    lo = bo = plan = None
    for _ in range(args.rounds):  # A B A B
        torch.manual_seed(7)
        t, (lo, lrows) = timed(lambda: run_loop(model, data, kw))
        res["loop_s"].append(round(t, 3))
        torch.manual_seed(7)
        t, (bo, brows, plan) = timed(lambda: run_batched(model, data, kw, args.batch_size, args.max_frames))
        res["batched_s"].append(round(t, 3))
        print(f"{name}: loop {res['loop_s'][-1]} s, batch_size {args.batch_size} {res['batched_s'][-1]} s", flush=True)
    n = len(data)
    res["loop_files_per_s"] = round(n / min(res["loop_s"]), 2)
    res["batched_files_per_s"] = round(n / min(res["batched_s"]), 2)
    res["speedup"] = round(min(res["loop_s"]) / min(res["batched_s"]), 2)
    hist = collections.Counter(len(b) for b in plan)
    res["batches"] = len(plan)
    res["batch_size_histogram"] = {str(k): hist[k] for k in sorted(hist)}
    res["max_rel_rms_batched_vs_loop"] = max(rel(bo[i], lo[i]) for i in range(n))
    res["max_si_sdr_abs_diff_db"] = max(abs(brows[i][1] - lrows[i][1]) for i in range(n))
    res["range_guard"] = {k: (v if isinstance(v, (list, bool, int)) else str(v)) for k, v in (model.last_guard or {}).items()}
    return res


def bench_ode(model, data, args):
    """The ODE leg: the per-file enhance(sampler_type="ode") loop (the path before the batched route, untouched by
    it) against enhance_batch's per-row RK45 at --batch-size, --ode-rounds runs each, interleaved A B A B A B.  The
    two legs draw different priors (torch's generator / per-file Philox seeds), so only throughput is compared."""
    kw = dict(sampler_type="ode", rtol=args.ode_tol, atol=args.ode_tol)
    n = len(data)
    res = {"model": "ode_rk45", "rtol": args.ode_tol, "atol": args.ode_tol, "loop_s": [], "batched_s": []}
    torch.manual_seed(1)
    run_loop(model, data[:2], kw)
    run_batched(model, data[:2], kw, args.batch_size, args.max_frames)
    stats = plan = None
    for _ in range(args.ode_rounds):
        torch.manual_seed(7)
        t, _r = timed(lambda: run_loop(model, data, kw))
        res["loop_s"].append(round(t, 3))
        print(f"ode: loop {res['loop_s'][-1]} s", flush=True)
        torch.manual_seed(7)
        stats = []

        def batched():
            # enhance_batch is called once per planned batch: collect each call's solver statistics
            from snrse import batching, evaluate
            seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in data]
            pl = batching.plan_batches([len(y) for _, y in data], args.batch_size, args.max_frames)
            for b in pl:
                hs = model.enhance_batch([data[i][1] for i in b], seeds=[seeds[i] for i in b], batch_size=len(b),
                                         max_frames=args.max_frames, **kw)
                evaluate.score_batch(hs, [data[i][0] for i in b], [data[i][1] for i in b])
                stats.extend(model.last_ode_stats)
            return pl

        t, plan = timed(batched)
        res["batched_s"].append(round(t, 3))
        print(f"ode: batch_size {args.batch_size} {res['batched_s'][-1]} s", flush=True)
    lf = [n / t for t in res["loop_s"]]
    bf = [n / t for t in res["batched_s"]]
    res["loop_files_per_s"] = [round(v, 3) for v in lf]
    res["batched_files_per_s"] = [round(v, 3) for v in bf]
    res["loop_spread_files_per_s"] = round(max(lf) - min(lf), 3)
    res["batched_spread_files_per_s"] = round(max(bf) - min(bf), 3)
    res["speedup_median"] = round(float(np.median(bf) / np.median(lf)), 2)
    res["batched_faster_beyond_spread"] = bool(min(bf) - max(lf) > max(max(lf) - min(lf), max(bf) - min(bf)))
    nfev = [v for s in stats for v in s["nfev"]]
    res["nfev_min"], res["nfev_max"], res["nfev_mean"] = min(nfev), max(nfev), round(float(np.mean(nfev)), 1)
    res["utilisation"] = round(sum(s["row_evals"] for s in stats) / sum(s["evals"] * len(s["files"]) for s in stats), 3)
    hist = collections.Counter(len(b) for b in plan)
    res["batches"] = len(plan)
    res["batch_size_histogram"] = {str(k): hist[k] for k in sorted(hist)}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--max-frames", type=int, default=16384)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--models", default="pc,snr", help="comma list of pc, snr, ode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_batch.json"))
    ap.add_argument("--ode-tol", type=float, default=1e-3, help="rtol = atol of the ODE leg")
    ap.add_argument("--ode-rounds", type=int, default=3)
    ap.add_argument("--ode-out", default=os.path.join(ROOT, "profiles", "eval_batch_ode.json"))
    args = ap.parse_args(argv)
    from sgmse.model import set_snr_model
    data = clips(args.clips)
    secs = [len(y) / 16000.0 for _, y in data]
    out = {"clips": args.clips, "seconds_total": round(sum(secs), 2), "seconds_min": round(min(secs), 2),
           "seconds_max": round(max(secs), 2), "batch_size": args.batch_size, "max_frames": args.max_frames,
           "dtype": args.dtype, "device": torch.cuda.get_device_name(0), "results": []}
    if "pc" in args.models.split(","):
        m, _ = formula_model("bbed", "false", args.dtype)
        out["results"].append(bench_model(f"pc_N{args.N}", m, data, dict(sampler_type="pc", N=args.N), args))
        del m
    if "snr" in args.models.split(","):
        m, keys = formula_model("sebridge_v3", "true", args.dtype, fixed_snr=0.17783)
        set_snr_model(formula_snr_estimator(keys))
        out["results"].append(bench_model("snr_aligned_one_step", m, data, dict(sampler_type="pc", N=args.N), args))
    if "ode" in args.models.split(","):
        m, _ = formula_model("bbed", "false", args.dtype)
        ode = dict({k: v for k, v in out.items() if k != "results"}, results=[bench_ode(m, data, args)])
        os.makedirs(os.path.dirname(os.path.abspath(args.ode_out)), exist_ok=True)
        with open(args.ode_out, "w") as f:
            json.dump(ode, f, indent=1)
            f.write("\n")
        print(json.dumps(ode))
        del m
    if not out["results"]:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
