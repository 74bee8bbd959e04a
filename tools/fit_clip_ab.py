"""Cost of the device-side gradient clip on the `bench.py --config train` step.

One process, one model (run_train's: sebridge_v3 'true', formula weights, B x [256, T] synthetic pairs, fp32):
the training step with the default optimizer launch (arm `default`: the launches of the tree without the clip,
whose Adam kernel has the same instructions) and with clip_grad_norm = 1.0 (arm `clip`: + snrse_grad_sumsq,
snrse_grad_clip_coef, the scaled Adam launch), alternated default / clip ROUNDS times; then the optimizer step
alone on the gradients the last step left, both arms, timed with device events.  Prints JSON lines
(profiles/fit_clip_ab.jsonl): the runs, the medians, the default arm's own run-to-run spread, and the extra
optimizer time against one read of every gradient.

    python tools/fit_clip_ab.py [--batch 8 --frames 256 --steps 4 --warmup 1 --rounds 3 --out FILE]
    python tools/fit_clip_ab.py --tree OTHER_CHECKOUT --only default   # one run of one arm on another (built) tree:
                                                                       # alternate such processes for a tree-vs-tree A/B
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:  # before the package imports: they come from that tree
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
for p in (ROOT, os.path.join(ROOT, "snr-aligned_diffse_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--opt-iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--tree", type=str, default=None, help="run on this checkout (built) instead of the tool's own")
    ap.add_argument("--only", choices=["default", "clip"], default=None, help="one run of one arm, one line")
    ap.add_argument("--tag", type=str, default=None)
    a = ap.parse_args()
    from sgmse.model import ScoreModel
    from snrse import formula
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        shapes = {k: tuple(s) for k, s in json.load(f)["ncsnpp"]}
    m = ScoreModel(backbone="ncsnpp", sde="ouve", model_type="sebridge_v3", snr_conditioned="true", theta=1.5,
                   sigma_min=0.05, sigma_max=0.5, N=30, compute_dtype="fp32", fixed_snr=0.17783, loss_type="mse")
    m.dnn.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(shapes).items()})
    m = m.cuda().train()
    opt = m.configure_optimizers()
    B, T = a.batch, a.frames
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, 1, 256, T, dtype=torch.complex64, device=dev, generator=g) * 0.4
    y = x + torch.randn(B, 1, 256, T, dtype=torch.complex64, device=dev, generator=g) * 0.4
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def step(i):
        loss = m.training_step((x, y), i)
        loss.backward()
        m.optimizer_step(opt)
        opt.zero_grad(set_to_none=False)

    def run(clip, tag):
        opt.clip_grad_norm = clip
        for w in range(a.warmup):
            step(w)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(a.steps):
            step(a.warmup + k)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        emit({"run": tag, "arm": "clip 1.0" if clip else "default", "ms_per_step": round(ms, 3),
              "samples_per_s": round(B / ms * 1e3, 3), "steps": a.steps, "warmup": a.warmup})
        return ms

    step(0)  # first-use allocations and the chunk tables, outside every timed run
    if a.only:
        run(1.0 if a.only == "clip" else None, a.tag or a.only)
        lines[-1]["tree"] = ROOT
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(lines[-1]) + "\n")
        return
    res = {"default": [], "clip": []}
    for r in range(1, a.rounds + 1):
        res["default"].append(run(None, f"default{r}"))
        res["clip"].append(run(1.0, f"clip{r}"))
    md, mc = statistics.median(res["default"]), statistics.median(res["clip"])
    spread = (max(res["default"]) - min(res["default"])) / md
    # the optimizer step alone, on the gradients the last step left (zero_grad(set_to_none=False) keeps them)
    gbytes = sum(p.grad.numel() * 4 for p in m.parameters() if p.grad is not None)
    opt_ms = {}
    for tag, clip in (("default", None), ("clip", 1.0), ("default_again", None), ("clip_again", 1.0)):
        opt.clip_grad_norm = clip
        m.optimizer_step(opt)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.opt_iters):
            m.optimizer_step(opt)
        e1.record()
        torch.cuda.synchronize()
        opt_ms[tag] = e0.elapsed_time(e1) / a.opt_iters
    extra = statistics.mean([opt_ms["clip"], opt_ms["clip_again"]]) - statistics.mean(
        [opt_ms["default"], opt_ms["default_again"]])
    # the two added launches alone: the last clipped step's calls replayed back to back (its buffers are alive in
    # the optimizer), so the events bracket device time, not the host's table building
    from snrse import train as strain
    seen, real_call = {}, strain._call

    def spy(name, *args):
        seen[name] = args
        real_call(name, *args)

    strain._call = spy
    try:
        opt.clip_grad_norm = 1.0
        m.optimizer_step(opt)
    finally:
        strain._call = real_call
    kern_us = {}
    for name in ("snrse_grad_sumsq", "snrse_grad_clip_coef"):
        real_call(name, *seen[name])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            real_call(name, *seen[name])
        e1.record()
        torch.cuda.synchronize()
        kern_us[name] = e0.elapsed_time(e1) / 50 * 1e3
    emit({"kernels_us": {k: round(v, 2) for k, v in kern_us.items()}, "gradient_bytes": gbytes,
          "grad_sumsq_read_TBps": round(gbytes / (kern_us["snrse_grad_sumsq"] * 1e-6) / 1e12, 3),
          "chunks": int(seen["snrse_grad_sumsq"][3])})
    emit({"summary": f"training step B={B} x [256, {T}], default / clip alternated {a.rounds} times on one device",
          "median_ms_default": round(md, 3), "median_ms_clip": round(mc, 3),
          "clip_over_default_pct": round((mc / md - 1) * 100, 3), "default_spread_pct": round(spread * 100, 3),
          "optimizer_step_ms": {k: round(v, 4) for k, v in opt_ms.items()},
          "optimizer_extra_ms": round(extra, 4), "gradient_bytes": gbytes,
          "extra_as_gradient_read_TBps": round(gbytes / (extra * 1e-3) / 1e12, 3) if extra > 0 else None,
          "extra_pct_of_step": round(extra / md * 100, 4)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
