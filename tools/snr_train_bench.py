#!/usr/bin/env python3
"""ms per SNR-estimator training step (perturb + forward + backward + Adam / EMA) at B=8, T=256 on one GPU.

Two paths on the same device in the same run, alternated step by step after a warm-up, HIP events around each
step, median of --steps (>= 20) steps:
  hip    SNRModel._step -> loss.backward() -> optimizer_step (csrc/snrnet_train.hip + snrse_adam_ema)
  torch  what a user would otherwise run: torch-ROCm autograd over oracle.snrnet_ref.snrnet_forward (fp32),
         the perturbation as torch expressions, torch.optim.Adam and the torch_ema update rule
The hip path is also split into its four phases with events of their own (a separate pass, so the step
figure carries no extra events).  For the per-kernel table run the hip path alone under the profiler:
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/snr_train_bench.py --only hip`
and summarise DIR/run_kernel_stats.csv with tools/prof_summary.py.

    python tools/snr_train_bench.py [--steps 30] [--warmup 5] [--out profiles/snr_train_step.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "snr-aligned_diffse_amd"))

from oracle import snrnet_ref  # noqa: E402
from sgmse.snr_estimator import SNRModel  # noqa: E402
from snrse import formula, snr_train  # noqa: E402


def formula_sd():
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        keys = json.load(f)["snrnet"]
    vals = formula.formula_state_dict({"snrnet." + k: tuple(s) for k, s in keys})
    return {k[len("snrnet."):]: torch.from_numpy(v) for k, v in vals.items()}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps < 20 and args.only is None:
        ap.error("--steps >= 20")
    dev = torch.device("cuda:0")
    B, T = args.batch, args.frames
    x = (torch.from_numpy(formula.normal_tensor("bench.snrtrain.x", (B, 1, 256, T), True)) * 0.4).to(torch.complex64).to(dev)
    y = x + (torch.from_numpy(formula.normal_tensor("bench.snrtrain.n", (B, 1, 256, T), True)) * 0.4).to(torch.complex64).to(dev)
    gt = torch.linspace(0.1, 0.9, B, device=dev)

    m = SNRModel()
    m.dnn.load_state_dict(formula_sd())
    m = m.to(dev).train()
    opt = m.configure_optimizers()

    def hip_step():
        opt.zero_grad()
        loss = m._step((x, y), 0, gt=gt)
        loss.backward()
        m.optimizer_step(opt)
        return loss

    sd = {k: v.to(dev).requires_grad_(True) for k, v in formula_sd().items()}
    topt = torch.optim.Adam(list(sd.values()), lr=1e-4)
    shadow = [p.detach().clone() for p in sd.values()]
    n_up = [0]

    def torch_step():
        topt.zero_grad()
        SNR = (gt / (1 - gt)).unsqueeze(1).unsqueeze(2).unsqueeze(3)
        yp = x + (y - x) * 0.56234 * SNR
        yp = yp * (2.040166 / ((1 + SNR ** 2) ** 0.5))
        yr = torch.view_as_real(yp).permute(0, 4, 2, 3, 1).squeeze(4)
        est = snrnet_ref.snrnet_forward(yr, sd)
        loss = torch.nn.functional.mse_loss(gt, est.squeeze(1))
        loss.backward()
        topt.step()
        n_up[0] += 1
        decay = min(0.999, (1 + n_up[0]) / (10 + n_up[0]))
        with torch.no_grad():
            torch._foreach_sub_(shadow, torch._foreach_mul(torch._foreach_sub(shadow, list(sd.values())), 1 - decay))
        return loss

    paths = {"hip": hip_step, "torch": torch_step}
    if args.only:
        paths = {args.only: paths[args.only]}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in paths}
    for _ in range(args.steps):
        for k, fn in paths.items():  # alternated
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    res = {"batch": B, "frames": T, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    for k, pairs in ev.items():
        ms = [a.elapsed_time(b) for a, b in pairs]
        res[f"{k}_ms_median"] = statistics.median(ms)
        res[f"{k}_ms_min"] = min(ms)
        res[f"{k}_ms_max"] = max(ms)
    if "hip" in paths:
        # the phases of the hip step, each between events of its own
        split = {"perturb": [], "forward": [], "backward": [], "adam_ema": []}
        for _ in range(args.steps):
            opt.zero_grad()
            box = {}
            e = timed(lambda: box.__setitem__("yp", snr_train.perturb(x, y, gt)))
            split["perturb"].append(e)
            e = timed(lambda: box.__setitem__("loss", m._loss(gt, m.dnn.forward_train(box["yp"]))))
            split["forward"].append(e)
            split["backward"].append(timed(lambda: box["loss"].backward()))
            split["adam_ema"].append(timed(lambda: m.optimizer_step(opt)))
        torch.cuda.synchronize()
        res["hip_phase_ms_median"] = {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in split.items()}
    if "hip_ms_median" in res and "torch_ms_median" in res:
        res["torch_over_hip"] = res["torch_ms_median"] / res["hip_ms_median"]
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
