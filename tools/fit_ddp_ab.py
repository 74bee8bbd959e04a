"""Cost of the data-parallel gradient exchange on the `bench.py --config train` step, on one device.

One process, one model (run_train's: sebridge_v3 'true', formula weights, B x [256, T] synthetic pairs, fp32), in
the exact and the fp32x3 GEMM modes: the training step as snrse.fit runs it (arm A: training_step -> backward ->
optimizer_step -> zero_grad) and the same step with a snrse.dist.GradReducer in an RCCL ('nccl') group of one
rank in front of the optimizer step (arm B: + snrse_grad_pack over the 262 MB of gradients, a one-rank
all-reduce, the .grads re-pointed into the flat buffer), alternated A B A B A B.  Every turn is WARMUP + STEPS
steps and its timed window ends in a device synchronise.  Then the pack launch alone, timed with device events.
Prints JSON lines (profiles/fit_ddp_ab.jsonl): the runs, each arm's median and spread, B over A.

What this cannot show: the all-reduce between devices.  With one rank RCCL moves nothing; the 1 -> N scaling of
training needs a node with N devices (python -m snrse.fit ... --gpus 8).

    python tools/fit_ddp_ab.py [--batch 8 --frames 256 --steps 4 --warmup 1 --rounds 3 --modes exact,x3 --out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "snr-aligned_diffse_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", type=str, default="exact,x3")
    ap.add_argument("--pack-iters", type=int, default=50)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    from sgmse.model import ScoreModel
    from snrse import dist as sdist
    from snrse import formula
    from snrse import train as strain
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(sdist.free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")) as f:
        shapes = {k: tuple(s) for k, s in json.load(f)["ncsnpp"]}
    m = ScoreModel(backbone="ncsnpp", sde="ouve", model_type="sebridge_v3", snr_conditioned="true", theta=1.5,
                   sigma_min=0.05, sigma_max=0.5, N=30, compute_dtype="fp32", fixed_snr=0.17783, loss_type="mse")
    m.dnn.load_state_dict({k: torch.from_numpy(v) for k, v in formula.formula_state_dict(shapes).items()})
    m = m.cuda().train()
    opt = m.configure_optimizers()
    red = sdist.GradReducer(list(m.named_parameters()), 1, dev)
    B, T = a.batch, a.frames
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, 1, 256, T, dtype=torch.complex64, device=dev, generator=g) * 0.4
    y = x + torch.randn(B, 1, 256, T, dtype=torch.complex64, device=dev, generator=g) * 0.4
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def step(i, reduce):
        loss = m.training_step((x, y), i)
        loss.backward()
        if reduce:
            t = time.perf_counter()
            red.reduce(opt, loss=loss.detach())
            host["reduce"] += time.perf_counter() - t
        t = time.perf_counter()
        m.optimizer_step(opt)
        host["optimizer"] += time.perf_counter() - t
        opt.zero_grad()

    host = {"reduce": 0.0, "optimizer": 0.0}

    def run(mode, reduce, tag):
        for w in range(a.warmup):
            step(w, reduce)
        torch.cuda.synchronize()
        host.update(reduce=0.0, optimizer=0.0)
        t0 = time.perf_counter()
        for k in range(a.steps):
            step(a.warmup + k, reduce)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        # host time spent inside the two calls (a call that waits for the device counts its wait)
        emit({"run": tag, "gemm": mode, "arm": "B reducer" if reduce else "A plain", "ms_per_step": round(ms, 3),
              "samples_per_s": round(B / ms * 1e3, 3), "steps": a.steps, "warmup": a.warmup,
              "host_ms_in_reduce": round(host["reduce"] / a.steps * 1e3, 3),
              "host_ms_in_optimizer_step": round(host["optimizer"] / a.steps * 1e3, 3)})
        return ms

    try:
        for mode in [s for s in a.modes.split(",") if s]:
            strain.set_gemm(mode)
            step(0, False)  # first-use allocations, the chunk tables and RCCL's start-up, outside every timed run
            step(0, True)
            res = {"A": [], "B": []}
            for r in range(1, a.rounds + 1):
                res["A"].append(run(mode, False, f"A{r}"))
                res["B"].append(run(mode, True, f"B{r}"))
            ma, mb = statistics.median(res["A"]), statistics.median(res["B"])
            spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in res.items()}
            over = mb / ma - 1
            emit({"summary": f"training step B={B} x [256, {T}], gemm {mode}: plain (A) / GradReducer in a one-rank "
                             f"RCCL group (B) alternated {a.rounds} times on one device",
                  "gemm": mode, "median_ms_A": round(ma, 3), "median_ms_B": round(mb, 3),
                  "B_over_A_pct": round(over * 100, 3), "spread_A_pct": round(spread["A"] * 100, 3),
                  "spread_B_pct": round(spread["B"] * 100, 3),
                  "within_bar": bool(over <= max(spread["A"], 0.005)),
                  "bar": "B within A's own run-to-run spread, or within 0.5 %"})
        # the pack launch alone on gradients of the model's sizes: device events bracket device time
        loss = m.training_step((x, y), 0)
        loss.backward()
        table, tix, starts, keep = opt.grad_table(red.params)
        gbytes = sum(p.numel() * 4 for p in red.params)
        args = (table.data_ptr(), tix.data_ptr(), starts.data_ptr(), int(tix.numel()), red.flat_off.data_ptr(), 1.0,
                red.flat.data_ptr())
        strain._call("snrse_grad_pack", *args)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.pack_iters):
            strain._call("snrse_grad_pack", *args)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / a.pack_iters * 1e3
        e0.record()
        for _ in range(a.pack_iters):
            dist.all_reduce(red.flat)
        e1.record()
        torch.cuda.synchronize()
        ar_us = e0.elapsed_time(e1) / a.pack_iters * 1e3
        emit({"kernels_us": {"snrse_grad_pack": round(us, 2), "all_reduce_world1": round(ar_us, 2)},
              "gradient_bytes": gbytes, "chunks": int(tix.numel()),
              "grad_pack_read_plus_write_TBps": round(2 * gbytes / (us * 1e-6) / 1e12, 3)})
    finally:
        dist.destroy_process_group()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
