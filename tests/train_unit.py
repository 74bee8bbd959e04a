"""Shared pieces of the training unit tests (test_gpu_train_kernels.py, test_gpu_train_autograd.py).

The bound of a HIP result against the float64 reference is not a number picked in advance: the same
operation is also computed by torch in float32 from the same inputs, and

    err(HIP vs fp64) <= 4 * err(torch-fp32 vs fp64) + floor

with err the relative RMS over the full tensor (elementwise kernels: max abs difference over max abs
reference) and floor one fp32 ulp of the reference's RMS, in the units of err.  The factor 4 covers another
summation order, atomics and expf / sinf implementations of the same precision.  Every measured pair is
appended to train_unit_errors.json under SNRSE_REPORT_DIR (as tests/test_gpu_train.py writes its reports),
before the assertion.
"""
import json
import os

import numpy as np
import torch

from test_gpu_train import REPORT_DIR  # SNRSE_REPORT_DIR, or that module's default: one place for all reports

REPORT = os.path.join(REPORT_DIR, "train_unit_errors.json")
FACTOR = 4.0


def rel_rms(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def rel_max(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())


def _floor(ref, kind):
    ref = ref.detach().double().cpu()
    rms = float(ref.pow(2).mean().sqrt())
    den = rms if kind == "rms" else float(ref.abs().max())
    return float(np.spacing(np.float32(rms))) / den


def record(kernel, case, hip_err, f32_err=None, bound=None):
    """Append one measured pair to the report (merged by (kernel, case), so a rerun replaces its entries)."""
    os.makedirs(REPORT_DIR, exist_ok=True)
    try:
        with open(REPORT) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data[f"{kernel} | {case}"] = {"hip_err": hip_err, "f32_err": f32_err, "bound": bound,
                                  "ratio": None if not f32_err else hip_err / f32_err}
    with open(REPORT, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)


def check(kernel, case, hip, f32, ref, kind="rms", floor_of=None, allow=0.0):
    """The measured rule: `hip` (the kernel's result), `f32` (torch float32 of the same inputs) and `ref`
    (torch float64 on the CPU), all of one shape.  `floor_of`: a tensor of the magnitudes that the result is a
    difference of, where it cancels -- the floor is then one fp32 ulp of THEIR RMS (no fp32 evaluation can do
    better).  `allow`: a further allowance in the units of err, derived and explained by the caller."""
    assert hip.shape == ref.shape == f32.shape, (kernel, case, hip.shape, f32.shape, ref.shape)
    assert torch.isfinite(hip).all(), f"{kernel} {case}: non-finite output"
    err = rel_rms if kind == "rms" else rel_max
    e_hip, e_f32 = err(hip, ref), err(f32, ref)
    floor = _floor(ref, kind)
    if floor_of is not None:
        fo = floor_of.detach().double().cpu()
        floor = max(floor, float(np.spacing(np.float32(fo.pow(2).mean().sqrt()))) / float(ref.double().pow(2).mean().sqrt()))
    bound = FACTOR * e_f32 + floor + allow
    record(kernel, case, e_hip, e_f32, bound)
    print(f"{kernel} [{case}]: HIP {e_hip:.3e}  torch-fp32 {e_f32:.3e}  bound {bound:.3e}")
    assert e_hip <= bound, f"{kernel} {case}: HIP err {e_hip:.3e} > 4 x fp32 err {e_f32:.3e} + floor = {bound:.3e}"


def check_fixed(kernel, case, hip, ref, tol):
    """A bound the project already has (weight gradients, attention, the fp32x3 mode)."""
    assert hip.shape == ref.shape, (kernel, case, hip.shape, ref.shape)
    assert torch.isfinite(hip).all(), f"{kernel} {case}: non-finite output"
    e = rel_rms(hip, ref)
    record(kernel, case, e, None, tol)
    print(f"{kernel} [{case}]: HIP {e:.3e}  fixed bound {tol:.1e}")
    assert e < tol, f"{kernel} {case}: rel RMS {e:.3e} >= {tol:.1e}"


def gen(seed):
    return torch.Generator().manual_seed(seed)
