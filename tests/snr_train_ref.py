"""Shared reference of the SNR-estimator training tests (test_snr_train_host.py, test_gpu_snr_train.py):
the training step of snr_estimator.py:93-98, 105-109, 81-83 over oracle.snrnet_ref.snrnet_forward in
float64 under torch autograd on the CPU, computed once per case and left unchanged.

Bounds (the project's training bounds, tests/test_gpu_train.py / DESIGN 7e): loss 1e-5 relative, every
gradient tensor 5e-5 relative RMS ||g - g_ref|| / ||g_ref||, per-tensor sums of squares 2e-4.
"""
import functools

import numpy as np
import torch

from conftest import fnormal, formula_sd
from oracle import snrnet_ref

LOSS_RTOL = 1e-5
GRAD_RTOL = 5e-5
SUMSQ_RTOL = 2e-4


def formula_snr_sd():
    return {k: torch.from_numpy(v) for k, v in formula_sd("snrnet", "snrnet.").items()}


def batch(tag, B, T, zero_tail=0):
    """(x, y) complex64 [B, 1, 256, T]: clean and clean + noise, both formula normals x 0.4; the last
    `zero_tail` frames of both set to exact zero (pad_spec_16 / short-clip padding)."""
    x = torch.from_numpy(fnormal(f"{tag}.x", (B, 1, 256, T), complex_=True)) * 0.4
    n = torch.from_numpy(fnormal(f"{tag}.n", (B, 1, 256, T), complex_=True)) * 0.4
    y = x + n
    if zero_tail:
        x[..., T - zero_tail:] = 0
        y[..., T - zero_tail:] = 0
    return x.to(torch.complex64), y.to(torch.complex64)


def default_gt(B):
    return torch.linspace(0.15, 0.85, B, dtype=torch.float32)


def perturb_ref(x, y, gt):
    """snr_estimator.py:93-98 as written (any dtype / device)."""
    SNR = gt / (1 - gt)
    SNR = SNR.unsqueeze(1).unsqueeze(2).unsqueeze(3)
    y = x + (y - x) * 0.56234 * SNR
    normfac_ = (2.040166) * (0.240253 + 0.759747 * 1 ** 2) ** 0.5 / ((1 + (SNR / 1) ** 2) ** 0.5)
    return y * normfac_


def oracle_step(x, y, gt):
    """float64 loss, est [B, 1] and the 22 gradients of one training step."""
    sd = {k: v.double().requires_grad_(True) for k, v in formula_snr_sd().items()}
    gt = gt.double()
    yp = perturb_ref(x.to(torch.complex128), y.to(torch.complex128), gt)
    yr = torch.view_as_real(yp).permute(0, 4, 2, 3, 1).squeeze(4)
    est = snrnet_ref.snrnet_forward(yr, sd)
    loss = torch.nn.functional.mse_loss(gt, est.squeeze(1))
    loss.backward()
    return float(loss.detach()), est.detach(), {k: v.grad.detach() for k, v in sd.items()}


# A max-pool's gradient jumps where the top two of a window tie, and fp32 -- the reference's own included --
# resolves a gap below its rounding error either way.  The inputs of a case are therefore the draw SEED[(B, T)]
# of the formula normals, picked on the CPU with the reference arithmetic only: the first draw in which no window
# of the 2x2 or the (2, 1) pool has a float64 top-two gap within 4x the largest fp32-vs-float64 difference of
# that conv's output (pool_margins below; test_snr_train_host.py asserts it).  At (5, 272) the 2.8 M windows of
# the first pool make such a draw out of reach (10 to 20 windows lie within twice that difference in every draw
# tried); draw 0 is used and the bounds stay as they are.
SEED = {(2, 32): 1, (3, 48): 2, (5, 272): 0}


@functools.lru_cache(maxsize=None)
def case(B, T, zero_tail=0):
    """The (x, y, gt) of a parity case and its oracle step; computed once, shared, not to be modified."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    x, y = batch(f"t.snrtrain.{B}.{T}.{SEED[(B, T)]}", B, T, zero_tail)
    gt = default_gt(B)
    return x, y, gt, oracle_step(x, y, gt)


def pool_margins(x, y, gt):
    """Per conv pool (2x2, then (2, 1)): (the smallest float64 top-two gap over the windows, the largest
    |fp32 - float64| of the conv output), both from the reference arithmetic on the CPU."""
    import torch.nn.functional as F
    sd = formula_snr_sd()
    yp = perturb_ref(x.to(torch.complex128), y.to(torch.complex128), gt.double())
    yr = torch.view_as_real(yp).permute(0, 4, 2, 3, 1).squeeze(4)
    xs = yr.permute(0, 3, 1, 2).reshape(-1, 16, 2, 256).permute(0, 2, 3, 1)
    pre = {}
    for dt in (torch.float64, torch.float32):
        w = {k: v.to(dt) for k, v in sd.items()}
        f1 = F.conv2d(xs.to(dt), w["conv5x5_1.weight"], w["conv5x5_1.bias"], padding=2)
        f2 = F.conv2d(F.max_pool2d(f1, 2), w["conv3x3_1.weight"], w["conv3x3_1.bias"], padding=1)
        pre[dt] = (f1, f2)
    f1, f2 = pre[torch.float64]
    t = F.unfold(f1.reshape(-1, 1, 256, 16), 2, stride=2).topk(2, dim=1).values
    u = F.unfold(f2.reshape(-1, 1, 128, 8), (2, 1), stride=(2, 1))
    gaps = (float((t[:, 0] - t[:, 1]).min()), float((u[:, 0] - u[:, 1]).abs().min()))
    errs = tuple(float((a - b.double()).abs().max()) for a, b in zip(pre[torch.float64], pre[torch.float32]))
    return tuple(zip(gaps, errs))


def rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.sum((got - ref) ** 2)) / np.sqrt(np.sum(ref ** 2)))
