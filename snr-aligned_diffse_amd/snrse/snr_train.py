"""Training of the SNR estimator on the HIP kernels of csrc/snrnet_train.hip (reference
sgmse/snr_estimator.py:81-116 around SNRNet, snrnet.py:47-97).  fp32, as the reference trains.

  perturb(x, y, gt)          the batch perturbation of snr_estimator.py:93-98, one kernel
  snrnet_train(spec, params) a torch.autograd.Function over the 22 SNRNet parameters in state-dict
                             layout: forward est [B, 1] (the stage kernels of the inference path, saving the
                             pool winners / LSTM gates / head arg-extrema), backward the reference-layout
                             gradients of every parameter (snrse_snrnet_backward)

HIP device tensors only (no CPU fallback); T must be a multiple of 16 and at least 32 (a single chunk
makes the reference's unbiased std over the chunks, and with it the loss, NaN).
"""
from __future__ import annotations

import torch

from . import _lib, ops


def _s():
    return torch.cuda.current_stream().cuda_stream


def check_frames(T: int):
    if T % 16 or T < 32:
        raise ValueError(f"SNRNet training needs T % 16 == 0 and T >= 32 frames (two 16-frame chunks), got T = {T}")


def _need_hip(*ts):
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("SNRNet training: HIP device tensors required (no CPU fallback)")


def perturb(x, y, gt):
    """y' = (x + (y - x) 0.56234 SNR) normfac(1, SNR, 1), SNR = gt / (1 - gt), per utterance
    (snr_estimator.py:93-98).  x, y complex64 [B, ...]; gt float32 [B]."""
    _need_hip(x, y, gt)
    B = x.shape[0]
    if x.shape != y.shape or gt.numel() != B:
        raise ValueError(f"perturb: x {tuple(x.shape)}, y {tuple(y.shape)}, gt {tuple(gt.shape)}")
    x = x.to(torch.complex64).contiguous()
    y = y.to(torch.complex64).contiguous()
    gt = gt.to(torch.float32).contiguous()
    out = torch.empty_like(y)
    _lib.call("snrse_snr_perturb", x.data_ptr(), y.data_ptr(), gt.data_ptr(), B, x.numel() // B, out.data_ptr(), _s())
    return out


# packed slot (ops.pack_snrnet order) of every directly stored tensor; the LSTM tensors are stacked [fwd, reverse]
_DIRECT = {k: i for i, k in enumerate(ops.SNRNET_KEYS)}
_WIH, _BSUM, _WHH, _FCW, _FCB = 12, 13, 14, 15, 16


class _SNRNetTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, keys, *params):
        sd = dict(zip(keys, params))
        packed = ops.pack_snrnet(sd, spec.device)
        B, _, T = spec.shape
        nbytes = int(_lib.load().snrse_snrnet_train_workspace(B, T))
        tws = torch.empty(nbytes, device=spec.device, dtype=torch.uint8)
        out = torch.empty(B, device=spec.device, dtype=torch.float32)
        _lib.call("snrse_snrnet_train_fwd", spec.data_ptr(), B, T, *[p.data_ptr() for p in packed], tws.data_ptr(),
                  out.data_ptr(), _s())
        ctx.keys, ctx.packed, ctx.tws, ctx.spec, ctx.est = keys, packed, tws, spec, out
        return out.clone()[:, None]

    @staticmethod
    def backward(ctx, dest):
        spec, packed = ctx.spec, ctx.packed
        B, _, T = spec.shape
        dest = dest.reshape(B).to(torch.float32).contiguous()
        g = [torch.empty_like(p) for p in packed]
        w3, wt, wih, whh, fcw = packed[2], packed[4:8], packed[_WIH], packed[_WHH], packed[_FCW]
        _lib.call("snrse_snrnet_backward", spec.data_ptr(), B, T, ctx.est.data_ptr(), dest.data_ptr(), w3.data_ptr(),
                  *[w.data_ptr() for w in wt], wih.data_ptr(), whh.data_ptr(), fcw.data_ptr(), ctx.tws.data_ptr(),
                  *[t.data_ptr() for t in g], _s())
        grads = []
        for k in ctx.keys:
            if k in _DIRECT:
                grads.append(g[_DIRECT[k]])
            elif k == "fc.weight":
                grads.append(g[_FCW].reshape(1, -1))
            elif k == "fc.bias":
                grads.append(g[_FCB])
            else:
                d = 1 if k.endswith("_reverse") else 0
                slot = _WIH if "weight_ih" in k else _WHH if "weight_hh" in k else _BSUM
                # b_ih and b_hh enter the gates as their sum: one gradient, a copy for each
                grads.append(g[slot][d].clone())
        return (None, None, *grads)


def snrnet_train(spec, params):
    """Differentiable SNRNet forward.  spec: complex64 [B, 256, T] device tensor; params: the module's
    parameters by state-dict key (all 22 of tests/golden/state_dict_keys.json['snrnet']).  Returns est [B, 1];
    est.backward() fills every parameter's .grad."""
    if spec.dim() != 3 or spec.shape[1] != 256:
        raise ValueError(f"snrnet_train: spec [B, 256, T] expected, got {tuple(spec.shape)}")
    check_frames(spec.shape[-1])
    _need_hip(spec, *params.values())
    keys = tuple(params)
    return _SNRNetTrain.apply(spec.to(torch.complex64).contiguous(), keys, *[params[k] for k in keys])


__all__ = ["perturb", "snrnet_train", "check_frames"]
