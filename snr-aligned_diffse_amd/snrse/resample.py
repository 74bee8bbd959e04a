"""Recordings at any sample rate in front of the 16 kHz networks: the host side of ops.resample_poly.

convert(sigs, rates_in, rates_out) brings a list of 1-D signals from one rate each to another rate each on the
device: the signals of one (rate in, rate out) pair share one ragged upload and one snrse_resample_poly launch,
whatever their lengths.  When no signal needs converting the list is handed back as it came and no device is
touched.  What ScoreModel.enhance_batch(sample_rates=...), snrse.enhance_files and snrse.evaluate --resample run.
There is no CPU fallback: without a HIP device the first list that needs converting raises.
"""
from __future__ import annotations

import numpy as np
import torch

from . import audio, ops
from .batching import pack_rows


def as_signal(y):
    """[L] / [1, L] numpy or tensor -> 1-D float32 tensor (ScoreModel.enhance_batch's own conversion)."""
    return torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(torch.float32).reshape(-1)


def convert(sigs, rates_in, rates_out, on_device=False):
    """sigs: 1-D signals (numpy / CPU tensors); rates_in / rates_out: one rate per signal, or one for all.
    -> list in input order of signals of resampled_length(L_i, in_i, out_i) samples.

    on_device=False: numpy float32 arrays (one download per rate pair); a signal whose rates are equal is the
    input object itself.  on_device=True: 1-D device tensors and no read-back at all -- views into the launches'
    outputs, and the signals whose rates are equal are uploaded together as one more padded batch -- for a consumer
    that goes on working on the device (enhance_batch gathers its ragged batches from them)."""
    n = len(sigs)
    rin = [int(rates_in)] * n if np.isscalar(rates_in) else [int(r) for r in rates_in]
    rout = [int(rates_out)] * n if np.isscalar(rates_out) else [int(r) for r in rates_out]
    if len(rin) != n or len(rout) != n:
        raise ValueError(f"snrse: {len(rin)} / {len(rout)} sample rates for {n} signals")
    groups = {}
    for i in range(n):
        if rin[i] != rout[i] or on_device:
            groups.setdefault((rin[i], rout[i]) if rin[i] != rout[i] else None, []).append(i)
    out = list(sigs)
    if not groups or set(groups) == {None}:
        return out
    dev = ops.current_device()
    for key, rows in groups.items():
        buf, lens = pack_rows([sigs[i] for i in rows])
        y = buf.to(dev)
        if key is not None:
            y, _ = ops.resample_poly(y, *audio.rational(*key), lengths=lens)
            lens = [audio.resampled_length(L, *key) for L in lens]
        if not on_device:
            y = y.cpu().numpy()
        for r, i in enumerate(rows):
            out[i] = y[r, :lens[r]] if on_device else y[r, :lens[r]].copy()
    return out
