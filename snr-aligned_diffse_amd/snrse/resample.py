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


HIGHBAND_POLICIES = ("drop", "keep", "follow")


def highband_policy(policy):
    """What happens to the band above 8 kHz of a recording at more than 16 kHz when it is written back at its own
    rate -> "drop" (the networks' band alone, as before), "keep" (gain 1), "follow" (the gain the network applied
    to the top octave it saw, ops.band_gain) or a float, a fixed gain in dB <= 0.  Anything else raises."""
    if isinstance(policy, str):
        if policy not in HIGHBAND_POLICIES:
            raise ValueError(f"snrse: highband is one of {HIGHBAND_POLICIES} or a gain in dB <= 0, got {policy!r}")
        return policy
    if isinstance(policy, bool) or not isinstance(policy, (int, float, np.integer, np.floating)):
        raise ValueError(f"snrse: highband is one of {HIGHBAND_POLICIES} or a gain in dB <= 0, got {policy!r}")
    db = float(policy)
    if not np.isfinite(db) or db > 0.0:
        raise ValueError(f"snrse: a fixed highband gain is a finite number of dB <= 0, got {policy!r}")
    return db


def check_highband(policy, floor_db, sample_rates, output_rate):
    """enhance_batch's argument check, before any device work -> the normalised policy.  A band can only be kept
    where the results go back to the recordings' own rates."""
    policy = highband_policy(policy)
    floor_db = float(floor_db)
    if not np.isfinite(floor_db) or floor_db < 0.0:
        raise ValueError(f"snrse: highband_floor_db is a finite number of dB >= 0, got {floor_db}")
    if policy != "drop" and (sample_rates is None or output_rate != "input"):
        raise ValueError(f"snrse: highband={policy!r} needs sample_rates and output_rate='input': the band above "
                         f"8 kHz exists only at the recordings' own rates")
    return policy


def check_follow_lengths(lengths, rates):
    """highband="follow" takes an STFT of the 16 kHz signals, whose reflect padding needs 256 samples: a shorter
    recording above 16 kHz raises here, by its index, before any device work."""
    for i, (L, r) in enumerate(zip(lengths, rates)):
        if int(r) > audio.MODEL_RATE and audio.resampled_length(L, int(r), audio.MODEL_RATE) < 256:
            raise ValueError(f"snrse: highband='follow' needs at least 256 samples at 16 kHz (the STFT's reflect "
                             f"padding); recording {i} has {L} at {int(r)} Hz")


def restore_highband(enhanced16, noisy16, originals, rates, policy="keep", floor_db=30.0):
    """The enhanced 16 kHz signals back at the recordings' own rates with the band above 8 kHz of the recordings:
    out = U(x) + g (y - U(u)) (ops.resample_mix; the definition stands in include/snrse.h).  enhanced16, noisy16:
    the 16 kHz results and what the enhancers consumed (numpy / CPU tensors, or 1-D device tensors as
    convert(on_device=True) returns them); originals: the recordings; rates: one per recording; policy: "keep",
    "follow" or a gain in dB <= 0 ("drop" is plain convert) -> list of numpy float32 [L_i], L_i the recordings'
    lengths.  The rows of one rate above 16 kHz share one upload, the gain launches ("follow"), one mix launch and
    one download; a row at 16 kHz or below has no band to keep and goes through convert whatever the policy."""
    policy = highband_policy(policy)
    n = len(originals)
    rates = [int(r) for r in rates]
    if not (len(enhanced16) == len(noisy16) == len(rates) == n):
        raise ValueError(f"snrse: restore_highband takes one result, one 16 kHz input and one rate per recording, got "
                         f"{len(enhanced16)}, {len(noisy16)}, {len(rates)} for {n}")
    lens = [int(as_signal(y).numel()) if not (torch.is_tensor(y) and y.is_cuda) else int(y.numel()) for y in originals]
    if policy == "follow":
        check_follow_lengths(lens, rates)
    plain = [i for i in range(n) if policy == "drop" or rates[i] <= audio.MODEL_RATE]
    out = [None] * n
    if plain:
        back = convert([enhanced16[i] for i in plain], audio.MODEL_RATE, [rates[i] for i in plain])
        for i, h in zip(plain, back):
            out[i] = np.asarray(h.cpu() if torch.is_tensor(h) else h, np.float32)[:lens[i]]
    groups = {}
    for i in range(n):
        if out[i] is None:
            groups.setdefault(rates[i], []).append(i)
    if not groups:
        return out
    dev = ops.current_device()
    for rate, rows in groups.items():
        B = len(rows)
        l16 = [audio.resampled_length(lens[i], rate, audio.MODEL_RATE) for i in rows]
        for i, L in zip(rows, l16):
            if int(enhanced16[i].shape[-1]) != L or int(noisy16[i].shape[-1]) != L:
                raise ValueError(f"snrse: recording {i} has {lens[i]} samples at {rate} Hz, {L} at 16 kHz, but its "
                                 f"16 kHz signals have {enhanced16[i].shape[-1]} and {noisy16[i].shape[-1]}")
        s16, sR = max(max(l16), 1), max(max(lens[i] for i in rows), 1)
        # one host buffer, one upload: the rows of x, then of y, then -- unless they are on the device already -- of u
        u_dev = all(torch.is_tensor(noisy16[i]) and noisy16[i].is_cuda for i in rows)
        host = torch.zeros(B * (s16 + sR) + (0 if u_dev else B * s16), dtype=torch.float32)
        hx, hy = host[:B * s16].view(B, s16), host[B * s16:B * (s16 + sR)].view(B, sR)
        for r, i in enumerate(rows):
            hx[r, :l16[r]] = as_signal(enhanced16[i].cpu() if torch.is_tensor(enhanced16[i]) else enhanced16[i])
            hy[r, :lens[i]] = as_signal(originals[i].cpu() if torch.is_tensor(originals[i]) else originals[i])
        if u_dev:
            u = pack_rows([noisy16[i] for i in rows])[0]
        else:
            hu = host[B * (s16 + sR):].view(B, s16)
            for r, i in enumerate(rows):
                hu[r, :l16[r]] = as_signal(noisy16[i].cpu() if torch.is_tensor(noisy16[i]) else noisy16[i])
        d = host.to(dev)
        x, y = d[:B * s16].view(B, s16), d[B * s16:B * (s16 + sR)].view(B, sR)
        if not u_dev:
            u = d[B * (s16 + sR):].view(B, s16)
        if policy == "follow":
            gain = ops.band_gain(u, x, l16, floor_db)[0]  # its frame counts are resample_mix's default
        else:
            gain = 1.0 if policy == "keep" else 10.0 ** (policy / 20.0)
        mixed = ops.resample_mix(x, u, y, l16, [lens[i] for i in rows], rate, gain).cpu().numpy()
        for r, i in enumerate(rows):
            out[i] = mixed[r, :lens[i]].copy()
    return out


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
