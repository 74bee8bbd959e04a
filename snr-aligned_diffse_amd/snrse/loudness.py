"""Programme loudness of recordings: the host layer over ops.loudness / ops.peak_oversampled / ops.gain_to_pcm16, and
a meter for a folder.

The measure is ITU-R BS.1770-4 integrated loudness as include/snrse.h states it at snrse_kweight_sums: K-weighting
re-discretised for the file's rate, 400-ms blocks at a 100-ms hop, the absolute gate at -70 and the relative gate 10
LU under the mean of what passed it.  What it is not: every channel has weight 1 (the files carry no channel layout,
so the standard's 1.41 for surround channels is never applied), there is no loudness range and no momentary or
short-term read-out, and the peak is max |.| of the signal oversampled 4x by the project's own resampling filter
(audio.resample_taps(4, 1), 81 taps) -- a 4x peak, not the true peak of the standard's Annex 2, whose 48-tap filter
is not what runs here; it is never called dBTP.

    python -m snrse.loudness DIR [--csv FILE]

lists filename, rate, channels, seconds, lufs, peak_db of every readable *.wav of DIR, so that a target for
snrse.enhance_files --loudness can be chosen before a run.
"""
from __future__ import annotations

import functools
import math

import numpy as np

SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)  # f0 Hz, gain dB, Q
SHELF_VB_EXP = 0.4996667741545416
HIGHPASS = (38.13547087602444, 0.5003270373238773)  # f0 Hz, Q


def kweighting(rate):
    """The ten K-weighting coefficients for `rate` Hz, float64: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (each
    a0 is 1): the standard's analog prototype through the bilinear transform, its 48 kHz table to 1e-13."""
    fs = float(rate)
    if not fs > 0:
        raise ValueError(f"snrse: a sample rate must be positive, got {rate}")
    f0, G, Q = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(shelf + hp, np.float64)


def step_matrix(coef):
    """The 4 x 4 zero-input transition A of one sample on the state (shelf w1, w2, high-pass w1, w2) of the two
    biquads in transposed direct form II, the second fed by the first."""
    b0, b1, b2, a1, a2, h0, h1, h2, c1, c2 = (float(v) for v in coef)
    # x = 0: y = w1s, z = h0 y + w1h
    return np.array([[-a1, 1.0, 0.0, 0.0],
                     [-a2, 0.0, 0.0, 0.0],
                     [h1 - c1 * h0, 0.0, -c1, 1.0],
                     [h2 - c2 * h0, 0.0, -c2, 0.0]], np.float64)


def chunk_transition(rate, C):
    """A^C for `rate`: what C samples of silence make of a filter state (float64 [4, 4])."""
    return np.linalg.matrix_power(step_matrix(kweighting(rate)), int(C))


def n100(rate):
    """Samples of a 100-ms sub-block: (rate + 5) // 10."""
    return (int(rate) + 5) // 10


@functools.lru_cache(maxsize=64)
def kernel_params(rate, C, S):
    """One row of snrse_kweight_sums's parameter table: the coefficients, A^C, A^(C S) -> float64 [42]."""
    A = step_matrix(kweighting(rate))
    AC = np.linalg.matrix_power(A, int(C))
    return np.concatenate([kweighting(rate), AC.reshape(-1), np.linalg.matrix_power(AC, int(S)).reshape(-1)])


def parse_target(value):
    """--loudness: "off" -> None, "input" -> "input", a number (LUFS) -> float."""
    if value is None:
        return None
    if isinstance(value, str):
        v = value.strip().lower()
        if v == "off":
            return None
        if v == "input":
            return "input"
        try:
            value = float(v)
        except ValueError:
            raise ValueError(f"snrse: loudness is off, input or a level in LUFS, got {value!r}") from None
    value = float(value)
    if not math.isfinite(value):
        raise ValueError(f"snrse: a loudness target must be finite, got {value}")
    return value


def check_ceiling(peak_db):
    peak_db = float(peak_db)
    if not peak_db <= 0.0:
        raise ValueError(f"snrse: the peak ceiling is at most 0 dB, got {peak_db}")
    return peak_db


def plan_gain(lufs_measured, target, peak, ceiling_db=-1.0):
    """-> (gain, limited): g = 10^((target - I) / 20); when g peak would pass c = 10^(ceiling_db / 20), g = c / peak
    and limited is True: a plain gain reduction, no limiter.  I = -inf (silence, or under 400 ms) gives g = 1."""
    I = float(lufs_measured)
    if I == -math.inf or math.isnan(I):
        return 1.0, False
    g = 10.0 ** ((float(target) - I) / 20.0)
    c = 10.0 ** (float(ceiling_db) / 20.0)
    peak = float(peak)
    if g * peak > c:
        return c / peak, True
    return g, False


def db(v):
    v = float(v)
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def batch_rows(files, device):
    """files: [(x [C, L] or [L] float array / tensor, rate)] -> (rows [R, Lmax] f32 on the device, lengths, rates,
    groups: host lists per row), the padding zero.  One upload for host arrays."""
    import torch
    lens, rates, groups, chans = [], [], [], []
    for k, (x, sr) in enumerate(files):
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32)))
        x = x[None] if x.dim() == 1 else x
        if x.dim() != 2:
            raise ValueError("snrse: measure takes [channels, samples] (or [samples]) signals")
        for c in range(x.shape[0]):
            chans.append(x[c])
            lens.append(int(x.shape[1]))
            rates.append(int(sr))
            groups.append(k)
    Lmax = max(max(lens, default=0), 1)
    if all(c.is_cuda for c in chans):
        rows = torch.zeros(len(chans), Lmax, device=device, dtype=torch.float32)
        for r, c in enumerate(chans):
            rows[r, :lens[r]] = c
    else:
        host = torch.zeros(len(chans), Lmax, dtype=torch.float32)
        for r, c in enumerate(chans):
            host[r, :lens[r]] = c.to(torch.float32).cpu()
        rows = host.to(device)
    return rows, lens, rates, groups


def measure_rows(rows, lens, rates, groups):
    """Device rows -> ([G] f64 lufs, [G] f32 4x peak of each file: the largest of its rows), on the device."""
    import torch
    from . import ops
    lufs = ops.loudness(rows, lengths=lens, rate=rates, groups=groups)
    pk = ops.peak_oversampled(rows, lengths=lens)
    G = int(lufs.numel())
    fpk = torch.zeros(G, device=rows.device, dtype=torch.float32)
    fpk.scatter_reduce_(0, torch.as_tensor(groups, device=rows.device, dtype=torch.int64), pk, reduce="amax")
    return lufs, fpk


def measure(files, device=None):
    """files: [(x, rate)] with x a [channels, samples] float array or tensor -> [(lufs, peak_db)] per file, the
    channels of a file measured together.  One upload and one read-back per call."""
    import torch
    from . import ops
    if not files:
        return []
    device = device or ops.current_device()
    rows, lens, rates, groups = batch_rows(files, device)
    lufs, fpk = measure_rows(rows, lens, rates, groups)
    back = torch.cat([lufs, fpk.to(torch.float64)]).cpu().numpy()
    G = len(files)
    return [(float(back[k]), db(back[G + k])) for k in range(G)]


def meter(folder, csv=None, files_per_call=8):
    """-> rows (filename, rate, channels, seconds, lufs, peak_db) of the readable *.wav files of `folder`, printed
    and, with csv, written there."""
    import os
    from glob import glob
    from . import audio
    paths = [f for f in sorted(glob(os.path.join(folder, "*.wav"))) if audio.readable(f)]
    out = []
    for i in range(0, len(paths), files_per_call):
        part = paths[i:i + files_per_call]
        loaded = [audio.load(p) for p in part]
        for p, (x, sr), (lufs, pk) in zip(part, loaded, measure(loaded)):
            out.append((os.path.basename(p), sr, int(x.shape[0]), x.shape[1] / sr, lufs, pk))
    lines = ["filename,rate,channels,seconds,lufs,peak_db"]
    lines += [f"{n},{sr},{ch},{sec!r},{lufs:.4f},{pk:.4f}" for n, sr, ch, sec, lufs, pk in out]
    print("\n".join(lines))
    if csv:
        with open(csv, "w") as f:
            f.write("\n".join(lines) + "\n")
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="integrated loudness (BS.1770-4) and 4x peak of the *.wav files of a folder")
    ap.add_argument("folder", type=str)
    ap.add_argument("--csv", type=str, default=None)
    a = ap.parse_args(argv)
    meter(a.folder, a.csv)


if __name__ == "__main__":
    main()
