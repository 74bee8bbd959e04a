"""Prepare the fixed-SNR dataset: remix every clean / noise pair of a corpus to one *active* SNR on the device.

snrse.fit and snrse.evaluate --oracle read the `VBD_SNR-5` layout: every pair remixed to -5 dB active SNR under
{clean,noise,noisy}/, plus active_rms.txt (name, clean active RMS, noise active RMS) for the validation split.  This
tool produces it from a VoiceBank-DEMAND style download (the steps: INTEGRATION.md):

    python -m snrse.snrize --clean_dir A (--noise_dir B | --noisy_dir C) --destination_folder OUT \\
        [--snr_db -5] [--rate 16000] [--batch_size 32] [--rms_only] [--max_corr X]

The definition (include/snrse.h at snrse_active_window_sums): 100-ms windows W = int(rate 0.1),
non-overlapping from sample 0; a window is active iff the NOISE's RMS over it exceeds 10^(-50/20) (max |noise| + eps);
clean_rms and noise_rms are the RMS over the active windows' samples (eps when none is active);
noise' = clean_rms / noise_rms 10^(-snr_db/20) noise, noisy = clean + noise'; if max |noisy| > 0.99 all three signals
are scaled to a peak of 0.99 - eps; 16-bit PCM out.  ops.snr_remix does all of it in four launches per batch.

Files are paired by name (sorted, as Specs globs them); every *.wav of --clean_dir needs its partner.  Mono only.  A
pair whose two files differ in length or rate, or a file with more than one channel, raises ValueError naming the
file, before anything is computed.  Without --noise_dir the noise is noisy - clean.

--rate R resamples both signals on the device first (ops.resample_poly, scipy's default filter), so the 48 kHz
corpus can be used as it is; with --noisy_dir the difference noisy - clean is formed after resampling.  The default
keeps each file's rate.  Files are batched by --batch_size in name order (rows of different rates inside a batch run
as separate launches; no length bucketing: no kernel mixes rows, and a row's results do not depend on its batch).

Remix mode writes OUT/{clean,noise,noisy}/<name>, OUT/active_rms.txt with the OUTPUT files' clean and noise active
RMS (analytic: clean_rms s and noise_rms g s from the unquantised signals, g the gain and s the clip guard's scale;
the activity mask does not change under a common scale of the noise), and OUT/snrize_manifest.tsv with the columns
MANIFEST_COLUMNS.  --rms_only writes only OUT/active_rms.txt of the INPUTS and the manifest (no audio, clip_scale
nan): point it at an existing split.

--max_corr X (off by default) leaves out pairs with |corr| > X and lists them in OUT/excluded.txt (they keep their
manifest rows).  The reference's readme mentions a 0.02 correlation filter of clean against noise but gives no code
and no definition; the Pearson coefficient over the whole (resampled) signals, compared by absolute value, is this
project's reading.  It cannot be combined with --rms_only, whose rows must stay aligned with the split's files.

File reads and writes go through a pool of at most 8 threads.
"""
from __future__ import annotations

import argparse
import math
import os
from concurrent.futures import ThreadPoolExecutor
from glob import glob
from os.path import basename, join

import numpy as np
import torch

from . import audio, ops
from .batching import pack_rows

MANIFEST_COLUMNS = ("name", "rate", "samples", "clean_rms_in", "noise_rms_in", "snr_in_db", "gain", "clip_scale",
                    "active_windows", "windows", "corr")
MAX_WORKERS = 8


def rms_line(name, clean_rms, noise_rms):
    """One line of active_rms.txt: name, clean RMS, noise RMS, tab-separated, the numbers with repr precision."""
    return f"{name}\t{float(clean_rms)!r}\t{float(noise_rms)!r}\n"


def manifest_line(row):
    """One line of snrize_manifest.tsv from a dict keyed by MANIFEST_COLUMNS (floats with repr precision)."""
    return "\t".join(repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)
                     for v in (row[k] for k in MANIFEST_COLUMNS)) + "\n"


def pair_files(clean_dir, other_dir):
    """-> [(name, clean path, other path, frames, rate)], sorted by name, from the headers alone.  ValueError naming
    the file for a missing partner, a file snrse.audio cannot read, more than one channel, or a pair that differs
    in length or rate."""
    clean = sorted(glob(join(clean_dir, "*.wav")))
    if not clean:
        raise ValueError(f"snrize: no *.wav files in {clean_dir}")
    out = []
    for f in clean:
        name = basename(f)
        g = join(other_dir, name)
        if not os.path.exists(g):
            raise ValueError(f"snrize: {name} has no partner in {other_dir}")
        for p in (f, g):
            if not audio.readable(p):
                raise ValueError(f"snrize: {p} is not a WAVE file snrse.audio reads")
        (n0, ch0, sr0), (n1, ch1, sr1) = audio.info(f), audio.info(g)
        if ch0 != 1 or ch1 != 1:
            raise ValueError(f"snrize: {name} is not mono ({ch0} / {ch1} channels); only mono files are supported")
        if n0 != n1 or sr0 != sr1:
            raise ValueError(f"snrize: {name}: the clean file has {n0} samples at {sr0} Hz, its partner {n1} at "
                             f"{sr1} Hz; a pair must agree in both")
        if n0 < 1:
            raise ValueError(f"snrize: {name} is empty")
        out.append((name, f, g, n0, sr0))
    return out


def _read(path):
    return audio.read_wav(path)[0][:, 0]


def prepare_batch(clean, other, sr, rate=None, other_is_noisy=False):
    """Host signals of one rate -> (clean, noise [B, L] f32 on the device, lengths numpy [B], fs): packed, resampled
    to `rate` when it differs from sr, the noise formed as other - clean after that when other_is_noisy."""
    dev = ops.current_device()
    c, lens = pack_rows(clean)
    o, _ = pack_rows(other)
    c, o = c.to(dev), o.to(dev)
    lens = np.asarray(lens, np.int64)
    fs = int(sr)
    if rate is not None and int(rate) != fs:
        up, down = audio.rational(fs, int(rate))
        c, _ = ops.resample_poly(c, up, down, lengths=lens)
        o, _ = ops.resample_poly(o, up, down, lengths=lens)
        lens = np.asarray([audio.resampled_length(L, fs, int(rate)) for L in lens], np.int64)
        fs = int(rate)
    if other_is_noisy:
        o = o - c
    return c.contiguous(), o.contiguous(), lens, fs


def remix_files(clean_dir, destination_folder, noise_dir=None, noisy_dir=None, snr_db=-5.0, rate=None,
                batch_size=32, rms_only=False, max_corr=None):
    """The tool as a function (the module docstring describes it) -> the manifest rows, one dict per pair keyed by
    MANIFEST_COLUMNS plus 'excluded' (bool), 'clean_rms_out' and 'noise_rms_out' (what active_rms.txt holds)."""
    if (noise_dir is None) == (noisy_dir is None):
        raise ValueError("snrize: give exactly one of noise_dir and noisy_dir")
    if rms_only and max_corr is not None:
        raise ValueError("snrize: max_corr cannot be combined with rms_only (active_rms.txt must keep one row per "
                         "file of the split)")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"snrize: batch_size must be at least 1, got {batch_size}")
    if rate is not None and int(rate) < 10:
        raise ValueError(f"snrize: rate {rate} Hz leaves no 100-ms window")
    pairs = pair_files(clean_dir, noisy_dir if noise_dir is None else noise_dir)
    os.makedirs(destination_folder, exist_ok=True)
    if not rms_only:
        for sub in ("clean", "noise", "noisy"):
            os.makedirs(join(destination_folder, sub), exist_ok=True)
    rows, writes = [None] * len(pairs), []
    with ThreadPoolExecutor(max_workers=MAX_WORKERS) as pool:
        for b0 in range(0, len(pairs), batch_size):
            batch = pairs[b0:b0 + batch_size]
            cs = list(pool.map(_read, [p[1] for p in batch]))
            os_ = list(pool.map(_read, [p[2] for p in batch]))
            for sr in sorted({p[4] for p in batch}):
                idx = [i for i, p in enumerate(batch) if p[4] == sr]
                c, n, lens, fs = prepare_batch([cs[i] for i in idx], [os_[i] for i in idx], sr, rate,
                                               other_is_noisy=noise_dir is None)
                if rms_only:
                    rms, info = ops.active_rms(c, n, lengths=lens, fs=fs, snr_db=snr_db, return_info=True)
                    pcm = None
                    scale = np.full(len(idx), math.nan)
                else:
                    cq, nq, yq, info = ops.snr_remix(c, n, lengths=lens, fs=fs, snr_db=snr_db, pcm16=True)
                    rms = info["rms"]
                    pcm = [t.cpu().numpy() for t in (cq, nq, yq)]
                    scale = info["scale"].cpu().numpy()
                rms, gain, corr = rms.cpu().numpy(), info["gain"].cpu().numpy(), info["corr"].cpu().numpy()
                act, nwin = info["active_windows"].cpu().numpy(), info["windows"].numpy()
                for j, i in enumerate(idx):
                    name, L = batch[i][0], int(lens[j])
                    cr, nr = float(rms[j, 0]), float(rms[j, 1])
                    row = dict(name=name, rate=fs, samples=L, clean_rms_in=cr, noise_rms_in=nr,
                               snr_in_db=20.0 * math.log10(cr / nr) if cr > 0 else -math.inf, gain=float(gain[j]), clip_scale=float(scale[j]),
                               active_windows=int(act[j]), windows=int(nwin[j]), corr=float(corr[j]))
                    row["excluded"] = max_corr is not None and abs(row["corr"]) > float(max_corr)
                    if rms_only:
                        row["clean_rms_out"], row["noise_rms_out"] = cr, nr
                    else:
                        row["clean_rms_out"] = cr * row["clip_scale"]
                        row["noise_rms_out"] = nr * row["gain"] * row["clip_scale"]
                    rows[b0 + i] = row
                    if pcm is not None and not row["excluded"]:
                        for sub, q in zip(("clean", "noise", "noisy"), pcm):
                            writes.append(pool.submit(audio.write_wav, join(destination_folder, sub, name),
                                                      q[j, :L].copy(), fs, 16))
        for w in writes:
            w.result()
    with open(join(destination_folder, "active_rms.txt"), "w") as f:
        for r in rows:
            if not r["excluded"]:
                f.write(rms_line(r["name"], r["clean_rms_out"], r["noise_rms_out"]))
    with open(join(destination_folder, "snrize_manifest.tsv"), "w") as f:
        f.write("\t".join(MANIFEST_COLUMNS) + "\n")
        for r in rows:
            f.write(manifest_line(r))
    if max_corr is not None:
        with open(join(destination_folder, "excluded.txt"), "w") as f:
            for r in rows:
                if r["excluded"]:
                    f.write(r["name"] + "\n")
    return rows


def parser():
    ap = argparse.ArgumentParser(description="remix clean / noise pairs to a fixed active SNR on the MI355X path")
    ap.add_argument("--clean_dir", type=str, required=True)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--noise_dir", type=str, default=None, help="noise files, paired with the clean ones by name")
    g.add_argument("--noisy_dir", type=str, default=None, help="noisy files: the noise is noisy - clean")
    ap.add_argument("--destination_folder", type=str, required=True)
    ap.add_argument("--snr_db", type=float, default=-5.0, help="target active SNR in dB")
    ap.add_argument("--rate", type=int, default=None, help="resample to this rate first (default: keep the file's)")
    ap.add_argument("--batch_size", type=int, default=32, help="pairs per ragged batch")
    ap.add_argument("--rms_only", action="store_true",
                    help="write only active_rms.txt of the inputs and the manifest, no audio")
    ap.add_argument("--max_corr", type=float, default=None,
                    help="leave out pairs whose |Pearson coefficient| of clean and noise exceeds this")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.rms_only and a.max_corr is not None:
        ap.error("--max_corr cannot be combined with --rms_only")
    rows = remix_files(a.clean_dir, a.destination_folder, noise_dir=a.noise_dir, noisy_dir=a.noisy_dir,
                       snr_db=a.snr_db, rate=a.rate, batch_size=a.batch_size, rms_only=a.rms_only,
                       max_corr=a.max_corr)
    kept = sum(not r["excluded"] for r in rows)
    print(f"snrize: {len(rows)} pairs analysed, {kept} {'listed' if a.rms_only else 'written'} under "
          f"{a.destination_folder}" + (f", {len(rows) - kept} excluded by --max_corr" if a.max_corr is not None else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
