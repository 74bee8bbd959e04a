"""Enhance a folder of noisy recordings: no clean reference, any sample rate, any channel count.

Every *.wav of <noisy_dir> that snrse.audio can read (sorted by name) is taken; every channel of a file is one
utterance with a noise seed of its own.  The utterances are planned from the WAV headers alone (their lengths at
16 kHz, snrse.audio.resampled_length), grouped into ragged batches as snrse.evaluate --batch_size does
(snrse.batching.plan_batches), and each batch is one ScoreModel.enhance_batch(sample_rates=...) call: channels that
are not at 16 kHz are resampled on the device (snrse_resample_poly), everything runs through the ragged-batch
enhancers, so the range guard, --sampler_type ode and the one-step route come with it.  The channels are put back
into a 16-bit PCM file of the same name and channel count under <destination_folder>: at 16 kHz, or with
--output_rate input at the file's own rate and frame count.  _enhanced.csv lists name, input rate, channels,
seconds and output rate of every file.

--window_frames F (off by default) is for recordings longer than the network's training crops -- meetings, podcasts,
anything from about ten seconds up: without it a file is one network input, whose memory grows with its length (and
with its square in the attention) until the device runs out.  With it every channel is cut into overlapping windows
of F frames (512 = 8.2 s is the flagship shape), the windows of a call share the ragged batches, and their results
are cross-faded over --overlap_frames frames (ScoreModel.enhance_batch(window_frames=...), snrse.longform); a file
of at most (F - 1) 128 samples at 16 kHz is enhanced exactly as without the flag, and _enhanced.csv gets a `windows`
column (windows per channel).

The seeds are drawn first, one torch.randint(0, 2**62) per (file, channel), in file order then channel order: for
a folder of 16 kHz mono files these are the draws, the plan and the calls of snrse.evaluate --batch_size B, and the
files written are byte for byte those it writes into <destination_folder>/all.  Files shard contiguously over
ranks (snrse.dist.shard_range); rank 0 writes the csv, which needs the headers only.

    python -m snrse.enhance_files --noisy_dir DIR --ckpt CKPT --destination_folder OUT \\
        [--batch_size 32] [--output_rate model|input] [--seed S] [--N 30 --sampler_type pc ...] \\
        [--window_frames 512 [--overlap_frames 64]] \\
        [--highband drop|keep|follow | --highband_gain_db X] [--highband_floor_db 30] \\
        [--loudness off|input|LUFS [--peak_db -1.0]]

--highband (with --output_rate input) says what becomes of the band above 8 kHz of a file at more than 16 kHz, which
the 16 kHz networks never see: drop (the default) writes the networks' band alone, as before; keep adds the file's own
band back unchanged, --highband_gain_db X adds it at X dB (<= 0), and follow attenuates it frame by frame as much as
the network attenuated the top octave it saw, by at most --highband_floor_db dB (ScoreModel.enhance_batch(highband=...)).

--loudness (off by default) sets the level of the written files, which otherwise is whatever the noisy peak made it:
a number brings every file to that integrated loudness in LUFS (ITU-R BS.1770-4 as snrse.loudness states it: -23 is
EBU R 128, podcasts use -16 .. -19), `input` gives it the integrated loudness of the noisy file it came from, measured
at that file's own rate.  Once all channels of a file are done they are measured together on the device at the rate
they are written at, ONE gain is applied to all of them (the stereo image is kept) and the 16-bit samples come from
the device conversion (ops.gain_to_pcm16).  --peak_db X (default -1, at most 0) is a ceiling on the 4x-oversampled
peak: where the gain would pass it the gain is reduced to meet it -- a plain gain reduction, no limiter -- and the file
is marked `limited`.  A file with no 400-ms block above -70 LUFS (silence, or shorter than 400 ms) is written with
gain 1.  _enhanced.csv then ends with the columns input_lufs (the noisy file), enhanced_lufs (the enhanced file before
the gain), gain_db, peak_db (the 4x peak after the gain) and limited (0 / 1); written loudness = enhanced_lufs +
gain_db.  It works with every --output_rate, --window_frames and --highband setting.
"""
from __future__ import annotations

import argparse
import os
import warnings
from glob import glob
from os.path import join

import numpy as np
import torch

from . import audio, dist as sdist, longform, resample
from .batching import plan_batches
from .evaluate import load_model, reverse_start, sampler_arguments, sampler_kwargs
from .sampler import draw_seed

CSV_COLUMNS = ("filename", "input_rate", "channels", "seconds", "output_rate")


def list_files(noisy_dir):
    """-> [(path, frames, channels, rate)] of the readable *.wav files of noisy_dir, sorted; the others are named
    in a warning and left out."""
    out = []
    for f in sorted(glob(join(noisy_dir, "*.wav"))):
        if not audio.readable(f):
            warnings.warn(f"enhance_files: skipping {f}: not a WAVE file snrse.audio reads")
            continue
        out.append((f, *audio.info(f)))
    return out


def utterances(files):
    """[(file index, channel)] in file order then channel order: one utterance, one seed each."""
    return [(k, c) for k, (_, _, ch, _) in enumerate(files) for c in range(ch)]


def draw_seeds(n):
    """n draws of the evaluation driver's per-file seed, in order."""
    return [draw_seed() for _ in range(n)]


LOUDNESS_COLUMNS = ("input_lufs", "enhanced_lufs", "gain_db", "peak_db", "limited")


def write_csv(files, output_rate, target_dir, window=None, loud=None):
    """window: None, or (window_frames, overlap_frames): one more column, the windows of each channel.  loud: None,
    or one row of LOUDNESS_COLUMNS values per file: five more columns, after every other."""
    with open(join(target_dir, "_enhanced.csv"), "w") as f:
        f.write(",".join(CSV_COLUMNS + (("windows",) if window else ()) + (LOUDNESS_COLUMNS if loud is not None else ()))
                + "\n")
        for i, (path, n, ch, sr) in enumerate(files):
            ro = sr if output_rate == "input" else audio.MODEL_RATE
            row = f"{os.path.basename(path)},{sr},{ch},{n / sr!r},{ro}"
            if window:
                W, V, _ = longform.geometry(*window)
                row += f",{len(longform.window_starts(audio.resampled_length(n, sr, audio.MODEL_RATE), W, V))}"
            if loud is not None:
                a, b, g, p, lim = (float(v) for v in loud[i])
                row += f",{a!r},{b!r},{g!r},{p!r},{int(lim)}"
            f.write(row + "\n")


def level_file(x, ro, noisy, sr, target, peak_db):
    """One finished file through the loudness stage: x = its enhanced channels (float32 arrays at rate ro), noisy =
    the file it came from ([channels, frames] at rate sr) -> (int16 [frames, channels] or [frames], the
    LOUDNESS_COLUMNS values).  Both files are measured in one batch (one upload, one read-back); the gain applied
    is 10^(gain_db / 20) of the gain_db reported, so the csv says exactly what was done."""
    from . import loudness as ld, ops
    dev = ops.current_device()
    rows, lens, rates, groups = ld.batch_rows([(np.stack(x), ro), (noisy, sr)], dev)
    lufs, pk = ld.measure_rows(rows, lens, rates, groups)
    back = torch.cat([lufs, pk.to(torch.float64)]).cpu().numpy()
    l_enh, l_in, p_enh = float(back[0]), float(back[1]), float(back[2])
    want = l_in if target == "input" else target
    if want == -np.inf:  # a silent noisy file sets no level
        gain, limited = 1.0, False
    else:
        gain, limited = ld.plan_gain(l_enh, want, p_enh, peak_db)
    gain_db = ld.db(gain)
    gain = 10.0 ** (gain_db / 20.0)
    ch, n = len(x), len(x[0])
    q = ops.gain_to_pcm16(rows[:ch], torch.full((ch,), gain, device=dev, dtype=torch.float64), lengths=lens[:ch])
    q = q[:, :n].cpu().numpy()
    return (q[0] if ch == 1 else np.ascontiguousarray(q.T)), (l_in, l_enh, gain_db, ld.db(gain * p_enh), float(limited))


def enhance_files(model, noisy_dir, target_dir, batch_size=32, max_frames=16384, output_rate="model", rank=0,
                  world=1, sampler_type="pc", predictor="reverse_diffusion", corrector="ald", corrector_steps=1,
                  snr=0.5, N=30, reverse_starting_point=1.0, force_N=0, atol=1e-5, rtol=1e-5,
                  timestep_type="linear", correct_stepsize=False, window_frames=None, overlap_frames=64,
                  highband="drop", highband_floor_db=30.0, loudness="off", peak_db=-1.0, **enhance_kw):
    """-> the list_files() rows of every file (all ranks'); this rank's share is enhanced and written.
    window_frames / overlap_frames: ScoreModel.enhance_batch's (None: every channel is one network input), and so
    are highband / highband_floor_db (anything but "drop" needs output_rate="input").  loudness: "off", "input" or a
    level in LUFS, peak_db: the ceiling on the 4x peak (module docstring)."""
    if output_rate not in ("model", "input"):
        raise ValueError(f"enhance_files: output_rate is 'model' or 'input', got {output_rate!r}")
    highband = resample.check_highband(highband, highband_floor_db, (), output_rate)
    target = None
    if loudness is not None and loudness != "off":  # off: the loudness layer is not even imported
        from . import loudness as ld
        target, peak_db = ld.parse_target(loudness), ld.check_ceiling(peak_db)
    levels = []
    window = None
    if window_frames is not None:
        longform.geometry(window_frames, overlap_frames)
        window = (window_frames, overlap_frames)
    os.makedirs(target_dir, exist_ok=True)
    N = reverse_start(model, reverse_starting_point, N, force_N)
    files = list_files(noisy_dir)
    a, b = sdist.shard_range(len(files), rank, world)
    mine = files[a:b]
    utts = utterances(mine)
    kw = dict(sampler_type=sampler_type, predictor=predictor, corrector=corrector, corrector_steps=corrector_steps,
              N=N, snr=snr, atol=atol, rtol=rtol, timestep_type=timestep_type, correct_stepsize=correct_stepsize,
              **enhance_kw)
    # settings without a batched enhancer run enhance_batch's per-utterance loop, which draws as it goes
    seeds = draw_seeds(len(utts)) if model._batch_route(sampler_type, corrector, enhance_kw) is not None else None
    if window:  # the calls are planned as without it, by the channels' whole lengths; the windows inside each call
        kw.update(window_frames=window_frames, overlap_frames=overlap_frames)
    if highband != "drop":
        kw.update(highband=highband, highband_floor_db=highband_floor_db)
    lens = [audio.resampled_length(mine[k][1], mine[k][3], audio.MODEL_RATE) for k, _ in utts]
    done = {k: [None] * f[2] for k, f in enumerate(mine)}
    for batch in plan_batches(lens, batch_size, max_frames):
        loaded = {}
        for u in batch:
            k = utts[u][0]
            if k not in loaded:
                loaded[k] = audio.load(mine[k][0])[0]
        hs = model.enhance_batch([loaded[utts[u][0]][utts[u][1]] for u in batch],
                                 seeds=None if seeds is None else [seeds[u] for u in batch],
                                 batch_size=batch_size if window else len(batch),  # windows: rows per enhancer call
                                 max_frames=max_frames, sample_rates=[mine[utts[u][0]][3] for u in batch],
                                 output_rate=output_rate, **kw)
        for u, h in zip(batch, hs):
            k, c = utts[u]
            done[k][c] = np.asarray(h, np.float32)
            if all(v is not None for v in done[k]):
                path, _, ch, sr = mine[k]
                x = done.pop(k)
                ro = sr if output_rate == "input" else audio.MODEL_RATE
                if target is None:
                    audio.write_wav(join(target_dir, os.path.basename(path)), x[0] if ch == 1 else np.stack(x, 1), ro,
                                    bits=16)
                    continue
                q, row = level_file(x, ro, loaded[k] if k in loaded else audio.load(path)[0], sr, target, peak_db)
                levels.append((k, row))
                audio.write_wav(join(target_dir, os.path.basename(path)), q, ro, bits=16)
    loud = None
    if target is not None:  # rank 0 writes every rank's rows
        from . import ops
        vals = np.zeros((len(mine), len(LOUDNESS_COLUMNS)), np.float64)
        for k, row in levels:
            vals[k] = row
        loud = sdist.gather_metrics(vals, len(files), rank, world, ops.current_device()).cpu().numpy()
    if rank == 0:
        write_csv(files, output_rate, target_dir, window, loud)
    return files


def parser():
    ap = argparse.ArgumentParser(description="enhance a folder of noisy recordings on the MI355X path")
    ap.add_argument("--noisy_dir", type=str, required=True)
    ap.add_argument("--ckpt", type=str, required=True)
    ap.add_argument("--destination_folder", type=str, required=True)
    ap.add_argument("--batch_size", type=int, default=32, help="utterances (file channels) per ragged batch")
    ap.add_argument("--output_rate", type=str, choices=("model", "input"), default="model",
                    help="write at 16 kHz (model) or at each file's own rate and frame count (input)")
    ap.add_argument("--seed", type=int, default=None, help="torch.manual_seed before the noise seeds are drawn")
    ap.add_argument("--window_frames", type=int, default=None,
                    help="enhance long recordings in overlapping windows of this many frames (a multiple of 64; 512 "
                         "= 8.2 s is the flagship shape); off by default")
    ap.add_argument("--overlap_frames", type=int, default=64,
                    help="frames over which neighbouring windows are cross-faded (with --window_frames)")
    hb = ap.add_mutually_exclusive_group()
    hb.add_argument("--highband", type=str, choices=resample.HIGHBAND_POLICIES, default="drop",
                    help="the band above 8 kHz of files at more than 16 kHz (with --output_rate input): drop it (as "
                         "before), keep it, or let it follow the network's attenuation of the top octave it saw")
    hb.add_argument("--highband_gain_db", type=float, default=None,
                    help="keep that band at this fixed gain in dB (<= 0) instead")
    ap.add_argument("--highband_floor_db", type=float, default=30.0,
                    help="the most --highband follow attenuates the band, in dB")
    ap.add_argument("--loudness", type=str, default="off",
                    help="off (as before), input (the integrated loudness of the noisy file) or a target in LUFS, e.g. "
                         "-23: one gain per file, applied on the device before the 16-bit conversion")
    ap.add_argument("--peak_db", type=float, default=-1.0,
                    help="ceiling in dB (<= 0) on the 4x-oversampled peak of a file written with --loudness")
    sampler_arguments(ap)
    return ap


def highband_argument(a):
    """The parsed --highband / --highband_gain_db pair -> enhance_batch's highband."""
    return a.highband if a.highband_gain_db is None else float(a.highband_gain_db)


def main(argv=None):
    a = parser().parse_args(argv)
    rank, world, _ = sdist.init_from_env()
    model = load_model(a.ckpt)
    if a.seed is not None:
        torch.manual_seed(a.seed)
    enhance_files(model, a.noisy_dir, a.destination_folder, batch_size=a.batch_size, output_rate=a.output_rate,
                  rank=rank, world=world, window_frames=a.window_frames, overlap_frames=a.overlap_frames,
                  highband=highband_argument(a), highband_floor_db=a.highband_floor_db, loudness=a.loudness,
                  peak_db=a.peak_db, **sampler_kwargs(a))


if __name__ == "__main__":
    main()
