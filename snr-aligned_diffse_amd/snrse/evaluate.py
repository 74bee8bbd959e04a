"""Evaluation driver: the loop of the reference's eval.py (eval.py:94-170) on the HIP path.

For every noisy file of <test_dir>/noisy (sorted): enhance with ScoreModel.enhance (PC or ODE
sampler), write <target_dir>/all/<name> (16-bit PCM, as soundfile's default for .wav), and
score it against <test_dir>/clean/<name>: PESQ (wide-band, 16 kHz) when the `pesq` package is
importable -- NaN otherwise, which is what the reference's try/except records on failure -- and
SI-SDR / SI-SIR / SI-SAR (utils.py:10-35, the columns the reference keeps commented out) from
the batched device kernel snrse_energy_ratios with n = y - x.  Results go to _results.csv and
_avg_results.txt ("mean ± std" over non-NaN values, utils.py:112-125).

--estoi adds ESTOI (Jensen & Taal 2016 with pystoi's conventions) as a fifth metric, computed on the device by
snrse.ops.estoi (csrc/estoi.hip) from the published definition: pystoi is not a dependency, parity with it is
unverified, and without the flag neither the column nor the computation exists.

Multi-GPU: files shard contiguously over ranks (snrse.dist.shard_range); the
per-file metric rows meet on every rank with one all_gather (RCCL over xGMI on the GPU box,
gloo in the CPU tests) and rank 0 writes the tables.

--batch_size B > 1 batches the rank's files: their lengths are read from the WAV headers, files whose
spectrograms pad to the same frame count share a ragged batch (snrse.batching.plan_batches), each batch is one
ScoreModel.enhance_batch call and one ragged snrse_energy_ratios launch.  Every file keeps the noise seed the
per-file loop would draw for it, so the results do not depend on B beyond GEMM summation order.  The default,
B = 1, is the per-file loop.  With --sampler_type ode a batch integrates every file with its own adaptive RK45
steps (snrse.enhance.ODEEnhancer); there B > 1 takes the prior from the per-file seeds, B = 1 from torch's device
generator, so the two are different noise realisations.

--resample: clean and noisy files whose header rate is not 16 kHz are brought to 16 kHz on the device
(snrse.resample.convert, the polyphase kernel snrse_resample_poly) as they are loaded; the enhancement, the written
files, the scoring and PESQ's rate are then those of 16 kHz signals.  Without the flag the rate is not looked at.

    python -m snrse.evaluate --test_dir DIR --ckpt CKPT --destination_folder OUT [--N 30 --batch_size 32 ...]
"""
from __future__ import annotations

import argparse
import os
from glob import glob
from os.path import join

import numpy as np
import torch

from . import audio, dist as sdist, ops
from .batching import pack_rows, plan_batches
from .sampler import draw_seed

METRICS = ("pesq", "si_sdr", "si_sir", "si_sar")


def _pesq_fn():
    try:
        from pesq import pesq  # noqa: WPS433  (optional: absent in this image)
    except ImportError:
        return None
    return pesq


def pesq_or_nan(fn, sr, ref, deg):
    """Wide-band PESQ of `deg` against `ref` through fn (_pesq_fn()); NaN without the package and for any failure,
    which is what the reference's try/except records (eval.py:147-150, deep_eval.py:134-137)."""
    if fn is None:
        return float("nan")
    try:
        return float(fn(sr, ref, deg, "wb"))
    except Exception:
        return float("nan")


def reverse_start(model, reverse_starting_point, N, force_N=0):
    """The drivers' prelude (eval.py:105-112): the reverse process starts at reverse_starting_point (OUVE keeps it
    in _T) -> its step count, N scaled by it unless force_N is given."""
    if model.sde.__class__.__name__ == "OUVESDE":
        model.sde._T = reverse_starting_point
    else:
        model.sde.T = reverse_starting_point
    N = int(reverse_starting_point / (1 / N))
    return force_N if force_N else N


def load_model(ckpt):
    """The checkpoint as the command lines run it: EMA weights, eval mode, on the device."""
    from sgmse.model import ScoreModel
    model = ScoreModel.load_from_checkpoint(ckpt, base_dir="", batch_size=16, num_workers=0, kwargs=dict(gpu=False))
    model.eval(no_ema=False)
    model.cuda()
    return model


def gather_table(rows, n_files, ncol, rank, world):
    """Every rank's per-file metric rows -> numpy [n_files, ncol] on every rank: one all_gather, on the device
    under nccl and on the CPU otherwise."""
    dev = ops.current_device() if world > 1 and sdist_backend_is_nccl() else torch.device("cpu")
    allm = sdist.gather_metrics(rows if rows else np.zeros((0, ncol)), n_files, rank, world, dev)
    return allm.reshape(n_files, ncol).cpu().numpy()


def print_mean_std(data, decimal=2):
    """utils.py:112-125: 'mean ± std' over the non-NaN values."""
    a = np.asarray(data, dtype=np.float64)
    a = a[~np.isnan(a)]
    if a.size == 0:
        return "nan ± nan"
    m, s = float(np.mean(a)), float(np.std(a))
    return f"{m:.3f} ± {s:.3f}" if decimal == 3 else f"{m:.2f} ± {s:.2f}"


def score_files(x_hat, x, y, sr=16000, pesq_fn=None):
    """One file's metric row (pesq, si_sdr, si_sir, si_sar); x_hat, x, y 1-D numpy float32."""
    L = min(len(x_hat), len(x), len(y))
    p = pesq_or_nan(pesq_fn, sr, x[:L], x_hat[:L])
    sig = torch.from_numpy(np.stack([x_hat[:L], x[:L], y[:L] - x[:L]]).astype(np.float32)).to(ops.current_device())
    er = ops.energy_ratios(sig[0:1], sig[1:2], sig[2:3])[0].cpu().numpy()
    return [p, float(er[0]), float(er[1]), float(er[2])]


def load_pair(clean_path, noisy_path, resample=False):
    """-> (x [channels, L], y [channels, L], sample rate) of one clean / noisy pair.  resample: a file whose rate is
    not 16 kHz is brought to it on the device, every channel a row of the one launch, and the rate returned is
    16000."""
    x, sr = audio.load(clean_path)
    y, sry = audio.load(noisy_path)
    if resample and (sr != audio.MODEL_RATE or sry != audio.MODEL_RATE):
        from .resample import convert
        rows = convert(list(x) + list(y), [sr] * len(x) + [sry] * len(y), audio.MODEL_RATE)
        x = torch.stack([torch.as_tensor(r) for r in rows[:len(x)]])
        y = torch.stack([torch.as_tensor(r) for r in rows[len(x):]])
        sr = audio.MODEL_RATE
    return x, y, sr


def evaluate(model, test_dir, target_dir, sampler_type="pc", predictor="reverse_diffusion", corrector="ald",
             corrector_steps=1, snr=0.5, N=30, reverse_starting_point=1.0, force_N=0, atol=1e-5, rtol=1e-5,
             timestep_type="linear", correct_stepsize=False, oracle=False, rank=0, world=1, batch_size=1,
             max_frames=16384, resample=False, estoi=False, **enhance_kw):
    """-> dict with 'filename' and METRICS lists (all files, every rank).  batch_size > 1: the rank's files run
    as ragged batches of at most batch_size rows and max_frames spectrogram frames (_evaluate_batched).

    sampler_type="ode" with batch_size > 1 runs ScoreModel.enhance_batch's ODE route: every file integrates with
    its own adaptive step sizes and draws its prior from its own Philox seed, so the results do not depend on
    batch_size as long as it is > 1 -- but they are a different noise realisation from batch_size = 1, whose
    per-file enhance() loop draws the prior from torch's device generator.

    estoi=True: every row gains a fifth value, the device ESTOI of the enhanced file against the clean one
    (estoi_batch -> snrse.ops.estoi; built from the published definition, parity with pystoi unverified), the
    dict an 'estoi' list, _results.csv an estoi column after si_sar and _avg_results.txt an ESTOI line.  Off, the
    default, nothing of it runs and the tables are the four-metric ones."""
    metrics = METRICS + ("estoi",) if estoi else METRICS
    clean_dir, noisy_dir = join(test_dir, "clean"), join(test_dir, "noisy")
    os.makedirs(join(target_dir, "all"), exist_ok=True)
    N = reverse_start(model, reverse_starting_point, N, force_N)
    clean_rms = noise_rms = None
    if oracle:  # per-file active RMS (eval.py:86-92 reads them from active_rms.txt)
        rows = [ln.split("\t") for ln in open(join(test_dir, "active_rms.txt")) if ln.strip()]
        clean_rms = [float(r[1]) for r in rows]
        noise_rms = [float(r[2]) for r in rows]
    files = sorted(glob(f"{noisy_dir}/*.wav"))
    a, b = sdist.shard_range(len(files), rank, world)
    pesq_fn = _pesq_fn()
    rows = []
    if batch_size > 1 and model._batch_route(sampler_type, corrector, enhance_kw) is None:
        batch_size = 1  # no batched enhancer for these settings (langevin, sebridge / sebridge_v2): the per-file loop
    if batch_size > 1:
        rows = _evaluate_batched(model, files, a, b, clean_dir, target_dir, pesq_fn, batch_size, max_frames,
                                 clean_rms, noise_rms, resample,
                                 dict(sampler_type=sampler_type, predictor=predictor, corrector=corrector,
                                      corrector_steps=corrector_steps, N=N, snr=snr, atol=atol, rtol=rtol,
                                      timestep_type=timestep_type, correct_stepsize=correct_stepsize, oracle=oracle,
                                      **enhance_kw), **(dict(estoi=True) if estoi else {}))
        a = b  # the per-file loop below has nothing left
    for i in range(a, b):
        name = os.path.basename(files[i])
        x, y, sr = load_pair(join(clean_dir, name), files[i], resample)
        x_hat = model.enhance(x, y, sampler_type=sampler_type, predictor=predictor, corrector=corrector,
                              corrector_steps=corrector_steps, N=N, snr=snr, atol=atol, rtol=rtol,
                              timestep_type=timestep_type, correct_stepsize=correct_stepsize, oracle=oracle,
                              clean_rms=clean_rms[i] if oracle else 1, noise_rms=noise_rms[i] if oracle else 1,
                              **enhance_kw)
        audio.write_wav(join(target_dir, "all", name), x_hat, 16000, bits=16)
        rows.append(score_files(np.asarray(x_hat, np.float32), x[0].numpy(), y[0].numpy(), sr, pesq_fn))
        if estoi:
            st = estoi_batch([np.asarray(x_hat, np.float32)], [x[0].numpy()], sr=sr)
            rows[-1] = list(rows[-1]) + [float(st[0])]
    allm = gather_table(rows, len(files), len(metrics), rank, world)
    data = {"filename": [os.path.basename(f) for f in files]}
    for k, m in enumerate(metrics):
        data[m] = [float(v) for v in allm[:, k]]
    if rank == 0:
        write_tables(data, target_dir)
    return data


def _upload_cropped(lists, Ls, dev=None):
    """Lists of files (each a list of 1-D numpy float32), file b cut to Ls[b] samples -> [len(lists), B, max L]
    float32 on the device, zero past each file's length: one upload."""
    return torch.stack([pack_rows([s[:L] for s, L in zip(sigs, Ls)])[0] for sigs in lists]).to(
        dev or ops.current_device())


def score_batch(x_hat, x, y, dev=None):
    """SI-SDR / SI-SIR / SI-SAR of a batch of files of different lengths (lists of 1-D numpy float32) in one
    ragged snrse_energy_ratios launch: one [3, B, max L] upload, n = y - x formed on the device, file b scored
    over its first L_b = min(len x_hat, len x, len y) samples as score_files does.  -> ([B, 3] numpy f64, [L_b])."""
    Ls = [min(len(h), len(c), len(n)) for h, c, n in zip(x_hat, x, y)]
    sd = _upload_cropped((x_hat, x, y), Ls, dev)
    return ops.energy_ratios(sd[0], sd[1], sd[2] - sd[1], lengths=Ls).cpu().numpy(), Ls


def estoi_batch(x_hat, x, dev=None, sr=16000):
    """ESTOI of a batch of files of different lengths (lists of 1-D numpy float32: enhanced, clean) at `sr` Hz in
    one ragged snrse.ops.estoi call: one [2, B, max L] upload, file b scored over its first
    L_b = min(len x_hat, len x) samples as score_files crops them.  -> [B] numpy f64 (one read-back)."""
    Ls = [min(len(h), len(c)) for h, c in zip(x_hat, x)]
    sd = _upload_cropped((x, x_hat), Ls, dev)
    return ops.estoi(sd[0], sd[1], lengths=Ls, fs=sr).cpu().numpy()


def _evaluate_batched(model, files, a, b, clean_dir, target_dir, pesq_fn, batch_size, max_frames, clean_rms,
                      noise_rms, resample, kw, estoi=False):
    """Metric rows of files [a, b), enhanced as ragged batches: lengths from the WAV headers, the plan, then per
    batch one load, one enhance_batch call, the 16-bit files and one ragged energy_ratios launch with n = y - x
    formed on the device; PESQ on the host, file by file.  The seeds are drawn first, one per file in file order:
    the draws of the per-file loop under the same torch RNG state."""
    idx = list(range(a, b))
    seeds = [draw_seed() for _ in idx]
    lens = [audio.info(files[i])[0] for i in idx]
    if resample:  # the plan is made of the 16 kHz lengths, still from the headers alone
        lens = [audio.resampled_length(L, audio.info(files[i])[2], audio.MODEL_RATE) for L, i in zip(lens, idx)]
    dev = ops.current_device()
    rows = [None] * len(idx)
    oracle = kw["oracle"]
    for batch in plan_batches(lens, batch_size, max_frames):
        names = [os.path.basename(files[idx[k]]) for k in batch]
        pairs = [load_pair(join(clean_dir, nm), files[idx[k]], resample) for nm, k in zip(names, batch)]
        xs = [(x, sr) for x, _, sr in pairs]
        ys = [y for _, y, _ in pairs]
        x_hat = model.enhance_batch([y[0] for y in ys], seeds=[seeds[k] for k in batch], batch_size=len(batch),
                                    max_frames=max_frames,
                                    clean_rms=[clean_rms[idx[k]] for k in batch] if oracle else None,
                                    noise_rms=[noise_rms[idx[k]] for k in batch] if oracle else None, **kw)
        for nm, h in zip(names, x_hat):
            audio.write_wav(join(target_dir, "all", nm), h, 16000, bits=16)
        er, Ls = score_batch(x_hat, [x[0].numpy() for x, _ in xs], [y[0].numpy() for y in ys], dev)
        for r, k in enumerate(batch):
            p = pesq_or_nan(pesq_fn, xs[r][1], xs[r][0][0, :Ls[r]].numpy(), x_hat[r][:Ls[r]])
            rows[k] = [p, float(er[r, 0]), float(er[r, 1]), float(er[r, 2])]
        if estoi:  # files of one batch may differ in rate without --resample: one call per rate
            for sr in sorted({s for _, s in xs}):
                sel = [r for r in range(len(batch)) if xs[r][1] == sr]
                st = estoi_batch([x_hat[r] for r in sel], [xs[r][0][0].numpy() for r in sel], dev, sr)
                for r, v in zip(sel, st):
                    rows[batch[r]].append(float(v))
    return rows


def sdist_backend_is_nccl():
    import torch.distributed as tdist
    return tdist.is_available() and tdist.is_initialized() and tdist.get_backend() == "nccl"


def write_tables(data, target_dir):
    """_results.csv (one row per file) and _avg_results.txt (eval.py:159-170); with an 'estoi' list in data, the
    estoi column after si_sar and the ESTOI line."""
    metrics = METRICS + ("estoi",) if "estoi" in data else METRICS
    with open(join(target_dir, "_results.csv"), "w") as f:
        f.write(",".join(["filename", *metrics]) + "\n")
        for i, name in enumerate(data["filename"]):
            f.write(",".join([name] + [repr(float(data[m][i])) for m in metrics]) + "\n")
    with open(join(target_dir, "_avg_results.txt"), "w") as f:
        f.write(f"PESQ: {print_mean_std(data['pesq'])} \n")
        f.write(f"SI-SDR: {print_mean_std(data['si_sdr'])} \n")
        f.write(f"SI-SIR: {print_mean_std(data['si_sir'])} \n")
        f.write(f"SI-SAR: {print_mean_std(data['si_sar'])} \n")
        if "estoi" in data:
            f.write(f"ESTOI: {print_mean_std(data['estoi'])} \n")


def sampler_arguments(ap, correct_stepsize=False):
    """The sampler options of eval.py (shared with snrse.enhance_files and, where --correct_stepsize defaults to
    on and --no_correct_stepsize turns it off, with snrse.deep_evaluate)."""
    ap.add_argument("--sampler_type", type=str, choices=("pc", "ode"), default="pc")
    ap.add_argument("--predictor", type=str, default="reverse_diffusion")
    ap.add_argument("--reverse_starting_point", type=float, default=1.0)
    ap.add_argument("--force_N", type=int, default=0)
    ap.add_argument("--corrector", type=str, choices=("ald", "none"), default="ald")
    ap.add_argument("--corrector_steps", type=int, default=1)
    ap.add_argument("--snr", type=float, default=0.5)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--atol", type=float, default=1e-5)
    ap.add_argument("--rtol", type=float, default=1e-5)
    ap.add_argument("--timestep_type", type=str, default="linear")
    ap.add_argument("--correct_stepsize", action="store_true", default=correct_stepsize)


def sampler_kwargs(a):
    """evaluate()'s sampler keywords from the parsed sampler_arguments."""
    return dict(sampler_type=a.sampler_type, predictor=a.predictor, corrector=a.corrector,
                corrector_steps=a.corrector_steps, snr=a.snr, N=a.N, reverse_starting_point=a.reverse_starting_point,
                force_N=a.force_N, atol=a.atol, rtol=a.rtol, timestep_type=a.timestep_type,
                correct_stepsize=a.correct_stepsize)


def main(argv=None):
    ap = argparse.ArgumentParser(description="eval.py on the MI355X path")
    ap.add_argument("--destination_folder", type=str, required=True)
    ap.add_argument("--test_dir", type=str, required=True)
    ap.add_argument("--ckpt", type=str, required=True)
    sampler_arguments(ap)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--resample", action="store_true",
                    help="bring clean / noisy files that are not at 16 kHz to 16 kHz on the device first")
    ap.add_argument("--batch_size", type=int, default=1,
                    help="files per ragged batch (1 = the per-file loop; files of one batch share their padded "
                         "frame count)")
    ap.add_argument("--estoi", action="store_true",
                    help="add the ESTOI column, computed on the device (snrse.ops.estoi; pystoi parity unverified)")
    a = ap.parse_args(argv)
    rank, world, _ = sdist.init_from_env()
    evaluate(load_model(a.ckpt), a.test_dir, a.destination_folder, **sampler_kwargs(a), oracle=a.oracle, rank=rank,
             world=world, batch_size=a.batch_size, resample=a.resample, **(dict(estoi=True) if a.estoi else {}))


if __name__ == "__main__":
    main()
