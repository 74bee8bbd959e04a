"""eval_snr_est.py of the reference (lines 53-116) on the MI355X path.

    python -m snrse.evaluate_snr_est --test_dir DIR --ckpt CKPT [--destination_folder OUT] [--seed N]

Per file of DIR/noisy (clean twin in DIR/clean): centre crop / zero-pad both to 255 * 128 samples, draw
SNR ~ U(0, 40) dB, re-mix y = x + (y - x) 10^(-SNR / 20), normalise by max|y|, raw STFT (256 frames),
estimate g = SNRModel(Y) and compare 20 log10((1 - g) / g) with SNR - 5 (the reference's offset).  One
line per file as the reference prints; unlike the reference (which saves nothing) the per-file table goes to
OUT/_snr_est_results.csv and the mean absolute error to OUT/_snr_est_avg_results.txt.  The draws come from
numpy's RandomState(seed), one per file in sorted order.
"""
from __future__ import annotations

import argparse
import csv
import os
from glob import glob
from os.path import join

import numpy as np
import torch

NUM_FRAMES, HOP = 256, 128
SNR_OFFSET_DB = 5.0  # eval_snr_est.py:88


def mix_clip(x, y, snr_db, est_gt=None, num_frames=NUM_FRAMES, hop=HOP):
    """The host arithmetic of eval_snr_est.py:71-100, 113 on float32 tensors [..., L]: crop / pad to
    (num_frames - 1) * hop samples, re-mix at snr_db, normalise by max|y|.  Returns (y, real_db, est_db):
    the network input signal, the label SNR - 5 and, when est_gt is given, 20 log10((1 - est_gt) / est_gt)."""
    x, y = torch.as_tensor(x, dtype=torch.float32), torch.as_tensor(y, dtype=torch.float32)
    target_len = (num_frames - 1) * hop
    current_len = x.size(-1)
    pad = max(target_len - current_len, 0)
    if pad == 0:
        start = int((current_len - target_len) / 2)
        x = x[..., start:start + target_len]
        y = y[..., start:start + target_len]
    else:
        x = torch.nn.functional.pad(x, (pad // 2, pad // 2 + (pad % 2)), mode="constant")
        y = torch.nn.functional.pad(y, (pad // 2, pad // 2 + (pad % 2)), mode="constant")
    y = x + (y - x) * (10 ** (-snr_db / 20))
    y = y / y.abs().max()
    est_db = None
    if est_gt is not None:
        g = torch.as_tensor(est_gt, dtype=torch.float32)
        est_db = 20 * torch.log10((1 - g) / g)
    return y, snr_db - SNR_OFFSET_DB, est_db


def evaluate(model, test_dir, target_dir=None, seed=0, device="cuda"):
    from . import audio, ops
    rng = np.random.RandomState(seed)
    noisy_files = sorted(glob(join(test_dir, "noisy", "*.wav")))
    rows = []
    for noisy_file in noisy_files:
        name = os.path.basename(noisy_file)
        x, _ = audio.load(join(test_dir, "clean", name))
        y, _ = audio.load(noisy_file)
        snr = rng.rand() * 40
        yn, real, _ = mix_clip(x[:1], y[:1], snr)
        Y = ops.stft(yn.contiguous().to(device), 1.0, mode=0)  # raw STFT [1, 256, 256]
        with torch.no_grad():
            g = model.dnn.forward_complex(Y)[0, 0].cpu()
        est = float(mix_clip(x[:1], y[:1], snr, est_gt=g)[2])
        print("real:{0:.1f}/est:{1:.1f}".format(real, est))
        rows.append((name, real, est))
    mae = float(np.mean([abs(r - e) for _, r, e in rows])) if rows else float("nan")
    if target_dir:
        os.makedirs(target_dir, exist_ok=True)
        with open(join(target_dir, "_snr_est_results.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["filename", "real_snr_db", "est_snr_db"])
            w.writerows(rows)
        with open(join(target_dir, "_snr_est_avg_results.txt"), "w") as f:
            f.write("mean absolute SNR error: {0:.3f} dB over {1} files (seed {2})\n".format(mae, len(rows), seed))
    print("mean absolute SNR error: {0:.3f} dB".format(mae))
    return rows, mae


def main(argv=None):
    ap = argparse.ArgumentParser(description="eval_snr_est.py on the MI355X path")
    ap.add_argument("--destination_folder", type=str, default=None)
    ap.add_argument("--test_dir", type=str, required=True)
    ap.add_argument("--ckpt", type=str, required=True)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    from sgmse.snr_estimator import SNRModel
    model = SNRModel.load_from_checkpoint(args.ckpt, base_dir="", batch_size=1, num_workers=0, kwargs=dict(gpu=False))
    model.eval(no_ema=False)
    model.cuda()
    evaluate(model, args.test_dir, args.destination_folder, seed=args.seed)


if __name__ == "__main__":
    main()
