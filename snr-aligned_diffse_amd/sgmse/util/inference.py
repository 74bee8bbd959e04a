"""evaluate_model -- the enhancement metrics of the validation step (reference sgmse/util/inference.py:85-318,
called from model.py:408-429) on the HIP path.

The reference walks the chosen validation files one by one through a copy of enhance()'s branch for the
model type.  Here the files go through ScoreModel.enhance_batch (ragged batches on the batched enhancers,
the enhance() loop for the settings that have none), SI-SDR comes from one ragged snrse_energy_ratios launch
per call (snrse.evaluate.score_batch), PESQ from the `pesq` package where it is installed (NaN otherwise,
as snrse.evaluate) and ESTOI is NaN unless asked for (estoi=True: the device ESTOI of snrse.ops.estoi, built from
the published definition; pystoi is not a dependency and parity with it is unverified).
"""
from __future__ import annotations

import numpy as np
import torch


def eval_indices(total_num_files, num_eval_files):
    """The validation files evaluate_model picks (inference.py:97-103): num_eval_files indices spread evenly
    over [0, total), -1 meaning every file."""
    if num_eval_files == -1:
        num_eval_files = total_num_files
    return [int(i) for i in torch.linspace(0, total_num_files - 1, num_eval_files, dtype=torch.int)]


def evaluate_model(model, num_eval_files, batch_size=8, seeds=None, estoi=False, **enhance_kw):
    """-> (pesq, si_sdr, estoi), means over the chosen files of data_module.valid_set (valid_set_2 for
    snr_conditioned='fixed'), enhanced with the EMA weights (model.eval(no_ema=False)).  The live weights and
    train mode are back when it returns, also when enhance raises -- as it does for snr_conditioned='fixed'
    (NotImplementedError, model.py:792-793: that mode has no inference).  seeds: one noise seed per chosen
    file (default: drawn from the torch RNG in file order, the draws a loop of enhance() calls makes).
    estoi=True: the third value is the mean device ESTOI of the files (snrse.evaluate.estoi_batch, one ragged
    snrse.ops.estoi call; its parity with pystoi is unverified, the package being absent); False: NaN."""
    from snrse import audio
    from snrse.evaluate import _pesq_fn, pesq_or_nan, score_batch
    dm = model.data_module
    vs = dm.valid_set_2 if model.snr_conditioned == "fixed" else dm.valid_set
    idx = eval_indices(len(vs.clean_files), num_eval_files)
    if not idx:
        raise ValueError("evaluate_model: no validation files chosen")
    xs = [audio.load(vs.clean_files[i]) for i in idx]
    ys = [audio.load(vs.noisy_files[i])[0] for i in idx]
    model.eval(no_ema=False)
    try:
        x_hat = model.enhance_batch([y[0] for y in ys], seeds=seeds, batch_size=batch_size, **enhance_kw)
    finally:
        model.train(True)
    er, Ls = score_batch([np.asarray(h, np.float32) for h in x_hat], [x[0].numpy() for x, _ in xs],
                         [y[0].numpy() for y in ys])
    pesq_fn = _pesq_fn()
    pesq = [pesq_or_nan(pesq_fn, sr, x[0, :L].numpy(), np.asarray(h[:L])) for (x, sr), h, L in zip(xs, x_hat, Ls)]
    st = float("nan")
    if estoi:
        from snrse.evaluate import estoi_batch
        st = float(np.mean(estoi_batch([np.asarray(h, np.float32) for h in x_hat], [x[0].numpy() for x, _ in xs],
                                       sr=xs[0][1])))
    return float(np.mean(pesq)), float(np.mean(er[:, 0])), st


__all__ = ["evaluate_model", "eval_indices"]
