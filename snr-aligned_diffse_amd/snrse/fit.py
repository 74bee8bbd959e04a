"""The training loop: what pl.Trainer.fit does for the reference's train.py / train_snr_est.py, on the HIP path.

fit(model) runs epochs of model.training_step -> backward -> model.optimizer_step (the fused Adam + EMA launch,
with the device-side gradient clip when gradient_clip_val is set), validates, writes Lightning-layout
checkpoints (sgmse.ema.save_checkpoint) and a JSON-lines log.  The Trainer arguments that change the numbers
keep Lightning's meaning: accumulate_grad_batches (each micro-batch loss is divided by k, the optimizer steps
on every k-th batch and on the last one of the epoch), gradient_clip_val (clip_grad_norm_, norm_type 2),
check_val_every_n_epoch, limit_train_batches / limit_val_batches (int: that many batches, float: that
fraction), max_epochs / max_steps.  One device, no DDP, no W&B / TensorBoard.

Everything random in an epoch hangs off (seed, epoch): the order of the clips, numpy's generator (the crop
starts of Specs._crop) and torch's (the consistency step's grid indices and noise keys), so a run resumed from
the checkpoint of epoch e continues with the batches a straight run would have seen.

    python -m snrse.fit --base_dir DIR --modeltype sebridge_v3 --snr_conditioned true --transform_type exponent \\
        --loss_type mse --sigma-max 1.0 --fixed_snr 0.17783 --num_eval_files -1 --ckpt_dir OUT [--max_epochs N ...]
    python -m snrse.fit --estimator --base_dir DIR --transform_type none --ckpt_dir OUT
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import re
import shutil
import sys
import time

import numpy as np

LOG_EVERY_N_STEPS = 10  # train.py:109: the gradient norm is read back on these steps only
SAVE_TOP_K = 2          # train.py:100-101


# ----------------------------------------------------------------------------- schedules (host only)
def epoch_permutation(n, seed, epoch):
    """The order of the n training clips in `epoch`: a function of (seed, epoch) only."""
    return np.random.default_rng([int(seed), int(epoch)]).permutation(n)


def _limit(n, limit):
    """Lightning's limit_*_batches: None = all, int = that many, float = that fraction of the n batches."""
    if limit is None:
        return n
    if isinstance(limit, float):
        return min(n, int(n * limit))
    return min(n, int(limit))


def epoch_batches(n, batch_size, seed, epoch, limit=None):
    """Index groups of one epoch: the seeded permutation cut into batch_size groups, the remainder dropped."""
    perm = epoch_permutation(n, seed, epoch)
    groups = [[int(i) for i in perm[b:b + batch_size]] for b in range(0, n - batch_size + 1, batch_size)]
    return groups[:_limit(len(groups), limit)]


def accumulation_steps(n_batches, k):
    """1-based batch numbers after which the optimizer steps: every k-th and the epoch's last."""
    k = max(1, int(k))
    return [b for b in range(1, n_batches + 1) if b % k == 0 or b == n_batches]


def seed_epoch(seed, epoch):
    import torch
    s = (int(seed) * 1000003 + int(epoch)) % (2 ** 32)
    np.random.seed(s)
    torch.manual_seed(s)


def check_supported(model_type, snr_conditioned):
    """The branches ScoreModel._step is built for; anything else is the error it raises, before any device work."""
    from sgmse.model import TRAIN_UNSUPPORTED
    if model_type != "sebridge_v3" or snr_conditioned not in ("true", "fixed"):
        raise NotImplementedError(TRAIN_UNSUPPORTED)


# ----------------------------------------------------------------------------- log
class _Log:
    """JSON lines, one per optimizer step and per validation (a non-finite value is written as null).  Step
    records hold device tensors until the next flush (every LOG_EVERY_N_STEPS steps and at the end of an epoch),
    so the loop reads nothing back in between; samples/s is the rate over the flushed span."""

    def __init__(self, path):
        self.path, self.pending, self.records = path, [], []
        self.t0, self.samples = time.time(), 0
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def step(self, step, epoch, losses, grad_norm, samples):
        self.pending.append((step, epoch, losses, grad_norm))
        self.samples += samples

    def _write(self, rec):
        rec = {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in rec.items()}
        self.records.append(rec)
        if self.path:
            with open(self.path, "a") as f:
                f.write(json.dumps(rec) + "\n")

    def flush(self):
        if not self.pending:
            return
        import torch
        vals = [(s, e, float(torch.stack(ls).mean()), None if g is None else float(g)) for s, e, ls, g in self.pending]
        dt = max(time.time() - self.t0, 1e-9)
        for s, e, loss, g in vals:
            self._write({"step": s, "epoch": e, "train_loss": loss, "grad_norm": g,
                         "samples_per_s": self.samples / dt})
        self.pending, self.samples, self.t0 = [], 0, time.time()

    def validation(self, rec):
        self.flush()
        self._write(rec)
        self.t0 = time.time()


# ----------------------------------------------------------------------------- validation
def _val_groups(n, batch_size, limit):
    groups = [list(range(b, min(n, b + batch_size))) for b in range(0, n, batch_size)]
    return groups[:_limit(len(groups), limit)]


def validate(model, limit_val_batches=None):
    """One pass over the validation set with the EMA weights (Lightning puts the module in eval(), which the
    reference overrides to swap them in): valid_loss, the mean of validation_step over the clips; for a
    ScoreModel with num_eval_files != 0 also pesq / si_sdr / estoi (sgmse.util.inference.evaluate_model; not for
    snr_conditioned='fixed', which has no inference); for an SNRModel snr_error, the mean absolute error in dB."""
    import torch
    from sgmse.snr_estimator import SNRModel
    dm = model.data_module
    vs = dm.valid_set
    n = min(len(vs), len(vs.clean_rms))
    is_snr = isinstance(model, SNRModel)
    out = {}
    model.eval(no_ema=False)
    try:
        tot, err, cnt = 0.0, 0.0, 0
        for bi, idx in enumerate(_val_groups(n, dm.batch_size, limit_val_batches)):
            X, Y = vs.batch(idx)
            s = torch.tensor([vs.clean_rms[i] for i in idx], dtype=torch.float32)
            nz = torch.tensor([vs.noise_rms[i] for i in idx], dtype=torch.float32)
            loss = float(model.validation_step((X, Y, s, nz), bi))
            tot += loss * len(idx)
            if is_snr:
                err += model.snr_error * len(idx)
            cnt += len(idx)
    finally:
        model.train(True)
    if cnt:
        out["valid_loss"] = tot / cnt
        if is_snr:
            out["snr_error"] = err / cnt
    if not is_snr and model.num_eval_files != 0 and model.snr_conditioned != "fixed":
        from sgmse.util.inference import evaluate_model
        out["pesq"], out["si_sdr"], out["estoi"] = evaluate_model(model, model.num_eval_files)
    return out


# ----------------------------------------------------------------------------- checkpoints
def _topk_files(ckpt_dir, monitor):
    pat = re.compile(rf"epoch=(\d+)-{monitor}=(-?[\d.]+|-?inf|nan)\.ckpt$")
    found = []
    for f in glob.glob(os.path.join(ckpt_dir, f"epoch=*-{monitor}=*.ckpt")):
        m = pat.search(os.path.basename(f))
        if m:
            found.append((float(m.group(2)), f))
    return found


def _save_topk(ckpt_dir, last, monitor, mode, value, epoch, best):
    """Keep the SAVE_TOP_K best checkpoints by `monitor` as copies of the epoch's last.ckpt under train.py's
    naming; the ones that drop out are removed.  `best`: [(value, path)], updated in place."""
    if value is None or not math.isfinite(value):
        return
    path = os.path.join(ckpt_dir, f"epoch={epoch}-{monitor}={value:.2f}.ckpt")
    sign = -1.0 if mode == "max" else 1.0
    ranked = sorted(best + [(value, path)], key=lambda vp: sign * vp[0])
    keep, drop = ranked[:SAVE_TOP_K], ranked[SAVE_TOP_K:]
    if (value, path) in keep:
        shutil.copyfile(last, path)
    for _, p in drop:
        if p != path and os.path.exists(p):
            os.remove(p)
    best[:] = keep


# ----------------------------------------------------------------------------- the loop
def fit(model, max_epochs=None, max_steps=None, accumulate_grad_batches=1, gradient_clip_val=0.0,
        check_val_every_n_epoch=1, limit_train_batches=None, limit_val_batches=None, ckpt_dir=None, resume=None,
        seed=0, log_path=None):
    """Train `model` (a ScoreModel of the built branches or an SNRModel) on its data module's train set.
    -> dict(epoch, global_step, epochs_run, optimizer, history (the validation records), log (every record))."""
    import torch
    from sgmse.ema import resume_checkpoint
    from sgmse.snr_estimator import SNRModel
    is_snr = isinstance(model, SNRModel)
    if not is_snr:
        check_supported(model.model_type, model.snr_conditioned)
    if max_epochs is None and max_steps is None:
        max_epochs = 1000  # pl.Trainer's default
    if not torch.cuda.is_available():
        raise RuntimeError("snrse.fit: the training step runs on the HIP device (no CPU fallback)")
    k = max(1, int(accumulate_grad_batches))
    monitor, mode = ("valid_loss", "min") if is_snr else ("si_sdr", "max")
    dm = model.data_module
    dm.setup(stage="fit")
    model.cuda()
    model.train(True)
    opt = model.configure_optimizers()
    opt.clip_grad_norm = float(gradient_clip_val) if gradient_clip_val else None
    epoch0, global_step, best = 0, 0, []
    if resume:
        resume_checkpoint(model, resume, optimizer=opt)
        epoch0, global_step = model.resume["epoch"] + 1, model.resume["global_step"]
    if ckpt_dir:
        os.makedirs(ckpt_dir, exist_ok=True)
        best = _topk_files(ckpt_dir, monitor)
    log = _Log(log_path)
    history, epochs_run, epoch, done = [], 0, epoch0 - 1, False
    n_train = len(dm.train_set)
    for epoch in range(epoch0, max_epochs if max_epochs is not None else 2 ** 31):
        if max_steps is not None and global_step >= max_steps:
            break
        seed_epoch(seed, epoch)
        batches = epoch_batches(n_train, dm.batch_size, seed, epoch, limit_train_batches)
        if not batches:
            raise ValueError(f"snrse.fit: {n_train} training clips give no batch of {dm.batch_size}")
        stops = set(accumulation_steps(len(batches), k))
        opt.zero_grad()
        losses, samples = [], 0
        for bi, idx in enumerate(batches, 1):
            loss = model.training_step(dm.train_set.batch(idx), bi - 1)
            (loss / k if k > 1 else loss).backward()
            losses.append(loss.detach())
            samples += len(idx)
            if bi in stops:
                model.optimizer_step(opt)
                global_step += 1
                opt.zero_grad()
                norm = opt.last_grad_norm if global_step % LOG_EVERY_N_STEPS == 0 else None
                log.step(global_step, epoch, losses, norm, samples)
                losses, samples = [], 0
                if global_step % LOG_EVERY_N_STEPS == 0:
                    log.flush()
                if max_steps is not None and global_step >= max_steps:
                    done = True
                    break
        log.flush()
        epochs_run += 1
        metrics = {}
        if check_val_every_n_epoch and (epoch + 1) % check_val_every_n_epoch == 0:
            metrics = validate(model, limit_val_batches)
            rec = dict(step=global_step, epoch=epoch, **metrics)
            history.append(rec)
            log.validation(rec)
        if ckpt_dir:
            last = os.path.join(ckpt_dir, "last.ckpt")
            model.save_checkpoint(last, optimizer=opt, epoch=epoch, global_step=global_step, metrics=metrics)
            _save_topk(ckpt_dir, last, monitor, mode, metrics.get(monitor), epoch, best)
        if done:
            break
    torch.cuda.synchronize()
    return dict(epoch=epoch, global_step=global_step, epochs_run=epochs_run, optimizer=opt, history=history,
                log=log.records)


# ----------------------------------------------------------------------------- entry point
def _num(v):
    """limit_*_batches as Lightning reads it: an int count or a float fraction."""
    return float(v) if any(c in v for c in ".eE") else int(v)


def build_parser(argv=None):
    """train.py's parser (train.py:24-57) -- or train_snr_est.py's with --estimator -- with the Trainer arguments
    the loop implements.  Returns (parser, base args)."""
    base = argparse.ArgumentParser(add_help=False)
    parser = argparse.ArgumentParser(prog="python -m snrse.fit", description=__doc__.split("\n\n")[0])
    for p in (base, parser):
        p.add_argument("--estimator", action="store_true", help="train the SNR estimator (train_snr_est.py)")
        p.add_argument("--backbone", type=str, default=None)
        p.add_argument("--sde", type=str, default="ouve")
        p.add_argument("--nolog", action="store_true", help="no log file (development)")
        p.add_argument("--modeltype", type=str, choices=["bbed", "sebridge", "sebridge_v2", "sebridge_v3"],
                       default="bbed")
        p.add_argument("--snr_conditioned", type=str, choices=["false", "true", "fixed"], default="false")
        p.add_argument("--fixed_snr", type=float, default=1.0)
    tr = parser.add_argument_group("Trainer")
    tr.add_argument("--max_epochs", type=int, default=None)
    tr.add_argument("--max_steps", type=int, default=None)
    tr.add_argument("--gradient_clip_val", type=float, default=0.0)
    tr.add_argument("--accumulate_grad_batches", type=int, default=1)
    tr.add_argument("--check_val_every_n_epoch", type=int, default=1)
    tr.add_argument("--limit_train_batches", type=_num, default=None)
    tr.add_argument("--limit_val_batches", type=_num, default=None)
    tr.add_argument("--resume_from_checkpoint", type=str, default=None)
    tr.add_argument("--ckpt_dir", type=str, default=None, help="default ./savedir/<experiment name>")
    tr.add_argument("--gpus", type=int, default=1, help="accepted for train.py's command lines; one device runs")
    tr.add_argument("--seed", type=int, default=0)
    tr.add_argument("--log_path", type=str, default=None, help="default <ckpt_dir>/log.jsonl")
    temp, _ = base.parse_known_args(argv)
    return parser, temp


def _group(parser, args, title):
    for g in parser._action_groups:
        if g.title == title:
            return {a.dest: getattr(args, a.dest, None) for a in g._group_actions}
    return {}


def main(argv=None):
    parser, temp = build_parser(argv)
    if not temp.estimator:
        check_supported(temp.modeltype, temp.snr_conditioned)  # before anything that needs a device
    from sgmse.data_module import SpecsDataModule
    if temp.estimator:
        from sgmse.snr_estimator import SNRModel
        SNRModel.add_argparse_args(parser.add_argument_group("SNRModel"))
        SpecsDataModule.add_argparse_args(parser.add_argument_group("DataModule"))
        args = parser.parse_args(argv)
        model = SNRModel(backbone=args.backbone or "snrnet", data_module_cls=SpecsDataModule,
                         **{**_group(parser, args, "SNRModel"), **_group(parser, args, "DataModule")})
        name = "snr_estimator"
    else:
        from sgmse.backbones import BackboneRegistry
        from sgmse.model import ScoreModel
        from sgmse.sdes import SDERegistry
        backbone = temp.backbone or "ncsnpp"
        backbone_cls = BackboneRegistry.get_by_name(backbone)
        sde_cls = SDERegistry.get_by_name(temp.sde)
        ScoreModel.add_argparse_args(parser.add_argument_group("ScoreModel"))
        sde_cls.add_argparse_args(parser.add_argument_group("SDE"))
        backbone_cls.add_argparse_args(parser.add_argument_group("Backbone"))
        SpecsDataModule.add_argparse_args(parser.add_argument_group("DataModule"))
        args = parser.parse_args(argv)
        model = ScoreModel(backbone=backbone, sde=args.sde, model_type=args.modeltype,
                           snr_conditioned=args.snr_conditioned, data_module_cls=SpecsDataModule,
                           fixed_snr=args.fixed_snr,
                           **{**_group(parser, args, "ScoreModel"), **_group(parser, args, "SDE"),
                              **_group(parser, args, "Backbone"), **_group(parser, args, "DataModule")})
        name = f"{args.modeltype}_{args.snr_conditioned}{args.fixed_snr}_{args.sigma_max}"  # train.py:75-76
    ckpt_dir = args.ckpt_dir or os.path.join(".", "savedir", name)
    log_path = None if args.nolog else (args.log_path or os.path.join(ckpt_dir, "log.jsonl"))
    res = fit(model, max_epochs=args.max_epochs, max_steps=args.max_steps,
              accumulate_grad_batches=args.accumulate_grad_batches, gradient_clip_val=args.gradient_clip_val,
              check_val_every_n_epoch=args.check_val_every_n_epoch, limit_train_batches=args.limit_train_batches,
              limit_val_batches=args.limit_val_batches, ckpt_dir=ckpt_dir, resume=args.resume_from_checkpoint,
              seed=args.seed, log_path=log_path)
    print(json.dumps({"epoch": res["epoch"], "global_step": res["global_step"], "ckpt_dir": ckpt_dir,
                      "last": res["history"][-1] if res["history"] else None}))
    return res


if __name__ == "__main__":
    try:
        main()
    except NotImplementedError as e:
        sys.exit(f"snrse.fit: {e}")
