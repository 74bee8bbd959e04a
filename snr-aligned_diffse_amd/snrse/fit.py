"""The training loop: what pl.Trainer.fit does for the reference's train.py / train_snr_est.py, on the HIP path.

fit(model) runs epochs of model.training_step -> backward -> model.optimizer_step (the fused Adam + EMA launch,
with the device-side gradient clip when gradient_clip_val is set), validates, writes Lightning-layout
checkpoints (sgmse.ema.save_checkpoint) and a JSON-lines log.  The Trainer arguments that change the numbers
keep Lightning's meaning: accumulate_grad_batches (each micro-batch loss is divided by k, the optimizer steps
on every k-th batch and on the last one of the epoch), gradient_clip_val (clip_grad_norm_, norm_type 2),
check_val_every_n_epoch, limit_train_batches / limit_val_batches (int: that many batches, float: that
fraction), max_epochs / max_steps, and gpus: --gpus N trains data-parallel on N devices of one node, one process
per device, the gradients averaged over RCCL once per optimizer step (snrse.dist.GradReducer: one pack launch,
one all-reduce, no unpack), as the reference's DDPPlugin does; the global batch is N x batch_size x
accumulate_grad_batches and lr is not scaled.  Validation is sharded over the ranks, rank 0 alone writes
checkpoints and the log.  No bucketed overlap of the all-reduce with the backward, no multi-node run, no
data-loader workers, no W&B / TensorBoard.

Everything random in an epoch hangs off (seed, epoch): the order of the clips, numpy's generator (the crop
starts of Specs._crop) and torch's (the consistency step's grid indices and noise keys), so a run resumed from
the checkpoint of epoch e continues with the batches a straight run would have seen.  With more than one rank
(and with --batch_seeding on one) the generators are seeded per batch from (seed, epoch, global batch index)
instead, so a batch draws the same numbers whichever rank meets it.

    python -m snrse.fit --base_dir DIR --modeltype sebridge_v3 --snr_conditioned true --transform_type exponent \\
        --loss_type mse --sigma-max 1.0 --fixed_snr 0.17783 --num_eval_files -1 --ckpt_dir OUT [--max_epochs N ...]
    python -m snrse.fit --estimator --base_dir DIR --transform_type none --ckpt_dir OUT
    python -m snrse.fit ... --gpus 8        (or: torchrun --nproc_per_node 8 -m snrse.fit ...)
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


VAL_INDEX0 = 1 << 32   # seed_batch index of validation batch 0: far above any epoch's training batches
EVAL_INDEX = 1 << 33   # ... and of the evaluate_model pass


def seed_batch(seed, epoch, j):
    """Seed numpy and torch (CPU and device generators) from (seed, epoch, global batch index j): called before
    batch j is loaded and stepped, its crop starts, grid indices, noise keys and gt depend on the batch and not
    on which rank met it, or after which other batches."""
    import torch
    st = np.random.SeedSequence([int(seed) % 2 ** 64, int(epoch), int(j)]).generate_state(2)
    np.random.seed(int(st[0]))
    torch.manual_seed((int(st[0]) << 32) | int(st[1]))


def rank_batches(batches, rank, world):
    """Rank `rank`'s share of an epoch's batches: every rank gets the same count, local batch b is global batch
    b * world + rank, and the tail of fewer than `world` batches is dropped.  (Lightning's DistributedSampler
    pads the tail by repeating samples instead, so every sample is seen and a few are seen twice; here no
    sample is repeated and up to world - 1 batches of the epoch's permutation are left out.)"""
    world = max(1, int(world))
    return batches[:len(batches) // world * world][rank::world]


def check_supported(model_type, snr_conditioned):
    """The branches ScoreModel._step is built for; anything else is the error it raises, before any device work."""
    from sgmse.model import TRAIN_UNSUPPORTED
    if model_type != "sebridge_v3" or snr_conditioned not in ("true", "fixed"):
        raise NotImplementedError(TRAIN_UNSUPPORTED)


# ----------------------------------------------------------------------------- log
class _Log:
    """JSON lines, one per optimizer step and per validation (a non-finite value is written as null).  Step
    records hold device tensors until the next flush (every LOG_EVERY_N_STEPS steps and at the end of an epoch),
    so the loop reads nothing back in between; samples/s is the rate over the flushed span (global samples: all
    ranks').  Every record carries "world", the number of ranks of the run."""

    def __init__(self, path, world=1):
        self.path, self.pending, self.records, self.world = path, [], [], int(world)
        self.t0, self.samples = time.time(), 0
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def step(self, step, epoch, losses, grad_norm, samples):
        self.pending.append((step, epoch, losses, grad_norm))
        self.samples += samples

    def _write(self, rec):
        rec = {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in rec.items()}
        rec["world"] = self.world
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


def validate(model, limit_val_batches=None, rank=0, world=1, seeder=None, estoi=False):
    """One pass over the validation set with the EMA weights (Lightning puts the module in eval(), which the
    reference overrides to swap them in): valid_loss, the mean of validation_step over the clips; for a
    ScoreModel with num_eval_files != 0 also pesq / si_sdr / estoi (sgmse.util.inference.evaluate_model; not for
    snr_conditioned='fixed', which has no inference); for an SNRModel snr_error, the mean absolute error in dB.

    world > 1: rank r takes the batches r, r + world, ...; the fp64 sums (loss x count, error x count, count) are
    all-reduced, so the values are the full set's means on every rank.  evaluate_model runs on rank 0 alone and
    its three numbers are broadcast.  seeder(j), when given, is called before validation batch j with
    j = VAL_INDEX0 + batch number, and with EVAL_INDEX before evaluate_model (per-batch seeding).  estoi: the
    record's estoi is the device ESTOI of the chosen files (evaluate_model(estoi=True)) instead of NaN."""
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
        groups = _val_groups(n, dm.batch_size, limit_val_batches)
        for bi in range(rank, len(groups), world):
            idx = groups[bi]
            if seeder is not None:
                seeder(VAL_INDEX0 + bi)
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
    if world > 1:
        from . import dist as sdist, ops
        device = ops.current_device()
        tot, err, cnt = sdist.sum_over_ranks([tot, err, cnt], device)
    if cnt:
        out["valid_loss"] = tot / cnt
        if is_snr:
            out["snr_error"] = err / cnt
    if not is_snr and model.num_eval_files != 0 and model.snr_conditioned != "fixed":
        from sgmse.util.inference import evaluate_model
        three = None
        if rank == 0:
            if seeder is not None:
                seeder(EVAL_INDEX)
            three = evaluate_model(model, model.num_eval_files, estoi=True) if estoi else \
                evaluate_model(model, model.num_eval_files)
        if world > 1:
            # one NFE per file: not worth sharding yet; the other ranks wait here for rank 0's numbers
            three = sdist.broadcast_floats(three, 3, device, src=0)
        out["pesq"], out["si_sdr"], out["estoi"] = three
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
        seed=0, log_path=None, rank=0, world=1, batch_seeding=False, estoi=False):
    """Train `model` (a ScoreModel of the built branches or an SNRModel) on its data module's train set.
    -> dict(epoch, global_step, epochs_run, optimizer, history (the validation records), log (every record)).

    world > 1 (one process per rank, torch.distributed initialised, the rank's device current): data-parallel
    training as under Lightning's DDP.  Rank r steps the global batches r, r + world, ... (rank_batches) with its
    own accumulate_grad_batches = k micro-batches per optimizer step, the gradients are averaged over the ranks
    once per optimizer step (snrse.dist.GradReducer), so the global batch is world x batch_size x k and lr is not
    scaled; world = W with accumulation k walks the global batches of world = 1 with accumulation k W.  The clip
    and the Adam + EMA launch then run on gradients that are bit-identical on every rank, and so stay
    parameters, moments and shadows (checked once per epoch, dist.check_replicas).  Validation is sharded,
    rank 0 writes the checkpoints and the log.  batch_seeding (always on for world > 1): every batch is seeded
    from (seed, epoch, its global index) -- seed_batch -- so a one-rank run with batch_seeding=True and
    accumulation k W sees the batches, crops and draws of the W-rank run.  estoi: the validation records carry
    the device ESTOI (snrse.ops.estoi) of the evaluated files instead of null."""
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
    rank, world = int(rank), max(1, int(world))
    if not 0 <= rank < world:
        raise ValueError(f"snrse.fit: rank {rank} of world {world}")
    per_batch = bool(batch_seeding) or world > 1
    reducer = sdist = None
    if world > 1:
        from . import dist as sdist, ops
        if not sdist.dist.is_initialized() or sdist.dist.get_world_size() != world:
            raise RuntimeError(f"snrse.fit: world = {world} needs torch.distributed initialised with that many "
                               "ranks (snrse.dist.init_from_env() in every rank's process)")
        device = ops.current_device()
        # torch DDP's construction: every replica starts from rank 0's module state (after a resume, which
        # every rank loads onto its own device, this copies equal values)
        sdist.broadcast_tensors(list(model.state_dict().values()), device)
        name_of = {id(p): n for n, p in model.named_parameters()}
        reducer = sdist.GradReducer([(name_of.get(id(p)), p) for g in opt.param_groups for p in g["params"]],
                                    world, device)
    if ckpt_dir and rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    if sdist is not None:
        sdist.barrier()
    if ckpt_dir:
        best = _topk_files(ckpt_dir, monitor)
    log = _Log(log_path if rank == 0 else None, world)
    history, epochs_run, epoch, done = [], 0, epoch0 - 1, False
    n_train = len(dm.train_set)
    for epoch in range(epoch0, max_epochs if max_epochs is not None else 2 ** 31):
        if max_steps is not None and global_step >= max_steps:
            break
        if not per_batch:
            seed_epoch(seed, epoch)
        batches = epoch_batches(n_train, dm.batch_size, seed, epoch, limit_train_batches)
        if world > 1:
            batches = rank_batches(batches, rank, world)
        if not batches:
            raise ValueError(f"snrse.fit: {n_train} training clips give no batch of {dm.batch_size}"
                             + (f" for each of {world} ranks" if world > 1 else ""))
        stops = set(accumulation_steps(len(batches), k))
        opt.zero_grad()
        losses, samples = [], 0
        for bi, idx in enumerate(batches, 1):
            if per_batch:
                seed_batch(seed, epoch, (bi - 1) * world + rank)
            loss = model.training_step(dm.train_set.batch(idx), bi - 1)
            (loss / k if k > 1 else loss).backward()
            losses.append(loss.detach())
            samples += len(idx) * world
            if bi in stops:
                if reducer is not None:
                    # the step's loss rides in the gradient buffer's last slot: the mean over ranks at no
                    # second collective
                    mean = losses[0] if len(losses) == 1 else torch.stack(losses).mean()
                    losses = [reducer.reduce(opt, loss=mean).clone().reshape(())]
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
        if reducer is not None:
            reducer.check_replicas()  # one fp64 checksum per rank, compared as bits
        if check_val_every_n_epoch and (epoch + 1) % check_val_every_n_epoch == 0:
            metrics = validate(model, limit_val_batches, rank, world,
                               (lambda j, e=epoch: seed_batch(seed, e, j)) if per_batch else None,
                               **(dict(estoi=True) if estoi else {}))
            rec = dict(step=global_step, epoch=epoch, **metrics)
            history.append(rec)
            log.validation(rec)
        if ckpt_dir:
            if rank == 0:
                last = os.path.join(ckpt_dir, "last.ckpt")
                model.save_checkpoint(last, optimizer=opt, epoch=epoch, global_step=global_step, metrics=metrics)
                _save_topk(ckpt_dir, last, monitor, mode, metrics.get(monitor), epoch, best)
            if sdist is not None:
                sdist.barrier()  # the other ranks wait for the write
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
    tr.add_argument("--gpus", type=int, default=1,
                    help="data-parallel training on N devices of this node: one process per device, the gradients "
                         "averaged over RCCL once per optimizer step; the global batch is N x batch_size x "
                         "accumulate_grad_batches (under torchrun the launcher's WORLD_SIZE decides)")
    tr.add_argument("--batch_seeding", action="store_true",
                    help="seed every batch from (seed, epoch, global batch index), as a run on several devices "
                         "always does: a one-device run then reproduces a multi-device one")
    base.add_argument("--gpus", type=int, default=1)
    tr.add_argument("--estoi", action="store_true",
                    help="score the validation files with ESTOI on the device (snrse.ops.estoi): the validation "
                         "record's estoi is then a number instead of null")
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
    """--gpus N (N > 1) outside a torchrun environment: the parent starts N fresh interpreters
    (snrse.dist.spawn_ranks) before anything touches the GPU, and each runs this function again as its rank;
    under torchrun (WORLD_SIZE > 1 already set) the process is that rank directly."""
    parser, temp = build_parser(argv)
    if not temp.estimator:
        check_supported(temp.modeltype, temp.snr_conditioned)  # before anything that needs a device
    if temp.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        from . import dist as sdist
        rc = sdist.spawn_ranks(temp.gpus, main, (list(sys.argv[1:] if argv is None else argv),))
        if rc:
            sys.exit(f"snrse.fit: a rank ended with exit code {rc}")
        return None
    rank, world = 0, 1
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as tdist

        from . import dist as sdist
        rank, world, _ = sdist.init_from_env()
        if rank == 0 and sdist.oversubscribed(world):
            print(f"snrse.fit: {world} ranks on fewer devices: a rehearsal on shared devices over gloo, "
                  "not a measurement", file=sys.stderr, flush=True)
        try:
            return _run(parser, temp, argv, rank, world)
        finally:
            if tdist.is_initialized():
                tdist.destroy_process_group()
    return _run(parser, temp, argv, rank, world)


def _run(parser, temp, argv, rank, world):
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
              seed=args.seed, log_path=log_path, rank=rank, world=world, batch_seeding=args.batch_seeding,
              **(dict(estoi=True) if args.estoi else {}))
    if rank == 0:
        print(json.dumps({"epoch": res["epoch"], "global_step": res["global_step"], "ckpt_dir": ckpt_dir,
                          "last": res["history"][-1] if res["history"] else None}))
    return res


if __name__ == "__main__":
    try:
        main()
    except NotImplementedError as e:
        sys.exit(f"snrse.fit: {e}")
