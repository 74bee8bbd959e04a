"""ScoreModel — inference half of the reference's sgmse/model.py (ScoreModel, 32-1016).

Same constructor / attribute / method surface that eval.py and deep_eval.py use
(load_from_checkpoint, eval(no_ema), sde, dnn, enhance, forward, get_pc_sampler, to_audio,
_stft, _istft, _forward_transform, _backward_transform, t_eps, sigma_max, fixed_snr,
model_type, snr_conditioned) on top of the HIP runtime, plus the consistency-training step of the paper's model
(_step / training_step / configure_optimizers / optimizer_step for sebridge_v3 with
snr_conditioned 'true' / 'fixed', SURVEY.md §8(f) 2, snrse/train.py), validation_step and
save_checkpoint for the training loop of snrse/fit.py.  The deep-inference validation block and
the dead debug helpers (enhance_debug, prior_tests2, get_prior) are out of scope.

Defined behaviour where the reference cannot run:
  * sebridge forward accepts t of shape [B] as well as [B,1,1,1] (the reference's
    t.squeeze(3) fails on the PC sampler's [B] time vector), so PC sampling works for every
    model_type;
  * enhance(timeit=True) reports nfe = 1 on the one-step branches (undefined in the reference);
  * the SNR-estimator checkpoint is loaded lazily on first use instead of at import (the
    reference loads './sgmse-bbed/sgmse/snr_estimator.ckpt' onto CUDA when the module is
    imported, model.py:25-30); its path can be overridden with SNRSE_SNR_CKPT.
"""
from __future__ import annotations

import contextlib
import os
import time
import warnings
from math import ceil

import numpy as np
import torch
import torch.nn as nn

from snrse import enhance as _enh
from snrse import guard as _guard
from snrse import ops
from snrse import sampler as _samp

from . import sampling
from .backbones import BackboneRegistry
from .data_module import SpecsDataModule
from .ema import EMAState, load_checkpoint
from .ema import save_checkpoint as _save_checkpoint
from .sdes import SDERegistry
from .util.other import pad_spec, pad_spec_16, snr_dB  # noqa: F401  (re-exported like the reference)

t_30 = _enh.T_30  # the reference's module-level time grid (model.py:22-23) under its name

# what ScoreModel._step and the training entry point (snrse.fit) say for the branches that are not built
TRAIN_UNSUPPORTED = ("the HIP training step is built for model_type='sebridge_v3' with "
                     "snr_conditioned 'true' / 'fixed' (the paper's consistency training)")

SNR_CKPT = os.environ.get("SNRSE_SNR_CKPT", "./sgmse-bbed/sgmse/snr_estimator.ckpt")
_snr_model = None


def get_snr_model():
    """The SNR estimator used by enhance() when snr_conditioned == 'true' and oracle is off."""
    global _snr_model
    if _snr_model is None:
        from .snr_estimator import SNRModel
        if not os.path.exists(SNR_CKPT):
            raise FileNotFoundError(f"SNR-estimator checkpoint not found at {SNR_CKPT}; set SNRSE_SNR_CKPT or "
                                    "call enhance(..., oracle=True, clean_rms=..., noise_rms=...)")
        m = SNRModel.load_from_checkpoint(SNR_CKPT, base_dir="", batch_size=1, num_workers=0)
        m.eval()
        _snr_model = m.to("cuda")
    return _snr_model


def set_snr_model(model):
    global _snr_model
    _snr_model = model


class ScoreModel(nn.Module):
    @staticmethod
    def add_argparse_args(parser):
        parser.add_argument("--lr", type=float, default=1e-4, help="The learning rate (1e-4 by default)")
        parser.add_argument("--ema_decay", type=float, default=0.999, help="The parameter EMA decay constant")
        parser.add_argument("--t_eps", type=float, default=0.03, help="The minimum time (3e-2 by default)")
        parser.add_argument("--num_eval_files", type=int, default=10)
        parser.add_argument("--loss_type", type=str, default="mse")
        parser.add_argument("--loss_abs_exponent", type=float, default=0.5)
        return parser

    def __init__(self, backbone, sde, model_type="sebridge", snr_conditioned="false", fixed_snr=1.0, lr=1e-4,
                 ema_decay=0.999, t_eps=3e-2, loss_abs_exponent=0.5, num_eval_files=10, loss_type="mse",
                 data_module_cls=None, **kwargs):
        super().__init__()
        self.dnn = BackboneRegistry.get_by_name(backbone)(**kwargs)
        if sde == "bbve":  # old checkpoints (model.py:67-74)
            sde = "bbed"
            kwargs["k"] = kwargs.pop("sigma_max")
            kwargs.pop("sigma_min", None)
            kwargs.setdefault("sigma_max", kwargs["k"])
        self.sde = SDERegistry.get_by_name(sde)(**kwargs)
        self.sigma_max = kwargs.get("sigma_max", getattr(self.sde, "sigma_max", None))
        self.model_type = model_type
        self.snr_conditioned = snr_conditioned
        self.fixed_snr = fixed_snr
        self.lr, self.ema_decay = lr, ema_decay
        self.ema = EMAState(self, ema_decay)
        self.t_eps = t_eps
        self.loss_type, self.num_eval_files, self.loss_abs_exponent = loss_type, num_eval_files, loss_abs_exponent
        self.hparams = dict(backbone=backbone, sde=sde, model_type=model_type, snr_conditioned=snr_conditioned,
                            fixed_snr=fixed_snr, t_eps=t_eps, **kwargs)
        dm = data_module_cls or SpecsDataModule
        self.data_module = dm(**{k: v for k, v in kwargs.items() if k != "fixed_snr"}, fixed_snr=self.fixed_snr,
                              gpu=kwargs.get("gpus", 0) > 0)

    # ------------------------------------------------------------------ checkpoints / EMA
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location="cpu", weights_only=None, optimizer=None,
                             **overrides):
        return load_checkpoint(cls, checkpoint_path, map_location, weights_only, overrides, optimizer=optimizer)

    def save_checkpoint(self, path, optimizer=None, epoch=0, global_step=0, metrics=None):
        """The Lightning checkpoint of this model (sgmse.ema.save_checkpoint): what load_from_checkpoint here
        and the reference's read.  hyper_parameters are the constructor's arguments (model.py:93
        save_hyperparameters), data_module_cls by name."""
        hp = dict(self.hparams, lr=self.lr, ema_decay=self.ema_decay, loss_abs_exponent=self.loss_abs_exponent,
                  num_eval_files=self.num_eval_files, loss_type=self.loss_type)
        return _save_checkpoint(self, path, hp, optimizer, epoch, global_step, metrics)

    def train(self, mode=True, no_ema=False):
        res = super().train(mode)
        self.ema.on_train(mode, no_ema)
        return res

    def eval(self, no_ema=False):
        return self.train(False, no_ema=no_ema)

    # ------------------------------------------------------------------ score
    def _score_mode(self):
        if self.snr_conditioned == "false" and self.model_type == "bbed":
            return 0
        if self.model_type in ("sebridge", "sebridge_v2", "sebridge_v3"):
            if self.snr_conditioned == "fixed" and self.model_type == "sebridge_v2":
                raise NotImplementedError("snr_conditioned='fixed' sebridge_v2 preconditioning (model.py:515-521)")
            return 1
        raise NotImplementedError(f"model_type={self.model_type!r} / snr_conditioned={self.snr_conditioned!r}")

    def forward(self, x, t, y, s=None):
        """Preconditioned score (model.py:481-543): -dnn for 'bbed', c_skip x + c_out dnn for sebridge*."""
        if s is not None:
            raise NotImplementedError("the sigma-conditioned forward needs NCSNpp_snr, which the reference "
                                      "cannot call either (model.py:541 vs ncsnpp_snr.py:264)")
        mode = self._score_mode()
        B = x.shape[0]
        tv = t.reshape(B, -1)[:, 0].to(torch.float32).contiguous()
        net = self.dnn.hip(x.device)
        xc = x.to(torch.complex64).reshape(B, x.shape[-2], x.shape[-1]).contiguous()
        yc = y.to(torch.complex64).reshape(B, y.shape[-2], y.shape[-1]).contiguous()
        return net.score(xc, yc, tv, mode)[:, None]

    def fused_score_step(self, Yc):
        """Step function for the PC loop: NCSN++ pyramid + output head + SDE update in one kernel."""
        return _enh.fused_step(self.dnn.hip(Yc.device), Yc, self._score_mode())

    # ------------------------------------------------------------------ training
    def configure_optimizers(self):
        """model.py:99-101: Adam(self.parameters(), lr) -- here the fused HIP Adam (snrse.train.FusedAdam)."""
        from snrse.train import FusedAdam
        return FusedAdam(self.parameters(), lr=self.lr)

    def optimizer_step(self, optimizer, *args, **kwargs):
        """model.py:103-106: the optimizer step, then the EMA update of the parameters; both run in the
        single fused launch (the EMA shadows are updated with torch_ema's decay schedule)."""
        optimizer.ema = self.ema
        optimizer.step()

    def _step(self, batch, batch_idx, valid=False, n=None, noise=None):
        """Consistency-training loss of one batch (model.py:159-394) for model_type 'sebridge_v3' with
        snr_conditioned 'true' (361-390) or 'fixed' (293-326), loss_type 'mse' / 'sqrt_mse'.
        batch: (x, y) clean / noisy spectrograms [B, 1, F, T] (a Specs batch; valid=True takes
        (x, y, s, n)).  n: grid indices [B] in 1..29 (default torch.randint(1, 30)); noise: the standard
        complex normal draw of torch.randn_like(x) [B, 1, F, T] (default: in-kernel Philox).  Returns the
        loss tensor; loss.backward() runs the HIP backward kernels and fills the parameters' .grad."""
        from snrse import train as _train
        if self.model_type != "sebridge_v3" or self.snr_conditioned not in ("true", "fixed"):
            raise NotImplementedError(TRAIN_UNSUPPORTED)
        self.data_module._check()
        x, y = batch[0], batch[1]
        B = x.shape[0]
        dev = ops.current_device()
        X = x.to(dev, torch.complex64).reshape(B, x.shape[-2], x.shape[-1]).contiguous()
        Y = y.to(dev, torch.complex64).reshape(B, y.shape[-2], y.shape[-1]).contiguous()
        if n is None:
            n = torch.randint(1, 30, (B,)).numpy()
        n = np.asarray(n.cpu() if torch.is_tensor(n) else n).reshape(B)
        if noise is None:
            coef = torch.tensor([[0.0, 0.0, 0.0, 1.0]] * B, device=dev)
            z = ops.axpby_noise(coef, like=X, seed=_samp.draw_seed())
        else:
            z = noise.to(dev, torch.complex64).reshape(X.shape).contiguous()
        return _train.consistency_loss(self.dnn, X, Y, n, z, float(self.sigma_max), self.loss_type,
                                       fixed_snr=float(self.fixed_snr) if self.snr_conditioned == "fixed" else None,
                                       transform=self.data_module.transform_type == "exponent")

    def training_step(self, batch, batch_idx):
        return self._step(batch, batch_idx, valid=False)

    def validation_step(self, batch, batch_idx):
        """model.py:402-404 without the Lightning logging: the loss of _step(valid=True), no autograd graph.
        The enhancement metrics of model.py:408-429 come from sgmse.util.inference.evaluate_model, which the
        training loop (snrse.fit) calls once per validation."""
        with torch.no_grad():
            return self._step(batch, batch_idx, valid=True)

    # ------------------------------------------------------------------ samplers
    def get_pc_sampler(self, predictor_name, corrector_name, y, Y_prior=None, N=None, minibatch=None,
                       timestep_type=None, **kwargs):
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, **kwargs}
        if minibatch is None:
            return sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, Y=y,
                                           Y_prior=Y_prior, timestep_type=timestep_type, **kwargs)
        M = y.shape[0]

        def batched_sampling_fn():
            samples, ns = [], []
            for i in range(int(ceil(M / minibatch))):
                y_mini = y[i * minibatch:(i + 1) * minibatch]
                yp = None if Y_prior is None else Y_prior[i * minibatch:(i + 1) * minibatch]
                sampler = sampling.get_pc_sampler(predictor_name, corrector_name, sde=sde, score_fn=self, Y=y_mini,
                                                  Y_prior=yp, **kwargs)
                sample, n = sampler()
                samples.append(sample)
                ns.append(n)
            return torch.cat(samples, dim=0), ns

        return batched_sampling_fn

    def get_ode_sampler(self, y, Y_prior=None, N=None, minibatch=None, timestep_type=None, **kwargs):
        """model.py:574-595.  As in the reference, the minibatched variant returns the LAST
        minibatch's sample (`return sample, ns`, model.py:594) -- kept for drop-in behaviour."""
        N = self.sde.N if N is None else N
        sde = self.sde.copy()
        sde.N = N
        kwargs = {"eps": self.t_eps, **kwargs}
        if minibatch is None:
            return sampling.get_ode_sampler(sde, self, y=y, Y_prior=Y_prior, timestep_type=timestep_type, **kwargs)
        M = y.shape[0]

        def batched_sampling_fn():
            samples, ns = [], []
            sample = None
            for i in range(int(ceil(M / minibatch))):
                y_mini = y[i * minibatch:(i + 1) * minibatch]
                sampler = sampling.get_ode_sampler(sde, self, y=y_mini, **kwargs)
                sample, n = sampler()
                samples.append(sample)
                ns.append(n)
            return sample, ns

        return batched_sampling_fn

    # ------------------------------------------------------------------ spectrogram glue
    def to_audio(self, spec, length=None):
        return self._istft(self._backward_transform(spec), length)

    def _forward_transform(self, spec):
        return self.data_module.spec_fwd(spec)

    def _backward_transform(self, spec):
        return self.data_module.spec_back(spec)

    def _stft(self, sig):
        return self.data_module.stft(sig)

    def _istft(self, spec, length=None):
        return self.data_module.istft(spec, length)

    def calculate_snr_direct(self, s, n, fixed_snr):
        return (n / s) / (10 ** 0.25 * fixed_snr)

    def calculate_normfac_direct(self, s, n, fixed_snr):
        return 2.040166 * (0.240253 + 0.759747 * fixed_snr ** 2) ** 0.5 / ((1 + (n / s) ** 2) ** 0.5)

    # ------------------------------------------------------------------ enhance
    @torch.no_grad()
    def enhance(self, x, y, sampler_type="pc", predictor="reverse_diffusion", corrector="ald", N=30,
                corrector_steps=1, snr=0.5, timeit=False, oracle=False, clean_rms=1, noise_rms=1, range_guard="auto",
                **kwargs):
        """One-call enhancement of noisy speech y [1, L] (model.py:702-839) -> numpy [L].

        range_guard (snrse.guard policies; "auto" = "fallback" when the backbone's compute_dtype is fp16, off
        otherwise): the spectrogram is checked before the iSTFT; when fp16 could not hold the utterance (it is all
        NaN then) the same branch runs again with the backbone in RANGE_FALLBACK ("bf16") under the torch RNG state
        saved at entry, so the result is what a bf16 model returns under the same torch.manual_seed.  The fallback
        is sticky: after the first hit this model runs the fallback format for the rest of the process and has
        warned once, so a loop over the files of such a checkpoint does not pay twice per file."""
        start = time.time()
        # the checkpoint's data-module hparams pick the front / back end (_forward_transform(_stft(.)),
        # model.py:749, to_audio 612-613): fused exponent transform or raw, anything else raises
        mode = self.data_module.hip_mode()
        if self.snr_conditioned == "fixed":
            # model.py:792-793: the reference refuses inference for this training-only mode (it raises after
            # the STFT, before any network call; here before any device work)
            raise NotImplementedError("snr fixed is only for experiment purpose, not real inference.")
        if self.snr_conditioned not in ("true", "false"):
            # the reference falls through every branch and fails on the unbound `sample` (model.py:826)
            raise NotImplementedError(f"snr_conditioned={self.snr_conditioned!r} has no enhance branch")
        dev = ops.current_device()
        T_orig = y.size(1)
        yd = y.to(dev, torch.float32).reshape(1, -1).contiguous()
        nf = ops.absmax(yd)  # norm_factor = max|y| (model.py:726), taken once: a fallback run divides by the same
        noise_tape = kwargs.get("noise_tape")

        def run():
            """The network part: normalised utterance -> (enhanced spectrogram [1, F, Tp], nfe, iSTFT scale), in
            the backbone's current compute_dtype."""
            nfe, div = 1, nf
            if self.snr_conditioned == "true":
                if self.model_type != "sebridge_v3":
                    raise NotImplementedError("snr_conditioned='true' is implemented for model_type='sebridge_v3' "
                                              "(the sebridge_v2 branch needs the 3-argument NCSNpp_snr)")
                if oracle:
                    est_snr = float(noise_rms) / float(clean_rms)  # model.py:722-724
                else:  # y / max|y|, raw STFT, pad_spec_16
                    raw = ops.stft(yd, 1.0, tpad=_enh.pad_frames(1 + T_orig // 128, 16), mode=0, in_div=nf)
                    est_snr = float(get_snr_model().estimate_from_spec(raw)[0])
                # calculate_snr_direct snapped to t_30, calculate_normfac_direct there (model.py:734-736, 810-817)
                t_hat = float(_enh.snap_t(est_snr, self.fixed_snr)[0])
                div = nf * float(_enh.normfac(t_hat, self.fixed_snr))
                Y = _enh.front_end(yd, mode, div=div)[0]
                Z = noise_tape(0) if noise_tape is not None else None
                coef = torch.tensor([[0.0, 1.0, 0.0, float(self.sigma_max) * t_hat]], device=dev)
                X_T = ops.axpby_noise(coef, y=Y, noise=Z, seed=_samp.draw_seed())
                sample = self(X_T[:, None], torch.full((1, 1, 1, 1), t_hat, device=dev), Y[:, None])[:, 0]
                return sample, nfe, div
            Y = _enh.front_end(yd, mode, div=div)[0]
            if self.model_type == "bbed":
                if sampler_type == "pc":
                    sampler = self.get_pc_sampler(predictor, corrector, Y[:, None], N=N,
                                                  corrector_steps=corrector_steps, snr=snr, noise_tape=noise_tape)
                elif sampler_type == "ode":
                    sampler = self.get_ode_sampler(Y[:, None], N=N, **kwargs)
                else:
                    raise ValueError(f"{sampler_type} is not a valid sampler type!")
                sample, nfe = sampler()
                sample = sample[:, 0]
            elif self.model_type in ("sebridge", "sebridge_v2"):
                t = 0.999
                zs = 0.0 if self.model_type == "sebridge" else float(self.sigma_max) * t
                Z = noise_tape(0) if (noise_tape is not None and zs) else None
                X_T = ops.axpby_noise(torch.tensor([[0.0, 1.0, 0.0, zs]], device=dev), y=Y, noise=Z,
                                      seed=_samp.draw_seed())
                sample = self(X_T[:, None], torch.full((1, 1, 1, 1), t, device=dev), Y[:, None])[:, 0]
            else:
                raise NotImplementedError(f"model_type={self.model_type!r} with snr_conditioned='false'")
            return sample, nfe, div

        fmt = self.dnn.compute_dtype
        policy = _guard.resolve(range_guard, torch.float16 if fmt in ("fp16", torch.float16) else None)
        if policy == "fallback" and self._range_fallback:
            with self._compute_format(self.RANGE_FALLBACK):
                sample, nfe, out_scale = run()
            self.last_guard = {"flagged": [], "policy": policy, "fallback_dtype": self.RANGE_FALLBACK, "sticky": True}
        else:
            rng = (torch.get_rng_state(), torch.cuda.get_rng_state(dev)) if policy == "fallback" else None
            sample, nfe, out_scale = run()
            rows = _guard.flagged_rows(sample.contiguous()) if policy != "off" else []
            if _guard.report(self, rows, policy, self.RANGE_FALLBACK, fmt):
                self._range_fallback = True
                torch.set_rng_state(rng[0])
                torch.cuda.set_rng_state(rng[1], dev)
                with self._compute_format(self.RANGE_FALLBACK):
                    sample, nfe, out_scale = run()
        x_hat = _enh.back_end(sample, T_orig, mode, out_scale.reshape(1))[0].cpu().numpy()
        if timeit:
            rtf = (time.time() - start) / (len(x_hat) / 16000)
            return x_hat, nfe, rtf
        return x_hat

    def _batch_route(self, sampler_type, corrector, kwargs):
        """Which batched enhancer serves these settings: "pc", "ode", "snr", or None (the per-utterance loop)."""
        if "noise_tape" in kwargs:
            return None
        if self.snr_conditioned == "true" and self.model_type == "sebridge_v3":
            return "snr"
        if (self.snr_conditioned == "false" and self.model_type == "bbed" and sampler_type == "pc"
                and corrector in ("ald", "none")):
            return "pc"
        if self.snr_conditioned == "false" and self.model_type == "bbed" and sampler_type == "ode":
            return "ode"  # the corrector plays no part in the probability-flow ODE
        return None  # the batch-mean `langevin` corrector, sebridge / sebridge_v2

    def batched_enhancer(self, route, net, range_guard="auto", predictor="reverse_diffusion", corrector="ald", N=30,
                         corrector_steps=1, snr=0.5, oracle=False, rtol=1e-5, atol=1e-5):
        """The snrse.enhance enhancer of a _batch_route `route` on the executor `net` (self.dnn.hip(dev)), set up
        from this model's SDE, t_eps, fixed_snr, sigma_max and data-module transform."""
        common = dict(transform="exponent" if self.data_module.hip_mode() == 1 else "none", guard=range_guard)
        if route == "pc":
            return _enh.PCEnhancer(net, self.sde.copy().spec(), N=N, eps=self.t_eps, snr=snr, predictor=predictor,
                                   corrector=corrector, corrector_steps=corrector_steps,
                                   score_mode=self._score_mode(), **common)
        if route == "ode":
            return _enh.ODEEnhancer(net, self.sde.copy().spec(), eps=self.t_eps, rtol=rtol, atol=atol,
                                    score_mode=self._score_mode(), **common)
        snr_fn = None if oracle else (lambda raw: get_snr_model().estimate_from_spec(raw))
        return _enh.SNRAlignedEnhancer(net, snr_fn=snr_fn, fixed_snr=float(self.fixed_snr),
                                       sigma_max=float(self.sigma_max), **common)

    @torch.no_grad()
    def enhance_batch(self, ys, seeds=None, batch_size=32, max_frames=16384, sampler_type="pc",
                      predictor="reverse_diffusion", corrector="ald", N=30, corrector_steps=1, snr=0.5, oracle=False,
                      clean_rms=None, noise_rms=None, range_guard="auto", sample_rates=None, output_rate="model",
                      window_frames=None, overlap_frames=64, highband="drop", highband_floor_db=30.0, **kwargs):
        """enhance() for a list of noisy utterances of different lengths (each [L], [1, L], numpy or tensor) ->
        list of numpy [L_i] in input order.  Utterances whose spectrograms pad to the same frame count share a
        ragged batch (snrse.batching.plan_batches: at most batch_size rows and max_frames frames per batch).

        seeds: one noise seed per utterance; None draws one torch.randint(0, 2**62) each, in input order and before
        any device work -- the draws a loop of enhance() calls makes, so under the same torch.manual_seed the
        results are that loop's up to GEMM summation order, whatever batch_size is.  The PC sampler of a 'bbed'
        model with the `ald` / `none` corrector runs on PCEnhancer and the SNR-conditioned 'sebridge_v3' one-step
        model on SNRAlignedEnhancer (oracle=True takes clean_rms / noise_rms as sequences); every other setting
        (`langevin`, whose step size is a batch mean, sebridge / sebridge_v2, a noise_tape) loops
        over enhance() and returns what it returns (seeds is not used there).  range_guard: enhance()'s
        policies; "fallback" recomputes the flagged rows of a batch with the bf16 executor.

        sampler_type="ode" on a 'bbed' model runs on ODEEnhancer: every row integrates the probability-flow ODE
        with its own adaptive step sizes (kwargs rtol / atol, default 1e-5 as get_ode_sampler; N, timestep_type
        and correct_stepsize are accepted and ignored).  Its prior is drawn from the per-utterance Philox seeds
        like the PC route's, so the results do not depend on batch_size -- but they are a different noise
        realisation from a loop over enhance(sampler_type="ode"), whose prior comes from torch's device
        generator (sde.prior_sampling).

        sample_rates: None (every utterance is at the model's 16 kHz; output_rate is not looked at), or one rate per
        utterance: those not at 16 kHz are resampled on the device first (snrse.resample.convert: one ragged
        ops.resample_poly launch per distinct rate), and everything above -- the batch plan, max|y|, the results'
        lengths -- is that of the 16 kHz signals, resampled_length(L_i, rate_i, 16000) samples each.  The seeds
        are drawn as without it, before any device work.  output_rate "model" returns the 16 kHz waveforms,
        "input" resamples each back to its own rate and cuts it to exactly L_i samples.

        window_frames: None (every utterance is one network input, however long), or the frame count of a window
        (a multiple of 64; 512 is the flagship shape): recordings of any length.  Every utterance is cut, at 16 kHz
        and on the device, into overlapping windows (snrse.longform: one window when it has at most
        (window_frames - 1) 128 samples, and then its result is bit for bit the unwindowed one), the windows of all
        utterances run as rows of the same batched enhancers -- each with its own max|y|, SNR estimate and seed
        (the utterance's for its window 0, longform.window_seed(seed, k) for window k) -- and one
        ops.window_merge launch cross-fades them over overlap_frames frames.  No enhancer call sees more than
        batch_size rows or max_frames frames, so device memory does not grow with the recording beyond about three
        copies of its samples.  A window of digital silence (max|y| = 0) is not sent to the network and counts as
        zeros.  last_guard["flagged"] lists utterances as before, last_guard["flagged_windows"] the
        (utterance, window) pairs.

        highband (with sample_rates and output_rate="input" only; anything else but "drop" raises before any device
        work): what becomes of the band above 8 kHz of a recording at more than 16 kHz, which the networks never
        see.  "drop" (the default) resamples the result back as before, bit for bit.  "keep" adds the recording's
        own band back unchanged, a float adds it at that gain in dB (<= 0), and "follow" attenuates it frame by
        frame as much as the network attenuated the top octave it saw (4 - 8 kHz), by at most highband_floor_db dB
        (snrse.resample.restore_highband: out = U(x) + g (y - U(u)), one ops.resample_mix launch per distinct
        rate; include/snrse.h has the definition).  It costs two more copies of the call's recordings at their
        own rates on the device while the results are mixed.  Recordings at 16 kHz or below are not affected."""
        from snrse import batching
        hb = "drop"
        if not (isinstance(highband, str) and highband == "drop"):  # the default stays clear of snrse.resample
            from snrse import resample as _rs
            hb = _rs.check_highband(highband, highband_floor_db, sample_rates, output_rate)
        if window_frames is not None:
            return self._enhance_windowed(ys, seeds, batch_size, max_frames, sample_rates, output_rate,
                                          window_frames, overlap_frames, oracle, clean_rms, noise_rms, range_guard,
                                          dict(sampler_type=sampler_type, predictor=predictor, corrector=corrector,
                                               N=N, corrector_steps=corrector_steps, snr=snr), kwargs,
                                          hb, highband_floor_db)
        n = len(ys)
        route = self._batch_route(sampler_type, corrector, kwargs)
        if sample_rates is not None:
            from snrse import audio, resample
            if output_rate not in ("model", "input"):
                raise ValueError(f"enhance_batch: output_rate is 'model' or 'input', got {output_rate!r}")
            if len(sample_rates) != n:
                raise ValueError(f"enhance_batch: {len(sample_rates)} sample rates for {n} utterances")
            if seeds is None and route is not None:
                seeds = [_samp.draw_seed() for _ in range(n)]
            lens_in = [int(resample.as_signal(y).numel()) for y in ys]
            if hb == "follow":
                resample.check_follow_lengths(lens_in, sample_rates)
            # the batched enhancers gather their ragged batches on the device, where the resampled rows already are
            ys16 = resample.convert(ys, sample_rates, audio.MODEL_RATE, on_device=route is not None)
            out = self.enhance_batch(ys16, seeds=seeds, batch_size=batch_size, max_frames=max_frames,
                                     sampler_type=sampler_type, predictor=predictor, corrector=corrector, N=N,
                                     corrector_steps=corrector_steps, snr=snr, oracle=oracle, clean_rms=clean_rms,
                                     noise_rms=noise_rms, range_guard=range_guard, **kwargs)
            if output_rate == "input" and hb != "drop":  # the ys16 of above serve as the band split's 16 kHz side
                out = resample.restore_highband(out, ys16, ys, sample_rates, hb, highband_floor_db)
            elif output_rate == "input":
                back = resample.convert(out, audio.MODEL_RATE, sample_rates)
                out = [np.asarray(h)[:L] for h, L in zip(back, lens_in)]
            return out
        if route is None:
            out = []
            for i, y in enumerate(ys):
                y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).reshape(1, -1)
                out.append(self.enhance(y, y, sampler_type=sampler_type, predictor=predictor, corrector=corrector,
                                        N=N, corrector_steps=corrector_steps, snr=snr, oracle=oracle,
                                        clean_rms=clean_rms[i] if oracle else 1,
                                        noise_rms=noise_rms[i] if oracle else 1, range_guard=range_guard, **kwargs))
            return out
        if seeds is None:
            seeds = [_samp.draw_seed() for _ in range(n)]
        if len(seeds) != n:
            raise ValueError(f"enhance_batch: {len(seeds)} seeds for {n} utterances")
        if oracle and (clean_rms is None or noise_rms is None or len(clean_rms) != n or len(noise_rms) != n):
            raise ValueError("enhance_batch(oracle=True) takes clean_rms and noise_rms, one value per utterance")
        self.data_module.hip_mode()  # a configuration the kernels are not built for fails before any device work
        sigs = [torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(torch.float32).reshape(-1)
                for y in ys]
        lens = [int(s.numel()) for s in sigs]
        plan = batching.plan_batches(lens, batch_size, max_frames)
        dev = ops.current_device()
        out = [None] * n
        with self._compute_format(self.RANGE_FALLBACK if self._range_fallback else self.dnn.compute_dtype):
            enh = self.batched_enhancer(route, self.dnn.hip(dev), range_guard, predictor, corrector, N,
                                        corrector_steps, snr, oracle, kwargs.get("rtol", 1e-5),
                                        kwargs.get("atol", 1e-5))
            flagged = []
            ode_stats = self.last_ode_stats = []
            for rows in plan:
                # rows resampled on the device (sample_rates) are packed there: all of a call's rows are, or none
                buf, ln = batching.pack_rows([sigs[i] for i in rows])
                yb = buf.to(dev)
                rs = torch.tensor([seeds[i] for i in rows], dtype=torch.int64, device=dev)
                if route in ("pc", "ode"):
                    xb, nfe = enh(yb, noise=_samp.NoiseSource(row_seeds=rs), lengths=ln)
                    if route == "ode":
                        ode_stats.append(dict(enh.last_stats, files=list(rows), nfev=[int(v) for v in nfe]))
                else:
                    est = [float(noise_rms[i]) / float(clean_rms[i]) for i in rows] if oracle else None
                    xb, _ = enh(yb, est_snr=est, lengths=ln, row_seeds=rs)
                flagged += [rows[r] for r in (enh.last_guard or {}).get("flagged", [])]
                xb = xb.cpu().numpy()
                for r, i in enumerate(rows):
                    out[i] = xb[r, :lens[i]].copy()
            self.last_guard = dict(enh.last_guard or {}, flagged=sorted(flagged))
        return out

    def _enhance_windowed(self, ys, seeds, batch_size, max_frames, sample_rates, output_rate, window_frames,
                          overlap_frames, oracle, clean_rms, noise_rms, range_guard, skw, kwargs, highband="drop",
                          highband_floor_db=30.0):
        """enhance_batch(window_frames=...): plan (snrse.longform) -> one gather -> the windows through the route's
        enhancer, batch by batch, their results written back over the windows -> one merge.  skw: the sampler
        keywords of enhance()."""
        from snrse import audio, batching, longform, resample
        W, V, _ = longform.geometry(window_frames, overlap_frames)  # bad arguments fail before any device work
        n = len(ys)
        route = self._batch_route(skw["sampler_type"], skw["corrector"], kwargs)
        if sample_rates is not None:
            if output_rate not in ("model", "input"):
                raise ValueError(f"enhance_batch: output_rate is 'model' or 'input', got {output_rate!r}")
            if len(sample_rates) != n:
                raise ValueError(f"enhance_batch: {len(sample_rates)} sample rates for {n} utterances")
        if route is not None and seeds is None:
            seeds = [_samp.draw_seed() for _ in range(n)]
        if route is not None and len(seeds) != n:
            raise ValueError(f"enhance_batch: {len(seeds)} seeds for {n} utterances")
        if oracle and (clean_rms is None or noise_rms is None or len(clean_rms) != n or len(noise_rms) != n):
            raise ValueError("enhance_batch(oracle=True) takes clean_rms and noise_rms, one value per utterance")
        self.data_module.hip_mode()
        if n == 0:
            return []
        sigs = [resample.as_signal(y) for y in ys]
        lens_in = [int(s.numel()) for s in sigs]
        if highband == "follow":
            resample.check_follow_lengths(lens_in, sample_rates)
        if sample_rates is not None:
            sigs = resample.convert(sigs, sample_rates, audio.MODEL_RATE, on_device=True)
        lens = [int(s.numel()) for s in sigs]
        for i, L in enumerate(lens):
            if L < batching.MIN_LENGTH:
                raise ValueError(f"enhance_batch: utterance {i} has {L} samples; the STFT's reflect padding needs at "
                                 f"least {batching.MIN_LENGTH}")
        plan = longform.Plan(lens, window_frames, overlap_frames)
        dev = ops.current_device()
        # the recordings go up once; every window is cut on the device, and the enhancers' results overwrite it
        src = sigs[0].reshape(1, -1) if n == 1 else batching.pack_rows(sigs)[0]  # one recording needs no packing
        wins = ops.window_gather(src.to(dev).contiguous(), lens, plan.table, W)
        noisy16 = sigs if highband != "drop" else None  # the band split's 16 kHz side: kept until the merge
        del sigs, src
        wl = np.asarray(plan.win_lengths, np.int64)
        silent = ops.absmax(wins, lengths=wl).cpu().numpy() == 0  # the call's one read-back before the results
        live = [j for j in range(len(plan)) if not silent[j]]
        wseeds = plan.seeds(seeds) if route is not None else None
        flagged = []
        ode_stats = self.last_ode_stats = []
        guard = {}
        if route is None:
            for j in live:
                u = plan.utt[j]
                y = wins[j, :wl[j]].cpu().reshape(1, -1)
                x = self.enhance(y, y, oracle=oracle, clean_rms=clean_rms[u] if oracle else 1,
                                 noise_rms=noise_rms[u] if oracle else 1, range_guard=range_guard, **skw, **kwargs)
                flagged += [(u, plan.k[j])] if (self.last_guard or {}).get("flagged") else []
                guard = self.last_guard or {}
                wins[j, :wl[j]] = torch.from_numpy(np.asarray(x, np.float32)).to(dev)
        elif live:
            with self._compute_format(self.RANGE_FALLBACK if self._range_fallback else self.dnn.compute_dtype):
                enh = self.batched_enhancer(route, self.dnn.hip(dev), range_guard, skw["predictor"],
                                            skw["corrector"], skw["N"], skw["corrector_steps"], skw["snr"], oracle,
                                            kwargs.get("rtol", 1e-5), kwargs.get("atol", 1e-5))
                for rows in batching.plan_batches([wl[j] for j in live], batch_size, max_frames):
                    js = [live[r] for r in rows]
                    ln = [int(wl[j]) for j in js]
                    idx = torch.tensor(js, device=dev)
                    yb = wins[idx][:, :max(ln)].contiguous()
                    rs = torch.tensor([wseeds[j] for j in js], dtype=torch.int64, device=dev)
                    if route in ("pc", "ode"):
                        xb, nfe = enh(yb, noise=_samp.NoiseSource(row_seeds=rs), lengths=ln)
                        if route == "ode":
                            ode_stats.append(dict(enh.last_stats, files=[plan.utt[j] for j in js],
                                                  windows=[plan.k[j] for j in js], nfev=[int(v) for v in nfe]))
                    else:
                        est = [float(noise_rms[plan.utt[j]]) / float(clean_rms[plan.utt[j]]) for j in js] \
                            if oracle else None
                        xb, _ = enh(yb, est_snr=est, lengths=ln, row_seeds=rs)
                    flagged += [(plan.utt[js[r]], plan.k[js[r]]) for r in (enh.last_guard or {}).get("flagged", [])]
                    wins[idx, :max(ln)] = xb
                guard = enh.last_guard or {}
        out = ops.window_merge(wins, plan.starts, plan.first, lens, V, silent=torch.from_numpy(silent),
                               stride_out=max(lens)).cpu().numpy()
        self.last_guard = dict(guard, flagged=sorted({u for u, _ in flagged}), flagged_windows=sorted(flagged))
        self.last_windows = plan.counts()
        out = [out[r, :lens[r]].copy() for r in range(n)]
        if sample_rates is not None and output_rate == "input" and highband != "drop":
            out = resample.restore_highband(out, noisy16, ys, sample_rates, highband, highband_floor_db)
        elif sample_rates is not None and output_rate == "input":
            back = resample.convert(out, audio.MODEL_RATE, sample_rates)
            out = [np.asarray(h)[:L] for h, L in zip(back, lens_in)]
        return out

    def enhance_long(self, y, sample_rate=16000, **kw):
        """One recording of any length, y [L] / [1, L] at `sample_rate` -> numpy [L'] (at 16 kHz, or with
        output_rate="input" at its own rate and length): enhance_batch([y], sample_rates=[sample_rate],
        window_frames=512, ...) -- windows of 512 frames (8.2 s) cross-faded over overlap_frames = 64 (0.5 s) unless
        the keywords say otherwise."""
        kw.setdefault("window_frames", 512)
        return self.enhance_batch([y], sample_rates=[int(sample_rate)], **kw)[0]

    RANGE_FALLBACK = "bf16"   # compute_dtype enhance() falls back to when fp16 overflows
    _range_fallback = False   # set by the first hit: this model then runs RANGE_FALLBACK
    last_guard = None         # the latest enhance() call's guard record (snrse.guard.report)
    last_windows = None       # the latest enhance_batch(window_frames=...) call's window count per utterance
    last_ode_stats = None     # the latest enhance_batch() call's ODE batches: ODEEnhancer.last_stats + files, nfev

    @contextlib.contextmanager
    def _compute_format(self, fmt):
        """The backbone in another compute_dtype for the duration (it keeps one packed executor per format)."""
        prev, self.dnn.compute_dtype = self.dnn.compute_dtype, fmt
        try:
            yield
        finally:
            self.dnn.compute_dtype = prev


__all__ = ["ScoreModel", "t_30", "get_snr_model", "set_snr_model", "warnings"]
