"""Batched, device-resident ScoreModel.enhance() (reference sgmse/model.py:702-839).

Two branches, as the reference:
  * PC sampler (model_type 'bbed', snr_conditioned 'false', model.py:756-768): STFT ->
    exponent transform -> pad -> prior -> N x (corrector, predictor), each NFE fused with its
    SDE update -> iSTFT.  2 NFE per step for reverse_diffusion + ald.
  * one-step SNR-aligned (model_type 'sebridge_v3', snr_conditioned 'true',
    model.py:713-740, 810-825): t_hat from the SNR (estimator or oracle rms) snapped to the
    t_30 grid, X_T = Y + sigma_max t_hat Z, one preconditioned NFE.
The 'bbed' branch's other sampler, the probability-flow ODE (model.py:762-763, sampling/__init__.py:95-171), is
ODEEnhancer: an adaptive RK45 in which every utterance of the batch keeps its own step sizes.
Utterances are processed as a batch (the reference loops B=1); per-utterance scalars
(norm factors, t_hat) stay per batch element.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import guard as _guard
from . import ops, sampler

T_30 = (0.001 ** (1 / 7) + (np.arange(1, 31) - 1) / 29 * (1 - 0.001 ** (1 / 7))) ** 7  # model.py:22-23


def snap_t(est_snr, fixed_snr):
    """calculate_snr_direct + nearest t_30 (model.py:627-629, 810-817), per utterance."""
    t = np.asarray(est_snr, dtype=np.float64) / (10 ** 0.25 * fixed_snr)
    return T_30[np.abs(T_30[None, :] - t.reshape(-1, 1)).argmin(axis=1)]


def normfac(t_hat, fixed_snr):
    """calculate_normfac_direct at est_snr_ = 10^0.25 fixed_snr t_hat (model.py:631-634, 734-736)."""
    s = 10 ** 0.25 * fixed_snr * np.asarray(t_hat, dtype=np.float64)
    return 2.040166 * (0.240253 + 0.759747 * fixed_snr ** 2) ** 0.5 / np.sqrt(1 + s ** 2)


def pad_frames(T, mult=64):
    return T + ((mult - T % mult) % mult)


TRANSFORM_MODES = {"exponent": 1, "none": 0}  # fused spec_fwd/spec_back (|c|^0.5 e^{i angle} 0.15) or raw


def transform_mode(transform):
    if transform not in TRANSFORM_MODES:
        raise NotImplementedError(f"transform_type {transform!r} is not built for the HIP path")
    return TRANSFORM_MODES[transform]


def ragged_lengths(lengths, y):
    """(ops.Lengths, Tpad) of a ragged [B, Lstride] batch.  The rows must share Tpad = pad_frames(1 + L_b // 128):
    then the network's shapes are those of each row's own run and the extra frames are the zero padding it would
    have had alone (snrse.batching.plan_batches groups a file list this way)."""
    B, L = y.shape
    ln = ops.as_lengths(lengths, B, L, y.device)
    tp = sorted({pad_frames(1 + int(v) // 128) for v in ln.host})
    if len(tp) != 1:
        raise ValueError(f"snrse: the rows of a ragged batch must share Tpad, got {tp} "
                         "(snrse.batching.plan_batches groups utterances by it)")
    return ln, tp[0]


def crop_rows(x, ln):
    """Zero x [B, Lstride] at and past each row's length.  The iSTFT's overlap-add depends on the frame count and
    the sample index only, so computing to Lstride and cropping is exact on [0, L_b)."""
    keep = torch.arange(x.shape[1], device=x.device)[None, :] < ln.dev[:, None]
    return torch.where(keep, x, torch.zeros((), device=x.device, dtype=x.dtype))


def front_end(y, mode, lengths=None, div=None):
    """The front end of every enhancement: y [B, L] f32 device -> (Y = STFT(y / div) padded to Tpad frames and
    transformed by `mode`, div, ln).  div: per-row divisor, default max|y| (norm_factor, model.py:726).  lengths: a
    ragged batch (ragged_lengths: the rows share Tpad), ln its ops.Lengths; None: ln is None and
    Tpad = pad_frames(1 + L // 128)."""
    ln, tpad = (None, pad_frames(1 + y.shape[1] // 128)) if lengths is None else ragged_lengths(lengths, y)
    if div is None:
        div = ops.absmax(y, lengths=ln)
    return ops.stft(y, 1.0, tpad=tpad, mode=mode, in_div=div, lengths=ln), div, ln


def back_end(x, L, mode, div, ln=None):
    """front_end's inverse: spectrogram x [B, F, Tpad] -> waveforms [B, L] scaled by div, zero past each row's
    length when ln is set."""
    out = ops.istft(x.contiguous(), L, mode=mode, out_scale=div)
    return out if ln is None else crop_rows(out, ln)


def fused_step(net, Y, score_mode):
    """The PC loop's score_step on an NCSNppHIP network: one evaluation (the pyramid) with the output head, the
    score and the SDE update fused in one kernel."""

    def step(x, tv, coef, z, seed, off):
        pyr = net.pyramid(x, Y, tv)
        xo, xm, _ = ops.score_update(pyr, net.W["out_w"], net.W["out_b"], tv, score_mode, x, Y, coef=coef, noise=z,
                                     offset=off, **sampler.row_seed_kw(seed))
        return xo, xm

    return step


class PCEnhancer:
    """PC-sampler enhancement of a batch of noisy waveforms with an NCSNppHIP network.

    streams > 1 splits the batch into that many lanes, each on its own HIP stream with its own
    GroupNorm-statistics arena and split-K workspace, and issues their network evaluations
    alternately (sampler.pc_sample_lockstep): one lane's latency-bound low-resolution levels overlap
    the other lane's full-resolution GEMMs.  stagger: lane k starts when lane k-1's first evaluation
    has reached the middle of the network (an event recorded between its down and up paths), so the
    lanes run half an evaluation apart instead of in phase.  The noise draws are the whole-batch ones
    (LaneNoise), so the result equals the single-stream run.

    guard (snrse.guard): "auto" (= "fallback" for an fp16 network, off otherwise), None / "off", "warn", "raise",
    "fallback".  After the loop (the lanes joined) one range_stats launch and one B-element read-back look at the
    returned spectrogram; an utterance the network's format could not hold is all NaN there.  "fallback" re-runs
    those rows, run by run and on one stream, through net.fallback(fallback_dtype) with the draws the whole-batch
    run took for them, and warns once per enhancer.  last_guard describes the latest call."""

    def __init__(self, net, sde: sampler.SDESpec, N=30, eps=0.03, snr=0.5, predictor="reverse_diffusion",
                 corrector="ald", corrector_steps=1, score_mode=0, transform="exponent", streams=1, stagger=True,
                 guard="auto", fallback_dtype=torch.bfloat16):
        _guard.resolve(guard, net.dtype)  # a bad policy fails here, not at the first call
        self.guard, self.fallback_dtype = guard, fallback_dtype
        self.last_guard = None
        self.net, self.sde, self.N, self.eps, self.snr = net, sde, N, eps, snr
        self.mode = transform_mode(transform)
        self.predictor, self.corrector, self.corrector_steps = predictor, corrector, corrector_steps
        self.score_mode = score_mode
        self.streams = int(streams)
        self.stagger = bool(stagger)
        self._lane_streams = {}

    def _step(self, Y, net):
        """The score_step of one lane (a subclass may wrap it, as tools/agree3.py does to record the states)."""
        return fused_step(net, Y, self.score_mode)

    def _iter(self, Y, noise, net=None):
        net = net or self.net

        def score_tensor(x, tv):
            return net.score(x, Y, tv, self.score_mode)

        return sampler.pc_sample_iter(self._step(Y, net), Y, self.sde, N=self.N, eps=self.eps, snr=self.snr,
                                      predictor=self.predictor, corrector=self.corrector,
                                      corrector_steps=self.corrector_steps, noise=noise, score_tensor=score_tensor)

    def sample(self, Y, noise: sampler.NoiseSource | None = None):
        return _guard.guarded(self, self._sample, Y, noise)

    def _sample(self, Y, noise, net):
        """The whole batch over the enhancer's streams; a guard re-run (another net) on one stream."""
        B = Y.shape[0]
        nl = min(self.streams, B) if net is self.net else 1
        if nl <= 1:
            return sampler.drain(self._iter(Y, noise, net=net))
        cur = torch.cuda.current_stream(Y.device)
        bounds = [(B * h // nl, B * (h + 1) // nl) for h in range(nl)]
        lanes, lane_noise = [], []
        for h, (a, b) in enumerate(bounds):
            s = self._lane_streams.get((Y.device, h))
            if s is None:
                s = self._lane_streams[(Y.device, h)] = torch.cuda.Stream(device=Y.device)
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                Yh = Y[a:b].contiguous()
                lane_noise.append(sampler.LaneNoise(noise, a, b, B))
                lanes.append((s, self._iter(Yh, lane_noise[-1])))
        starts = None
        if self.stagger:
            # lane k's first launch waits for lane k-1's first evaluation to pass the bottleneck
            evs = [torch.cuda.Event() for _ in range(nl - 1)]

            def arm(k):
                if k + 1 < nl:
                    self.net.mid_hook = lambda: evs[k].record(torch.cuda.current_stream())

            def start(k):
                if k > 0:
                    torch.cuda.current_stream().wait_event(evs[k - 1])
                arm(k)

            starts = start
        res = sampler.pc_sample_lockstep(lanes, on_first=starts)
        self.net.mid_hook = None
        noise.i = lane_noise[0].i  # the parent has now supplied the lanes' draws (as the one-stream run does)
        for (s, _), (x, _) in zip(lanes, res):
            cur.wait_stream(s)
            x.record_stream(cur)
        return torch.cat([x for x, _ in res]), res[0][1]

    def __call__(self, y, noise=None, lengths=None):
        """y [B, L] f32 device -> (x_hat [B, L] f32, nfe).  lengths: a ragged batch, row b valid on [0, L_b) of
        the [B, Lstride] buffer (what lies past L_b is never read); the rows must share Tpad (ragged_lengths),
        the result is zero past L_b.  A row's result equals its run alone up to GEMM summation order when
        `noise` is row-seeded (sampler.NoiseSource(row_seeds=...)) and the corrector is not `langevin`."""
        Y, nf, ln = front_end(y, self.mode, lengths)
        x, nfe = self.sample(Y, noise)
        return back_end(x, y.shape[1], self.mode, nf, ln), nfe


class ODEEnhancer:
    """Probability-flow ODE enhancement of a batch (the reference's get_ode_sampler, sampling/__init__.py:95-171,
    which integrates one utterance at a time): prior x_T = Y + std(T) z, then dx/dt = kappa(t) (Y - x) - g(t)^2 / 2
    score(x, t, Y) from T down to eps with the per-row adaptive RK45 (snrse.ode.rk45_solve_rows), then (denoise)
    one noise-free reverse-diffusion update at eps with step size 0.03.

    Every row has its own time, step size and accept / reject history, so a row's result is the solve it would have
    had alone (up to GEMM summation order), however hard the rows it shares the batch with are; rows that reach
    eps leave the batch and the network runs on the ones still integrating.  The drift is one net.pyramid plus one
    fused ops.score_update with the per-row coefficients (-kappa, kappa, -g^2 / 2, 0), whose x_mean output is the
    drift itself; kappa and g are taken at float32(t_b), the time the network is given (the per-utterance path
    rounds its time vector the same way).  The RK45 stage combinations, error norms and per-row accepts are the
    fp64 kernels of csrc/ode.hip; the controller is host float64 with one read-back (the B error norms) per attempt.

    guard / fallback_dtype: PCEnhancer's policies.  A row whose error norm is not finite leaves the solve at once
    (status -2); such rows and rows with a non-finite result are flagged, and "fallback" re-runs them through
    net.fallback(fallback_dtype) from the same prior.  last_stats describes the latest sample(): `evals` calls of
    the network, `row_evals` rows summed over them, per-row `attempts` and `status` (fallback re-runs excluded)."""

    def __init__(self, net, sde: sampler.SDESpec, eps=0.03, rtol=1e-5, atol=1e-5, denoise=True, score_mode=0,
                 transform="exponent", guard="auto", fallback_dtype=torch.bfloat16):
        _guard.resolve(guard, net.dtype)
        self.guard, self.fallback_dtype = guard, fallback_dtype
        self.last_guard = self.last_stats = None
        self.net, self.sde, self.eps, self.rtol, self.atol = net, sde, float(eps), float(rtol), float(atol)
        self.denoise, self.score_mode = bool(denoise), score_mode
        self.mode = transform_mode(transform)

    def _fused(self, net, x32, Y, t64, coef_of):
        """x_mean of one network evaluation + fused update at the per-row times t64 (host float64): the network
        and the coefficients both see float32(t_b)."""
        t32 = np.asarray(t64, dtype=np.float64).astype(np.float32)
        coef = np.asarray([coef_of(float(t)) for t in t32], dtype=np.float32)
        dev = Y.device
        tv = torch.from_numpy(t32).pin_memory().to(dev, non_blocking=True)
        cf = torch.from_numpy(coef).pin_memory().to(dev, non_blocking=True)
        pyr = net.pyramid(x32, Y, tv)
        return ops.score_update(pyr, net.W["out_w"], net.W["out_b"], tv, self.score_mode, x32, Y, coef=cf)[1]

    def _pf_coef(self, t):
        kap, g = self.sde.drift_coef(t), self.sde.g(t)
        return (-kap, kap, -0.5 * g * g, 0.0)

    def _denoise_coef(self, t, st=0.03):
        kap, G = self.sde.drift_coef(t), self.sde.g(t) * math.sqrt(st)
        return (1.0 + kap * st, -kap * st, G * G, 0.0)

    def _solve(self, Y, noise, net):
        from .ode import rk45_solve_rows
        B = Y.shape[0]
        prior = (0.0, 1.0, 0.0, self.sde.std(self.sde.T))  # build_schedule's prior coefficients
        z, off = noise.next(Y.numel())
        coef = torch.tensor([prior] * B, dtype=torch.float32, device=Y.device)
        x0 = ops.axpby_noise(coef, y=Y, noise=z, offset=off, **sampler.row_seed_kw(noise.key))
        cache = {"rows": None, "Y": Y}

        def drift(t, x, rows, x32):
            if len(rows) != B:  # the live rows' Y, gathered once per change of the live set
                key = tuple(int(r) for r in rows)
                if cache["rows"] != key:
                    cache["rows"], cache["Y"] = key, Y[rows.to(Y.device)].contiguous()
            return self._fused(net, x32, cache["Y"] if len(rows) != B else Y, t.numpy(), self._pf_coef)

        res = rk45_solve_rows(drift, self.sde.T, self.eps, x0, rtol=self.rtol, atol=self.atol, cast32=True)
        x = res.y.to(torch.complex64)
        if self.denoise:
            x = self._fused(net, x, Y, [self.eps] * B, self._denoise_coef)
        if net is self.net:  # the whole-batch solve: the guard's re-runs stay out of last_stats
            self.last_stats = {"evals": res.evals, "row_evals": res.row_evals, "status": [int(s) for s in res.status],
                               "attempts": [len(h) + int(s == -2) for h, s in zip(res.history, res.status)]}
        return x, res

    def sample(self, Y, noise: sampler.NoiseSource | None = None):
        """Y [B, F, T] complex64 -> (x [B, F, T] complex64, nfev numpy [B]): each row's evaluation count as
        get_ode_sampler reports it for that row alone (2 + 6 x its attempts; the denoise step is not counted)."""

        def merge(res, again, a, b):
            res.nfev[a:b] = again.nfev

        x, res = _guard.guarded(self, self._solve, Y, noise, failed=lambda r: np.nonzero(r.status == -2)[0],
                                merge=merge)
        return x, res.nfev

    def __call__(self, y, noise=None, lengths=None):
        """y [B, L] f32 device -> (x_hat [B, L] f32, nfev numpy [B]).  lengths: a ragged batch under PCEnhancer's
        rule (rows sharing Tpad, the result zero past L_b); with a row-seeded `noise` a row's result is its run
        alone."""
        Y, nf, ln = front_end(y, self.mode, lengths)
        x, nfev = self.sample(Y, noise)
        return back_end(x, y.shape[1], self.mode, nf, ln), nfev


class SNRAlignedEnhancer:
    """One-step SNR-aligned enhancement of a batch (C4: model_type 'sebridge_v3',
    snr_conditioned 'true'; model.py:713-740, 810-833), the reference's per-utterance loop as one
    batched pass: y / max|y| -> raw STFT padded to 16 frames -> SNR estimate (`snr_fn`, e.g.
    SNRNet's forward_complex -> g / (1 - g), or oracle noise/clean rms) -> t_hat snapped to t_30
    -> Y = spec_fwd(STFT(y / (max|y| normfac))) -> X_T = Y + sigma_max t_hat Z -> one
    preconditioned NCSN++ evaluation at t_hat (c_skip x + c_out dnn, score mode 1) -> iSTFT x
    max|y| normfac.  The per-utterance scalars (t_hat, normfac) are host float64 as in the
    reference (one B-element copy).  Returns (x_hat [B, L], t_hat numpy [B]).  guard / fallback_dtype: the range
    guard of PCEnhancer, checked on the network's output before the iSTFT."""

    def __init__(self, net, snr_fn=None, fixed_snr=0.17783, sigma_max=0.5, transform="exponent", guard="auto",
                 fallback_dtype=torch.bfloat16):
        _guard.resolve(guard, net.dtype)
        self.guard, self.fallback_dtype = guard, fallback_dtype
        self.last_guard = None
        self.net, self.snr_fn = net, snr_fn
        self.mode = transform_mode(transform)
        self.fixed_snr, self.sigma_max = float(fixed_snr), float(sigma_max)

    def __call__(self, y, est_snr=None, noise=None, seed=0, lengths=None, row_seeds=None):
        """lengths: a ragged batch (PCEnhancer.__call__), rows sharing Tpad; the SNR estimator, which reads a
        spectrogram padded to 16 frames, runs once per group of rows with the same pad_frames(T_b, 16)
        (batching.snr_groups) and the NCSN++ pass stays whole.  row_seeds (one per row): row b's prior noise is
        Philox(row_seeds[b], e), what seed=row_seeds[b] draws for that row alone."""
        B, L = y.shape
        ln = None if lengths is None else ragged_lengths(lengths, y)[0]
        nf = ops.absmax(y, lengths=ln)
        if est_snr is None and ln is not None:
            from .batching import snr_groups
            est = torch.empty(B, dtype=torch.float64, device=y.device)
            for T16, rows in snr_groups(ln.host):
                idx = torch.tensor(rows, device=y.device)
                sub = ops.Lengths(ln.host[rows], ln.dev[idx].contiguous())
                raw = ops.stft(y[idx].contiguous(), 1.0, tpad=T16, mode=0, in_div=nf[idx].contiguous(), lengths=sub)
                est[idx] = self.snr_fn(raw).reshape(len(rows)).double()
            est_snr = est.cpu().numpy()
        elif est_snr is None:
            T16 = pad_frames(1 + L // 128, 16)
            raw = ops.stft(y, 1.0, tpad=T16, mode=0, in_div=nf)  # no spec transform (model.py:715-719)
            est_snr = self.snr_fn(raw).reshape(B).double().cpu().numpy()
        t_hat = snap_t(est_snr, self.fixed_snr)
        div = nf * torch.from_numpy(normfac(t_hat, self.fixed_snr)).to(nf.device, torch.float32)
        Y, div, ln = front_end(y, self.mode, ln, div)
        coef = torch.zeros(B, 4, dtype=torch.float32)
        coef[:, 1] = 1.0
        coef[:, 3] = torch.from_numpy(self.sigma_max * t_hat).float()
        X_T = ops.axpby_noise(coef.to(Y.device), y=Y, noise=noise, seed=seed, row_seeds=row_seeds)
        tv = torch.from_numpy(t_hat).to(Y.device, torch.float32)
        sample = self.net.score(X_T, Y, tv, 1)
        # range guard (PCEnhancer): X_T does not depend on the network's format, so the flagged rows are one more
        # evaluation of the fallback executor on the same X_T
        policy = _guard.resolve(self.guard, self.net.dtype)
        rows = _guard.flagged_rows(sample) if policy != "off" else []
        if _guard.report(self, rows, policy, self.fallback_dtype, self.net.dtype):
            fb = _guard.fallback_net(self.net, self.fallback_dtype)
            sample[rows] = fb.score(X_T[rows].contiguous(), Y[rows].contiguous(), tv[rows].contiguous(), 1)
        return back_end(sample, L, self.mode, div, ln), t_hat
