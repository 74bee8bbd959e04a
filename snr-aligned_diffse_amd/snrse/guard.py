"""Range guard of the 16-bit fast path: detect an utterance the format could not hold, fall back, report.

fp16 tops out at 65504 and the kernels pack with round-to-nearest, so a larger activation is stored as +-inf,
the next GEMM turns it into NaN and GroupNorm spreads it over the image.  The damage is sticky and stays inside
one utterance: every later tensor of that batch row is NaN, through score_update into x and so into every later
step of the sampler, while convolutions, GroupNorm, attention, the split-K sums and the ALD step never mix rows
(the `langevin` corrector does, through its batch-mean norms -- there every row is flagged, which is still
right).  So ONE look at the returned spectrogram per call (ops.range_stats, one B-element read-back) tells
exactly which utterances were damaged, at no cost per network evaluation.

Policies (resolve): "off" / None, "warn" (return the rows as they are and warn), "raise" (FloatRangeError),
"fallback" (recompute the flagged rows with a second executor packed from the original fp32 weights in a format
that holds them, NCSNppHIP.fallback(), drawing the noise the whole-batch run drew for those rows), and "auto" =
"fallback" for an fp16 network, off for bf16 / fp32 ones, whose exponent range is fp32's.
"""
from __future__ import annotations

import warnings

import torch

from . import ops, sampler

POLICIES = ("off", "warn", "raise", "fallback")


class FloatRangeError(RuntimeError):
    """Batch rows whose result is not finite (`.rows`, sorted)."""

    def __init__(self, rows, what="result"):
        self.rows = list(rows)
        super().__init__(f"snrse: {what} of batch rows {self.rows} is not finite: the network's 16-bit format "
                         "overflowed (python -m snrse.range_check shows where); run it with dtype=torch.bfloat16 "
                         "or guard='fallback'")


class RangeFallbackWarning(UserWarning):
    """The 16-bit format overflowed on some utterances (recomputed in the fallback format, or returned as is)."""


def resolve(policy, dtype):
    """The policy in force for a network of `dtype`: one of POLICIES."""
    if policy is None:
        return "off"
    if policy == "auto":
        return "fallback" if dtype == torch.float16 else "off"
    if policy not in POLICIES:
        raise ValueError(f"snrse: range guard policy {policy!r} (one of 'auto', None, {', '.join(map(repr, POLICIES))})")
    return policy


def runs(rows):
    """Maximal contiguous [a, b) runs of a sorted index list."""
    out = []
    for r in rows:
        if out and out[-1][1] == r:
            out[-1] = (out[-1][0], r + 1)
        else:
            out.append((r, r + 1))
    return out


def snapshot(noise: sampler.NoiseSource | None):
    """A NoiseSource as the caller's is now (seed, tape, row seeds, draw index), left untouched by the call it is
    taken for."""
    noise = noise or sampler.NoiseSource()
    snap = sampler.NoiseSource(noise.seed, noise.tape, noise.row_seeds)
    snap.i = noise.i
    return snap


def run_noise(snap, rows_flagged, B):
    """[(a, b, LaneNoise)] per contiguous run of the flagged rows: the draws of rows [a, b) of the whole-batch run
    that started at `snap` (a row-seeded snapshot hands each run the seeds of its rows).  The draws are those of
    the whole batch as it was sampled: on a ragged batch each row's full Tpad-frame draws, which is what it drew."""
    return [(a, b, sampler.LaneNoise(snap, a, b, B)) for a, b in runs(rows_flagged)]


def flagged_rows(x):
    """Rows of x (leading dimension) that hold an inf or NaN: one range_stats launch, one B-element read-back."""
    _, nonfinite = ops.range_stats(x)
    return [int(r) for r in torch.nonzero(nonfinite.cpu()).flatten()]


def fallback_net(net, fallback_dtype):
    """net.fallback() for a torch dtype, or "fp32x3" for the split-bf16 fp32 mode."""
    if fallback_dtype == "fp32x3":
        return net.fallback(torch.float32, gemm="x3")
    return net.fallback(fallback_dtype)


def report(owner, rows, policy, fallback_dtype, net_dtype):
    """Record owner.last_guard and act on a hit short of recomputing: raise, or warn (once per owner for the
    fallback).  Returns True when the caller has to recompute `rows`."""
    owner.last_guard = {"flagged": list(rows), "policy": policy, "fallback_dtype": fallback_dtype}
    if not rows or policy == "off":
        return False
    if policy == "raise":
        raise FloatRangeError(rows)
    if policy == "warn":
        warnings.warn(f"snrse: batch rows {list(rows)} are not finite: the {net_dtype} network overflowed its range; "
                      "they are returned as they are", RangeFallbackWarning, stacklevel=3)
        return False
    if not getattr(owner, "_guard_warned", False):
        owner._guard_warned = True
        warnings.warn(f"snrse: the {net_dtype} network overflowed its range on batch rows {list(rows)}; recomputing them "
                      f"in {fallback_dtype} (python -m snrse.range_check shows where the range is left)",
                      RangeFallbackWarning, stacklevel=3)
    return True


def guarded(owner, solve, Y, noise=None, failed=None, merge=None):
    """The guard flow of a sampling enhancer (owner: .guard, .fallback_dtype, .net, .last_guard):
    solve(Y, noise, net) -> (x, aux) on the whole batch with owner.net; the rows of x that are not finite, and the
    rows failed(aux) names, are flagged and reported; under "fallback" each contiguous run [a, b) of them is solved
    again through the fallback network with the draws the whole-batch run took for it, x[a:b] replaced and
    merge(aux, aux_rerun, a, b) called.  -> (x, aux)."""
    policy = resolve(owner.guard, owner.net.dtype)
    noise = noise or sampler.NoiseSource()
    snap = snapshot(noise) if policy == "fallback" else None
    x, aux = solve(Y, noise, owner.net)
    rows = []
    if policy != "off":
        rows = sorted(set(flagged_rows(x)) | {int(b) for b in (failed(aux) if failed else ())})
    if report(owner, rows, policy, owner.fallback_dtype, owner.net.dtype):
        fb = fallback_net(owner.net, owner.fallback_dtype)
        for a, b, lane in run_noise(snap, rows, Y.shape[0]):
            x[a:b], again = solve(Y[a:b].contiguous(), lane, fb)
            if merge:
                merge(aux, again, a, b)
    return x, aux
