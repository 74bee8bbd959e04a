"""Device-resident Dormand-Prince RK45 for the probability-flow ODE sampler.

The reference integrates the probability-flow ODE with `scipy.integrate.solve_ivp(...,
method='RK45')` on host numpy copies of the state (sgmse/sampling/__init__.py:95-171; scipy
pinned to 1.8.0 in requirements.txt).  Here the same algorithm runs on the device tensors: the
state stays complex128 in HBM (scipy promotes the complex64 state to complex128), every stage
combination is a device op, and only the scalar error norm of each attempted step crosses to
the host (step acceptance).  Restated from scipy 1.8.0's `RungeKutta` / `RK45`:

* tableau: Dormand-Prince 5(4), FSAL (`RK45.A/B/C/E`), error estimator order 4, error exponent
  -1/5, SAFETY 0.9, MIN_FACTOR 0.2, MAX_FACTOR 10;
* initial step (`common.select_initial_step`, Hairer-Norsett-Wanner II.4):
  h0 = 0.01 d0/d1 (1e-6 when d0 or d1 < 1e-5), h1 = (0.01/max(d1, d2))^(1/5) (max(1e-6,
  1e-3 h0) when both <= 1e-15), h = min(100 h0, h1); scipy >= 1.12 also clips h0 and h to the
  interval length and max_step (`clip_initial=True` reproduces that);
* step (`RungeKutta._step_impl`): min_step = 10 ulp(t); clip to t_bound; error norm
  = RMS(|h K^T E| / (atol + rtol max(|y|, |y_new|))); accept when < 1;
* `rk_step`: 5 stage evaluations + f(t+h, y_new) (FSAL) per attempted step, so
  nfev = 2 + 6 x attempts, as `solve_ivp(...).nfev` counts.

Test infrastructure checks it against scipy itself (tests/test_ode.py).

`rk45_solve_rows` is the same algorithm for a batch of independent ODEs, the controller's scalars kept per row
(tests/test_ode_rows.py against scipy row by row; its per-element work runs on the kernels of csrc/ode.hip).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

# Dormand-Prince 5(4) (scipy RK45.A / B / C / E)
_A = [
    [],
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
]
_B = [35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]
_C = [0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0]
_E = [-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]
_ORDER = 4  # error estimator order
_EXP = -1.0 / (_ORDER + 1)
SAFETY, MIN_FACTOR, MAX_FACTOR = 0.9, 0.2, 10.0


@dataclass
class OdeResult:
    y: torch.Tensor      # final state (the dtype the solver worked in)
    t: float
    nfev: int
    status: int          # 0 reached t_bound, -1 step size fell below 10 ulp(t)
    message: str
    n_accepted: int
    n_rejected: int


def _rms(x: torch.Tensor) -> float:
    """np.linalg.norm(x) / sqrt(x.size) (scipy common.norm), complex-aware, one host sync."""
    return math.sqrt(float(x.abs().double().pow(2).sum()) / x.numel())


def _lincomb(ks, coefs):
    """sum_i coefs[i] * ks[i], in stage order (the order of numpy's dot over K[:s])."""
    acc = None
    for k, c in zip(ks, coefs):
        if c == 0.0:
            continue
        acc = k * c if acc is None else acc + k * c
    return acc if acc is not None else torch.zeros_like(ks[0])


def select_initial_step(fun, t0, y0, f0, direction, rtol, atol, t_bound=None, max_step=math.inf,
                        clip_initial=False):
    scale = atol + y0.abs() * rtol
    d0 = _rms(y0 / scale)
    d1 = _rms(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    interval = abs(t_bound - t0) if t_bound is not None else math.inf
    if clip_initial:
        if interval == 0.0:
            return 0.0
        h0 = min(h0, interval)
    y1 = y0 + (h0 * direction) * f0
    f1 = fun(t0 + h0 * direction, y1)
    d2 = _rms((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1 / (_ORDER + 1))
    if clip_initial:
        return min(100 * h0, h1, interval, max_step)
    return min(100 * h0, h1)


def rk45_solve(fun: Callable[[float, torch.Tensor], torch.Tensor], t0: float, t_bound: float, y0: torch.Tensor,
               rtol: float = 1e-3, atol: float = 1e-6, max_step: float = math.inf, first_step=None,
               clip_initial: bool = False) -> OdeResult:
    """solve_ivp(fun, (t0, t_bound), y0, method='RK45') on device tensors; returns the final state.

    `fun(t, y)` receives a python float and a tensor shaped like y0 (the solver's dtype) and
    returns dy/dt of the same shape (any float/complex dtype: it is promoted like scipy does)."""
    if not (rtol > 0 and atol >= 0):
        raise ValueError("rtol must be > 0 and atol >= 0")
    if rtol < 100 * np.finfo(float).eps:
        rtol = 100 * np.finfo(float).eps  # scipy validate_tol
    dtype = torch.complex128 if y0.is_complex() else torch.float64
    y = y0.to(dtype)
    nfev = 0

    def f_eval(t, yy):
        nonlocal nfev
        nfev += 1
        return fun(float(t), yy).to(dtype)

    t = float(t0)
    direction = float(np.sign(t_bound - t0)) if t_bound != t0 else 1.0
    f = f_eval(t, y)
    if first_step is None:
        h_abs = select_initial_step(f_eval, t, y, f, direction, rtol, atol, t_bound, max_step, clip_initial)
    else:
        h_abs = float(first_step)
    n_acc = n_rej = 0
    status, message = None, ""
    if y.numel() == 0 or t == t_bound:
        status = 0
    while status is None:
        min_step = 10 * abs(np.nextafter(t, direction * np.inf) - t)
        h_abs = max_step if h_abs > max_step else (min_step if h_abs < min_step else h_abs)
        accepted = rejected = False
        while not accepted:
            if h_abs < min_step:
                status, message = -1, "Required step size is less than spacing between numbers."
                break
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = abs(h)
            K = [f]
            for s in range(1, 6):
                K.append(f_eval(t + _C[s] * h, y + _lincomb(K, _A[s]) * h))
            y_new = y + h * _lincomb(K, _B)
            f_new = f_eval(t + h, y_new)
            K.append(f_new)
            scale = atol + torch.maximum(y.abs(), y_new.abs()) * rtol
            err = _rms(_lincomb(K, _E) * h / scale)
            if err < 1:
                factor = MAX_FACTOR if err == 0 else min(MAX_FACTOR, SAFETY * err ** _EXP)
                if rejected:
                    factor = min(1.0, factor)
                h_abs *= factor
                accepted = True
                n_acc += 1
            else:
                h_abs *= max(MIN_FACTOR, SAFETY * err ** _EXP)
                rejected = True
                n_rej += 1
        if status is not None:
            break
        t, y, f = t_new, y_new, f_new
        if direction * (t - t_bound) >= 0:
            status = 0
    return OdeResult(y=y, t=t, nfev=nfev, status=status, message=message or "The solver successfully reached "
                     "the end of the integration interval.", n_accepted=n_acc, n_rejected=n_rej)


# ---------------------------------------------------------------------------------------------------------------
# Per-row solver: a batch of independent ODEs, every row with its own time, step size and accept / reject history


@dataclass
class OdeRowsResult:
    y: torch.Tensor          # [B, ...] final states (the solver's dtype); all NaN for a row with status -2
    t: np.ndarray            # [B] float64 time each row stopped at
    nfev: np.ndarray         # [B] evaluations of each row (2 + 6 x its attempts)
    status: np.ndarray       # [B] 0 reached t_bound, -1 step below 10 ulp(t), -2 error norm not finite
    n_accepted: np.ndarray   # [B]
    n_rejected: np.ndarray   # [B]
    evals: int               # calls of fun
    row_evals: int           # rows summed over those calls
    history: list            # per row: its attempts in order, True accepted / False rejected


class _TorchStages:
    """The three per-element operations of an attempt with torch ops, on any device (the restatement that is
    checked against scipy)."""

    @staticmethod
    def _rowvec(v, like):
        return v.reshape(-1, *([1] * (like.dim() - 1)))

    def combine(self, y, h, ks, coefs, want32):
        out = y + _lincomb([k.to(y.dtype) for k in ks], coefs) * self._rowvec(h, y)
        return out, (out.to(torch.complex64 if out.is_complex() else torch.float32) if want32 else None)

    def rownorm(self, vs, coefs, a, b2, rtol, atol, m=None):
        v = _lincomb([k.to(a.dtype) for k in vs], coefs)
        if m is not None:
            v = v * self._rowvec(m, a)
        scale = atol + torch.maximum(a.abs(), b2.abs()) * rtol
        q = (v / scale).abs().double().pow(2).reshape(a.shape[0], -1)
        return torch.sqrt(q.sum(1) / q.shape[1])

    def accept(self, mask, y, y_new, f, f_new):
        idx = torch.nonzero(mask).flatten()
        y[idx] = y_new[idx]
        f[idx] = f_new[idx]


class _HipStages:
    """The same three operations on the kernels of csrc/ode.hip (device tensors only)."""

    def combine(self, y, h, ks, coefs, want32):
        from . import ops
        return ops.rk45_combine(y, h, ks, coefs, want32)

    def rownorm(self, vs, coefs, a, b2, rtol, atol, m=None):
        from . import ops
        return ops.rk45_rownorm(vs, coefs, a, b2, rtol, atol, m)

    def accept(self, mask, y, y_new, f, f_new):
        from . import ops
        ops.rk45_accept(mask, y, y_new, f, f_new)


def _upload(a: np.ndarray, dev):
    """A small host array as a device tensor: pinned and non-blocking (train.FusedAdam.grad_table), so the
    controller's per-attempt step sizes and masks do not synchronise."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dev.type == "cpu":
        return t
    return t.pin_memory().to(dev, non_blocking=True)


def rk45_solve_rows(fun, t0: float, t_bound: float, y0: torch.Tensor, rtol: float = 1e-3, atol: float = 1e-6,
                    max_step: float = math.inf, first_step=None, clip_initial: bool = False, compact: bool = True,
                    impl: str | None = None, cast32: bool = False) -> OdeRowsResult:
    """rk45_solve for a batch of B independent ODEs y0 [B, ...] over one interval (t0, t_bound): the algorithm above
    with every scalar of the controller per row -- t, h_abs, min_step = 10 ulp(t), the clip to t_bound, the
    rejected-in-this-step flag, the initial step's three norms, FSAL, status and the counters.  One attempt advances
    all live rows at once, each by its own h, so a row's trajectory is the sequence of its own attempts: what
    rk45_solve gives it alone (nfev = 2 + 6 x its attempts).  A row that reaches t_bound (status 0) or falls below
    min_step (-1) leaves the live set and the others go on; a row whose error norm is not finite leaves at once
    with status -2 and a NaN state (rk45_solve would reject and shrink it some 50 times before min_step ends it).

    fun(t, y, rows) -> dy/dt [b, ...] (float32 / complex64 or float64 / complex128; promotion is exact) for the b
    rows being integrated: t float64 [b] and rows int64 [b] (their indices in y0) are HOST tensors -- the controller
    keeps the times on the host, so a drift that needs per-row scalars computes them without a read-back --
    and y [b, ...] is the state in the solver's dtype on y0's device.  cast32: fun is called as
    fun(t, y, rows, y32) with y's float32 / complex64 cast (the HIP combine kernel writes it with the state, which
    saves the network's input a pass).

    compact=True evaluates fun on the live rows only (their state is gathered when a row leaves); compact=False
    keeps finished rows in the batch with h = 0 (for tests).  impl "torch" runs the per-element work with torch ops
    on any device; "hip" (the default for device tensors) on snrse_rk45_combine / _rownorm / _accept.  The
    controller is host float64 either way: per attempt the live rows' error norms come back in one read-back (the
    one synchronisation rk45_solve takes too) and h and the accept mask go up as small pinned arrays."""
    if not (rtol > 0 and atol >= 0):
        raise ValueError("rtol must be > 0 and atol >= 0")
    if rtol < 100 * np.finfo(float).eps:
        rtol = 100 * np.finfo(float).eps
    if y0.dim() < 1 or y0.shape[0] == 0:
        raise ValueError("rk45_solve_rows: y0 is [B, ...] with B >= 1")
    dev = y0.device
    if impl is None:
        impl = "hip" if dev.type == "cuda" else "torch"
    if impl not in ("torch", "hip"):
        raise ValueError(f"rk45_solve_rows: impl {impl!r} (one of 'torch', 'hip')")
    if impl == "hip" and dev.type != "cuda":
        raise RuntimeError("rk45_solve_rows: impl='hip' needs HIP device tensors (no CPU fallback)")
    st = _HipStages() if impl == "hip" else _TorchStages()
    dtype = torch.complex128 if y0.is_complex() else torch.float64
    dtype32 = torch.complex64 if y0.is_complex() else torch.float32
    B = y0.shape[0]
    t0, t_bound = float(t0), float(t_bound)
    direction = float(np.sign(t_bound - t0)) if t_bound != t0 else 1.0

    y_out = y0.to(dtype).contiguous().clone()        # finished rows' states, by original index
    t_row = np.full(B, t0)
    h_abs = np.zeros(B)
    nfev = np.zeros(B, dtype=np.int64)
    status = np.full(B, 1, dtype=np.int64)           # 1: still integrating
    n_acc = np.zeros(B, dtype=np.int64)
    n_rej = np.zeros(B, dtype=np.int64)
    fresh = np.ones(B, dtype=bool)                   # the next attempt opens a step (min_step clip, rejected = False)
    rejected = np.zeros(B, dtype=bool)
    history = [[] for _ in range(B)]
    evals = row_evals = 0

    rows = np.arange(B)                              # original index of every row of the working state
    y = y_out.clone()
    y32 = y0.contiguous() if (cast32 and y0.dtype == dtype32) else (y.to(dtype32) if cast32 else None)

    def f_eval(tt, yy, yy32):
        nonlocal evals, row_evals
        evals += 1
        row_evals += len(rows)
        nfev[rows[status[rows] == 1]] += 1
        args = (torch.from_numpy(np.ascontiguousarray(tt, dtype=np.float64)), yy, torch.from_numpy(rows.copy()))
        out = fun(*args, yy32) if cast32 else fun(*args)
        if impl == "torch":
            out = out.to(dtype)
        return out.contiguous()

    def retire(keep):
        """Finished rows leave: their states go to y_out; with compact the working state is gathered to `keep`."""
        nonlocal y, f, rows
        gone = ~keep
        if gone.any():
            src = _upload(np.nonzero(gone)[0], dev)
            y_out[_upload(rows[gone], dev)] = y[src]
        if compact and gone.any():
            idx = _upload(np.nonzero(keep)[0], dev)
            y, f = y[idx].contiguous(), f[idx].contiguous()
            rows = rows[keep]

    f = f_eval(t_row, y, y32)
    interval = abs(t_bound - t0)
    if first_step is not None:
        h_abs[:] = float(first_step)
    elif clip_initial and interval == 0.0:
        h_abs[:] = 0.0
    else:
        # select_initial_step per row: d0, d1 in one read-back, then the probe, then d2
        d01 = torch.stack([st.rownorm([y], [1.0], y, y, rtol, atol), st.rownorm([f], [1.0], y, y, rtol, atol)]).cpu()
        d0, d1 = d01[0].numpy(), d01[1].numpy()
        h0 = np.empty(B)
        for b in range(B):
            h0[b] = 1e-6 if (d0[b] < 1e-5 or d1[b] < 1e-5) else 0.01 * float(d0[b]) / float(d1[b])
            if clip_initial:
                h0[b] = min(h0[b], interval)
        y1, y1_32 = st.combine(y, _upload(h0 * direction, dev), [f], [1.0], cast32)
        f1 = f_eval(t0 + h0 * direction, y1, y1_32)
        d2 = st.rownorm([f1, f], [1.0, -1.0], y, y, rtol, atol).cpu().numpy()
        for b in range(B):
            d2b = float(d2[b]) / h0[b]
            if d1[b] <= 1e-15 and d2b <= 1e-15:
                h1 = max(1e-6, h0[b] * 1e-3)
            else:
                h1 = (0.01 / max(float(d1[b]), d2b)) ** (1 / (_ORDER + 1))
            h_abs[b] = min(100 * h0[b], h1, interval, max_step) if clip_initial else min(100 * h0[b], h1)
        del y1, y1_32, f1
    if y[0].numel() == 0 or t0 == t_bound:
        status[:] = 0

    while True:
        live = status[rows] == 1
        if not live.any():
            break
        if compact and not live.all():
            retire(live)
            live = np.ones(len(rows), dtype=bool)
        n = len(rows)
        h = np.zeros(n)
        t_new = t_row[rows].copy()
        # open a step / check the retried one (RungeKutta._step_impl), row by row in Python floats
        for i, r in enumerate(rows):
            if not live[i]:
                continue
            t = float(t_row[r])
            min_step = 10 * abs(np.nextafter(t, direction * np.inf) - t)
            ha = float(h_abs[r])
            if fresh[r]:
                ha = max_step if ha > max_step else (min_step if ha < min_step else ha)
                fresh[r] = False
                rejected[r] = False
            if ha < min_step:
                status[r] = -1
                live[i] = False
                continue
            hh = ha * direction
            tn = t + hh
            if direction * (tn - t_bound) > 0:
                tn = t_bound
            hh = tn - t
            h[i], t_new[i], h_abs[r] = hh, tn, abs(hh)
        if not live.any():
            continue
        if compact and not live.all():
            retire(live)
            h, t_new = h[live], t_new[live]
            live = np.ones(len(rows), dtype=bool)
        tr = t_row[rows]
        h_dev = _upload(h, dev)
        K = [f]
        for s in range(1, 6):
            ys, ys32 = st.combine(y, h_dev, K, _A[s], cast32)
            K.append(f_eval(tr + _C[s] * h, ys, ys32))
        y_new, y_new32 = st.combine(y, h_dev, K, _B, cast32)
        f_new = f_eval(tr + h, y_new, y_new32)
        K.append(f_new)
        err_all = st.rownorm(K, _E, y, y_new, rtol, atol, m=h_dev).cpu().numpy()  # the attempt's one synchronisation
        mask = np.zeros(len(rows), dtype=np.int32)
        bad = np.zeros(len(rows), dtype=bool)
        for i, r in enumerate(rows):
            if not live[i]:
                continue
            err = float(err_all[i])
            ha = float(h_abs[r])
            if not math.isfinite(err):
                status[r] = -2
                bad[i] = True
                continue
            if err < 1:
                factor = MAX_FACTOR if err == 0 else min(MAX_FACTOR, SAFETY * err ** _EXP)
                if rejected[r]:
                    factor = min(1.0, factor)
                h_abs[r] = ha * factor
                n_acc[r] += 1
                history[r].append(True)
                mask[i] = 1
                fresh[r] = True
                t_row[r] = t_new[i]
                if direction * (t_new[i] - t_bound) >= 0:
                    status[r] = 0
            else:
                h_abs[r] = ha * max(MIN_FACTOR, SAFETY * err ** _EXP)
                rejected[r] = True
                n_rej[r] += 1
                history[r].append(False)
        if mask.any():
            st.accept(_upload(mask, dev), y, y_new, f, f_new)
        if bad.any():
            y[_upload(np.nonzero(bad)[0], dev)] = complex("nan+nanj") if y.is_complex() else float("nan")
    retire(np.zeros(len(rows), dtype=bool))
    return OdeRowsResult(y=y_out, t=t_row, nfev=nfev, status=status, n_accepted=n_acc, n_rejected=n_rej, evals=evals,
                         row_evals=row_evals, history=history)
