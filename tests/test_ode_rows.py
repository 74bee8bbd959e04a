"""Per-row adaptive RK45 (snrse.ode.rk45_solve_rows), CPU: impl="torch" against scipy.integrate.solve_ivp run row by
row -- every row of a batch must reproduce the solve it would have had alone (same nfev, same solution), although
the rows take different numbers of attempts and leave the batch at different times.  `clip_initial=True` is the
installed scipy's initial-step rule (tests/test_ode.py).

The problems are shared with tests/test_gpu_ode_rows.py, which runs the HIP stage kernels against impl="torch"."""
import math

import numpy as np
import pytest
import torch
from scipy import integrate

from snrse.ode import rk45_solve, rk45_solve_rows

STIFF_LAM = (20.0, 60.0, 150.0)
STIFF_Y0 = np.array([2.0, -1.0, 0.5])
PF_ROWS = ((0, 0.5), (1, 0.05), (2, 5.0))  # (seed, amplitude of y)


def stiff_problem(lams=STIFF_LAM):
    """Rows -lam (y - cos 3t) + 0.1 y^2, one lam per row (test_ode.test_rk45_rejections_match_scipy's ODE).
    Returns (y0 [B, 3] float64, f_np(b)(t, y) for scipy, fun(t, y, rows) for the row solver)."""
    def f_np(b):
        return lambda t, y: -lams[b] * (y - np.cos(3 * t)) + 0.1 * y ** 2

    def fun(t, y, rows):
        # each row with its own scalars in Python floats, exactly the expression a solo solve evaluates
        out = [-lams[int(r)] * (y[i] - math.cos(3 * float(t[i]))) + 0.1 * y[i] ** 2 for i, r in enumerate(rows)]
        return torch.stack(out)

    return torch.from_numpy(np.stack([STIFF_Y0] * len(lams))), f_np, fun


def pf_problem(specs=PF_ROWS, n=96):
    """test_ode._pf_problem per row, generalised to (seed, amplitude of y): dx/dt = theta (y - x) - 1/2 g(t)^2 s(x, t)
    with the OUVE g and the Gaussian score.  Returns (x0 [B, n] complex64, f_np(b), fun)."""
    theta, smin, smax = 1.5, 0.05, 0.5
    lg = math.log(smax / smin)
    ys, x0s = [], []
    for seed, amp in specs:
        rng = np.random.default_rng(seed)
        y = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * amp
        x0s.append((y + 0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / math.sqrt(2)).astype(np.complex64))
        ys.append(y)

    def g(t):
        return smin * (smax / smin) ** t * math.sqrt(2 * lg)

    def std(t):
        return math.sqrt(smin ** 2 * (math.exp(2 * t * lg) - math.exp(-2 * theta * t)) * lg / (theta + lg))

    def f_np(b):
        return lambda t, x: theta * (ys[b] - x) - 0.5 * g(t) ** 2 * (-(x - ys[b]) / std(t) ** 2)

    yt = [torch.from_numpy(y) for y in ys]

    def fun(t, x, rows):
        out = []
        for i, r in enumerate(rows):
            tt, yr = float(t[i]), yt[int(r)].to(x.device)
            out.append(theta * (yr - x[i]) - 0.5 * g(tt) ** 2 * (-(x[i] - yr) / std(tt) ** 2))
        return torch.stack(out)

    return torch.from_numpy(np.stack(x0s)), f_np, fun


def test_stiff_rows_match_scipy_row_by_row():
    y0, f_np, fun = stiff_problem()
    res = rk45_solve_rows(fun, 0.0, 0.7, y0, rtol=1e-6, atol=1e-8, clip_initial=True, impl="torch")
    nfevs = []
    for b in range(3):
        ref = integrate.solve_ivp(f_np(b), (0.0, 0.7), STIFF_Y0, rtol=1e-6, atol=1e-8, method="RK45")
        nfevs.append(ref.nfev)
        assert res.status[b] == 0 and res.t[b] == 0.7
        assert res.nfev[b] == ref.nfev, (b, res.nfev[b], ref.nfev)
        assert res.nfev[b] == 2 + 6 * (res.n_accepted[b] + res.n_rejected[b])
        assert res.n_rejected[b] > 0
        np.testing.assert_allclose(res.y[b].numpy(), ref.y[:, -1], rtol=1e-9, atol=1e-12)
    assert len(set(nfevs)) == 3  # the rows finish at different attempts
    # compaction: fun saw each row only while it was integrating
    assert res.row_evals == int(res.nfev.sum()) and res.evals == int(res.nfev.max())


@pytest.mark.parametrize("tol", [1e-3, 1e-5])
def test_probability_flow_rows_match_scipy_row_by_row(tol):
    x0, f_np, fun = pf_problem()
    res = rk45_solve_rows(fun, 1.0, 0.03, x0, rtol=tol, atol=tol, clip_initial=True, impl="torch")
    assert res.y.dtype == torch.complex128
    for b in range(3):
        ref = integrate.solve_ivp(f_np(b), (1.0, 0.03), x0[b].numpy(), rtol=tol, atol=tol, method="RK45")
        assert ref.status == 0 and res.status[b] == 0 and res.t[b] == 0.03
        assert res.nfev[b] == ref.nfev, (b, res.nfev[b], ref.nfev)
        np.testing.assert_allclose(res.y[b].numpy(), ref.y[:, -1], rtol=1e-10, atol=1e-12)
    assert len(set(int(v) for v in res.nfev)) > 1  # a condition of the test: change the amplitudes if scipy moves
    assert res.row_evals == int(res.nfev.sum()) < res.evals * 3


def test_compaction_permutation_and_single_row():
    x0, _, fun = pf_problem()
    kw = dict(rtol=1e-3, atol=1e-3, clip_initial=True, impl="torch")
    a = rk45_solve_rows(fun, 1.0, 0.03, x0, compact=True, **kw)
    b = rk45_solve_rows(fun, 1.0, 0.03, x0, compact=False, **kw)
    assert a.history == b.history and (a.nfev == b.nfev).all() and (a.status == b.status).all()
    np.testing.assert_allclose(a.y.numpy(), b.y.numpy(), rtol=0, atol=1e-12)
    assert b.row_evals == 3 * b.evals and a.row_evals < b.row_evals and a.evals == b.evals
    # permuting the rows permutes the results
    perm = [2, 0, 1]

    def fun_p(t, x, rows):
        return fun(t, x, torch.tensor([perm[int(r)] for r in rows]))

    p = rk45_solve_rows(fun_p, 1.0, 0.03, x0[perm].contiguous(), **kw)
    for i, src in enumerate(perm):
        assert p.history[i] == a.history[src] and p.nfev[i] == a.nfev[src]
        assert torch.equal(p.y[i], a.y[src])
    # B = 1 is rk45_solve
    for r in range(3):
        one = rk45_solve_rows(lambda t, x, rows: fun(t, x, torch.tensor([r])), 1.0, 0.03, x0[r:r + 1], **kw)
        solo = rk45_solve(lambda t, x: fun(torch.tensor([t], dtype=torch.float64), x[None], torch.tensor([r]))[0], 1.0, 0.03, x0[r],
                          rtol=1e-3, atol=1e-3, clip_initial=True)
        assert (one.nfev[0], one.n_accepted[0], one.n_rejected[0], one.status[0]) == \
            (solo.nfev, solo.n_accepted, solo.n_rejected, solo.status)
        assert one.nfev[0] == a.nfev[r] and one.t[0] == solo.t
        np.testing.assert_allclose(one.y[0].numpy(), solo.y.numpy(), rtol=0, atol=1e-12)


def test_non_finite_row_leaves_at_once():
    x0, _, fun = pf_problem()
    kw = dict(rtol=1e-5, atol=1e-5, clip_initial=True, impl="torch")
    nan_calls = []

    def fun_nan(t, x, rows):
        out = fun(t, x, rows)
        for i, r in enumerate(rows):
            if int(r) == 1 and float(t[i]) < 0.5:  # row 1's drift is NaN from t = 0.5 on (the interval runs down)
                out[i] = float("nan")
                nan_calls.append(float(t[i]))
        return out

    res = rk45_solve_rows(fun_nan, 1.0, 0.03, x0, **kw)
    assert list(res.status) == [0, -2, 0]
    assert torch.isnan(torch.view_as_real(res.y[1])).all()
    # one attempt saw the NaN (at most its 6 evaluations), and nothing was retried
    assert 1 <= len(nan_calls) <= 6 and res.t[1] >= 0.5
    assert res.nfev[1] == 2 + 6 * (res.n_accepted[1] + res.n_rejected[1] + 1)
    # the other rows keep the results they have without it
    others = rk45_solve_rows(lambda t, x, rows: fun(t, x, torch.tensor([(0, 2)[int(r)] for r in rows])), 1.0, 0.03,
                             x0[[0, 2]].contiguous(), **kw)
    for i, r in enumerate((0, 2)):
        assert res.history[r] == others.history[i] and res.nfev[r] == others.nfev[i]
        assert torch.equal(res.y[r], others.y[i])


def test_empty_interval():
    y0 = torch.ones(2, 4, dtype=torch.complex64)
    solo = rk45_solve(lambda t, y: -y, 0.5, 0.5, y0[0], clip_initial=True)
    res = rk45_solve_rows(lambda t, y, rows: -y, 0.5, 0.5, y0, clip_initial=True, impl="torch")
    assert (res.status == 0).all() and torch.equal(res.y, y0.to(torch.complex128))
    assert (res.nfev == solo.nfev).all() and solo.nfev == 1 and (res.t == 0.5).all()
    res18 = rk45_solve_rows(lambda t, y, rows: -y, 0.5, 0.5, y0, impl="torch")
    assert (res18.nfev == rk45_solve(lambda t, y: -y, 0.5, 0.5, y0[0]).nfev).all() and (res18.status == 0).all()
    with pytest.raises(ValueError):
        rk45_solve_rows(lambda t, y, rows: -y, 0.0, 1.0, y0, rtol=0.0, impl="torch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rk45_solve_rows(lambda t, y, rows: -y, 0.0, 1.0, y0, impl="hip")
