"""Batched probability-flow ODE sampler (GPU): the RK45 stage kernels of csrc/ode.hip against numpy float64 written
in the kernels' operation order, rk45_solve_rows(impl="hip") against impl="torch" on the device, ODEEnhancer's rows
against the same enhancer on each row alone and against the per-utterance loop (rk45_solve over rsde.sde), the
evaluation driver at batch_size 4, and the range guard on weights fp16 cannot hold.

The measured errors and evaluation counts go to profiles/ode_rows_errors.json."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, fnormal
from test_gpu_range_guard import nets, sds  # noqa: F401  (fixtures: the x 1e6 weights and their executors)
from test_ode_rows import pf_problem, stiff_problem

pytestmark = pytest.mark.gpu

ERRORS_JSON = os.path.join(ROOT, "profiles", "ode_rows_errors.json")


def record(**kw):
    data = {}
    if os.path.exists(ERRORS_JSON):
        with open(ERRORS_JSON) as f:
            data = json.load(f)
    data.update(kw)
    with open(ERRORS_JSON, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def rel(a, b):
    a = torch.as_tensor(a).detach().cpu()
    b = torch.as_tensor(b).detach().cpu()
    dt = torch.complex128 if (a.is_complex() or b.is_complex()) else torch.float64
    a, b = a.to(dt), b.to(dt)
    return float((a - b).abs().pow(2).mean().sqrt() / (b.abs().pow(2).mean().sqrt() + 1e-30))


# ------------------------------------------------------------------ 1. kernels against numpy
A1 = [1 / 5]
from snrse.ode import _B as TAB_B, _E as TAB_E  # noqa: E402  (6 and 7 coefficients, each with a zero entry)

ROW_LENGTHS = (3, 192, 2 * 4099, 2 * 256 * 64)  # doubles per row
H_ROWS = np.array([-0.37, 0.0, 1e-3])           # per-row h: mixed size, negative (direction -1) and 0


def draws(name, B, n, count, dtype):
    return [np.ascontiguousarray(fnormal(f"{name}.{i}", (B, n)).astype(dtype)) for i in range(count)]


def np_lincomb(ks, cs):
    """sum_s c_s K_s in stage order, zero coefficients skipped, the first term taken as it is (ode._lincomb)."""
    acc = None
    for k, c in zip(ks, cs):
        if c == 0.0:
            continue
        acc = c * k.astype(np.float64) if acc is None else acc + c * k.astype(np.float64)
    return acc


def np_rownorm(vs, cs, m, a, b2, rtol, atol, cplx):
    v = np_lincomb(vs, cs)
    if m is not None:
        v = m[:, None] * v
    if cplx:
        mod = lambda z: np.sqrt(z[:, 0::2] * z[:, 0::2] + z[:, 1::2] * z[:, 1::2])  # noqa: E731
        s = atol + rtol * np.maximum(mod(a), mod(b2))
        qr, qi = v[:, 0::2] / s, v[:, 1::2] / s
        terms = qr * qr + qi * qi
    else:
        q = v / (atol + rtol * np.maximum(np.abs(a), np.abs(b2)))
        terms = q * q
    return np.sqrt(terms.sum(1) / terms.shape[1])


@pytest.mark.parametrize("kdt", [np.float32, np.float64])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_combine_equals_numpy(gpu, n, B, kdt):
    from snrse import ops
    y = draws(f"ode.k.y.{n}", B, n, 1, np.float64)[0]
    ks = draws(f"ode.k.K.{n}", B, n, 7, kdt)
    h = H_ROWS[:B].copy()
    yd, hd = torch.from_numpy(y).to(gpu), torch.from_numpy(h).to(gpu)
    kd = [torch.from_numpy(k).to(gpu) for k in ks]
    for cs in (A1, TAB_B, TAB_E):
        want = y + h[:, None] * np_lincomb(ks, cs)
        out, out32 = ops.rk45_combine(yd, hd, kd[:len(cs)], cs, want32=True)
        assert out.dtype == torch.float64 and out32.dtype == torch.float32
        assert np.array_equal(out.cpu().numpy(), want), (n, B, len(cs))
        assert np.array_equal(out32.cpu().numpy(), want.astype(np.float32)), (n, B, len(cs))
        assert ops.rk45_combine(yd, hd, kd[:len(cs)], cs)[1] is None
    if B == 3:
        assert np.array_equal(out.cpu().numpy()[1], y[1])  # h = 0 leaves the row as it is
    if n % 2 == 0:  # a complex128 state is the same doubles
        yc = torch.view_as_complex(yd.reshape(B, n // 2, 2))
        kc = [torch.view_as_complex(k.reshape(B, n // 2, 2)) for k in kd]
        oc, oc32 = ops.rk45_combine(yc, hd, kc[:6], TAB_B, want32=True)
        want = y + h[:, None] * np_lincomb(ks, TAB_B)
        assert oc.dtype == torch.complex128 and oc32.dtype == torch.complex64
        assert np.array_equal(torch.view_as_real(oc).reshape(B, n).cpu().numpy(), want)
        assert np.array_equal(torch.view_as_real(oc32).reshape(B, n).cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("kdt", [np.float32, np.float64])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", ROW_LENGTHS + (6,))
def test_rownorm_matches_numpy_and_repeats(gpu, n, B, kdt):
    from snrse import ops
    a, b2 = draws(f"ode.n.a.{n}", B, n, 2, np.float64)
    vs = draws(f"ode.n.V.{n}", B, n, 7, kdt)
    m = H_ROWS[:B].copy()
    ad, bd, md = (torch.from_numpy(v).to(gpu) for v in (a, b2, m))
    vd = [torch.from_numpy(v).to(gpu) for v in vs]
    rtol, atol = 1e-3, 1e-6
    cases = [("error norm", vd, TAB_E, md, ad, bd), ("d0", [ad], [1.0], None, ad, ad),
             ("d2", vd[:2], [1.0, -1.0], None, ad, ad)]
    for cplx in ((False, True) if n % 2 == 0 else (False,)):
        def view(t):
            return torch.view_as_complex(t.reshape(B, n // 2, 2)) if cplx else t
        for name, v, cs, mm, aa, bb in cases:
            got = ops.rk45_rownorm([view(t) for t in v], cs, view(aa), view(bb), rtol, atol, m=mm)
            again = ops.rk45_rownorm([view(t) for t in v], cs, view(aa), view(bb), rtol, atol, m=mm)
            assert torch.equal(got, again), (name, n, B, cplx)  # the same bits on every launch
            want = np_rownorm([t.cpu().numpy() for t in v], cs, None if mm is None else m, aa.cpu().numpy(),
                              bb.cpu().numpy(), rtol, atol, cplx)
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0, err_msg=f"{name} {n} {B} {cplx}")
    if B == 3:
        assert float(got[1]) > 0 and float(ops.rk45_rownorm(vd, TAB_E, ad, bd, rtol, atol, m=md)[1]) == 0.0  # h = 0


@pytest.mark.parametrize("fdt", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_accept_copies_masked_rows_only(gpu, n, fdt):
    from snrse import ops
    B = 3
    y, y_new, f, f_new = (torch.from_numpy(v).to(gpu) for v in draws(f"ode.a.{n}", B, n, 4, np.float64))
    f, f_new = f.to(fdt), f_new.to(fdt)
    for mask in ([0, 0, 0], [1, 1, 1], [0, 1, 0], [1, 0, 1]):
        yy, ff = y.clone(), f.clone()
        ops.rk45_accept(torch.tensor(mask, dtype=torch.int32, device=gpu), yy, y_new, ff, f_new)
        for b, mk in enumerate(mask):
            assert torch.equal(yy[b], (y_new if mk else y)[b]) and torch.equal(ff[b], (f_new if mk else f)[b]), (mask, b)


def test_stage_kernels_refuse_bad_arguments(gpu):
    from snrse import ops
    y = torch.zeros(2, 8, dtype=torch.float64, device=gpu)
    h = torch.zeros(2, dtype=torch.float64, device=gpu)
    with pytest.raises(RuntimeError):
        ops.rk45_combine(y.cpu(), h.cpu(), [y.cpu()], [1.0])  # not on the device
    with pytest.raises(TypeError):
        ops.rk45_combine(y, h, [y, y.float()], [1.0, 2.0])  # stages of two dtypes
    with pytest.raises(ValueError):
        ops.rk45_combine(y, h, [y] * 8, [1.0] * 8)
    with pytest.raises(TypeError):
        ops.rk45_combine(y.float(), h, [y], [1.0])  # the state is float64
    with pytest.raises(RuntimeError):
        ops.rk45_combine(y.reshape(16)[1:15].reshape(2, 7), h, [y[:, :7].contiguous()], [1.0])  # base not 16-B aligned


# ------------------------------------------------------------------ 2. solver: hip against torch on the device
@pytest.mark.parametrize("case", ["stiff", "pf-1e-3", "pf-1e-5"])
def test_solver_hip_matches_torch_on_device(gpu, case):
    from snrse.ode import rk45_solve_rows
    if case == "stiff":
        y0, _, fun = stiff_problem()
        args, kw = (0.0, 0.7), dict(rtol=1e-6, atol=1e-8)
    else:
        y0, _, fun = pf_problem()
        tol = float(case[3:])
        args, kw = (1.0, 0.03), dict(rtol=tol, atol=tol)
    y0 = y0.to(gpu)
    a = rk45_solve_rows(fun, *args, y0, clip_initial=True, impl="hip", **kw)
    b = rk45_solve_rows(fun, *args, y0, clip_initial=True, impl="torch", **kw)
    assert a.history == b.history and (a.nfev == b.nfev).all() and (a.status == 0).all() and (b.status == 0).all()
    assert len({len(h) for h in a.history}) > 1  # rows left at different attempts
    err = float((a.y - b.y).abs().max())
    print(f"solver {case}: attempts {[len(h) for h in a.history]}, max |hip - torch| {err:.2e}")
    assert err < 1e-12, err
    assert a.row_evals == int(a.nfev.sum())


# ------------------------------------------------------------------ 3. network: rows against alone, alone against the loop
NET_TOL = dict(rtol=1e-3, atol=1e-3)
NET_SEEDS = (1234567, 2 ** 61 + 5, 42)


@pytest.fixture(scope="module")
def net_setup(gpu):
    from snrse import sampler
    from snrse.enhance import ODEEnhancer
    from test_gpu_dropin import score_model
    m = score_model("bbed", dtype="fp32")
    Y = torch.from_numpy(fnormal("ode.rows.y", (3, 256, 64), True))
    Y = (Y * torch.tensor([0.05, 0.3, 1.0]).reshape(3, 1, 1)).to(gpu).contiguous()
    enh = ODEEnhancer(m.dnn.hip(gpu), m.sde.copy().spec(), eps=m.t_eps, denoise=False, guard=None, **NET_TOL)
    alone = []
    for b, s in enumerate(NET_SEEDS):
        x, nfev = enh.sample(Y[b:b + 1].contiguous(), sampler.NoiseSource(row_seeds=[s]))
        alone.append((x[0].clone(), int(nfev[0])))
    return m, Y, enh, alone


def test_enhancer_rows_match_each_row_alone(gpu, net_setup):
    from snrse import sampler
    m, Y, enh, alone = net_setup
    solo_nfev = [n for _, n in alone]
    assert len(set(solo_nfev)) > 1, solo_nfev  # the condition that makes compaction run: change the scales if not
    x, nfev = enh.sample(Y, sampler.NoiseSource(row_seeds=NET_SEEDS))
    st = enh.last_stats
    errs = [rel(x[b], alone[b][0]) for b in range(3)]
    print(f"ode rows vs alone: nfev {nfev.tolist()} (alone {solo_nfev}), rel RMS {errs}, evals {st['evals']}, "
          f"row_evals {st['row_evals']}")
    record(rows_vs_alone={"nfev_batch": [int(v) for v in nfev], "nfev_alone": solo_nfev, "rel_rms": errs,
                          "evals": st["evals"], "row_evals": st["row_evals"]})
    assert nfev.tolist() == solo_nfev
    assert max(errs) < 1e-4, errs
    assert st["row_evals"] == sum(solo_nfev) and st["evals"] == max(solo_nfev) and st["status"] == [0, 0, 0]


def test_enhancer_row_alone_matches_the_per_utterance_loop(gpu, net_setup):
    """One row alone against what test_ode.test_ode_sampler_hip_vs_scipy_loop's device side runs: rk45_solve over
    rsde.sde (torch ops around the network's score), from the same prior."""
    from snrse import ops
    from snrse.ode import rk45_solve
    m, Y, enh, alone = net_setup
    b = 1
    sde = m.sde.copy()
    sp = sde.spec()
    Yb = Y[b:b + 1].contiguous()
    coef = torch.tensor([[0.0, 1.0, 0.0, sp.std(sp.T)]], dtype=torch.float32, device=gpu)
    x0 = ops.axpby_noise(coef, y=Yb, seed=NET_SEEDS[b], offset=0)
    rsde = sde.reverse(m, probability_flow=True)
    Y4 = Yb[:, None]

    def drift(t, xs):
        xc = xs.reshape(Y4.shape).to(torch.complex64)
        return rsde.sde(xc, torch.ones(1, device=gpu) * t, Y4)[0]

    res = rk45_solve(drift, float(sde.T), m.t_eps, x0[:, None], **NET_TOL)
    err = rel(alone[b][0], res.y.reshape(Yb.shape)[0].to(torch.complex64))
    print(f"ode row alone vs rk45_solve over rsde.sde: nfev {alone[b][1]} vs {res.nfev}, rel RMS {err:.2e}")
    record(alone_vs_loop={"nfev_enhancer": alone[b][1], "nfev_loop": int(res.nfev), "rel_rms": err})
    assert alone[b][1] == res.nfev
    assert err < 1e-4, err


# ------------------------------------------------------------------ 4. ragged batches through the evaluation driver
def test_evaluate_driver_ode_batches(gpu, tmp_path, monkeypatch):
    """Four files in two Tpad buckets (as test_gpu_batch_eval builds them): evaluate(sampler_type="ode",
    batch_size=4) calls enhance_batch with the two buckets, each waveform equals enhance_batch(batch_size=1) with
    the same seeds to 1e-4, and the enhancer's output is zero past each row's length."""
    from snrse import audio, enhance, evaluate
    from test_gpu_dropin import score_model
    root = tmp_path / "test"
    for d in ("clean", "noisy"):
        os.makedirs(root / d)
    lens = (7000, 9000, 8100, 12000)  # Tpad 64, 128, 64, 128
    rng = np.random.default_rng(3)
    noisy = []
    for k, L in enumerate(lens):
        c = (0.2 * np.sin(np.arange(L) * (0.02 + 0.01 * k))).astype(np.float32)
        y = (c + 0.05 * rng.standard_normal(L)).astype(np.float32)
        noisy.append(y)
        audio.write_wav(str(root / "clean" / f"f{k}.wav"), c, bits=32)
        audio.write_wav(str(root / "noisy" / f"f{k}.wav"), y, bits=32)
    m = score_model("bbed", dtype="fp32")
    assert m._batch_route("ode", "ald", {}) == "ode" and m._batch_route("ode", "ald", {"noise_tape": None}) is None
    calls, batch_out, seeds_of, enh_out = [], {}, {}, []
    enhance_batch = m.enhance_batch

    def rec_batch(ys, **kw):
        r = enhance_batch(ys, **kw)
        calls.append([len(y) for y in ys])
        for y, h, s in zip(ys, r, kw["seeds"]):
            batch_out[len(y)], seeds_of[len(y)] = h, s
        return r

    call = enhance.ODEEnhancer.__call__

    def rec_call(self, y, noise=None, lengths=None):
        out = call(self, y, noise=noise, lengths=lengths)
        enh_out.append((out[0].cpu().numpy(), list(lengths), out[1]))
        return out

    monkeypatch.setattr(enhance.ODEEnhancer, "__call__", rec_call)
    m.enhance_batch = rec_batch
    torch.manual_seed(7)
    data = evaluate.evaluate(m, str(root), str(tmp_path / "o4"), sampler_type="ode", batch_size=4, **NET_TOL)
    m.enhance_batch = enhance_batch
    assert calls == [[7000, 8100], [9000, 12000]] and data["filename"] == [f"f{k}.wav" for k in range(4)]
    assert [ln for _, ln, _ in enh_out] == [[7000, 8100], [9000, 12000]]
    for xb, ln, nfev in enh_out:
        assert xb.shape == (2, max(ln)) and np.isfinite(xb).all() and len(nfev) == 2
        for r, L in enumerate(ln):
            assert (xb[r, L:] == 0).all() and np.abs(xb[r, :L]).max() > 0
    one = enhance_batch(noisy, seeds=[seeds_of[L] for L in lens], batch_size=1, sampler_type="ode", **NET_TOL)
    for k, L in enumerate(lens):
        err = rel(batch_out[L], one[k])
        print(f"ode driver file {k}: batch_size 4 vs batch_size 1 rel RMS {err:.2e}")
        assert batch_out[L].shape == one[k].shape == (L,) and err < 1e-4, (k, err)
    assert np.isfinite(data["si_sdr"]).all()


def test_deep_evaluate_variants_are_one_ode_batch(gpu):
    """The SNR variants of one file share a length: enhance_variants(sampler_type="ode") runs them as one batch of
    the per-row solver, each variant equal to its own enhance_batch run under the seed it drew."""
    from snrse import deep_evaluate
    from test_gpu_dropin import score_model
    m = score_model("bbed", dtype="fp32")
    assert deep_evaluate._batched_kind(m, "ode") == "ode"
    L = 7000
    rng = np.random.default_rng(11)
    x = (0.2 * np.sin(np.arange(L) * 0.03)).astype(np.float32)
    ys, noise_rms = deep_evaluate.snr_variants(x, x + (0.1 * rng.standard_normal(L)).astype(np.float32))
    ys, noise_rms = ys[::4], noise_rms[::4]  # 3 of the 9 variants
    torch.manual_seed(5)
    xh = deep_evaluate.enhance_variants(m, ys, noise_rms, sampler_type="ode", **NET_TOL)
    assert xh.shape == ys.shape and np.isfinite(xh).all()
    assert len(m.last_ode_stats) == 1 and m.last_ode_stats[0]["files"] == [0, 1, 2]
    torch.manual_seed(5)
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(3)]
    one = m.enhance_batch(list(ys), seeds=seeds, batch_size=1, sampler_type="ode", **NET_TOL)
    errs = [rel(xh[k], one[k]) for k in range(3)]
    print(f"ode deep_evaluate variants vs alone: rel RMS {errs}")
    assert max(errs) < 1e-4, errs


# ------------------------------------------------------------------ 5. range guard
def test_guard_flags_the_overflowing_rows_and_falls_back(gpu, nets):  # noqa: F811
    """The x 1e6 weights of test_gpu_range_guard: the fp16 network's first drift is NaN, so each row's first error
    norm is not finite and the row leaves after ONE attempt (status -2), is flagged and re-run in bf16 from the
    same prior -- the result of a bf16 enhancer under the same seeds."""
    from snrse import guard, sampler
    from snrse.enhance import ODEEnhancer
    from test_gpu_range_guard import spec
    sde = sampler.SDESpec("ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5)
    Y = spec("ode.guard.Y", 2, gpu)
    seeds = (77, 2 ** 60 + 3)
    enh = ODEEnhancer(nets("scaled", torch.float16), sde, guard="fallback", **NET_TOL)
    src = sampler.NoiseSource(row_seeds=seeds)
    with pytest.warns(guard.RangeFallbackWarning):
        x, nfev = enh.sample(Y, src)
    assert enh.last_guard["flagged"] == [0, 1] and src.i == 1
    assert enh.last_stats["status"] == [-2, -2] and enh.last_stats["attempts"] == [1, 1]
    assert enh.last_stats["evals"] == 8  # f(t0), the initial-step probe, one attempt
    assert torch.isfinite(torch.view_as_real(x)).all()
    ref_enh = ODEEnhancer(nets("scaled", torch.bfloat16), sde, guard=None, **NET_TOL)
    ref, ref_nfev = ref_enh.sample(Y, sampler.NoiseSource(row_seeds=seeds))
    errs = [rel(x[b], ref[b]) for b in range(2)]
    print(f"ode guard fallback vs the bf16 enhancer: rel RMS {errs}, nfev {nfev.tolist()} vs {ref_nfev.tolist()}")
    record(guard_fallback={"rel_rms": errs, "nfev": [int(v) for v in nfev], "nfev_bf16": [int(v) for v in ref_nfev]})
    assert nfev.tolist() == ref_nfev.tolist()
    assert max(errs) < 1e-4, errs
