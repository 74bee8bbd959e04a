"""The kernels that run once per sampler step, each against a plain float64 / integer reference of the same
operation (tests/step_ref.py, itself checked on the CPU by tests/test_step_ref_host.py): the in-kernel
Philox4x32-10 / Box-Muller noise, the output head + preconditioning + SDE update (snrse_score_update,
snrse_sde_update, snrse_axpby_noise and their row-seeded forms), the time-embedding tables off the network's
shapes, the STFT / iSTFT at the edges of their length range, the spectrogram transform, the per-utterance
maximum and the energy ratios.

Bounds (none was chosen from a kernel's output; the measured figures are in profiles/step_unit_errors.json):
  noise        |z - z_ref| <= 4e-6 per part: with the float32 uniforms and angle reproduced in the reference what
               is left is logf, sqrtf, sincosf and two products on values <= 5.9, a few float32 ulps; a wrong
               integer stream differs by order 1
  step kernels |out - ref| <= 16 * 2^-24 * M per float component, M the sum of the absolute values of the terms
               that make up the output.  Sixteen roundings (each at most 2^-24 relative) bound the longest chain,
               the c_out dnn term of x_out in score mode 1: four in c_out (t - eps, t^2 and its sum halved by
               the square root, the root, the division), six in dnn (1 / t, the product, four fused
               multiply-adds), their product, the score's sum, c score, the two sums of x_mean and the sum with
               s z; a swapped coefficient or a wrong row is off by order M
  temb         relative RMS < 1e-5 (the bound of test_temb_golden)
  stft/istft   relative RMS < 1e-5 raw, < 2e-5 through the exponent transform (the bounds of
               test_stft_istft_golden / test_stft_batch_edge_lengths)
  spec         |err| <= 8 * 2^-24 * |ref| per element (two square roots, a division and the products)
  absmax       exact
  energy       1e-6 dB (the bound of test_energy_ratios_kernel_vs_numpy)
"""
import math

import numpy as np
import pytest
import torch

import step_ref as sr
from oracle import spec_ref

pytestmark = pytest.mark.gpu

C64 = torch.complex64
GRID = (8, 25)  # HW = 200: no multiple of the 64-lane wave or the 256-thread block, so a block spans two rows


def gen(seed):
    return torch.Generator().manual_seed(seed)


def crandn(g, *shape):
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


def cnp(t):
    """A device tensor as numpy [B, HW] (complex128 or float64), exactly."""
    t = t.detach().cpu()
    return t.reshape(t.shape[0], -1).numpy().astype(np.complex128 if t.is_complex() else np.float64)


def part_err(a, ref):
    """Largest |difference| over real and imaginary parts."""
    d = np.asarray(a).astype(np.complex128) - ref
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))


# ================================================================================================ noise
def draw(gpu, B, H, W, **kw):
    """z itself: x = y = NULL and coef = {0, 0, 0, 1}, so the kernel's sum is 0 + 0 + 1 z."""
    from snrse import ops
    coef = torch.tensor([[0.0, 0.0, 0.0, 1.0]] * B, device=gpu)
    like = torch.empty(B, H, W, dtype=C64, device=gpu)
    out = ops.axpby_noise(coef, like=like, **kw)
    torch.cuda.synchronize()
    assert out.shape == like.shape and out.dtype == C64
    return out.cpu().numpy().reshape(B, H * W)


def check_noise(case, z, ref):
    assert np.isfinite(z.real).all() and np.isfinite(z.imag).all(), case
    e = part_err(z, ref)
    sr.record("philox normals", case, e, sr.NOISE_ATOL, "max abs difference per part")
    assert e <= sr.NOISE_ATOL, f"{case}: the kernel's normals differ from Philox4x32-10 / Box-Muller by {e:.3e}"


def test_noise_batch_keyed_offsets(gpu):
    """Philox(seed, offset + p) over the whole batch: offset 0, an offset inside the tensor (element p of offset 5
    is element p + 5 of offset 0) and offset = B HW, which continues the stream without a shared counter."""
    B, (H, W), seed = 3, GRID, 0x1234
    n = B * H * W
    z = {off: draw(gpu, B, H, W, seed=seed, offset=off) for off in (0, 5, n)}
    for off in z:
        check_noise(f"batch-keyed seed 0x1234 offset {off}", z[off], sr.batch_normals(seed, off, B, H * W))
    assert np.array_equal(z[5].reshape(-1)[:n - 5], z[0].reshape(-1)[5:])
    both = np.concatenate([z[0].reshape(-1), z[n].reshape(-1)])
    check_noise("batch-keyed offsets 0 and B HW as one stream", both[None], sr.batch_normals(seed, 0, 1, 2 * n))
    assert len(np.unique(both)) == 2 * n  # no number of the first draw comes again in the second


@pytest.mark.parametrize("seed", [0x9E3779B97F4A7C15, 2 ** 64 - 1], ids=["golden-ratio", "all-ones"])
def test_noise_seed_high_word(gpu, seed):
    """key = {seed_lo, seed_hi}: the high word of the seed reaches the generator."""
    B, (H, W) = 3, GRID
    z = draw(gpu, B, H, W, seed=seed, offset=0)
    check_noise(f"seed {seed:#x}", z, sr.batch_normals(seed, 0, B, H * W))
    lo = draw(gpu, B, H, W, seed=seed & 0xFFFFFFFF, offset=0)
    check_noise(f"seed {seed & 0xFFFFFFFF:#x}", lo, sr.batch_normals(seed & 0xFFFFFFFF, 0, B, H * W))
    assert not np.any(z == lo)


@pytest.mark.parametrize("offset", [2 ** 32 - 100, 2 ** 40 + 7], ids=["wraps-low-word", "2^40+7"])
def test_noise_counter_high_word(gpu, offset):
    """counter = {ctr_lo, ctr_hi, 0x5eed, 0}: at offset 2^32 - 100 the low word wraps inside the tensor and the
    high word becomes 1; 2^40 + 7 has it set from the start."""
    B, (H, W), seed = 3, GRID, 0x1234
    z = draw(gpu, B, H, W, seed=seed, offset=offset)
    check_noise(f"offset {offset:#x}", z, sr.batch_normals(seed, offset, B, H * W))
    # what a counter without its high word would give: from the element whose high word is set, the numbers of
    # the same low words under a zero high word
    k = 2 ** 32 - offset if offset < 2 ** 32 else 0
    lo = draw(gpu, B, H, W, seed=seed, offset=(offset + k) & 0xFFFFFFFF)
    assert not np.any(z.reshape(-1)[k:] == lo.reshape(-1)[:z.size - k])


def test_noise_row_seeded(gpu):
    """Philox(row_seed[b], draw HW + e): a negative int64 seed (its 64-bit pattern is the key), two equal seeds
    (equal rows), draws 0, 3 and 2^33 (draw HW past 2^32)."""
    from snrse import ops
    B, (H, W) = 3, GRID
    seeds = [-0x123456789ABCDEF, 0x51CE0FF1CE, -0x123456789ABCDEF]
    assert sr.as_u64(seeds[0]) >> 63 == 1
    for d in (0, 3, 2 ** 33):
        z = draw(gpu, B, H, W, row_seeds=seeds, offset=d)
        check_noise(f"row-seeded draw {d}", z, sr.row_normals(seeds, d, H * W))
        assert np.array_equal(z[0], z[2]) and not np.any(z[0] == z[1])
        # what the batch-keyed form draws for the row alone
        one = draw(gpu, 1, H, W, seed=sr.as_u64(seeds[1]), offset=d * H * W)
        assert np.array_equal(one[0], z[1])
    with pytest.raises(ValueError):
        ops.axpby_noise(torch.zeros(B, 4, device=gpu), like=torch.empty(B, H, W, dtype=C64, device=gpu),
                        row_seeds=seeds[:2])


def test_noise_small_draw_correlations(gpu):
    """One [2, 256, 64] draw: real against imaginary parts and each against its neighbour in draw order."""
    B, H, W = sr.SMALL_DRAW_SHAPE
    z = draw(gpu, B, H, W, seed=sr.SMALL_DRAW_SEED, offset=0)
    check_noise("[2, 256, 64] draw", z, sr.batch_normals(sr.SMALL_DRAW_SEED, 0, B, H * W))
    _, _, corr, lag = sr.stream_stats(z)
    sr.record("philox normals", "[2, 256, 64] |corr(re, im)|", corr, sr.CORR_BOUND, "correlation")
    sr.record("philox normals", "[2, 256, 64] lag-1 autocorrelation", lag, sr.CORR_BOUND, "correlation")
    assert corr < sr.CORR_BOUND and lag < sr.CORR_BOUND


@pytest.mark.parametrize("row_seeded", [False, True], ids=["batch-keyed", "row-seeded"])
def test_sampler_draws_disjoint_and_replayed(gpu, row_seeded):
    """sampler.NoiseSource through pc_sample (OUVE, reverse diffusion + ALD, N = 3: the prior and six steps) with
    a zero score: the (seed, offset) pairs of all seven draws cover pairwise disjoint counter ranges, and the
    final x is the numpy replay of the schedule with the reference normals.  The bound carries each step's
    16 * 2^-24 * M + 4e-6 |s| through the later steps' |a|."""
    from snrse import ops, sampler
    B, (H, W), N = 2, GRID, 3
    HW = H * W
    seeds = [-77, 0x0123456789ABCDEF] if row_seeded else None
    Y = (crandn(gen(21), B, H, W) * 0.5).to(gpu)
    sde = sampler.SDESpec("ouve")
    log, got = [], []

    class Recording(sampler.NoiseSource):
        def next(self, numel):
            z, off = super().next(numel)
            assert z is None
            log.append(off)
            return z, off

    def step(x, tv, coef_row, z, key, off):
        got.append((key, off))
        return ops.sde_update(x, coef_row, y=Y, score=None, noise=z, offset=off, **sampler.row_seed_kw(key))

    def run(denoise):
        log.clear()
        got.clear()
        ns = Recording(seed=0xABCDEF0123, row_seeds=seeds)
        out, nfe = sampler.pc_sample(step, Y, sde, N=N, noise=ns, denoise=denoise)
        torch.cuda.synchronize()
        assert nfe == 2 * N and len(log) == 2 * N + 1 and [o for _, o in got] == log[1:]
        for key, _ in got:
            assert torch.equal(key.cpu(), torch.tensor(seeds)) if row_seeded else key == 0xABCDEF0123
        return cnp(out)

    x_gpu, xm_gpu = run(False), run(True)
    offsets = list(log)
    assert sr.ranges_disjoint([sr.counter_ranges(o, B, HW, seeds) for o in offsets])
    assert len(set(offsets)) == len(offsets)

    def z_ref(off):
        return sr.row_normals(seeds, off, HW) if row_seeded else sr.batch_normals(0xABCDEF0123, off, B, HW)

    steps, prior, _ = sampler.build_schedule(sde, N, 0.03, "reverse_diffusion", "ald", 0.5, 1)
    rows = [np.asarray(c, np.float32).astype(np.float64) for _, _, c in steps]  # the float32 table the loop uploads
    y = cnp(Y)
    cf = np.asarray(prior, np.float32).astype(np.float64)
    _, x, _, m = sr.update(np.zeros_like(y), [cf] * B, y=y, z=z_ref(offsets[0]))
    e = e_mean = sr.STEP_ROUNDINGS * sr.U * max(m.real.max(), m.imag.max()) + sr.NOISE_ATOL * abs(cf[3])
    xm = x
    for cf, off in zip(rows, offsets[1:]):
        xm, x, mm, mo = sr.update(x, [cf] * B, y=y, z=z_ref(off))
        e_mean = abs(cf[0]) * e + sr.STEP_ROUNDINGS * sr.U * max(mm.real.max(), mm.imag.max())
        e = abs(cf[0]) * e + sr.STEP_ROUNDINGS * sr.U * max(mo.real.max(), mo.imag.max()) + sr.NOISE_ATOL * abs(cf[3])
    kind = "row-seeded" if row_seeded else "batch-keyed"
    for name, a, ref, bound in (("x", x_gpu, x, e), ("x_mean", xm_gpu, xm, e_mean)):
        err = part_err(a, ref)
        sr.record("pc_sample zero-score replay", f"{kind} final {name}", err, bound, "max abs difference per part")
        assert err <= bound, (name, err, bound)


# ================================================================================================ step kernels
SHAPES = [(1, 8, 8), (3, 8, 25), (5, 16, 24)]  # the last two: one 256-thread block spans two batch rows
T_ROWS = [0.03, 0.17783, 0.5, 1.0]  # 0.03 is the sampler's lower limit; a fifth row takes the first value again
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]


def step_inputs(gpu, shape, dtype=torch.float32, seed=0):
    """Per-row t and coef rows that differ in all four entries; a pyramid, x, y, a score and a noise tape."""
    B, H, W = shape
    g = gen(100 + seed + B * H * W)
    d = {"pyr": torch.randn(B, H, W, 4, generator=g).to(dtype), "out_w": torch.randn(2, 4, generator=g) * 0.5,
         "out_b": torch.randn(2, generator=g) * 0.2, "t": torch.tensor([T_ROWS[b % 4] for b in range(B)]),
         "x": crandn(g, B, H, W), "y": crandn(g, B, H, W) * 0.7, "score": crandn(g, B, H, W) * 2.0,
         "z": crandn(g, B, H, W) * math.sqrt(0.5)}
    coef = torch.tensor([[1.0 + 0.21 * b, -0.35 - 0.13 * b, 0.02 + 0.017 * b, 0.11 + 0.07 * b] for b in range(B)])
    assert all(len(set(coef[:, i].tolist())) == B for i in range(4))
    d["coef"] = coef
    dev = {k: v.to(gpu).contiguous() for k, v in d.items()}
    ref = {k: cnp(d[k]) for k in ("x", "y", "score", "z")}
    ref["pyr"] = d["pyr"].float().double().numpy().reshape(B, H * W, 4)  # (bfloat16 upcasts exactly)
    for k in ("out_w", "out_b", "t", "coef"):
        ref[k] = d[k].double().numpy()
    return dev, ref


def check_step(kernel, case, out, ref, m):
    out = cnp(out)
    assert np.isfinite(out.real).all() and np.isfinite(out.imag).all(), (kernel, case)
    r = sr.ratio(out, ref, m)
    sr.record(kernel, case, r, sr.STEP_ROUNDINGS, "worst err / (2^-24 M)")
    assert r <= sr.STEP_ROUNDINGS, f"{kernel} {case}: err = {r:.2f} x 2^-24 M, more than {sr.STEP_ROUNDINGS:.0f} roundings"


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("score_mode", [0, 1])
def test_score_update_vs_fp64(gpu, score_mode, dtype, shape):
    """Head + score (both modes) + update with a noise tape: x_out, xmean_out and score_out, per-row t and coef."""
    from snrse import ops
    d, r = step_inputs(gpu, shape, dtype)
    xo, xm, sc = ops.score_update(d["pyr"], d["out_w"], d["out_b"], d["t"], score_mode, d["x"], d["y"],
                                  coef=d["coef"], noise=d["z"], want_score=True)
    torch.cuda.synchronize()
    sc_ref, m_sc = sr.head(r["pyr"], r["out_w"], r["out_b"], r["t"], score_mode, r["x"])
    xm_ref, xo_ref, mm, mo = sr.update(r["x"], r["coef"], y=r["y"], score=sc_ref, z=r["z"], m_score=m_sc)
    case = f"mode {score_mode} {'f32' if dtype == torch.float32 else 'bf16'} {'x'.join(map(str, shape))}"
    check_step("snrse_score_update score_out", case, sc, sc_ref, m_sc)
    check_step("snrse_score_update xmean_out", case, xm, xm_ref, mm)
    check_step("snrse_score_update x_out", case, xo, xo_ref, mo)


@pytest.mark.parametrize("score_mode", [0, 1])
def test_score_update_optional_arguments(gpu, score_mode):
    """coef=None writes the same score and nothing else; y=None is y = 0; given x_out / xmean_out buffers are
    the ones written; the row-seeded entry with a tape is the plain one; a float16 pyramid is refused."""
    from snrse import ops
    d, r = step_inputs(gpu, (3, 8, 25))
    head = (d["pyr"], d["out_w"], d["out_b"], d["t"], score_mode, d["x"])
    xo, xm, sc = ops.score_update(*head, d["y"], coef=d["coef"], noise=d["z"], want_score=True)
    n0, n1, sc_only = ops.score_update(*head, d["y"], want_score=True)
    assert n0 is None and n1 is None and torch.equal(sc_only, sc)
    sc_ref, m_sc = sr.head(r["pyr"], r["out_w"], r["out_b"], r["t"], score_mode, r["x"])
    check_step("snrse_score_update score_out", f"mode {score_mode} score only", sc_only, sc_ref, m_sc)
    # y = NULL
    a = ops.score_update(*head, None, coef=d["coef"], noise=d["z"])
    b = ops.score_update(*head, torch.zeros_like(d["y"]), coef=d["coef"], noise=d["z"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] is None
    xm_ref, xo_ref, mm, mo = sr.update(r["x"], r["coef"], score=sc_ref, z=r["z"], m_score=m_sc)
    check_step("snrse_score_update xmean_out", f"mode {score_mode} y NULL", a[1], xm_ref, mm)
    check_step("snrse_score_update x_out", f"mode {score_mode} y NULL", a[0], xo_ref, mo)
    # preallocated outputs
    bx = torch.full_like(d["x"], float("nan"))
    bm = torch.full_like(d["x"], float("nan"))
    px, pm, _ = ops.score_update(*head, d["y"], coef=d["coef"], noise=d["z"], x_out=bx, xmean_out=bm)
    assert px is bx and pm is bm and torch.equal(bx, xo) and torch.equal(bm, xm)
    # the row-seeded entry, tape given: the tape wins
    rx, rm, rs = ops.score_update(*head, d["y"], coef=d["coef"], noise=d["z"], want_score=True, row_seeds=[1, 2, 3],
                                  offset=9)
    assert torch.equal(rx, xo) and torch.equal(rm, xm) and torch.equal(rs, sc)
    with pytest.raises(TypeError):
        ops.score_update(d["pyr"].half(), *head[1:], d["y"], want_score=True)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("with_score", [True, False], ids=["score", "noscore"])
@pytest.mark.parametrize("with_y", [True, False], ids=["y", "noy"])
def test_sde_update_vs_fp64(gpu, with_y, with_score, shape):
    from snrse import ops
    d, r = step_inputs(gpu, shape, seed=1)
    y, s = (d["y"] if with_y else None), (d["score"] if with_score else None)
    xo, xm = ops.sde_update(d["x"], d["coef"], y=y, score=s, noise=d["z"])
    torch.cuda.synchronize()
    xm_ref, xo_ref, mm, mo = sr.update(r["x"], r["coef"], y=r["y"] if with_y else None,
                                       score=r["score"] if with_score else None, z=r["z"])
    case = f"{'y' if with_y else 'no y'}, {'score' if with_score else 'no score'} {'x'.join(map(str, shape))}"
    check_step("snrse_sde_update xmean_out", case, xm, xm_ref, mm)
    check_step("snrse_sde_update x_out", case, xo, xo_ref, mo)
    rx, rm = ops.sde_update(d["x"], d["coef"], y=y, score=s, noise=d["z"], row_seeds=list(range(shape[0])), offset=4)
    assert torch.equal(rx, xo) and torch.equal(rm, xm)
    bx, bm = torch.full_like(xo, float("nan")), torch.full_like(xo, float("nan"))
    px, pm = ops.sde_update(d["x"], d["coef"], y=y, score=s, noise=d["z"], x_out=bx, xmean_out=bm)
    assert px is bx and pm is bm and torch.equal(bx, xo) and torch.equal(bm, xm)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("with_x", [True, False], ids=["x", "nox"])
@pytest.mark.parametrize("with_y", [True, False], ids=["y", "noy"])
def test_axpby_noise_vs_fp64(gpu, with_y, with_x, shape):
    """out = a x + by y + s z (coef[2] is not used); x = y = NULL takes its shape from like=."""
    from snrse import ops
    d, r = step_inputs(gpu, shape, seed=2)
    x, y = (d["x"] if with_x else None), (d["y"] if with_y else None)
    out = ops.axpby_noise(d["coef"], x=x, y=y, noise=d["z"], like=d["x"])
    torch.cuda.synchronize()
    cf = r["coef"].copy()
    cf[:, 2] = 0.0
    _, ref, _, m = sr.update(r["x"] if with_x else np.zeros_like(r["x"]), cf, y=r["y"] if with_y else None, z=r["z"])
    case = f"{'x' if with_x else 'no x'}, {'y' if with_y else 'no y'} {'x'.join(map(str, shape))}"
    check_step("snrse_axpby_noise", case, out, ref, m)
    rs = ops.axpby_noise(d["coef"], x=x, y=y, noise=d["z"], like=d["x"], row_seeds=list(range(shape[0])), offset=2)
    assert torch.equal(rs, out)


@pytest.mark.parametrize("row_seeded", [False, True], ids=["batch-keyed", "row-seeded"])
@pytest.mark.parametrize("kernel", ["score_update", "sde_update"])
def test_in_kernel_noise_through_step_kernels(gpu, kernel, row_seeded):
    """x_out - xmean_out = s z with z drawn in the kernel: the row's own s, the element's own counter.  Bound:
    4e-6 |s| for z, plus the rounding of the product (2^-24 |s z|) and of the sum (2^-24 |x_out|)."""
    from snrse import ops
    shape = (3, 8, 25)
    B, HW = shape[0], shape[1] * shape[2]
    d, r = step_inputs(gpu, shape, seed=3)
    seeds = [-3, 0x7FFFFFFFFFFFFFFF, 12345]
    kw = {"row_seeds": seeds, "offset": 6} if row_seeded else {"seed": 0xFEEDFACECAFEBEEF, "offset": 2 ** 32 - 250}
    z_ref = sr.row_normals(seeds, 6, HW) if row_seeded else sr.batch_normals(0xFEEDFACECAFEBEEF, 2 ** 32 - 250, B, HW)
    if kernel == "score_update":
        xo, xm, _ = ops.score_update(d["pyr"], d["out_w"], d["out_b"], d["t"], 1, d["x"], d["y"], coef=d["coef"], **kw)
    else:
        xo, xm = ops.sde_update(d["x"], d["coef"], y=d["y"], score=d["score"], **kw)
    torch.cuda.synchronize()
    xo, xm = cnp(xo), cnp(xm)
    s = r["coef"][:, 3:4]
    want = s * z_ref
    diff = (xo - xm) - want
    tol_re = sr.NOISE_ATOL * np.abs(s) + sr.U * (np.abs(want.real) + np.abs(xo.real))
    tol_im = sr.NOISE_ATOL * np.abs(s) + sr.U * (np.abs(want.imag) + np.abs(xo.imag))
    worst = float(max((np.abs(diff.real) / tol_re).max(), (np.abs(diff.imag) / tol_im).max()))
    sr.record(f"snrse_{kernel} in-kernel noise", "row-seeded" if row_seeded else "batch-keyed", worst, 1.0,
              "worst |x_out - xmean_out - s z_ref| / tolerance")
    assert worst <= 1.0


def test_step_kernel_argument_checks(gpu):
    """SNRSE_EINVAL (hipErrorInvalidValue, code 1) and nothing written: an empty batch, x_out without coef, and the
    row-seeded entries with neither seeds nor tape."""
    from snrse import _lib
    d, _ = step_inputs(gpu, (3, 8, 25))
    B, HW = 3, 200
    outs = [torch.full_like(d["x"], complex("nan+nanj")) for _ in range(3)]
    p = {k: v.data_ptr() for k, v in d.items()}
    o = [t.data_ptr() for t in outs]
    rs = torch.tensor([1, 2, 3], dtype=torch.int64, device=gpu)
    st = torch.cuda.current_stream().cuda_stream
    head = (p["pyr"], 1, p["out_w"], p["out_b"], p["t"], 1)
    bad = [
        ("snrse_score_update", head + (0, HW, p["x"], p["y"], p["z"], 0, 0, p["coef"], o[0], o[1], o[2], st)),
        ("snrse_score_update", head + (B, 0, p["x"], p["y"], p["z"], 0, 0, p["coef"], o[0], o[1], o[2], st)),
        ("snrse_score_update", head + (B, HW, p["x"], p["y"], p["z"], 0, 0, None, o[0], o[1], o[2], st)),
        ("snrse_score_update_rs", head + (B, HW, p["x"], p["y"], None, None, 0, p["coef"], o[0], o[1], o[2], st)),
        ("snrse_sde_update", (p["x"], p["y"], p["score"], p["z"], 0, 0, p["coef"], 0, HW, o[0], o[1], st)),
        ("snrse_sde_update", (p["x"], p["y"], p["score"], p["z"], 0, 0, p["coef"], B, 0, o[0], o[1], st)),
        ("snrse_sde_update_rs", (p["x"], p["y"], p["score"], None, None, 0, p["coef"], B, HW, o[0], o[1], st)),
        ("snrse_axpby_noise", (p["x"], p["y"], p["z"], 0, 0, p["coef"], 0, HW, o[0], st)),
        ("snrse_axpby_noise", (p["x"], p["y"], p["z"], 0, 0, p["coef"], B, 0, o[0], st)),
        ("snrse_axpby_noise_rs", (p["x"], p["y"], None, None, 0, p["coef"], B, HW, o[0], st)),
    ]
    for name, args in bad:
        with pytest.raises(RuntimeError, match=r"\(code 1\)"):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert all(torch.isnan(torch.view_as_real(t)).all() for t in outs)
    # the same row-seeded calls with seeds go through
    _lib.call("snrse_axpby_noise_rs", p["x"], p["y"], None, rs.data_ptr(), 0, p["coef"], B, HW, o[0], st)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.view_as_real(outs[0])).all()


# ================================================================================================ time embedding
@pytest.mark.parametrize("B,R,D", [(1, 1, 4), (3, 70, 20), (33, 64, 512), (32, 65, 36), (40, 130, 256)])
def test_temb_dense_off_network_shapes(gpu, B, R, D):
    """out = silu(x) W^T + b for D that is no multiple of the 16-input step (20, 36), R that leaves a partial wave
    (65, 70, 130) and B past one 32-row LDS batch (33, 40).  x, W and b are the heads of larger buffers whose
    tails are NaN: the clamped row read past R and the table's zero fill past D and B do not leak."""
    from snrse import ops
    g = gen(B * 1000 + R + D)
    xb = torch.full((B * D + 2048,), float("nan"))
    wb = torch.full((R * D + 64 * 512,), float("nan"))
    bb = torch.full((R + 64,), float("nan"))
    xb[:B * D] = torch.randn(B * D, generator=g) * 1.5
    wb[:R * D] = torch.randn(R * D, generator=g) / math.sqrt(D)
    bb[:R] = torch.randn(R, generator=g) * 0.3
    xb, wb, bb = xb.to(gpu), wb.to(gpu), bb.to(gpu)
    x, W, b = xb[:B * D].view(B, D), wb[:R * D].view(R, D), bb[:R]
    out = ops.temb_dense(x, W, b)
    torch.cuda.synchronize()
    assert out.shape == (B, R) and torch.isfinite(out).all()
    ref = sr.temb_dense(x.cpu().numpy(), W.cpu().numpy(), b.cpu().numpy())
    e = sr.rel(out.cpu().numpy().astype(np.float64), ref)
    sr.record("snrse_temb_dense", f"B {B} R {R} D {D}", e, 1e-5, "relative RMS")
    assert e < 1e-5
    # every element written: the same call into a NaN-filled buffer through the C entry
    from snrse import _lib
    buf = torch.full((B * R + 256,), float("nan"), device=gpu)
    _lib.call("snrse_temb_dense", x.data_ptr(), W.data_ptr(), b.data_ptr(), buf.data_ptr(), B, R, D,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(buf[:B * R].view(B, R), out) and torch.isnan(buf[B * R:]).all()


def gfp_inputs(gpu, B, nf):
    g = gen(B * 100 + nf)
    t = torch.tensor([T_ROWS[i % 4] for i in range(B)]) * (1.0 - 0.01 * (torch.arange(B) // 4))
    t = t.clamp(min=0.03)
    d = {"t": t, "Wg": torch.randn(nf, generator=g), "W1": torch.randn(4 * nf, 2 * nf, generator=g) / math.sqrt(2 * nf),
         "b1": torch.randn(4 * nf, generator=g) * 0.3, "W2": torch.randn(4 * nf, 4 * nf, generator=g) / math.sqrt(4 * nf),
         "b2": torch.randn(4 * nf, generator=g) * 0.3}
    return {k: v.to(gpu).contiguous() for k, v in d.items()}, {k: v.double().numpy() for k, v in d.items()}


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("nf", [2, 6, 128])
def test_temb_gfp_dense_vs_fp64(gpu, nf, B):
    """W1 [sin, cos](2 pi log(t) Wg) + b1 through the C entry into a NaN-filled buffer, then the whole
    ops.temb_mlp(fused=False) pair, against the float64 Gaussian-Fourier projection."""
    from snrse import _lib, ops
    d, r = gfp_inputs(gpu, B, nf)
    buf = torch.full((B * 4 * nf + 256,), float("nan"), device=gpu)
    _lib.call("snrse_temb_gfp_dense", d["t"].data_ptr(), d["Wg"].data_ptr(), d["W1"].data_ptr(), d["b1"].data_ptr(),
              buf.data_ptr(), B, nf, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = buf[:B * 4 * nf].view(B, 4 * nf)
    assert torch.isfinite(out).all() and torch.isnan(buf[B * 4 * nf:]).all()
    ref = sr.gfp_dense(r["t"], r["Wg"], r["W1"], r["b1"])
    e = sr.rel(out.cpu().numpy().astype(np.float64), ref)
    sr.record("snrse_temb_gfp_dense", f"B {B} nf {nf}", e, 1e-5, "relative RMS")
    assert e < 1e-5
    te = ops.temb_mlp(d["t"], d["Wg"], d["W1"], d["b1"], d["W2"], d["b2"], fused=False)
    torch.cuda.synchronize()
    ref2 = sr.silu(ref) @ r["W2"].T + r["b2"]
    e2 = sr.rel(te.cpu().numpy().astype(np.float64), ref2)
    sr.record("temb_mlp(fused=False)", f"B {B} nf {nf}", e2, 1e-5, "relative RMS")
    assert te.shape == (B, 4 * nf) and e2 < 1e-5


@pytest.mark.parametrize("nf", [130, 3, 127, 0])
def test_temb_gfp_dense_refuses(gpu, nf):
    """4 nf > 512 does not fit the table of the second launch, an odd nf breaks the 4-float pieces."""
    from snrse import _lib
    n = max(nf, 1)
    t = torch.full((2,), 0.5, device=gpu)
    Wg, W1, b1 = torch.zeros(n, device=gpu), torch.zeros(4 * n, 2 * n, device=gpu), torch.zeros(4 * n, device=gpu)
    buf = torch.full((2 * 4 * n,), float("nan"), device=gpu)
    with pytest.raises(RuntimeError, match=r"\(code 1\)"):
        _lib.call("snrse_temb_gfp_dense", t.data_ptr(), Wg.data_ptr(), W1.data_ptr(), b1.data_ptr(), buf.data_ptr(), 2,
                  nf, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


# ================================================================================================ front end
STFT_LENGTHS = [256, 383, 384, 1023, 1024, 1025]  # the shortest; across a hop boundary; T = 8, 9, 9 frames


def stft_inputs(gpu, L):
    g = gen(7000 + L)
    sig = torch.randn(3, L, generator=g) * 0.3
    in_div = torch.tensor([0.5, 1.25, 2.0])
    out_scale = torch.tensor([0.75, 1.5, 0.3125])
    return sig, in_div, out_scale


@pytest.mark.parametrize("L", STFT_LENGTHS)
def test_stft_istft_edge_lengths(gpu, L):
    """L = 256 reflects to sample 0 and sample L - 1; 383 / 384 step the frame count; 1024 gives T = 9: one frame
    into a second 8-frame STFT block and a third 4-frame iSTFT block.  Per-row in_div and out_scale."""
    from snrse import ops
    sig, in_div, out_scale = stft_inputs(gpu, L)
    T = 1 + L // 128
    assert T == spec_ref.n_frames(L)
    in_scale = 0.75
    scaled = sig.double().numpy() * in_scale / in_div.double().numpy()[:, None]
    ref = spec_ref.stft(scaled)
    raw = ops.stft(sig.to(gpu), in_scale, mode=0, in_div=in_div.to(gpu))
    cmp = ops.stft(sig.to(gpu), in_scale, mode=1, in_div=in_div.to(gpu))
    torch.cuda.synchronize()
    assert raw.shape == (3, 256, T) and cmp.shape == (3, 256, T)
    e0 = sr.rel(raw.cpu().numpy().astype(np.complex128), ref)
    e1 = sr.rel(cmp.cpu().numpy().astype(np.complex128), spec_ref.spec_fwd(ref))
    sr.record("snrse_stft raw", f"L {L}", e0, 1e-5, "relative RMS")
    sr.record("snrse_stft exponent", f"L {L}", e1, 2e-5, "relative RMS")
    assert e0 < 1e-5 and e1 < 2e-5
    # per row, so that a row scaled with another row's in_div cannot hide in the batch's RMS
    for b in range(3):
        assert sr.rel(raw[b].cpu().numpy().astype(np.complex128), ref[b]) < 1e-5, b
    # the inverse of the kernel's own spectra (exact upcasts), per-row out_scale
    osc = out_scale.double().numpy()[:, None]
    for mode, spec, back, tol in ((0, raw, lambda s: s, 1e-5), (1, cmp, spec_ref.spec_back, 2e-5)):
        w = ops.istft(spec, L, mode=mode, out_scale=out_scale.to(gpu))
        torch.cuda.synchronize()
        wref = spec_ref.istft(back(spec.cpu().numpy().astype(np.complex128)), L) * osc
        assert w.shape == (3, L)
        e = sr.rel(w.cpu().numpy().astype(np.float64), wref)
        sr.record(f"snrse_istft mode {mode}", f"L {L}", e, tol, "relative RMS")
        assert e < tol
        for b in range(3):
            assert sr.rel(w[b].cpu().numpy().astype(np.float64), wref[b]) < tol, (mode, b)
        plain = ops.istft(spec, L, mode=mode)
        e = sr.rel(plain.cpu().numpy().astype(np.float64), wref / osc)
        assert e < tol


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("L", STFT_LENGTHS)
def test_stft_padded_frames(gpu, L, mode):
    """tpad in {T, T + 1, 64}: frames [T, tpad) are exactly zero and frames [0, T) the unpadded call's, bitwise."""
    from snrse import ops
    sig, in_div, _ = stft_inputs(gpu, L)
    T = 1 + L // 128
    base = ops.stft(sig.to(gpu), 0.75, mode=mode, in_div=in_div.to(gpu))
    for tpad in (T, T + 1, 64):
        out = ops.stft(sig.to(gpu), 0.75, tpad=tpad, mode=mode, in_div=in_div.to(gpu))
        torch.cuda.synchronize()
        assert out.shape == (3, 256, tpad)
        assert torch.equal(out[..., :T], base)
        assert torch.all(torch.view_as_real(out[..., T:].contiguous()) == 0)
        # the ragged entry at equal lengths is the same transform
        rag = ops.stft(sig.to(gpu), 0.75, tpad=tpad, mode=mode, in_div=in_div.to(gpu), lengths=[L] * 3)
        assert torch.equal(rag, out)


def test_stft_refuses_255_samples(gpu):
    """255 samples cannot be reflected by 255 (torch.stft refuses them too): plain and ragged."""
    from snrse import ops
    sig = torch.zeros(2, 255, device=gpu)
    with pytest.raises(RuntimeError):
        ops.stft(sig, 1.0, mode=0)
    with pytest.raises(RuntimeError):
        ops.stft(torch.zeros(2, 400, device=gpu), 1.0, mode=0, lengths=[400, 255])
    assert ops.stft(torch.zeros(2, 400, device=gpu), 1.0, mode=0, lengths=[400, 256]).shape == (2, 256, 4)


def spec_values(n):
    """Exact zero, purely real and purely imaginary values, magnitudes 1e-12 and 1e6, then normal draws."""
    special = torch.tensor([0j, 3.0 + 0j, -2.5j, -0.7 + 0j, 4.0j, 1e-12 * (0.6 + 0.8j), 1e6 * (-0.6 + 0.8j),
                            1e-12 + 0j, 1e6j, 0j], dtype=C64)
    v = torch.cat([special, crandn(gen(n), max(n, 1)) * 2.0])
    return v[:n].contiguous()


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_spec_transform_vs_complex128(gpu, n):
    """0.15 c / sqrt|c| and (s / 0.15) |s / 0.15| elementwise; 0 + 0j gives exactly 0 both ways; in place is out of
    place; back(fwd(x)) is x within the sum of both bounds."""
    from snrse import _lib, ops
    x = spec_values(n).to(gpu)
    xr = x.cpu().numpy().astype(np.complex128)
    outs = {}
    for direction, fn in ((0, sr.spec_fwd), (1, sr.spec_back)):
        out = ops.spec_transform(x, direction)
        torch.cuda.synchronize()
        outs[direction] = out
        o, ref = out.cpu().numpy().astype(np.complex128), fn(xr)
        assert out.shape == x.shape and np.isfinite(o.real).all() and np.isfinite(o.imag).all()
        zero = xr == 0
        assert np.all(o[zero] == 0) and np.all(o[~zero] != 0)
        assert np.all(o.imag[xr.imag == 0] == 0) and np.all(o.real[xr.real == 0] == 0)  # real stays real
        worst = float((np.abs(o - ref)[~zero] / (sr.U * np.abs(ref)[~zero])).max()) if (~zero).any() else 0.0
        sr.record(f"snrse_spec_transform direction {direction}", f"n {n}", worst, 8.0, "worst |err| / (2^-24 |ref|)")
        assert worst <= 8.0
        inplace = x.clone()
        _lib.call("snrse_spec_transform", inplace.data_ptr(), inplace.data_ptr(), n, direction,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(inplace), torch.view_as_real(out))
    rt = ops.spec_transform(outs[0], 1).cpu().numpy().astype(np.complex128)
    nz = xr != 0
    worst = float((np.abs(rt - xr)[nz] / (sr.U * np.abs(xr)[nz])).max()) if nz.any() else 0.0
    sr.record("snrse_spec_transform back(fwd(x))", f"n {n}", worst, 16.0, "worst |err| / (2^-24 |x|)")
    assert worst <= 16.0 and np.all(rt[~nz] == 0)


@pytest.mark.parametrize("L", [256, 1000])
def test_spec_transform_is_the_stft_and_istft_transform(gpu, L):
    """stft(mode=1) is spec_transform(stft(mode=0), 0), and istft(mode=1) is istft(spec_transform(., 1), mode=0),
    bitwise: one formula in three kernels."""
    from snrse import ops
    sig, in_div, out_scale = stft_inputs(gpu, L)
    raw = ops.stft(sig.to(gpu), 0.75, mode=0, in_div=in_div.to(gpu))
    cmp = ops.stft(sig.to(gpu), 0.75, mode=1, in_div=in_div.to(gpu))
    assert torch.equal(torch.view_as_real(ops.spec_transform(raw, 0)), torch.view_as_real(cmp))
    a = ops.istft(cmp, L, mode=1, out_scale=out_scale.to(gpu))
    b = ops.istft(ops.spec_transform(cmp, 1), L, mode=0, out_scale=out_scale.to(gpu))
    assert torch.equal(a, b)


@pytest.mark.parametrize("L", [1, 63, 64, 255, 256, 257, 1000])
def test_absmax_exact(gpu, L):
    """max |sig| per row, exactly: the maximum first, last, and negative; a row of zeros; rows with +-inf."""
    from snrse import ops
    g = gen(L)
    rows = torch.rand(7, L, generator=g) * 2.0 - 1.0
    rows[0, 0] = 1.5
    rows[1, L - 1] = 1.25
    rows[2, L // 2] = -1.75
    rows[3] = 0.0
    rows[4, L // 3] = float("inf")
    rows[5, L - 1] = float("-inf")
    rows[6] *= 1e-30  # small values: nothing is flushed or compared against a floor above 0
    out = ops.absmax(rows.to(gpu))
    torch.cuda.synchronize()
    ref = np.abs(rows.numpy()).max(axis=1)
    assert out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), ref)
    assert out[3] == 0 and out[4] == float("inf") and out[5] == float("inf")
    assert out[0] == 1.5 and out[1] == 1.25 and out[2] == 1.75
    rag = ops.absmax(rows.to(gpu), lengths=[L] * 7)
    assert torch.equal(rag, out)


def test_absmax_skips_nan(gpu):
    """The kernel folds with fmaxf, which returns its other operand for a NaN: a row's result is the maximum of
    its non-NaN samples (0 for a row of NaN only), where torch.abs().max() gives NaN (include/snrse.h)."""
    from snrse import ops
    rows = torch.rand(4, 300, generator=gen(9)) - 0.5
    rows[0, 0] = float("nan")
    rows[1, 299] = float("nan")
    rows[1, 17] = -3.0
    rows[2] = float("nan")
    rows[3, 100] = float("nan")
    rows[3, 101] = float("inf")
    out = ops.absmax(rows.to(gpu)).cpu().numpy()
    ref = np.nanmax(np.abs(np.where(np.isnan(rows.numpy()), 0.0, rows.numpy())), axis=1)
    assert np.array_equal(out, ref.astype(np.float32)) and out[1] == 3.0 and out[2] == 0.0 and out[3] == np.inf
    assert torch.isnan(rows.abs().max(dim=1).values).all()


@pytest.mark.parametrize("L", [2, 511, 512, 513])
def test_energy_ratios_edge_lengths(gpu, L):
    """SI-SDR / SI-SIR / SI-SAR around the 512-thread block and at two samples, with and without n."""
    from snrse import ops
    from test_metrics import np_energy_ratios
    g = gen(300 + L)
    s = torch.randn(3, L, generator=g) * 0.2
    n = torch.randn(3, L, generator=g) * 0.05
    sh = 0.9 * s + 0.6 * n + 0.03 * torch.randn(3, L, generator=g)
    out = ops.energy_ratios(sh.to(gpu), s.to(gpu), n.to(gpu)).cpu().numpy()
    only = ops.energy_ratios(sh.to(gpu), s.to(gpu)).cpu().numpy()
    ref = np.array([np_energy_ratios(sh[b].numpy(), s[b].numpy(), n[b].numpy()) for b in range(3)])
    e = float(np.abs(out - ref).max())
    sr.record("snrse_energy_ratios", f"L {L}", e, 1e-6, "max abs difference, dB")
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-6)
    np.testing.assert_allclose(only[:, 0], ref[:, 0], rtol=0, atol=1e-6)
    assert np.isnan(only[:, 1:]).all()
    # s_hat = 2 s exactly: every sum scales by a power of two, the distortion is exactly 0
    twice = ops.energy_ratios((2.0 * s).to(gpu), s.to(gpu), n.to(gpu)).cpu().numpy()
    assert np.all(twice[:, 0] == np.inf)
    assert np.all(ops.energy_ratios((2.0 * s).to(gpu), s.to(gpu)).cpu().numpy()[:, 0] == np.inf)
