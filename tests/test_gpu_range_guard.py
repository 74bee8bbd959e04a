"""GPU tests of the fp16 range guard: the snrse_range_stats kernel against torch, the range probe
(NCSNppHIP.range_report), and the guard of PCEnhancer / SNRAlignedEnhancer / ScoreModel.enhance on utterances and
weights that fp16 cannot hold.

"Matches" below is the project's bound for the same computation under another batch split
(test_pc_enhancer_two_streams_matches_one): per-row relative RMS < 2e-2 between 16-bit runs.  Bit equality is not
asked for: the order of the fp64 statistics atomics and the split-K choice depend on B."""
import warnings

import numpy as np
import pytest
import torch

from conftest import fnormal, formula_sd

pytestmark = pytest.mark.gpu

TOL16 = 2e-2
FP16_MAX = 65504.0
SCALED = ("all_modules.4.Conv_1.weight", "all_modules.4.Conv_1.bias")  # x 1e6: module 4's output leaves fp16


def rel(a, b):
    a = torch.as_tensor(a).detach().cpu()
    b = torch.as_tensor(b).detach().cpu()
    dt = torch.complex128 if (a.is_complex() or b.is_complex()) else torch.float64
    a, b = a.to(dt), b.to(dt)
    return float((a - b).abs().pow(2).mean().sqrt() / (b.abs().pow(2).mean().sqrt() + 1e-30))


def all_finite(x):
    return bool(torch.isfinite(torch.view_as_real(x) if x.is_complex() else x).all())


@pytest.fixture(scope="module")
def sds():
    sd = {k: torch.from_numpy(v) for k, v in formula_sd("ncsnpp").items()}
    big = dict(sd)
    for k in SCALED:
        big[k] = sd[k] * 1e6
    return {"formula": sd, "scaled": big}


@pytest.fixture(scope="module")
def nets(gpu, sds):
    """Executors built on first use: nets(weights, dtype)."""
    from snrse import ncsnpp
    held = {}

    def get(which, dtype):
        if (which, dtype) not in held:
            held[(which, dtype)] = ncsnpp.NCSNppHIP(sds[which], dtype=dtype, device=gpu)
        return held[(which, dtype)]

    return get


@pytest.fixture(scope="module")
def sde():
    from snrse import sampler
    return sampler.SDESpec("ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5)


def spec(name, B, gpu):
    return (torch.from_numpy(fnormal(name, (B, 256, 64), complex_=True)) * 0.5).to(gpu)


# ------------------------------------------------------------------ 1. kernel
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def planted(shape, dtype, seed):
    """Normal values with +inf, -inf, NaN, +-max-finite, -0 and a denormal in row 0, -max-finite last and a
    denormal first in the middle rows, and a last row that is entirely non-finite."""
    B, per = shape
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(B, per, generator=g) * 3).to(dtype)
    fi = torch.finfo(dtype)
    vals = [float("inf"), -float("inf"), float("nan"), fi.max, -fi.max, -0.0, fi.smallest_normal / 4]
    for k, v in enumerate(vals):
        t[0, (k * 977) % per] = v
    for r in range(1, B - 1):
        t[r, 0] = fi.smallest_normal / 4
        t[r, per - 1] = -fi.max
    t[B - 1] = torch.tensor([float("inf"), float("nan"), -float("inf")], dtype=dtype).repeat(per // 3 + 1)[:per]
    return t


def torch_stats(t):
    a = t.float().abs()
    fin = torch.isfinite(a)
    return torch.where(fin, a, torch.zeros_like(a)).amax(1), (~fin).sum(1).to(torch.int32)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(3, 1), (2, 7), (3, 4099), (2, 2 ** 21 + 8)])
def test_range_stats_matches_torch(gpu, shape, dt):
    """Exact equality with torch's |v| and isfinite: rows of one element, rows shorter than a 16-B vector,
    misaligned rows with a scalar tail (4099) and rows of more than one pass per block (2^21 + 8)."""
    from snrse import ops
    t = planted(shape, DTYPES[dt], 1)
    peak, nonfinite = ops.range_stats(t.to(gpu))
    rp, rn = (r.to(gpu) for r in torch_stats(t))  # the reference on the host
    assert peak.dtype == torch.float32 and nonfinite.dtype == torch.int32
    assert torch.equal(peak, rp), (peak.tolist(), rp.tolist())
    assert torch.equal(nonfinite, rn), (nonfinite.tolist(), rn.tolist())
    assert float(peak[-1]) == 0.0 and int(nonfinite[-1]) == shape[1]  # the all-non-finite row
    # accumulate over two tensors: max and sum
    t2 = planted(shape, DTYPES[dt], 2) * 0.5
    p2, n2 = (r.to(gpu) for r in torch_stats(t2))
    ops.range_stats(t2.to(gpu), peak, nonfinite, accumulate=True)
    assert torch.equal(peak, torch.maximum(rp, p2)) and torch.equal(nonfinite, rn + n2)


def test_range_stats_complex_and_saturation(gpu):
    """A complex64 spectrogram is read as 2 * per floats; the count saturates at INT_MAX."""
    from snrse import ops
    x = spec("range.cplx", 2, gpu)
    x[1, 3, 5] = complex(float("nan"), 2.0)
    peak, nonfinite = ops.range_stats(x)
    rp, rn = (r.to(gpu) for r in torch_stats(torch.view_as_real(x).reshape(2, -1).cpu()))
    assert torch.equal(peak, rp) and torch.equal(nonfinite, rn) and nonfinite.tolist() == [0, 1]
    full = torch.full((2,), 2 ** 31 - 2, device=gpu, dtype=torch.int32)
    ops.range_stats(torch.full((2, 5), float("inf"), device=gpu), torch.zeros(2, device=gpu), full, accumulate=True)
    assert full.tolist() == [2 ** 31 - 1] * 2


def test_range_stats_bad_arguments(gpu):
    from snrse import _lib, ops
    t = torch.zeros(2, 8, device=gpu)
    peak, nf = torch.zeros(2, device=gpu), torch.zeros(2, device=gpu, dtype=torch.int32)
    good = [t.data_ptr(), 2, 8, _lib.F32, peak.data_ptr(), nf.data_ptr(), 0, None]
    _lib.call("snrse_range_stats", *good)
    for i, bad in ((0, None), (4, None), (5, None), (1, 0), (1, -1), (2, 0), (3, _lib.F64), (3, _lib.F32X3), (3, 7)):
        args = list(good)
        args[i] = bad
        with pytest.raises(RuntimeError):
            _lib.call("snrse_range_stats", *args)
    with pytest.raises(RuntimeError):
        ops.range_stats(torch.zeros(2, 8, device=gpu)[:, ::2])  # not contiguous
    with pytest.raises(RuntimeError):
        ops.range_stats(torch.zeros(2, 8))  # not on the device
    assert _lib.load().snrse_abi_version() == 2  # a new entry, no changed signature


# ------------------------------------------------------------------ 2. probe
def probe(net, gpu):
    x, y = spec("range.probe.x", 2, gpu), spec("range.probe.y", 2, gpu)
    return net.range_report(x, y, torch.tensor([0.6, 0.9], device=gpu))


def test_probe_formula_weights(gpu, nets):
    reps = {dt: probe(nets("formula", dt), gpu) for dt in (torch.float16, torch.bfloat16)}
    names = [n for n, _, _ in reps[torch.float16]]
    assert names == [n for n, _, _ in reps[torch.bfloat16]] and len(set(names)) == len(names)
    net = nets("formula", torch.float16)
    seen = {int(n.split(".")[0]) for n in names}
    want = {m.idx for m in net.plan if m.kind in ("rb", "attn", "conv3x3")}
    assert want <= seen, sorted(want - seen)
    order = [int(n.split(".")[0]) for n in names if n.endswith((".conv1", ".nin3"))]
    assert order == sorted(order)  # execution order
    assert "4.rb.conv1" in names and names[0] == "3.conv"
    for rep in reps.values():
        for name, peak, nonfinite in rep:
            assert peak.shape == (2,) and nonfinite.shape == (2,)
            assert int(nonfinite.sum()) == 0, name
            assert float(peak.max()) < FP16_MAX, (name, float(peak.max()))
    assert net._probe is None


def test_probe_finds_the_overflowing_tensor(gpu, nets):
    rb, rh = probe(nets("scaled", torch.bfloat16), gpu), probe(nets("scaled", torch.float16), gpu)
    names = [n for n, _, _ in rb]
    assert names == [n for n, _, _ in rh]
    k = names.index("4.rb.conv1")
    # bf16: the peaks above 65504 come out as finite numbers, the first of them at module 4's Conv_1 output
    assert all(int(nf.sum()) == 0 for _, _, nf in rb)
    over = [n for n, p, _ in rb if float(p.max()) > FP16_MAX]
    assert over and over[0] == "4.rb.conv1", over[:3]
    # fp16: that tensor is stored as inf
    assert int(rh[k][2].sum()) > 0
    for rep in (rb, rh):
        for name, p, nf in rep[:k]:
            assert int(nf.sum()) == 0 and float(p.max()) <= FP16_MAX, name
    from snrse import range_check
    assert range_check.first_offender(rb) == range_check.first_offender(rh) == "4.rb.conv1"
    assert range_check.recommend(rb) == "bf16"


# ------------------------------------------------------------------ 3. per-utterance guard
@pytest.fixture(scope="module")
def loud(gpu):
    """B = 3 with row 1 of Y, and of every draw of the tape, x 1e6: 43 % of row 1's input-conv outputs are above
    65504 (row maximum 5.2e5), the other rows peak at 0.54."""
    Y = spec("range.loud.Y", 3, gpu)
    Y[1] *= 1e6
    draws = {}

    def tape(i):
        if i not in draws:
            z = torch.from_numpy(fnormal(f"range.loud.z.{i}", (3, 256, 64), complex_=True)).to(gpu)
            z[1] *= 1e6
            draws[i] = z
        return draws[i]

    return Y.contiguous(), tape


@pytest.fixture(scope="module")
def loud_unguarded(gpu, nets, sde, loud):
    """Guard-off runs of the whole batch, fp16 and bf16, computed once."""
    from snrse import sampler
    from snrse.enhance import PCEnhancer
    Y, tape = loud
    out = {}
    for dt in (torch.float16, torch.bfloat16):
        src = sampler.NoiseSource(tape=tape)
        x, nfe = PCEnhancer(nets("formula", dt), sde, N=2, guard=None).sample(Y, src)
        out[dt] = (x.clone(), nfe, src.i)
    return out


def test_guard_warn_and_raise(gpu, nets, sde, loud, loud_unguarded):
    from snrse import guard, sampler
    from snrse.enhance import PCEnhancer
    Y, tape = loud
    net = nets("formula", torch.float16)
    x0 = loud_unguarded[torch.float16][0]
    assert [all_finite(x0[k]) for k in range(3)] == [True, False, True]  # what the parent commit returns, silently
    enh = PCEnhancer(net, sde, N=2, guard="warn")
    with pytest.warns(guard.RangeFallbackWarning):
        x, nfe = enh.sample(Y, sampler.NoiseSource(tape=tape))
    assert nfe == 4 and [all_finite(x[k]) for k in range(3)] == [True, False, True]
    assert enh.last_guard["flagged"] == [1] and enh.last_guard["policy"] == "warn"
    with pytest.raises(guard.FloatRangeError) as ei:
        PCEnhancer(net, sde, N=2, guard="raise").sample(Y, sampler.NoiseSource(tape=tape))
    assert ei.value.rows == [1]
    with pytest.raises(ValueError):
        PCEnhancer(net, sde, N=2, guard="sometimes")


def test_guard_fallback_recomputes_the_flagged_row(gpu, nets, sde, loud, loud_unguarded):
    from snrse import guard, sampler
    from snrse.enhance import PCEnhancer
    Y, tape = loud
    net = nets("formula", torch.float16)
    enh = PCEnhancer(net, sde, N=2)  # guard="auto": fallback for an fp16 network
    src = sampler.NoiseSource(tape=tape)
    with pytest.warns(guard.RangeFallbackWarning):
        x, nfe = enh.sample(Y, src)
    assert nfe == 4 and all_finite(x)
    assert enh.last_guard == {"flagged": [1], "policy": "fallback", "fallback_dtype": torch.bfloat16}
    x16, _, i16 = loud_unguarded[torch.float16]
    xbf, _, _ = loud_unguarded[torch.bfloat16]
    assert src.i == i16 == 5
    errs = {1: rel(x[1], xbf[1]), 0: rel(x[0], x16[0]), 2: rel(x[2], x16[2])}
    print("per-row rel RMS:", errs)
    assert all(e < TOL16 for e in errs.values()), errs
    fb = net.fallback()
    assert fb is net.fallback() and fb.dtype == torch.bfloat16 and fb is not net
    assert net.fallback(torch.float16) is net
    with warnings.catch_warnings():  # once per enhancer
        warnings.simplefilter("error", guard.RangeFallbackWarning)
        x2, _ = enh.sample(Y, sampler.NoiseSource(tape=tape))
    assert all_finite(x2) and enh.last_guard["flagged"] == [1]


# ------------------------------------------------------------------ 4. all rows, Philox
def test_guard_all_rows_philox(gpu, nets, sde):
    from snrse import guard, sampler
    from snrse.enhance import PCEnhancer
    Y = spec("range.philox.Y", 2, gpu)
    enh = PCEnhancer(nets("scaled", torch.float16), sde, N=2, guard="fallback")
    src = sampler.NoiseSource(seed=4321)
    with pytest.warns(guard.RangeFallbackWarning):
        x, _ = enh.sample(Y, src)
    ref_src = sampler.NoiseSource(seed=4321)
    ref, _ = PCEnhancer(nets("scaled", torch.bfloat16), sde, N=2, guard=None).sample(Y, ref_src)
    assert enh.last_guard["flagged"] == [0, 1] and all_finite(x) and src.i == ref_src.i
    errs = [rel(x[k], ref[k]) for k in range(2)]
    print("per-row rel RMS:", errs)
    assert max(errs) < TOL16, errs


# ------------------------------------------------------------------ 5. one-step enhancer
def test_snr_aligned_enhancer_guard(gpu, nets):
    from snrse import guard
    from snrse.enhance import SNRAlignedEnhancer
    rng = np.random.default_rng(5)
    y = torch.from_numpy((0.3 * rng.standard_normal((2, 8000))).astype(np.float32)).to(gpu)
    est = np.array([0.1, 0.3])
    enh = SNRAlignedEnhancer(nets("scaled", torch.float16))
    with pytest.warns(guard.RangeFallbackWarning):
        xh, t_hat = enh(y, est_snr=est, seed=9)
    ref, t_ref = SNRAlignedEnhancer(nets("scaled", torch.bfloat16), guard=None)(y, est_snr=est, seed=9)
    assert enh.last_guard["flagged"] == [0, 1] and all_finite(xh) and np.array_equal(t_hat, t_ref)
    errs = [rel(xh[k], ref[k]) for k in range(2)]
    print("per-row rel RMS:", errs)
    assert max(errs) < TOL16, errs
    with pytest.raises(guard.FloatRangeError):
        SNRAlignedEnhancer(nets("scaled", torch.float16), guard="raise")(y, est_snr=est, seed=9)


# ------------------------------------------------------------------ 6. drop-in enhance
def score_model(sd, dtype):
    from sgmse.model import ScoreModel
    m = ScoreModel(backbone="ncsnpp", sde="ouve", model_type="bbed", snr_conditioned="false", theta=1.5,
                   sigma_min=0.05, sigma_max=0.5, N=30, compute_dtype=dtype)
    m.dnn.load_state_dict(sd)
    return m.cuda().eval()


def test_score_model_enhance_falls_back_and_sticks(gpu, sds, monkeypatch):
    from snrse import guard, ncsnpp
    rng = np.random.default_rng(6)
    y = torch.from_numpy((0.3 * rng.standard_normal((1, 16000))).astype(np.float32))
    m = score_model(sds["scaled"], "fp16")
    torch.manual_seed(31)
    with pytest.warns(guard.RangeFallbackWarning):
        x1 = m.enhance(y, y, N=2)
    assert x1.shape == (16000,) and np.isfinite(x1).all()
    assert m.last_guard["flagged"] == [0] and m.dnn.compute_dtype == "fp16"
    ref_m = score_model(sds["scaled"], "bf16")
    torch.manual_seed(31)
    ref = ref_m.enhance(y, y, N=2)
    assert ref_m.last_guard["policy"] == "off"
    e1 = rel(x1, ref)
    print("rel RMS vs the bf16 model:", e1)
    assert e1 < TOL16, e1
    # sticky: the second call runs the fallback format only, on the executors it already has, without a warning
    ran = []
    pyramid = ncsnpp.NCSNppHIP.pyramid
    built = ncsnpp.NCSNppHIP.__init__
    monkeypatch.setattr(ncsnpp.NCSNppHIP, "pyramid", lambda self, *a: (ran.append(self.dtype), pyramid(self, *a))[1])
    monkeypatch.setattr(ncsnpp.NCSNppHIP, "__init__", lambda self, *a, **k: (ran.append("built"), built(self, *a, **k))[1])
    torch.manual_seed(31)
    with warnings.catch_warnings():
        warnings.simplefilter("error", guard.RangeFallbackWarning)
        x2 = m.enhance(y, y, N=2)
    assert ran == [torch.bfloat16] * 4, ran
    assert np.isfinite(x2).all() and rel(x2, ref) < TOL16


# ------------------------------------------------------------------ 7. unchanged when clean
def test_guard_changes_nothing_when_clean(gpu, nets, sde):
    from snrse import sampler
    from snrse.enhance import PCEnhancer
    Y = spec("range.clean.Y", 2, gpu)
    net = nets("formula", torch.float16)
    ref, _ = PCEnhancer(net, sde, N=2, guard=None).sample(Y, sampler.NoiseSource(seed=3))
    held = dict(net._fallbacks)
    enh = PCEnhancer(net, sde, N=2)
    src = sampler.NoiseSource(seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x, nfe = enh.sample(Y, src)
    assert nfe == 4 and src.i == 5 and all_finite(x)
    assert enh.last_guard == {"flagged": [], "policy": "fallback", "fallback_dtype": torch.bfloat16}
    assert net._fallbacks == held  # no executor was built
    errs = [rel(x[k], ref[k]) for k in range(2)]
    assert max(errs) < TOL16, errs
    # two lanes: checked after the join, same result
    x2, _ = PCEnhancer(net, sde, N=2, streams=2).sample(Y, sampler.NoiseSource(seed=3))
    assert max(rel(x2[k], ref[k]) for k in range(2)) < TOL16
