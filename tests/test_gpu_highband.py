"""The high-band kernels on the GPU (snrse_resample_mix, snrse_band_gain through ops.resample_mix, ops.band_gain)
against the fp64 definition of tests/highband_ref.py, which tests/test_highband_host.py holds to scipy on the CPU.

Mix bound, per output sample and set before any kernel ran: (K + 8) 2^-24 (g|y[n]| + sum_j |h_j| (|x_j| + g|u_j|)),
the reference using the fp32 taps and the fp32 gain frames as the kernel gets them.  The kernel's own count of
roundings (csrc/highband.hip) stays inside it: K + 5 on a g|u||h| term, K + 2 on an |x||h| term, 4 on g|y|.
Gain bound, per frame: 4 |float32 restatement - fp64| + 2^-22, the restatement being torch.stft in float32 on the
CPU with float32 energies.  The worst shares of both go to profiles/highband_errors.json.

Rates 48000 (3/1), 32000 (2/1), 44100 (441/160), 22050 (441/320); per rate the rows with L16 in {256, 383, 384,
1025} (T = 3, 3, 4, 9 frames) and the rows of 767, 768, 769 output samples (the kernel's block is 256 outputs), each
as normals, an impulse at the first sample, an impulse at the last, a constant: one ragged batch, NaN from every
length on in x, u, y and the gain table."""
import json
import os

import numpy as np
import pytest
import torch

import highband_ref as hr
from conftest import ROOT, fnormal
from test_gpu_resample import ragged_nan

pytestmark = pytest.mark.gpu

ERRORS = os.path.join(ROOT, "profiles", "highband_errors.json")
RATES = (48000, 32000, 44100, 22050)
KINDS = ("normal", "impulse_first", "impulse_last", "constant")


def record(key, value):
    data = {}
    if os.path.exists(ERRORS):
        with open(ERRORS) as f:
            data = json.load(f)
    data[key] = value
    try:
        with open(ERRORS, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:  # a read-only tree: the figures are printed, the assertions do not depend on the file
        pass


def lengths_for(rate):
    """Recording lengths L: the longest with L16 = 256, 383, 384, 1025, and 767, 768, 769."""
    up, down = hr.ratio(rate)
    ls = [L16 * up // down for L16 in (256, 383, 384, 1025)]
    assert [hr.len16(L, rate) for L in ls] == [256, 383, 384, 1025]
    return ls + [767, 768, 769]


def signal(kind, tag, L, scale=0.3):
    if kind == "normal":
        return (fnormal(f"t.highband.{tag}.{L}", (L,)) * scale).astype(np.float32)
    v = np.zeros(L, np.float32)
    if kind == "impulse_first":
        v[0] = 1.0
    elif kind == "impulse_last":
        v[L - 1] = 1.0
    else:
        v[:] = scale
    return v


def batch_for(rate):
    """-> rows of (x, u, y, gain frames) float32, every length x every kind."""
    out = []
    for L in lengths_for(rate):
        L16 = hr.len16(L, rate)
        for kind in KINDS:
            gs = np.random.default_rng(L + rate).uniform(0.03, 1.0, hr.frames(L16)).astype(np.float32)
            out.append((signal(kind, f"x.{rate}", L16, 0.25), signal(kind, f"u.{rate}", L16, 0.3),
                        signal(kind, f"y.{rate}", L, 0.35), gs))
    return out


def launch(rows, rate, gain, gpu, idx=None):
    """ops.resample_mix on the rows `idx` (all) as one NaN-padded ragged batch; gain: "frames" or a constant."""
    idx = list(range(len(rows))) if idx is None else idx
    from snrse import ops
    x, u, y, g = (ragged_nan([rows[i][k] for i in idx], gpu) for k in range(4))
    l16, lR = [len(rows[i][0]) for i in idx], [len(rows[i][2]) for i in idx]
    if gain == "frames":
        return ops.resample_mix(x, u, y, l16, lR, rate, g, frames=[len(rows[i][3]) for i in idx])
    return ops.resample_mix(x, u, y, l16, lR, rate, gain)


@pytest.fixture(scope="module")
def mixed(gpu):
    """Per rate: the rows and the results of the frames launch; computed once, shared, left unchanged."""
    out = {}
    for rate in RATES:
        rows = batch_for(rate)
        out[rate] = (rows, launch(rows, rate, "frames", gpu))
    return out


def test_uploaded_taps_are_the_references(gpu):
    from snrse import audio, ops
    for rate in RATES:
        up, down = audio.rational(16000, rate)
        assert (up, down) == hr.ratio(rate)
        pm, half = ops.phase_major_taps(audio.resample_taps(up, down), up)
        h = hr.taps32(rate)
        assert half == (len(h) - 1) // 2 and pm.shape[1] == hr.terms(rate)
        flat = pm.T.reshape(-1)[:len(h)]
        assert np.array_equal(flat.astype(np.float64), h)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("gain", ["frames", 1.0, 0.5])
def test_every_sample_within_the_mix_bound(gpu, mixed, rate, gain):
    rows = mixed[rate][0]
    out = mixed[rate][1] if gain == "frames" else launch(rows, rate, gain, gpu)
    assert out.shape == (len(rows), max(len(r[2]) for r in rows)) and out.dtype == torch.float32
    out = out.cpu().numpy()
    worst, where = 0.0, None
    for b, (x, u, y, gs) in enumerate(rows):
        L = len(y)
        g = gs if gain == "frames" else gain
        ref, bnd = hr.mix(x, u, y, rate, g), hr.mix_bound(x, u, y, rate, g)
        err = np.abs(out[b, :L].astype(np.float64) - ref)
        assert np.isfinite(out[b]).all() and not out[b, L:].any(), (rate, b)
        assert (err <= bnd).all(), (rate, gain, b, L, float((err - bnd).max()))
        share = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
        if share > worst:
            worst, where = share, {"length": L, "signal": KINDS[b % len(KINDS)]}
    print(f"resample_mix {rate} gain {gain}: worst share of the bound {worst:.3f} at {where}")
    record(f"mix {rate} gain {gain}", {"terms": hr.terms(rate), "worst_share_of_bound": worst, "at": where})


@pytest.mark.parametrize("rate", RATES)
def test_rows_equal_their_solo_and_permuted_launches(gpu, mixed, rate):
    rows, out = mixed[rate]
    assert torch.equal(launch(rows, rate, "frames", gpu), out)  # two launches, the same bits
    perm = list(np.random.default_rng(5).permutation(len(rows)))
    outp = launch(rows, rate, "frames", gpu, perm)
    for r, i in enumerate(perm):
        assert torch.equal(outp[r], out[i]), (rate, r, i)
    for i in (0, 5, 14, 19, 27):  # one row of every kind, several lengths, the longest row among them
        L = len(rows[i][2])
        solo = launch(rows, rate, "frames", gpu, [i])
        assert solo.shape == (1, L) and torch.equal(solo[0], out[i, :L]), (rate, i)


@pytest.mark.parametrize("rate", RATES)
def test_keep_with_the_input_itself_returns_the_recording(gpu, rate):
    """x = u under gain 1: out = y within the mix bound -- as a constant the kernel's differences are exact zeros and
    out is y bit for bit; as frames of ones the interpolated gain may round one ulp below 1."""
    rows = [(u, u, y, np.ones_like(gs)) for _, u, y, gs in batch_for(rate)]
    for gain in (1.0, "frames"):
        out = launch(rows, rate, gain, gpu).cpu().numpy()
        for b, (x, u, y, gs) in enumerate(rows):
            err = np.abs(out[b, :len(y)].astype(np.float64) - y)
            assert (err <= hr.mix_bound(x, u, y, rate, 1.0)).all(), (rate, gain, b)
            assert gain == "frames" or np.array_equal(out[b, :len(y)], y), (rate, gain, b)


def test_twelve_kilohertz_tone_survives_keep(gpu):
    """48 kHz: a 12 kHz tone (above the network's band) plus a 1 kHz tone; u the fp64 16 kHz version, x = 0.5 u.
    Every sample within the mix bound under keep, gain 0 and a table of gain frames; under keep the tone's amplitude
    in the output is the reference's, under gain 0 it is gone from both."""
    import resample_ref as rr
    rate, L = 48000, 4800
    n = np.arange(L)
    y = (0.2 * np.sin(2 * np.pi * 12000 * n / rate) + 0.3 * np.sin(2 * np.pi * 1000 * n / rate)).astype(np.float32)
    u = rr.resample_poly(y.astype(np.float64), 1, 3).astype(np.float32)
    assert len(u) == hr.len16(L, rate) == 1600
    x = (0.5 * u).astype(np.float32)
    rows = [(x, u, y, np.ones(hr.frames(len(u)), np.float32))]
    probe = np.hanning(L) * np.exp(-2j * np.pi * 12000 * n / rate)
    probe /= np.hanning(L).sum() / 2

    def amplitude(v):
        return abs(np.dot(np.asarray(v, np.float64), probe))

    for gain, want in ((1.0, 0.2), (0.0, 0.0)):
        out = launch(rows, rate, gain, gpu).cpu().numpy()[0]
        ref, bnd = hr.mix(x, u, y, rate, gain), hr.mix_bound(x, u, y, rate, gain)
        a_out, a_ref = amplitude(out), amplitude(ref)
        print(f"12 kHz tone, gain {gain}: amplitude {a_out:.6f}, reference {a_ref:.6f}")
        assert abs(a_ref - want) < 2e-3
        assert abs(a_out - a_ref) <= 2.0 * bnd.max()  # the probe's weights sum to 2 in magnitude
        err = np.abs(out.astype(np.float64) - ref)
        assert np.isfinite(out).all() and (err <= bnd).all(), (gain, float((err - bnd).max()))
        record(f"tone 12 kHz gain {gain}", {"amplitude": float(a_out), "reference": float(a_ref),
                                            "worst_share_of_bound": float((err[bnd > 0] / bnd[bnd > 0]).max())})
    gs = np.random.default_rng(12).uniform(0.03, 1.0, hr.frames(len(u))).astype(np.float32)
    out = launch([(x, u, y, gs)], rate, "frames", gpu).cpu().numpy()[0]
    ref, bnd = hr.mix(x, u, y, rate, gs), hr.mix_bound(x, u, y, rate, gs)
    err = np.abs(out.astype(np.float64) - ref)
    assert np.isfinite(out).all() and (err <= bnd).all(), float((err - bnd).max())
    record("tone 12 kHz gain frames", {"worst_share_of_bound": float((err[bnd > 0] / bnd[bnd > 0]).max())})


# ------------------------------------------------------------------------------------------------------ the gain
def gain_rows():
    """(u, x) rows: normals with x an attenuated, noisier copy; x = 0 (the floor); x = 2 u (the clamp at 1); u with a
    frame of exact zeros (the g = 1 branch); lengths 256, 383, 384, 1025 and 2500 (20 frames, three blocks)."""
    rows = []
    for L in (256, 383, 384, 1025, 2500):
        u = signal("normal", "gain.u", L)
        e = signal("normal", "gain.e", L, 0.05)
        env = (0.2 + 0.8 * np.abs(np.sin(np.arange(L) / 200.0))).astype(np.float32)
        rows.append((u, (env * u * 0.7 + e).astype(np.float32)))
    u = signal("normal", "gain.u2", 1025)
    rows.append((u, np.zeros_like(u)))
    rows.append((u, (2.0 * u).astype(np.float32)))
    z = u.copy()
    z[300:900] = 0.0
    rows.append((z, (0.5 * u).astype(np.float32)))
    rows.append((z, (0.5 * z).astype(np.float32)))
    return rows


@pytest.mark.parametrize("floor_db", [30.0, 12.0])
def test_gain_frames_within_the_bound(gpu, floor_db):
    from snrse import ops
    rows = gain_rows()
    lens = [len(u) for u, _ in rows]
    u, x = ragged_nan([r[0] for r in rows], gpu), ragged_nan([r[1] for r in rows], gpu)
    g, fr = ops.band_gain(u, x, lens, floor_db)
    T = [hr.frames(L) for L in lens]
    assert g.shape == (len(rows), max(T)) and g.dtype == torch.float32 and fr.cpu().tolist() == T
    g2, _ = ops.band_gain(u, x, lens, floor_db)
    assert torch.equal(g, g2)
    g = g.cpu().numpy()
    worst, worst32 = 0.0, 0.0
    for b, (ub, xb) in enumerate(rows):
        ref, bnd = hr.band_gain(ub, xb, floor_db), hr.gain_bound(ub, xb, floor_db)
        err = np.abs(g[b, :T[b]].astype(np.float64) - ref)
        assert np.isfinite(g[b]).all() and not g[b, T[b]:].any(), b
        assert (err <= bnd).all(), (b, float((err / bnd).max()))
        worst = max(worst, float((err / bnd).max()))
        worst32 = max(worst32, float(np.abs(hr.band_gain_f32(ub, xb, floor_db) - ref).max()))
        solo, _ = ops.band_gain(ragged_nan([ub], gpu), ragged_nan([xb], gpu), [lens[b]], floor_db)
        assert torch.equal(solo[0].cpu(), torch.from_numpy(g[b, :T[b]])), b
    perm = [int(i) for i in np.random.default_rng(7).permutation(len(rows))]  # a row's bits do not depend on its place
    gp, _ = ops.band_gain(ragged_nan([rows[i][0] for i in perm], gpu), ragged_nan([rows[i][1] for i in perm], gpu),
                          [lens[i] for i in perm], floor_db)
    gp = gp.cpu().numpy()
    for r, i in enumerate(perm):
        assert np.array_equal(gp[r], g[i]), (r, i)
    floor = 10.0 ** (-floor_db / 20.0)
    assert np.array_equal(g[5, :9], np.full(9, np.float32(floor)))      # x = 0
    assert np.array_equal(g[6, :9], np.ones(9, np.float32))             # x = 2 u
    assert np.abs(g[8, :9] - np.array([0.5, 0.5, 0.5, 0.6, 0.6, 0.6, 0.6, 0.625, 0.5])).max() <= 2.0 ** -22
    print(f"band_gain floor {floor_db}: worst share of the bound {worst:.3f}; float32 restatement max error {worst32:.2e}")
    record(f"gain floor {floor_db}", {"worst_share_of_bound": worst, "float32_restatement_max_error": worst32})


def test_refusals(gpu):
    from snrse import ops
    z = torch.zeros(2, 600, device=gpu)
    y = torch.zeros(2, 1800, device=gpu)
    with pytest.raises(ValueError):
        ops.band_gain(z, z, [600, 255])           # too short to reflect
    with pytest.raises(ValueError):
        ops.band_gain(z, z, [600, 601])           # longer than the row stride
    with pytest.raises(ValueError):
        ops.band_gain(z, z, [600, 600], floor_db=-1.0)
    with pytest.raises(ValueError):
        ops.resample_mix(z, z, y, [600, 600], [1800, 1801], 48000, 1.0)
    with pytest.raises(ValueError):
        ops.resample_mix(z, z, y, [600, 600], [1800, 1800], 16000, 1.0)  # no band to keep
    with pytest.raises(ValueError):
        ops.resample_mix(z, z, y, [600, 600], [1800, 1800], 48000, 1.5)
    with pytest.raises(ValueError):
        ops.resample_mix(z, z, y, [600, 600], [1800, 1800], 48000, torch.ones(2, 3, device=gpu))  # 5 frames each
    # (the resampler's LDS refusal stands in snrse_resample_mix too, but no rate above 16 kHz reaches it with the
    # default filter: up > down keeps a block's span under 256 + K samples)
