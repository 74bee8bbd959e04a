"""CPU side of the high-band restoration: the fp64 reference of tests/highband_ref.py against scipy and against its
own definition, and the host layers -- ScoreModel.enhance_batch(highband=...)'s argument checks before any device
work, snrse.enhance_files' flags, and snrse.resample.restore_highband's routing of rows without a band to keep."""
import inspect
import types

import numpy as np
import pytest
import torch

import highband_ref as hr
import resample_ref as rr

RATES = (48000, 32000, 44100, 22050)


def rows(rate, L, seed=0):
    rng = np.random.default_rng(seed + rate + L)
    L16 = hr.len16(L, rate)
    return 0.3 * rng.standard_normal(L16), 0.3 * rng.standard_normal(L16), 0.3 * rng.standard_normal(L)


@pytest.mark.parametrize("rate", RATES)
def test_reference_upsampler_is_scipy(rate):
    from scipy import signal
    up, down = hr.ratio(rate)
    for L in (767, 1000):
        _, u, _ = rows(rate, L)
        assert len(u) == -((-L * 16000) // rate)
        want = signal.resample_poly(u, up, down)
        assert len(want) >= L
        assert np.abs(hr.upsample(u, rate, L, hr.taps64(rate)) - want[:L]).max() <= 1e-12
        assert np.abs(rr.resample_poly(u, up, down)[:L] - want[:L]).max() <= 1e-12


@pytest.mark.parametrize("rate", RATES)
def test_reference_reconstructs_perfectly(rate):
    """keep with x = u gives y; g = 0 is the plain resampler."""
    x, u, y = rows(rate, 900)
    assert np.abs(hr.mix(u, u, y, rate, 1.0) - y).max() <= 1e-12
    assert np.abs(hr.mix(u, u, y, rate, np.ones(hr.frames(len(u)), np.float32)) - y).max() <= 1e-12
    assert np.array_equal(hr.mix(x, u, y, rate, 0.0), hr.upsample(x, rate, len(y)))
    assert (hr.mix_bound(x, u, y, rate, 0.5) > 0).all()


def test_reference_follow_limits():
    rng = np.random.default_rng(3)
    u = 0.3 * rng.standard_normal(1025)
    assert np.array_equal(hr.band_gain(u, u), np.ones(9))
    assert np.array_equal(hr.band_gain(u, 2.0 * u), np.ones(9))
    for floor_db in (30.0, 12.0):
        g = hr.band_gain(u, np.zeros_like(u), floor_db)
        assert g.shape == (9,) and np.abs(g - 10.0 ** (-floor_db / 20.0)).max() <= 1e-15
    # half the amplitude in every bin is half the gain; a frame of exact zeros in u counts as gain 1
    assert np.abs(hr.band_gain(u, 0.5 * u) - 0.5).max() <= 1e-12
    z = u.copy()
    z[300:900] = 0.0  # frame 5 (samples 385 .. 894) sees zeros only
    eu = hr.band_energy(z)
    assert eu[4] != 0 and eu[5] == 0 and eu[6] != 0
    # g_f = 0.5 everywhere but 1 at frame 5: five frames with it average 0.6, the four of frame 7 0.625
    g = hr.band_gain(z, 0.5 * z)
    assert np.abs(g - np.array([0.5, 0.5, 0.5, 0.6, 0.6, 0.6, 0.6, 0.625, 0.5])).max() <= 1e-12
    # the truncated mean: frame 0 averages frames 0 .. 2, not five with two zeros
    gf = np.array([1.0, 0.5, 0.25, 1.0, 1.0, 1.0])
    assert hr.smooth(gf)[0] == (1.0 + 0.5 + 0.25) / 3 and hr.smooth(gf)[5] == 1.0
    assert np.abs(hr.band_gain_f32(u, 0.5 * u).astype(np.float64) - 0.5).max() < 1e-5


@pytest.mark.parametrize("rate", RATES)
def test_reference_interpolation_hits_the_frame_centres(rate):
    gs = np.random.default_rng(rate).uniform(0.03, 1.0, 9).astype(np.float32)
    L = 1025 * rate // 16000
    g = hr.interp_gain(gs, rate, L)
    den, hit = rate * 128, 0
    for n in range(L):
        if (n * 16000) % den == 0:
            assert g[n] == np.float64(gs[min(n * 16000 // den, 8)])
            hit += 1
    assert hit >= (8 if rate % 16000 == 0 else 1)  # at 441 / 160 and 441 / 320 few centres fall on a sample
    assert g.min() >= float(gs.min()) - 1e-15 and g.max() <= float(gs.max()) + 1e-15
    # between two centres it is the straight line; past the last centre it holds the last value
    n = den // 16000 // 2 if den % 32000 == 0 else None
    if n is not None:
        assert abs(g[n] - 0.5 * (float(gs[0]) + float(gs[1]))) <= 1e-15
    assert np.array_equal(hr.interp_gain(gs[:3], rate, L)[-1:], [np.float64(gs[2])])


# ------------------------------------------------------------------------------------------------ host layers
def fake_model():
    from sgmse.model import ScoreModel
    fake = types.SimpleNamespace(_batch_route=lambda *a: None, data_module=types.SimpleNamespace(hip_mode=lambda: None),
                                 enhance=lambda x, y, **kw: y[0].numpy() * 2)
    fake.enhance_batch = lambda ys, **kw: ScoreModel.enhance_batch(fake, ys, **kw)
    fake._enhance_windowed = lambda *a, **k: ScoreModel._enhance_windowed(fake, *a, **k)
    return fake


def test_enhance_batch_refuses_before_the_device(monkeypatch):
    from sgmse.model import ScoreModel
    from snrse import ops, resample
    sig = inspect.signature(ScoreModel.enhance_batch)
    assert sig.parameters["highband"].default == "drop" and sig.parameters["highband_floor_db"].default == 30.0

    def boom(*a, **k):
        raise AssertionError("device work before the argument check")

    for name in ("current_device", "resample_poly", "resample_mix", "band_gain"):
        monkeypatch.setattr(ops, name, boom)
    fake = fake_model()
    ys = [np.zeros(600, np.float32), np.zeros(700, np.float32)]
    sr = [48000, 44100]
    for policy in ("keep", "follow", -6.0):
        for kw in (dict(), dict(sample_rates=sr), dict(sample_rates=sr, output_rate="model"),
                   dict(output_rate="input"), dict(sample_rates=sr, output_rate="model", window_frames=64)):
            with pytest.raises(ValueError, match="highband"):
                ScoreModel.enhance_batch(fake, ys, highband=policy, **kw)
    for bad in ("loud", 3.0, float("nan"), None, True):
        with pytest.raises(ValueError, match="highband"):
            ScoreModel.enhance_batch(fake, ys, sample_rates=sr, output_rate="input", highband=bad)
    for bad in (-1.0, float("inf")):
        with pytest.raises(ValueError, match="highband_floor_db"):
            ScoreModel.enhance_batch(fake, ys, sample_rates=sr, output_rate="input", highband="follow",
                                     highband_floor_db=bad)
    # follow takes an STFT at 16 kHz: a recording too short for it is named before any device work, the others pass
    short = [np.zeros(700, np.float32), np.zeros(600, np.float32)]
    for kw in (dict(), dict(window_frames=64, overlap_frames=12)):
        with pytest.raises(ValueError, match="recording 1 has 600 at 48000"):
            ScoreModel.enhance_batch(fake, short, sample_rates=[16000, 48000], output_rate="input", highband="follow",
                                     **kw)
    with pytest.raises(ValueError, match="recording 0"):
        resample.restore_highband([np.zeros(200)], [np.zeros(200)], [np.zeros(600)], [48000], "follow")
    assert resample.highband_policy("follow") == "follow" and resample.highband_policy(-6) == -6.0
    assert resample.highband_policy(0) == 0.0
    # the default needs neither rates nor an output rate
    out = ScoreModel.enhance_batch(fake, ys, N=2, highband="drop")
    assert np.array_equal(out[0], ys[0] * 2)


def test_ops_exist_and_have_no_cpu_fallback():
    from snrse import _lib, ops
    assert {"snrse_resample_mix", "snrse_band_gain"} <= set(_lib.SIGNATURES)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.band_gain(torch.zeros(1, 512), torch.zeros(1, 512), [512])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_mix(torch.zeros(1, 512), torch.zeros(1, 512), torch.zeros(1, 1536), [512], [1536], 48000, 1.0)


def test_enhance_files_flags():
    from snrse import enhance_files
    ap = enhance_files.parser()
    base = ["--noisy_dir", "d", "--ckpt", "c", "--destination_folder", "o"]
    a = ap.parse_args(base)
    assert (a.highband, a.highband_gain_db, a.highband_floor_db) == ("drop", None, 30.0)
    assert enhance_files.highband_argument(a) == "drop"
    # everything else parses to what it did before the flags existed
    assert (a.batch_size, a.output_rate, a.seed, a.window_frames, a.overlap_frames, a.sampler_type, a.N,
            a.corrector) == (32, "model", None, None, 64, "pc", 30, "ald")
    a = ap.parse_args(base + ["--output_rate", "input", "--highband", "follow", "--highband_floor_db", "24"])
    assert enhance_files.highband_argument(a) == "follow" and a.highband_floor_db == 24.0
    a = ap.parse_args(base + ["--output_rate", "input", "--highband_gain_db", "-6"])
    assert enhance_files.highband_argument(a) == -6.0
    for bad in (["--highband", "keep", "--highband_gain_db", "-6"], ["--highband", "loud"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad)
    sig = inspect.signature(enhance_files.enhance_files)
    assert sig.parameters["highband"].default == "drop" and sig.parameters["highband_floor_db"].default == 30.0
    # a policy that needs the input rate is refused before the folder is looked at
    with pytest.raises(ValueError, match="highband"):
        enhance_files.enhance_files(None, "/nonexistent", "/nonexistent/out", highband="keep")
    with pytest.raises(ValueError, match="highband"):
        enhance_files.enhance_files(None, "/nonexistent", "/nonexistent/out", output_rate="input", highband=2.0)


def test_rows_without_a_band_go_through_convert(monkeypatch):
    """Rows at 16 kHz and 8 kHz under "keep": plain convert, no mix launch, no device."""
    from snrse import ops, resample

    def boom(*a, **k):
        raise AssertionError("a row at or below 16 kHz reached the device")

    for name in ("current_device", "resample_mix", "band_gain"):
        monkeypatch.setattr(ops, name, boom)
    seen = []

    def convert(sigs, rin, rout, on_device=False):
        seen.append((len(sigs), rin, list(rout)))
        return [np.repeat(np.asarray(s, np.float32), 2)[:2 * len(s) * r // 16000] if r != 16000 else s
                for s, r in zip(sigs, rout)]

    monkeypatch.setattr(resample, "convert", convert)
    x16 = [np.arange(10, dtype=np.float32), np.arange(8, dtype=np.float32)]
    ys = [np.zeros(10, np.float32), np.zeros(4, np.float32)]
    for policy in ("keep", "follow", -3.0, "drop"):
        seen.clear()
        out = resample.restore_highband(x16, x16, ys, [16000, 8000], policy)
        assert seen == [(2, 16000, [16000, 8000])]
        assert np.array_equal(out[0], x16[0]) and out[1].shape == (4,)
    with pytest.raises(ValueError, match="highband"):
        resample.restore_highband(x16, x16, ys, [16000, 8000], "loud")
    with pytest.raises(ValueError, match="one rate per recording"):
        resample.restore_highband(x16, x16[:1], ys, [16000, 8000], "keep")
