"""Host side of the sample-rate front end (no GPU): the fp64 closed form and the default filter of
tests/resample_ref.py against scipy, snrse.audio's ratio / length arithmetic, the phase-major tap layout the kernel
reads, snrse.enhance_files' arguments and seed order, and that enhance_batch(sample_rates=None) stays clear of the
new code."""
import inspect
import sys
import types

import numpy as np
import pytest
import torch

from scipy import signal

import resample_ref as rr

RATIOS = [(1, 3), (3, 1), (2, 1), (1, 2), (160, 441), (147, 160), (441, 160), (320, 441)]


@pytest.mark.parametrize("up,down", RATIOS)
def test_closed_form_equals_scipy(up, down):
    rng = np.random.default_rng(up * 1000 + down)
    w = rr.default_taps(up, down)
    half = 10 * max(up, down)
    ref_w = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
    assert len(w) == len(ref_w) and np.abs(w - ref_w).max() <= 1e-12
    short = rng.standard_normal(2 * (half // up) + 3)  # another filter, through window=
    short_w = short if len(short) % 2 else short[:-1]
    for L in (1, 2, 3, down - 1, down, down + 1, 257, 1000, 2205):
        if L < 1:
            continue
        x = rng.standard_normal(L)
        for taps in (None, w, short_w):
            want = signal.resample_poly(x, up, down, padtype="constant") if taps is None else \
                signal.resample_poly(x, up, down, window=taps, padtype="constant")
            got = rr.resample_poly(x, up, down, taps)
            assert got.shape == want.shape == (rr.n_out(L, up, down),), (L, got.shape, want.shape)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (up, down, L)
    assert rr.resample_poly(np.zeros(0), up, down).shape == (0,)


def test_bound_is_the_closed_form_of_magnitudes():
    x = np.array([0.5, -2.0, 0.25, 1.0, -1.0, 3.0, 0.0, -0.125])
    for up, down in ((1, 3), (3, 1), (160, 441)):
        w = rr.default_taps(up, down)
        b = rr.bound(x, up, down)
        want = signal.resample_poly(np.abs(x), up, down, window=np.abs(w), padtype="constant")
        K = -(-len(w) // up)
        assert rr.terms(up, w) == K
        np.testing.assert_allclose(b, (K + 3) * 2.0 ** -24 * want, rtol=1e-12, atol=1e-30)
    assert rr.terms(160, rr.default_taps(160, 441)) == 56 and len(rr.default_taps(160, 441)) == 8821
    assert len(rr.default_taps(1, 3)) == 61


def test_audio_ratio_length_and_taps():
    from snrse import audio
    assert audio.rational(48000, 16000) == (1, 3)
    assert audio.rational(44100, 16000) == (160, 441)
    assert audio.rational(16000, 16000) == (1, 1)
    assert audio.rational(16000, 44100) == (441, 160) and audio.rational(22050, 16000) == (320, 441)
    for sr_in, sr_out in ((48000, 16000), (44100, 16000), (16000, 16000), (16000, 48000), (16000, 44100)):
        up, down = audio.rational(sr_in, sr_out)
        assert (up, down) == rr.rational(sr_in, sr_out)
        for L in range(0, 1001):
            want = len(signal.resample_poly(np.zeros(L), up, down, window=np.ones(1))) if L else 0
            assert audio.resampled_length(L, sr_in, sr_out) == want == rr.n_out(L, up, down), (sr_in, sr_out, L)
        # back at the input rate a signal is never shorter than it was
        assert all(audio.resampled_length(audio.resampled_length(L, sr_in, sr_out), sr_out, sr_in) >= L
                   for L in range(0, 1001))
    for up, down in ((1, 3), (160, 441), (3, 1)):
        half = 10 * max(up, down)
        ref_w = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0))
        assert np.abs(audio.resample_taps(up, down) - ref_w).max() <= 1e-12
        assert np.array_equal(audio.resample_taps(up, down), rr.default_taps(up, down)) or \
            np.abs(audio.resample_taps(up, down) - rr.default_taps(up, down)).max() <= 1e-16
    with pytest.raises(ValueError):
        audio.rational(0, 16000)


def test_phase_major_taps_layout():
    from snrse import ops
    for up, n in ((1, 61), (3, 61), (160, 8821), (441, 8821), (7, 5)):
        w = np.random.default_rng(n).standard_normal(n)
        pm, half = ops.phase_major_taps(w, up)
        K = -(-n // up)
        assert half == (n - 1) // 2 and pm.shape == (up, K) and pm.dtype == np.float32 and pm.flags.c_contiguous
        for p in range(up):
            for j in range(K):
                k = p + j * up
                assert pm[p, j] == (np.float32(up * w[k]) if k < n else 0.0)
    with pytest.raises(ValueError, match="odd"):
        ops.phase_major_taps(np.ones(4), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_poly(torch.zeros(1, 8), 1, 3)


def test_enhance_files_arguments():
    from snrse import enhance_files
    ap = enhance_files.parser()
    a = ap.parse_args(["--noisy_dir", "d", "--ckpt", "c", "--destination_folder", "o"])
    assert (a.batch_size, a.output_rate, a.seed, a.sampler_type, a.N, a.corrector) == (32, "model", None, "pc", 30, "ald")
    a = ap.parse_args(["--noisy_dir", "d", "--ckpt", "c", "--destination_folder", "o", "--batch_size", "4",
                       "--output_rate", "input", "--seed", "7", "--sampler_type", "ode", "--N", "5", "--snr", "0.3"])
    assert (a.batch_size, a.output_rate, a.seed, a.sampler_type, a.N, a.snr) == (4, "input", 7, "ode", 5, 0.3)
    for bad in (["--output_rate", "48000"], ["--sampler_type", "euler"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--noisy_dir", "d", "--ckpt", "c", "--destination_folder", "o", *bad])
    with pytest.raises(SystemExit):
        ap.parse_args(["--ckpt", "c", "--destination_folder", "o"])  # no clean reference, but a noisy folder
    # evaluate keeps its options and gains --resample, off by default
    from snrse import evaluate
    sig = inspect.signature(evaluate.evaluate)
    assert sig.parameters["resample"].default is False


def test_seed_order_stereo_then_mono(tmp_path):
    """One draw per (file, channel), file order then channel order; an unreadable file takes none."""
    from snrse import audio, enhance_files
    audio.write_wav(str(tmp_path / "a.wav"), np.zeros((300, 2), np.float32), 48000)
    audio.write_wav(str(tmp_path / "b.wav"), np.zeros(400, np.float32), 16000)
    (tmp_path / "c.wav").write_bytes(b"not a wave file at all")
    audio.write_wav(str(tmp_path / "d.wav"), np.zeros((500, 3), np.float32), 44100, bits=32)
    with pytest.warns(UserWarning, match="c.wav"):
        files = enhance_files.list_files(str(tmp_path))
    assert [(f[0].rsplit("/", 1)[-1], *f[1:]) for f in files] == [("a.wav", 300, 2, 48000), ("b.wav", 400, 1, 16000),
                                                                 ("d.wav", 500, 3, 44100)]
    utts = enhance_files.utterances(files)
    assert utts == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1), (2, 2)]
    torch.manual_seed(11)
    seeds = enhance_files.draw_seeds(len(utts))
    torch.manual_seed(11)
    assert seeds == [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(6)] and len(set(seeds)) == 6
    enhance_files.write_csv(files, "input", str(tmp_path))
    rows = (tmp_path / "_enhanced.csv").read_text().strip().split("\n")
    assert rows[0] == "filename,input_rate,channels,seconds,output_rate" and len(rows) == 4
    assert rows[1] == "a.wav,48000,2,0.00625,48000" and rows[2] == "b.wav,16000,1,0.025,16000"
    enhance_files.write_csv(files, "model", str(tmp_path))
    assert (tmp_path / "_enhanced.csv").read_text().strip().split("\n")[3].endswith(",44100,3," + repr(500 / 44100) + ",16000")


def test_enhance_batch_without_sample_rates_stays_clear_of_the_resampler(monkeypatch):
    """sample_rates=None: the keyword's default, and a call neither imports snrse.resample nor reaches
    ops.resample_poly (run here on the per-utterance route with a stand-in enhance(), which needs no device)."""
    from sgmse.model import ScoreModel
    from snrse import ops
    sig = inspect.signature(ScoreModel.enhance_batch)
    assert sig.parameters["sample_rates"].default is None and sig.parameters["output_rate"].default == "model"

    def boom(*a, **k):
        raise AssertionError("ops.resample_poly reached without sample_rates")

    monkeypatch.setattr(ops, "resample_poly", boom)
    import snrse
    monkeypatch.delitem(sys.modules, "snrse.resample", raising=False)  # as in a process that never imported it
    monkeypatch.delattr(snrse, "resample", raising=False)
    calls = []
    fake = types.SimpleNamespace(_batch_route=lambda *a: None,
                                 enhance=lambda x, y, **kw: calls.append(y.shape) or y[0].numpy() * 2)
    fake.enhance_batch = lambda ys, **kw: ScoreModel.enhance_batch(fake, ys, **kw)
    ys = [np.arange(5, dtype=np.float32), np.arange(7, dtype=np.float32)]
    out = ScoreModel.enhance_batch(fake, ys, N=2)
    assert calls == [(1, 5), (1, 7)] and np.array_equal(out[1], ys[1] * 2)
    assert "snrse.resample" not in sys.modules and not hasattr(snrse, "resample")
    # with rates the same call goes through snrse.resample (and, all at 16 kHz, converts nothing)
    out = ScoreModel.enhance_batch(fake, ys, N=2, sample_rates=[16000, 16000])
    assert "snrse.resample" in sys.modules
    with pytest.raises(ValueError, match="sample rates"):
        ScoreModel.enhance_batch(fake, ys, sample_rates=[16000])
    with pytest.raises(ValueError, match="output_rate"):
        ScoreModel.enhance_batch(fake, ys, sample_rates=[16000, 16000], output_rate="48000")
