"""ScoreModel.enhance_batch(highband=...) and snrse.enhance_files end to end (GPU): formula weights in fp32, the
one-step route (sebridge_v3, oracle SNR) and the PC sampler with N = 2.  Four recordings in one call: two at 48 kHz
(0.3 s, and 0.5625 s = 9000 samples at 16 kHz so that window_frames=64 cuts it in two), one at 44.1 kHz (0.3 s),
one at 16 kHz.

With fixed seeds, output_rate="model" gives the enhanced 16 kHz rows; output_rate="input", highband=p must then be
the fp64 definition (tests/highband_ref.py) applied to them, to the 16 kHz inputs the call computed and to the
recordings, within the kernels' bounds: the mix bound for keep and a fixed gain; for follow the mix bound at the
reference's gain plus the gain bound (4 |float32 restatement - fp64| + 2^-22 per frame, interpolated like the gain)
times |y| + sum |h||u|, what a gain error of that size moves the output by."""
import os

import numpy as np
import pytest
import torch

import highband_ref as hr
from test_gpu_dropin import score_model
from test_gpu_enhance_files import clip

pytestmark = pytest.mark.gpu

RATES = [48000, 48000, 44100, 16000]
LENGTHS = [14400, 27000, 13230, 5000]
SEEDS = [11, 12, 13, 14]
POLICIES = ("keep", "follow", -6.0)
WIN = dict(window_frames=64, overlap_frames=12)


def recordings():
    ys = []
    for k, (L, sr) in enumerate(zip(LENGTHS, RATES)):
        y = clip(L, sr, k)
        if sr > 16000:  # something above 8 kHz to keep
            y = y + (0.002 * np.sin(2 * np.pi * 11000.0 * np.arange(L) / sr)).astype(np.float32)
        ys.append(y.astype(np.float32))
    return ys


ROUTES = {"onestep": (("sebridge_v3", "true"), dict(fixed_snr=0.17783),
                      dict(oracle=True, clean_rms=[1.0] * 4, noise_rms=[0.3] * 4)),
          "pc": (("bbed",), dict(dtype="fp32"), dict(N=2))}


@pytest.fixture(scope="module")
def pc_model(gpu):
    return score_model(*ROUTES["pc"][0], **ROUTES["pc"][1])


@pytest.fixture(scope="module", params=sorted(ROUTES))
def runs(gpu, request, pc_model):
    """Per route: the model, the recordings, their 16 kHz versions and the output_rate="model" results, plain and
    windowed; computed once, shared, left unchanged."""
    from snrse import resample
    args, mk, kw = ROUTES[request.param]
    m = pc_model if request.param == "pc" else score_model(*args, **mk)
    ys = recordings()
    y16 = [np.asarray(v, np.float32) for v in resample.convert(ys, RATES, 16000)]
    x16 = {w: m.enhance_batch(ys, seeds=SEEDS, sample_rates=RATES, output_rate="model", **kw, **extra)
           for w, extra in (("plain", {}), ("windowed", WIN))}
    assert m.last_windows == [1, 2, 1, 1]
    return m, kw, ys, y16, x16


def follow_slack(u, x, y, rate):
    """What the gain bound moves the output by, per sample."""
    dg = hr.interp_gain(hr.gain_bound(u, x), rate, len(y))
    ah = np.abs(hr.taps32(rate))
    return dg * (np.abs(np.asarray(y, np.float64)) + hr.upsample(np.abs(u), rate, len(y), ah))


@pytest.mark.parametrize("how", ["plain", "windowed"])
@pytest.mark.parametrize("policy", POLICIES)
def test_enhance_batch_is_the_definition(runs, policy, how):
    m, kw, ys, y16, x16 = runs
    extra = WIN if how == "windowed" else {}
    out = m.enhance_batch(ys, seeds=SEEDS, sample_rates=RATES, output_rate="input", highband=policy, **kw, **extra)
    worst = 0.0
    for i, (y, rate) in enumerate(zip(ys, RATES)):
        x, u = x16[how][i], y16[i]
        assert out[i].shape == y.shape and out[i].dtype == np.float32 and np.isfinite(out[i]).all()
        if rate <= 16000:
            assert np.array_equal(out[i], x)  # no band to keep: the 16 kHz result as it is
            continue
        assert len(x) == len(u) == hr.len16(len(y), rate)
        if policy == "follow":
            g = hr.band_gain(u, x)
            bnd = hr.mix_bound(x, u, y, rate, g) + follow_slack(u, x, y, rate)
        else:
            g = 1.0 if policy == "keep" else np.float64(np.float32(10.0 ** (policy / 20.0)))
            bnd = hr.mix_bound(x, u, y, rate, g)
        err = np.abs(out[i].astype(np.float64) - hr.mix(x, u, y, rate, g))
        assert (err <= bnd).all(), (policy, how, i, float((err / bnd).max()))
        worst = max(worst, float((err / bnd).max()))
    print(f"enhance_batch highband={policy} {how}: worst share of the bound {worst:.3f}")


def test_drop_is_the_call_without_the_argument(runs):
    m, kw, ys, y16, x16 = runs
    for extra in ({}, WIN):
        a = m.enhance_batch(ys, seeds=SEEDS, sample_rates=RATES, output_rate="input", **kw, **extra)
        b = m.enhance_batch(ys, seeds=SEEDS, sample_rates=RATES, output_rate="input", highband="drop", **kw, **extra)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    keep = m.enhance_batch(ys, seeds=SEEDS, sample_rates=RATES, output_rate="input", highband="keep", **kw)
    assert not np.array_equal(keep[0], a[0])  # and keep does change what is written


def test_enhance_files_cli_keeps_length_and_rate(pc_model, tmp_path, monkeypatch):
    """python -m snrse.enhance_files on a temporary folder, through main() with the checkpoint loader handing back
    the formula model: every policy writes files of the input length and rate, and what the flags say reaches
    enhance_batch."""
    from snrse import audio, enhance_files
    ys = recordings()
    noisy = tmp_path / "noisy"
    os.makedirs(noisy)
    audio.write_wav(str(noisy / "a.wav"), np.stack([ys[0], ys[0][::-1]], 1), 48000, bits=32)
    audio.write_wav(str(noisy / "b.wav"), ys[2], 44100, bits=32)
    audio.write_wav(str(noisy / "c.wav"), ys[3], 16000, bits=32)
    monkeypatch.setattr(enhance_files, "load_model", lambda ckpt: pc_model)
    seen, inner = [], pc_model.enhance_batch

    def spy(batch, **kw):
        if "sample_rates" in kw:
            seen.append((kw.get("highband", "drop"), kw.get("highband_floor_db", 30.0)))
        return inner(batch, **kw)

    monkeypatch.setattr(pc_model, "enhance_batch", spy, raising=False)
    flags = {"drop": [], "keep": ["--highband", "keep"], "gain": ["--highband_gain_db", "-6"],
             "follow": ["--highband", "follow", "--highband_floor_db", "24"]}
    want = {"drop": ("drop", 30.0), "keep": ("keep", 30.0), "gain": (-6.0, 30.0), "follow": ("follow", 24.0)}
    for name, extra in flags.items():
        del seen[:]
        enhance_files.main(["--noisy_dir", str(noisy), "--ckpt", "unused.ckpt", "--destination_folder",
                            str(tmp_path / name), "--output_rate", "input", "--seed", "5", "--N", "2", *extra])
        assert seen and all(s == want[name] for s in seen), (name, seen)
        assert audio.info(str(tmp_path / name / "a.wav")) == (14400, 2, 48000)
        assert audio.info(str(tmp_path / name / "b.wav")) == (13230, 1, 44100)
        assert audio.info(str(tmp_path / name / "c.wav")) == (5000, 1, 16000)
        x, _ = audio.load(str(tmp_path / name / "a.wav"))
        assert torch.isfinite(x).all() and float(x.abs().max()) > 1e-4
    a = {name: (tmp_path / name / "a.wav").read_bytes() for name in flags}
    # drop, keep and -6 dB write three different 48 kHz files; follow differs from drop (where the network does not
    # attenuate its top octave, as with formula weights, its gain is clamped at 1 and it may equal keep)
    assert len({a["drop"], a["keep"], a["gain"]}) == 3 and a["follow"] != a["drop"]
    for name in ("keep", "gain", "follow"):  # and the same 16 kHz file: it has no band to keep
        assert (tmp_path / "drop" / "c.wav").read_bytes() == (tmp_path / name / "c.wav").read_bytes()
    with pytest.raises(ValueError, match="highband"):  # the policy needs --output_rate input
        enhance_files.main(["--noisy_dir", str(noisy), "--ckpt", "unused.ckpt", "--destination_folder",
                            str(tmp_path / "bad"), "--highband", "keep"])
