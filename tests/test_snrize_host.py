"""Host checks of the fixed-SNR dataset preparation: the float64 restatement (tests/snrize_ref.py) against the data
files the reference ships (tests/golden/snrize), its edge cases, the formatting and argument checks of snrse.snrize,
and the condition the GPU tests rest on: no window of their synthetic inputs sits near the activity threshold."""
import os

import numpy as np
import pytest

import resample_ref
import snrize_ref as R
from conftest import GOLDEN

G = os.path.join(GOLDEN, "snrize")
W = 1600


def wav(rel):
    from snrse import audio
    x, sr = audio.read_wav(os.path.join(G, rel))
    assert sr == 16000 and x.shape[1] == 1
    return x[:, 0]


def golden_pair(name):
    """(clean, noise) float32 of the two shipped clips; p232's noise is noisy - clean (exact in float32)."""
    if name == "p226_001.wav":
        return wav("VBD/train/clean/" + name), wav("VBD/train/noise/" + name)
    c = wav("VBD_SNR-5/valid/clean/" + name)
    return c, wav("VBD_SNR-5/valid/noisy/" + name) - c


def test_active_rms_row_reproduced():
    with open(os.path.join(G, "active_rms_row1.txt")) as f:
        name, s, n = f.read().rstrip("\n").split("\t")
    assert name == "p232_001.wav"
    c, nz = golden_pair(name)
    a = R.analyse(c, nz)
    assert a["clean_rms"] == pytest.approx(float(s), rel=1e-15)
    assert a["noise_rms"] == pytest.approx(float(n), rel=1e-15)
    assert a["active"].all() and len(a["active"]) == 18


@pytest.mark.parametrize("name,out,nwin,corr", [("p226_001.wav", "VBD_SNR-5/train/", 23, 0.012387331561622727),
                                                ("p232_001.wav", "VBD_SNR-5/valid2/", 18, -0.002335082717693087)])
def test_golden_remix_reproduced(name, out, nwin, corr):
    c, n = golden_pair(name)
    c1, n1, y1, info = R.remix(c, n, snr_db=-5.0)
    assert info["clip_scale"] == 1.0 and info["active"].sum() == nwin == len(info["active"])
    assert abs(info["corr"] - corr) <= 1e-12
    assert np.array_equal(R.to_pcm16(c1), R.to_pcm16(wav(out + "clean/" + name)))
    assert np.array_equal(c1.astype(np.float32), wav(out + "clean/" + name))
    for sub, x in (("noise/", n1), ("noisy/", y1)):
        lsb = np.abs(x - wav(out + sub + name).astype(np.float64)).max() * 32768
        print(name, sub, "max LSB", lsb)
        assert lsb <= 1.0
    assert R.active_snr_db(c1, n1) == pytest.approx(-5.0, abs=1e-9)


def test_short_row_is_one_partial_window():
    c, n = R.synth_pair(W - 1, 1, silent=False)
    a = R.analyse(c, n)
    assert len(a["active"]) == 1 and a["counts"][0] == W - 1 and a["active"][0]
    n64 = n.astype(np.float64)
    assert a["noise_rms"] == pytest.approx(np.sqrt((n64 ** 2).mean()), rel=1e-14)


def test_partial_last_window_uses_its_true_length():
    L = 2 * W + 1
    c = np.full(L, 0.25, np.float32)
    n = np.zeros(L, np.float32)
    n[:W] = 1e-4           # 80 dB below the last sample: inactive
    n[W:2 * W] = 0.0       # silent: inactive
    n[-1] = 1.0            # a one-sample window: its mean is over 1 sample, not over W
    a = R.analyse(c, n)
    assert list(a["counts"]) == [W, W, 1] and list(a["active"]) == [False, False, True]
    assert a["win_rms"][2] == 1.0 and a["noise_rms"] == 1.0 and a["clean_rms"] == 0.25


def test_all_zero_noise_takes_the_eps_branch():
    c, _ = R.synth_pair(5000, 2)
    c1, n1, y1, info = R.remix(c, np.zeros_like(c), snr_db=-5.0)
    assert info["clean_rms"] == R.EPS and info["noise_rms"] == R.EPS and not info["active"].any()
    assert info["gain"] == pytest.approx(10 ** 0.25, rel=1e-15) and info["corr"] == 0.0
    assert np.array_equal(y1, c.astype(np.float64)) and not n1.any()


def test_clip_guard():
    (c0, n0), (c1, n1) = R.clip_cases()
    a, b, y, info = R.remix(c0, n0)
    assert info["peak"] == pytest.approx(R.CLIP_PEAKS[0], rel=1e-6) and info["clip_scale"] < 1
    assert np.abs(y).max() == pytest.approx(0.99, abs=1e-12) and np.abs(y).max() < 0.99
    s = info["clip_scale"]
    assert np.allclose(a, c0.astype(np.float64) * s, rtol=1e-15, atol=0)
    assert np.allclose(b, n0.astype(np.float64) * info["gain"] * s, rtol=1e-15, atol=0)
    assert R.active_snr_db(a, b) == pytest.approx(-5.0, abs=1e-9)
    a, b, y, info = R.remix(c1, n1)
    assert info["clip_scale"] == 1.0 and 0.989 < info["peak"] < 0.99
    assert np.array_equal(a, c1.astype(np.float64))


def all_gpu_inputs():
    """Every synthetic (label, clean, noise, fs) the GPU tests analyse, as the reference sees them."""
    out = [(f"case{i}", c, n, 16000) for i, (c, n) in enumerate(R.gpu_cases())]
    out += [(f"clip{i}", c, n, 16000) for i, (c, n) in enumerate(R.clip_cases())]
    out += [(k, R.pcm_to_float(c), R.pcm_to_float(n), 16000) for k, (c, n) in R.e2e_synth().items()]
    c, n = R.rate_pair()
    out.append(("rate16k", resample_ref.resample_poly(R.pcm_to_float(c), 1, 3),
                resample_ref.resample_poly(R.pcm_to_float(n), 1, 3), 16000))
    return out


def test_no_gpu_input_sits_near_the_threshold():
    """A window whose RMS is within 1e-6 of the threshold could flip with the summation order; none does, so a GPU
    mismatch is never a threshold flip.  Also: the inputs do exercise the mask."""
    mixed = 0
    for label, c, n, fs in all_gpu_inputs():
        a = R.analyse(c, n, fs)
        m = a["margin"]
        near = (m >= 1 - 1e-6) & (m <= 1 + 1e-6)
        assert not near.any(), (label, m[near])
        mixed += bool(a["active"].any() and not a["active"].all())
    assert mixed >= 3
    lens = [len(c) for c, _ in R.gpu_cases()]
    assert lens[:6] == [W - 1, W, 2 * W + 1, 5000, 9 * W + 37, 27861]
    assert not R.gpu_cases()[6][1].any()


def test_output_formats():
    from snrse import snrize
    line = snrize.rms_line("p232_001.wav", 0.09034279194278529, np.float64(0.01521404836098084))
    with open(os.path.join(G, "active_rms_row1.txt")) as f:
        assert line == f.read()
    row = dict(name="a.wav", rate=16000, samples=5, clean_rms_in=0.1, noise_rms_in=np.float64(0.2), snr_in_db=-6.0,
               gain=1.5, clip_scale=1.0, active_windows=1, windows=2, corr=0.25)
    assert snrize.manifest_line(row) == "a.wav\t16000\t5\t0.1\t0.2\t-6.0\t1.5\t1.0\t1\t2\t0.25\n"
    assert len(snrize.MANIFEST_COLUMNS) == 11 and snrize.MAX_WORKERS <= 8


def write_pair(tmp_path, clean, other, sr_other=16000, sub="noise"):
    from snrse import audio
    for d, x, sr in (("clean", clean, 16000), (sub, other, sr_other)):
        os.makedirs(tmp_path / d, exist_ok=True)
        audio.write_wav(str(tmp_path / d / "a.wav"), x, sr, bits=16)


def test_argument_errors(tmp_path):
    from snrse import snrize
    c, n = R.synth_pair(4000, 3)
    write_pair(tmp_path, c, n[:-1])
    kw = dict(clean_dir=str(tmp_path / "clean"), destination_folder=str(tmp_path / "out"))
    with pytest.raises(ValueError, match="a.wav"):
        snrize.remix_files(noise_dir=str(tmp_path / "noise"), **kw)
    write_pair(tmp_path, c, n, sr_other=8000)
    with pytest.raises(ValueError, match="a.wav"):
        snrize.remix_files(noise_dir=str(tmp_path / "noise"), **kw)
    write_pair(tmp_path, c, np.stack([n, n], 1))
    with pytest.raises(ValueError, match="mono"):
        snrize.remix_files(noise_dir=str(tmp_path / "noise"), **kw)
    with pytest.raises(ValueError, match="exactly one"):
        snrize.remix_files(**kw)
    with pytest.raises(ValueError, match="exactly one"):
        snrize.remix_files(noise_dir=str(tmp_path / "noise"), noisy_dir=str(tmp_path / "noise"), **kw)
    with pytest.raises(ValueError, match="rms_only"):
        snrize.remix_files(noise_dir=str(tmp_path / "noise"), rms_only=True, max_corr=0.02, **kw)
    with pytest.raises(ValueError, match="no partner"):
        snrize.remix_files(noisy_dir=str(tmp_path / "nowhere"), **kw)
    base = ["--clean_dir", kw["clean_dir"], "--destination_folder", kw["destination_folder"]]
    for extra in ([], ["--noise_dir", "x", "--noisy_dir", "y"]):
        with pytest.raises(SystemExit) as e:
            snrize.main(base + extra)
        assert e.value.code == 2
    assert not os.path.exists(tmp_path / "out")


def test_int16_samples_are_written_as_they_are(tmp_path):
    from snrse import audio
    q = np.array([0, 1, -1, 32767, -32768, 12345], np.int16)
    audio.write_wav(str(tmp_path / "q.wav"), q, 16000, bits=16)
    x, sr = audio.read_wav(str(tmp_path / "q.wav"))
    assert sr == 16000 and np.array_equal(x[:, 0], q.astype(np.float32) / 32768.0)
