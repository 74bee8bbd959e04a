"""CPU checks of the loudness layer: the K-weighting coefficients, the fp64 reference's conformance values, the
chunk transition A^C, the gain plan, the option parsing, the csv columns and the gain-to-PCM formula.  No kernel is
launched here."""
import math
import os

import numpy as np
import pytest
from scipy.signal import lfilter

import loudness_ref as ref

# ITU-R BS.1770-4 table 1 / 2 (48 kHz), as the issue quotes them
SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
SHELF_A = (1.0, -1.69065929318241, 0.73248077421585)
HP_A = (1.0, -1.99004745483398, 0.99007225036621)


def test_kweighting_48k_is_the_standards_table():
    from snrse import loudness
    c = loudness.kweighting(48000)
    assert c.dtype == np.float64 and c.shape == (10,)
    want = np.array(SHELF_B + SHELF_A[1:] + (1.0, -2.0, 1.0) + HP_A[1:])
    assert np.abs(c - want).max() <= 1e-12, np.abs(c - want).max()


@pytest.mark.parametrize("fs", (44100, 16000, 8000))
def test_kweighting_other_rates_follow_the_formulas(fs):
    from snrse import loudness
    c = loudness.kweighting(fs)
    # the formulas of the definition, evaluated here on their own
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Q = 0.7071752369554196
    Vh = 10 ** (3.999843853973347 / 20)
    Vb = Vh ** 0.4996667741545416
    a0 = 1 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0]
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0]
    assert np.abs(c - np.array(shelf + hp)).max() <= 1e-14
    bs, as_, bh, ah = ref.kweighting(fs)
    assert np.abs(c - np.concatenate([bs, as_[1:], bh, ah[1:]])).max() <= 1e-14


def test_reference_reads_the_conformance_sine():
    r = ref.integrated([ref.sine(997.0, 48000, 5.0)], 48000)
    assert abs(r["lufs"] - (-3.0103)) <= 1e-3, r["lufs"]
    r16 = ref.integrated([ref.sine(997.0, 16000, 5.0)], 16000)
    assert abs(r16["lufs"] - (-2.9700)) <= 1e-3, r16["lufs"]


def test_reference_two_level_signal_uses_the_relative_gate():
    r = ref.integrated([ref.two_level()], 48000)
    assert abs(r["lufs"] - (-23.2328)) <= 1e-3, r["lufs"]
    assert r["kept_rel"] == 30 and r["kept_abs"] == r["blocks"] == 57
    assert r["margin"] > 1e-3


def test_reference_silence_and_short_rows():
    assert ref.integrated([np.zeros(48000, np.float32)], 48000)["lufs"] == -math.inf
    short = ref.sine(997.0, 48000, 1.0)[:4 * ref.n100(48000) - 1]
    r = ref.integrated([short], 48000)
    assert r["lufs"] == -math.inf and r["blocks"] == 0
    assert ref.integrated([short, short], 48000)["lufs"] == -math.inf


def test_chunked_reference_is_the_one_pass_filter():
    x = (np.random.default_rng(5).standard_normal(3 * 48000) * 0.1).astype(np.float32)
    assert np.array_equal(ref.subblock_sums(x, 48000), ref.subblock_sums_chunked(x, 48000, 64))


@pytest.mark.parametrize("fs,C", ((48000, 64), (8000, 64), (44100, 32768)))
def test_chunk_transition_propagates_a_state_as_the_filter_does(fs, C):
    """M^C s equals C zero-input steps of the two biquads (scipy's transposed direct form II, zi = the state)."""
    from snrse import loudness
    bs, as_, bh, ah = ref.kweighting(fs)
    s = np.random.default_rng(fs).standard_normal(4)
    zeros = np.zeros(C)
    y, zs = lfilter(bs, as_, zeros, zi=s[:2])
    _, zh = lfilter(bh, ah, y, zi=s[2:])
    want = np.concatenate([zs, zh])
    got = loudness.chunk_transition(fs, C) @ s
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), (got, want)
    # and the table row the kernel gets holds that matrix and its group power
    row = loudness.kernel_params(fs, 64, 512)
    assert row.shape == (42,) and np.array_equal(row[:10], loudness.kweighting(fs))
    assert np.array_equal(row[10:26].reshape(4, 4), loudness.chunk_transition(fs, 64))
    big = loudness.chunk_transition(fs, 64 * 512)
    assert np.abs(row[26:].reshape(4, 4) - big).max() <= 1e-9 * max(1.0, np.abs(big).max())


def test_plan_gain():
    from snrse import loudness
    g, lim = loudness.plan_gain(-30.0, -23.0, 0.1, -1.0)
    assert not lim and g == pytest.approx(10 ** (7 / 20), rel=1e-15)
    g, lim = loudness.plan_gain(-30.0, -23.0, 0.5, -1.0)  # 0.5 * 2.24 > 0.891
    assert lim and g == pytest.approx(10 ** (-1 / 20) / 0.5, rel=1e-15)
    assert loudness.plan_gain(-math.inf, -23.0, 0.5, -1.0) == (1.0, False)
    assert loudness.plan_gain(-23.0, -23.0, 0.0, -1.0) == (1.0, False)
    g, lim = loudness.plan_gain(-10.0, -23.0, 1.2, -1.0)  # attenuation that already meets the ceiling
    assert not lim and g * 1.2 <= 10 ** (-1 / 20)


def test_parse_target():
    from snrse import loudness
    assert loudness.parse_target("off") is None and loudness.parse_target(None) is None
    assert loudness.parse_target("input") == "input" and loudness.parse_target(" INPUT ") == "input"
    assert loudness.parse_target("-23") == -23.0 and loudness.parse_target(-16) == -16.0
    for bad in ("loud", "nan", "inf", ""):
        with pytest.raises(ValueError):
            loudness.parse_target(bad)
    assert loudness.check_ceiling(-1) == -1.0 and loudness.check_ceiling(0) == 0.0
    with pytest.raises(ValueError):
        loudness.check_ceiling(0.5)


def test_csv_columns(tmp_path):
    from snrse import audio, enhance_files as ef
    wav = str(tmp_path / "a.wav")
    audio.write_wav(wav, np.zeros(1600, np.float32), 16000)
    files = [(wav, 1600, 1, 16000)]
    base = "filename,input_rate,channels,seconds,output_rate"

    def header_and_row(**kw):
        ef.write_csv(files, "model", str(tmp_path), **kw)
        with open(os.path.join(str(tmp_path), "_enhanced.csv")) as f:
            return f.read().splitlines()

    off = header_and_row()
    assert off == [base, "a.wav,16000,1,0.1,16000"]  # unchanged with the option off
    assert header_and_row(window=(512, 64)) == [base + ",windows", "a.wav,16000,1,0.1,16000,1"]
    loud = np.array([[-20.5, -math.inf, 0.0, -3.25, 0.0]])
    on = header_and_row(loud=loud)
    assert on[0] == base + ",input_lufs,enhanced_lufs,gain_db,peak_db,limited"
    assert on[1] == "a.wav,16000,1,0.1,16000,-20.5,-inf,0.0,-3.25,0"
    both = header_and_row(window=(512, 64), loud=loud)
    assert both[0] == base + ",windows,input_lufs,enhanced_lufs,gain_db,peak_db,limited"
    assert both[1].startswith("a.wav,16000,1,0.1,16000,1,-20.5,")
    a = ef.parser().parse_args(["--noisy_dir", "n", "--ckpt", "c", "--destination_folder", "d"])
    assert a.loudness == "off" and a.peak_db == -1.0
    a = ef.parser().parse_args(["--noisy_dir", "n", "--ckpt", "c", "--destination_folder", "d", "--loudness", "-23",
                                "--peak_db", "-2"])
    assert a.loudness == "-23" and a.peak_db == -2.0


def test_gain_to_pcm_formula_is_write_wavs(tmp_path):
    """clip(rint(fl32(fl32(g) x) 32768)) are the bytes audio.write_wav(bits=16) writes for the float32 product."""
    from snrse import audio
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4000).astype(np.float32) * 0.4,
                        np.array([1.0, -1.0, 1.5, -1.5, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768,
                                  -1.5 / 32768, 32766.5 / 32768, 0.0], np.float32)])
    for g in (1.0, 0.7079457843841379, 2.5):
        q = ref.gain_pcm16(x, g)
        path = str(tmp_path / "q.wav")
        audio.write_wav(path, (np.float32(g) * x).astype(np.float32), 16000, bits=16)
        with open(path, "rb") as f:
            data = f.read()[44:]
        assert data == q.astype("<i2").tobytes()
        audio.write_wav(path, q, 16000, bits=16)  # and the int16 samples go out as they are
        with open(path, "rb") as f:
            assert f.read()[44:] == data
    q1 = ref.gain_pcm16(x, 1.0)
    assert list(q1[-11:]) == [32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, 32766, 0]  # ties go to even
