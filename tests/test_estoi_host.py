"""ESTOI without a device: the reference of the GPU tests (tests/estoi_ref.py) against the properties the definition
implies, snrse.audio.stoi_resample_taps against the reference's filter, and the argument checks of snrse_estoi /
snrse_estoi_workspace, which return before any HIP call."""
import numpy as np
import pytest

import estoi_ref as er
from conftest import has_gpu

EINVAL = 1  # hipErrorInvalidValue
P = 0x10000  # a placeholder non-NULL address; never dereferenced on the host, never launched with


def test_band_table():
    assert tuple(er.band_edges()) == er.BANDS
    assert er.BANDS[0] == (7, 9) and er.BANDS[-1] == (174, 219)
    assert all(a[1] == b[0] for a, b in zip(er.BANDS, er.BANDS[1:]))  # contiguous


def test_resample_filter_16k():
    w = er.resample_filter(5, 8)
    assert len(w) == 581
    assert abs(w.sum() - 1.0) < 1e-14
    np.testing.assert_array_equal(w, w[::-1])


@pytest.mark.parametrize("ratio", [(5, 8), (5, 4), (5, 24), (100, 441)])
def test_audio_taps_equal_reference(ratio):
    from snrse import audio
    np.testing.assert_allclose(audio.stoi_resample_taps(*ratio), er.resample_filter(*ratio), rtol=0, atol=1e-16)
    assert audio.rational(16000, audio.STOI_RATE) == (5, 8)


def test_identity_and_scale():
    x, y = er.speechlike(1, 20000, snr_db=10.0)
    assert abs(er.estoi(x, x) - 1.0) < 1e-12
    d = er.estoi(x, y)
    assert 0.2 < d < 0.99
    assert abs(er.estoi(x, 7.0 * y.astype(np.float64)) - d) < 1e-12
    lo, hi = er.estoi(*er.speechlike(1, 20000, snr_db=0.0)), er.estoi(*er.speechlike(1, 20000, snr_db=30.0))
    assert lo < d < hi
    x16, y16 = er.speechlike(2, 16000, fs=16000)
    d16, info = er.estoi(x16, y16, fs=16000, details=True)
    assert info["nf"] == er.n_frames(10000) and 0.2 < d16 < 0.99


def test_too_few_frames_and_one_segment():
    x, y = er.speechlike(3, 256 + 128 * 31)
    for L, K, S in ((256 + 128 * 30, 30, 0), (256 + 128 * 30 + 1, 31, 1), (256 + 128 * 31, 31, 1), (200, 0, 0),
                    (256, 0, 0)):
        d, info = er.estoi(x[:L], y[:L], details=True)
        assert (info["K"], info["S"]) == (K, S), L
        assert (d == er.SENTINEL) == (S == 0)
    # one segment: the score is the correlation of the one 15 x 30 block
    d, info = er.estoi(x, y, details=True)
    Xb, Yb = (er.band_spectra(s.astype(np.float64), info["keep"], np.float64) for s in (x, y))
    assert Xb.shape == (15, 30)
    assert d == er.correlate(Xb, Yb)[0]


@pytest.mark.parametrize("k", [0, 1, 5, 40])
def test_frame_ending_at_L_is_dropped(k):
    L = 256 + 128 * k
    assert er.n_frames(L) == k and er.n_frames(L + 1) == k + 1 and er.n_frames(L - 1) == k
    x, _ = er.speechlike(4, L + 1)
    assert len(er.energies(x[:L])[0]) == k
    assert er.frames(x[:L + 1].astype(np.float64))[-1, -1] == x[L - 1]  # the last frame of L + 1 ends at L


def test_float32_mode_is_close():
    x, y = er.speechlike(5, 12000, snr_db=0.0)
    assert abs(er.estoi(x, y, dtype=np.float32) - er.estoi(x, y)) < 1e-6


def test_silent_frames_are_removed_and_zero_row():
    x, y = er.speechlike(6, 256 + 128 * 60)
    x, y = x.copy(), y.copy()
    x[128 * 20:128 * 30] *= 1e-4
    _, info = er.estoi(x, y, details=True)
    assert list(np.nonzero(~info["keep"])[0]) == list(range(20, 29)) and info["margin"] > 1.0
    z = np.zeros(8000, np.float32)
    d, info = er.estoi(z, z, details=True)
    assert d == 0.0 and info["keep"].all() and info["S"] == info["K"] - 30


def test_tables_and_flags(tmp_path):
    """The estoi column and line appear with an 'estoi' list in the data and not without; the CLIs know --estoi."""
    from snrse import evaluate, fit
    data = {"filename": ["a.wav", "b.wav"], "pesq": [float("nan")] * 2, "si_sdr": [1.0, 2.0], "si_sir": [3.0, 4.0],
            "si_sar": [5.0, 6.0]}
    evaluate.write_tables(data, str(tmp_path))
    assert open(tmp_path / "_results.csv").readline().strip() == "filename,pesq,si_sdr,si_sir,si_sar"
    assert len(open(tmp_path / "_avg_results.txt").read().splitlines()) == 4
    evaluate.write_tables(dict(data, estoi=[0.5, 0.75]), str(tmp_path))
    rows = open(tmp_path / "_results.csv").read().splitlines()
    assert rows[0] == "filename,pesq,si_sdr,si_sir,si_sar,estoi" and rows[2].endswith(",6.0,0.75")
    assert open(tmp_path / "_avg_results.txt").read().splitlines()[4] == "ESTOI: 0.62 ± 0.12 "
    parser, _ = fit.build_parser([])
    assert parser.parse_known_args(["--estoi"])[0].estoi and not parser.parse_known_args([])[0].estoi


def _lib():
    from snrse import _lib, build
    return _lib.load(build.build_library())


def _call(**kw):
    a = dict(x=P, y=P, lengths=P, B=2, stride=4096, work=P, work_bytes=None, out=P, info=P)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = max(int(_lib().snrse_estoi_workspace(max(a["B"], 1), max(a["stride"], 1))), 1)
    return _lib().snrse_estoi(a["x"], a["y"], a["lengths"], a["B"], a["stride"], a["work"], a["work_bytes"], a["out"],
                              a["info"], None)


@pytest.mark.skipif(has_gpu(), reason="placeholder device addresses: only without a HIP device")
@pytest.mark.parametrize("bad", [
    dict(B=0), dict(B=-1), dict(stride=0), dict(stride=-5), dict(x=None), dict(y=None), dict(lengths=None),
    dict(work=None), dict(out=None), dict(info=None), dict(work_bytes=0), dict(work_bytes=-1),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_estoi_rejects(bad):
    if bad.get("work_bytes") == -1:  # one byte short
        bad = dict(work_bytes=int(_lib().snrse_estoi_workspace(2, 4096)) - 1)
    assert _call(**bad) == EINVAL


def test_workspace_size():
    """No valid size for ruled-out arguments (0: snrse_estoi then refuses any buffer of that size); otherwise the
    size grows with B and the stride and is a multiple of 256."""
    ws = _lib().snrse_estoi_workspace
    assert ws(0, 4096) == 0 and ws(-1, 4096) == 0 and ws(2, 0) == 0 and ws(2, -1) == 0
    a, b, c = int(ws(1, 100)), int(ws(1, 40000)), int(ws(4, 40000))
    assert 0 < a < b < c and a % 256 == b % 256 == c % 256 == 0
    assert int(_lib().snrse_estoi_block()) >= 1
