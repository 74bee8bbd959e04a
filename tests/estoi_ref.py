"""Reference of ESTOI (Jensen & Taal 2016 with pystoi's conventions) in numpy, written from the definition that
stands as the comment of snrse_estoi in include/snrse.h; it imports nothing from snrse.  pystoi itself is not
available to these tests, so parity with it is not verified here.

estoi(x, y, fs) is float64 throughout.  dtype=np.float32 is the error yardstick of the GPU tests: the steps the
kernels run in fp32 -- resampling, overlap-add, windows, the 512-point spectrum (torch.fft.rfft on float32) and the
band magnitudes -- run in fp32, the steps they run in fp64 (frame energies and the keep decision, the segment
normalisation and correlation) stay fp64.  The GPU result has to stay within 4 x the distance between the two modes,
plus 2^-24.

Besides the score, estoi returns the frame energies, the keep mask and the frame / segment counts, so that a test
can assert that no energy lies near the keep threshold before it compares anything.
"""
import math

import numpy as np

FS = 10000
FRAME, HOP, NFFT, NBANDS, MINFREQ, SEG, DYN = 256, 128, 512, 15, 150.0, 30, 40.0
EPS = float(np.finfo(np.float64).eps)
SENTINEL = 1e-5
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
         (87, 109), (109, 138), (138, 174), (174, 219))  # what band_edges() has to give (test_estoi_host.py)


def window():
    """w[n] = 0.5 (1 - cos(2 pi (n + 1) / 257)), n = 0..255."""
    return np.hanning(FRAME + 2)[1:-1].astype(np.float64)


def band_edges():
    """[(lo, hi)] bins of the 15 third-octave bands: centres 150 2^(k/3), edges the geometric means with the
    neighbouring centres, each snapped to the nearest bin frequency."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NBANDS, dtype=np.float64)
    lo = MINFREQ * 2.0 ** ((2 * k - 1) / 6)
    hi = MINFREQ * 2.0 ** ((2 * k + 1) / 6)
    return [(int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi)]


def resample_filter(up, down):
    """The filter of the resampling step, float64 [2 Lh + 1], normalised to sum 1."""
    fc = 1.0 / (2 * max(up, down))
    width = fc / 10.0
    Lh = int(math.ceil((60.0 - 8.0) / (28.714 * width)))
    t = np.arange(-Lh, Lh + 1, dtype=np.float64)
    h = np.kaiser(2 * Lh + 1, 0.1102 * (60.0 - 8.7)) * 2 * up * fc * np.sinc(2 * fc * t)
    return h / h.sum()


def resample(sig, fs, dtype=np.float64):
    from scipy import signal
    g = math.gcd(FS, int(fs))
    up, down = FS // g, int(fs) // g
    if up == down:
        return np.asarray(sig, dtype)
    return signal.resample_poly(np.asarray(sig, dtype), up, down, window=resample_filter(up, down).astype(dtype))


def n_frames(L):
    """Frames start at 128 i for every i with 128 i < L - 256."""
    return max(0, -((-(L - FRAME)) // HOP))


def frames(sig):
    nf = n_frames(len(sig))
    return sig[HOP * np.arange(nf)[:, None] + np.arange(FRAME)[None, :]] if nf else np.zeros((0, FRAME), sig.dtype)


def energies(x):
    """e_i = 20 log10(|w x_i|_2 + eps), float64, and the keep mask e_i > max e - 40."""
    fr = frames(np.asarray(x, np.float64)) * window()
    e = 20.0 * np.log10(np.sqrt((fr * fr).sum(1)) + EPS)
    return e, (e > e.max() - DYN if len(e) else np.zeros(0, bool))


def band_spectra(sig, keep, dtype):
    """Kept frames of sig, windowed and overlap-added, framed again, windowed again -> [15, M] band magnitudes."""
    w = window().astype(dtype)
    fr = frames(sig)[keep] * w
    K = len(fr)
    ola = np.zeros((K + 1, HOP), dtype)
    ola[:-1] += fr[:, :HOP]
    ola[1:] += fr[:, HOP:]
    fr2 = frames(ola.reshape(-1)) * w  # M = K - 1 frames
    if dtype == np.float32:
        import torch
        spec = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr2)), n=NFFT, dim=1).numpy()
        assert spec.dtype == np.complex64
    else:
        spec = np.fft.rfft(fr2, n=NFFT, axis=1)
    p = (spec.real ** 2 + spec.imag ** 2).astype(dtype)
    return np.stack([np.sqrt(p[:, lo:hi].sum(1)) for lo, hi in band_edges()]).astype(dtype)


def correlate(Xb, Yb):
    """The normalised segment correlation of two [15, M] float64 arrays, M >= 30 -> (d, S)."""
    def norm(A):
        A = A - A.mean(2, keepdims=True)
        A = A / (np.sqrt((A * A).sum(2, keepdims=True)) + EPS)
        A = A - A.mean(1, keepdims=True)
        return A / (np.sqrt((A * A).sum(1, keepdims=True)) + EPS)

    def seg(A):  # [S, 15, 30]
        return np.lib.stride_tricks.sliding_window_view(A, SEG, axis=1).transpose(1, 0, 2)

    Ax, Ay = norm(seg(Xb.astype(np.float64))), norm(seg(Yb.astype(np.float64)))
    S = Ax.shape[0]
    return float((Ax * Ay).sum() / (SEG * S)), S


def estoi(x, y, fs=FS, dtype=np.float64, details=False):
    """ESTOI of x (clean) and y (processed), 1-D arrays of one length at fs Hz.  details: -> (d, dict) with the frame
    energies e, the keep mask, K, S (0 for the 1e-5 result) and margin = min |e_i - (max e - 40)| in dB."""
    assert len(x) == len(y)
    x, y = resample(x, fs, dtype), resample(y, fs, dtype)
    e, keep = energies(x)
    K = int(keep.sum())
    info = dict(e=e, keep=keep, K=K, S=0, nf=len(e),
                margin=float(np.abs(e - (e.max() - DYN)).min()) if len(e) else float("inf"))
    if K - 1 < SEG:
        d = SENTINEL
    else:
        d, info["S"] = correlate(band_spectra(x, keep, dtype), band_spectra(y, keep, dtype))
    return (d, info) if details else d


def speechlike(seed, L, fs=FS, snr_db=10.0):
    """A seeded test pair (x, y) float32: noise band-limited to 100 Hz .. 0.45 fs under a 4 Hz (syllable-rate)
    envelope between 0.1 and 1, and y = x + white noise at snr_db."""
    rng = np.random.default_rng(seed)
    n = max(int(L), 2)
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / fs)
    spec[(f < 100.0) | (f > 0.45 * fs)] = 0.0
    t = np.arange(n) / fs
    x = np.fft.irfft(spec, n) * (0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + rng.uniform(0, 2 * np.pi)))
    x *= 0.1 / np.sqrt(np.mean(x * x))
    v = rng.standard_normal(n)
    y = x + v * np.sqrt(np.mean(x * x) / np.mean(v * v)) * 10.0 ** (-snr_db / 20.0)
    return x[:L].astype(np.float32), y[:L].astype(np.float32)
