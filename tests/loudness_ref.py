"""Float64 numpy / scipy restatement of the loudness definition of include/snrse.h (snrse_kweight_sums,
snrse_loudness_gate): the reference the loudness tests compare the kernels and the written files with.  Nothing
here imports the package under test."""
import math

import numpy as np
from scipy.signal import lfilter, resample_poly


def kweighting(fs):
    """-> (b_shelf, a_shelf, b_hp, a_hp), the analog prototype of BS.1770 re-discretised for fs."""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    bs = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    as_ = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    bh = np.array([1.0, -2.0, 1.0])
    ah = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return bs, as_, bh, ah


def n100(fs):
    return (int(fs) + 5) // 10


def kweight(x, fs):
    """z = HP(shelf(x)) from a zero state; x is read as float32."""
    bs, as_, bh, ah = kweighting(fs)
    x = np.asarray(x, np.float32).astype(np.float64)
    return lfilter(bh, ah, lfilter(bs, as_, x))


def subblock_sums(x, fs):
    """s_i = sum z^2 over [i n100, (i + 1) n100), i < len(x) // n100."""
    n = n100(fs)
    z = kweight(x, fs)
    k = len(z) // n
    return (z[:k * n].reshape(k, n) ** 2).sum(1)


def subblock_sums_chunked(x, fs, C):
    """The same sums with the signal filtered C samples at a time, the 4-element state carried in zi."""
    bs, as_, bh, ah = kweighting(fs)
    x = np.asarray(x, np.float32).astype(np.float64)
    z = np.empty_like(x)
    zs, zh = np.zeros(2), np.zeros(2)
    for a in range(0, len(x), C):
        y, zs = lfilter(bs, as_, x[a:a + C], zi=zs)
        z[a:a + C], zh = lfilter(bh, ah, y, zi=zh)
    n = n100(fs)
    k = len(z) // n
    return (z[:k * n].reshape(k, n) ** 2).sum(1)


def block_energies(channels, fs):
    """e_j of a file: channels = list of 1-D signals of one rate (weight 1 each); the file has the fewest
    sub-blocks of its channels."""
    n = n100(fs)
    s = [subblock_sums(c, fs) for c in channels]
    k = min(len(v) for v in s)
    if k < 4:
        return np.zeros(0)
    return sum((v[0:k - 3] + v[1:k - 2] + v[2:k - 1] + v[3:k]) / (4.0 * n) for v in s)


def _l(e):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(e)


def integrated(channels, fs):
    """-> dict: lufs, block_l (every block's loudness), blocks, kept_abs, kept_rel, gamma, margin (the least
    |l_j - gate| over every comparison made)."""
    e = block_energies(channels, fs)
    l = _l(e)
    out = {"block_l": l, "blocks": len(e), "kept_abs": 0, "kept_rel": 0, "gamma": None, "margin": math.inf,
           "lufs": -math.inf}
    if len(e) == 0:
        return out
    out["margin"] = float(np.min(np.abs(l + 70.0)))
    ka = l > -70.0
    out["kept_abs"] = int(ka.sum())
    if not ka.any():
        return out
    gamma = float(_l(e[ka].mean()) - 10.0)
    out["gamma"] = gamma
    out["margin"] = min(out["margin"], float(np.min(np.abs(l[ka] - gamma))))
    kr = ka & (l > gamma)
    out["kept_rel"] = int(kr.sum())
    if kr.any():
        out["lufs"] = float(_l(e[kr].mean()))
    return out


def resample_taps_4x():
    """scipy.signal.resample_poly's default filter for (4, 1): firwin(81, 1 / 4, window=('kaiser', 5.0))."""
    n = np.arange(-40, 41, dtype=np.float64)
    w = 0.25 * np.sinc(0.25 * n) * np.kaiser(81, 5.0)
    return w / w.sum()


def peak4(x):
    """max |resample_poly(x, 4, 1)| with that filter, zero padding at the ends, float64."""
    x = np.asarray(x, np.float32).astype(np.float64)
    if len(x) == 0:
        return 0.0
    return float(np.abs(resample_poly(x, 4, 1, window=resample_taps_4x(), padtype="constant")).max())


def gain_pcm16(x, g):
    """int16 of fl32(fl32(g) x): what a 16-bit wav writer makes of the float32 product."""
    y = (np.float32(g) * np.asarray(x, np.float32)).astype(np.float32)
    return np.clip(np.round(y * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def sine(freq, fs, seconds, amp=1.0, phase=0.0):
    n = np.arange(int(round(seconds * fs)), dtype=np.float64)
    return (amp * np.sin(2.0 * np.pi * freq * n / fs + phase)).astype(np.float32)


def two_level(fs=48000):
    """3 s of 997 Hz at -20 dBFS, then 3 s at -50 dBFS."""
    return np.concatenate([sine(997.0, fs, 3.0, 10.0 ** (-20 / 20)), sine(997.0, fs, 3.0, 10.0 ** (-50 / 20))])
