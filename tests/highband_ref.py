"""fp64 reference of the high-band restoration (numpy only): the definition of include/snrse.h, snrse_resample_mix
and snrse_band_gain, and the bounds the kernels are held to.  tests/test_highband_host.py checks it on the CPU.

For one row at rate R > 16000: y the recording (L samples), u its 16 kHz version, x the enhanced 16 kHz row (L16 =
ceil(L 16000 / R) samples each), (up, down) = R / 16000 in lowest terms, h = up w the 16 k -> R filter, and
U(v)[n] = sum_j v[j] h[n down + half - j up], 0 <= n < L (resample_ref's closed form, cut to L):

    out[n] = U(x)[n] + g[n] (y[n] - U(u)[n])

The kernels' h is fp32 (taps32: h computed in float64 and rounded once, as snrse.ops.phase_major_taps uploads it), and
the mix takes its gain frames as fp32 values: the reference uses both as given, so neither rounding counts as error.

Mix bound, per sample: (K + 8) 2^-24 (g|y[n]| + sum_j |h_j| (|x_j| + g|u_j|)), K = ceil((2 half + 1) / up): the
resampler's K + 3 for the K-term chain plus five for the gain interpolation, the difference and the final fma.  The
kernel's own count (csrc/highband.hip) is K + 5 at most on a g|u||h| term, K + 2 on an |x||h| term, 4 on g|y|.
"""
import numpy as np

import resample_ref as rr

MODEL_RATE = 16000
N_FFT, HOP, BIN0 = 510, 128, 128
U24 = 2.0 ** -24


def ratio(rate):
    return rr.rational(MODEL_RATE, rate)


def len16(L, rate):
    up, down = ratio(rate)
    return -((-L * down) // up)


def taps64(rate):
    up, down = ratio(rate)
    return up * rr.default_taps(up, down)


def taps32(rate):
    """h as the kernels read it: float64, rounded to float32 once, back in float64."""
    return taps64(rate).astype(np.float32).astype(np.float64)


def terms(rate):
    up, down = ratio(rate)
    return rr.terms(up, rr.default_taps(up, down))


def upsample(v, rate, L, h=None):
    """U(v)[0 : L] in float64 with the taps h (None: taps32)."""
    up, down = ratio(rate)
    full = rr._closed_form(np.asarray(v, np.float64), taps32(rate) if h is None else h, up, down)
    assert L <= len(full)
    return full[:L]


def interp_gain(gs, rate, L):
    """g[n], n < L, from the frame values gs [T]: num = n 16000, den = R 128, i = num // den, a = (num % den) / den,
    g = (1 - a) gs[min(i, T - 1)] + a gs[min(i + 1, T - 1)] -- integers up to the one division."""
    gs = np.asarray(gs, np.float64)
    T = len(gs)
    num = np.arange(L, dtype=np.int64) * MODEL_RATE
    den = int(rate) * HOP
    i, rem = num // den, num % den
    a = rem.astype(np.float64) / den
    return (1.0 - a) * gs[np.minimum(i, T - 1)] + a * gs[np.minimum(i + 1, T - 1)]


def gain_track(gain, rate, L):
    return np.full(L, float(gain)) if np.ndim(gain) == 0 else interp_gain(gain, rate, L)


def mix(x, u, y, rate, gain, h=None):
    """out [L] float64; gain: a constant or the frame values [T]."""
    y = np.asarray(y, np.float64)
    L = len(y)
    g = gain_track(gain, rate, L)
    return upsample(x, rate, L, h) + g * (y - upsample(u, rate, L, h))


def mix_bound(x, u, y, rate, gain):
    y = np.asarray(y, np.float64)
    L = len(y)
    g = gain_track(gain, rate, L)
    ah = np.abs(taps32(rate))
    return (terms(rate) + 8) * U24 * (g * np.abs(y) + upsample(np.abs(x), rate, L, ah)
                                     + g * upsample(np.abs(u), rate, L, ah))


def frames(L16):
    return 1 + L16 // HOP


def band_energy(v):
    """E[t] = sum over bins 128 .. 255 of |S[k, t]|^2, S the raw STFT (n_fft 510, hop 128, periodic Hann, centred,
    reflect), float64 [1 + L // 128]."""
    v = np.asarray(v, np.float64)
    assert len(v) > N_FFT // 2
    p = np.pad(v, N_FFT // 2, mode="reflect")
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    idx = np.arange(frames(len(v)))[:, None] * HOP + np.arange(N_FFT)[None]
    S = np.fft.rfft(p[idx] * w, axis=1)
    return (np.abs(S[:, BIN0:]) ** 2).sum(1)


def smooth(gf):
    T = len(gf)
    return np.array([gf[max(0, t - 2):min(T - 1, t + 2) + 1].mean() for t in range(T)], gf.dtype)


def band_gain(u, x, floor_db=30.0):
    """g_s [T] float64: g_f = 1 where E_u == 0, else clamp(sqrt(E_x / E_u), 10^(-floor_db / 20), 1); g_s its
    truncated 5-frame mean."""
    eu, ex = band_energy(u), band_energy(x)
    gf = np.ones(len(eu), np.float64)
    nz = eu != 0
    gf[nz] = np.clip(np.sqrt(ex[nz] / eu[nz]), 10.0 ** (-floor_db / 20.0), 1.0)
    return smooth(gf)


def band_gain_f32(u, x, floor_db=30.0):
    """The same in float32 throughout (torch.stft in float32 on the CPU, float32 energies): the yardstick of the gain
    bound -- the kernel stays within 4 |this - band_gain| + 2^-22 per frame."""
    import torch
    win = torch.hann_window(N_FFT, periodic=True, dtype=torch.float32)

    def energy(v):
        S = torch.stft(torch.from_numpy(np.asarray(v, np.float32)), N_FFT, hop_length=HOP, window=win, center=True,
                       pad_mode="reflect", return_complex=True)
        return (S[BIN0:].real ** 2 + S[BIN0:].imag ** 2).sum(0).numpy().astype(np.float32)

    eu, ex = energy(u), energy(x)
    gf = np.ones(len(eu), np.float32)
    nz = eu != 0
    gf[nz] = np.clip(np.sqrt(ex[nz] / eu[nz]), np.float32(10.0 ** (-floor_db / 20.0)), np.float32(1.0))
    return smooth(gf)


def gain_bound(u, x, floor_db=30.0):
    return 4.0 * np.abs(band_gain_f32(u, x, floor_db).astype(np.float64) - band_gain(u, x, floor_db)) + 2.0 ** -22
