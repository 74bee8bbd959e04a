"""fp64 reference of the polyphase resampler (numpy only): the closed form of
scipy.signal.resample_poly(x, up, down, window=w, padtype='constant'), scipy's default filter, and the per-sample
error bound the fp32 kernel is held to.  tests/test_resample_host.py checks all three against scipy on the CPU.

With up, down reduced by their gcd, half = (len(w) - 1) // 2, h = up w and n_out = ceil(L up / down):

    y[m] = sum_n x[n] h[m down + half - n up]      0 <= n < L,  0 <= m down + half - n up <= 2 half

Bound: bound[m] = (K + 3) 2^-24 sum_n |x[n]| |h[...]|, K = ceil((2 half + 1) / up) the most terms an output has:
one rounding for the fp32 tap, one per product, at most K - 1 additions in any order, one spare.
"""
import math

import numpy as np

# (rate in, rate out) of the GPU tests
RATIOS = ((48000, 16000), (16000, 48000), (44100, 16000), (16000, 44100), (22050, 16000), (32000, 16000),
          (8000, 16000), (16000, 16000))


def rational(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def n_out(L, up, down):
    return -((-L * up) // down)


def default_taps(up, down):
    """firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)), half = 10 max(up, down), in numpy."""
    mx = max(up, down)
    half = 10 * mx
    n = np.arange(-half, half + 1, dtype=np.float64)
    w = np.sinc(n / mx) / mx * np.kaiser(2 * half + 1, 5.0)
    return w / w.sum()


def terms(up, w):
    """K = ceil((2 half + 1) / up)."""
    return (len(w) - 1) // 2 * 2 // up + 1


def _closed_form(x, h, up, down):
    """sum_n x[n] h[m down + half - n up] for m in [0, n_out), float64; term j of output m is n = (m down + half)
    // up - j, walked for all outputs at once."""
    x = np.asarray(x, np.float64)
    L, half = len(x), (len(h) - 1) // 2
    m = np.arange(n_out(L, up, down), dtype=np.int64)
    c = m * down + half
    nh, p = c // up, c % up
    y = np.zeros(len(m), np.float64)
    if L == 0:
        return y
    for j in range(2 * half // up + 1):
        n, k = nh - j, p + j * up
        ok = (n >= 0) & (n < L) & (k <= 2 * half)
        y += np.where(ok, x[np.clip(n, 0, L - 1)] * h[np.clip(k, 0, 2 * half)], 0.0)
    return y


def resample_poly(x, up, down, w=None):
    """The closed form in float64; w None is the default filter.  up == down (reduced) returns x."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down:
        return np.asarray(x, np.float64).copy()
    w = default_taps(up, down) if w is None else np.asarray(w, np.float64)
    assert len(w) % 2 == 1
    return _closed_form(x, up * w, up, down)


def bound(x, up, down, w=None):
    """(K + 3) 2^-24 times the closed form of |x|, |h|, with h the float64 taps; zero for a copy."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down:
        return np.zeros(len(x), np.float64)
    w = default_taps(up, down) if w is None else np.asarray(w, np.float64)
    return (terms(up, w) + 3) * 2.0 ** -24 * _closed_form(np.abs(np.asarray(x, np.float64)), np.abs(up * w), up, down)
