"""fp64 numpy restatement of the long-recording window layer (snrse/longform.py, csrc/window.hip): the plan, the
fade table, gather and merge, written from the rule and sharing no code with the package."""
import math

import numpy as np


def starts(L, W, V):
    if L <= W:
        return [0]
    H = W - V
    K = int(math.ceil((L - V) / H))
    return [(k * (L - W) + (K - 1) // 2) // (K - 1) for k in range(K)]


def fade(V):
    return np.array([math.sin(math.pi * (i + 0.5) / (2 * V)) ** 2 for i in range(V)], dtype=np.float64)


def gather(x, W, V):
    """1-D recording -> (windows [K, W] zero-padded, starts, lengths)."""
    x = np.asarray(x)
    st = starts(len(x), W, V)
    out = np.zeros((len(st), W), x.dtype)
    lens = []
    for k, s in enumerate(st):
        seg = x[s:s + W]
        out[k, :len(seg)] = seg
        lens.append(len(seg))
    return out, st, lens


def dominant(L, st, V):
    """Per sample: (k(n), whether n lies in window k's fade)."""
    k = np.searchsorted(np.asarray(st), np.arange(L), side="right") - 1
    s = np.asarray(st)[k]
    return k, (k > 0) & (np.arange(L) < s + V)


def merge(wins, st, L, V, silent=None):
    """Window results [K, W] of one recording -> (out [L] fp64, bound [L]): the rule with the fp64 fade table;
    bound = |a| + |b| of the two cross-faded terms inside a fade, 0 outside."""
    w = np.asarray(wins, dtype=np.float64)
    t = fade(V)
    out, bound = np.zeros(L), np.zeros(L)
    k, infade = dominant(L, st, V)
    for n in range(L):
        kk = int(k[n])
        i = n - st[kk]
        a = 0.0 if (silent is not None and silent[kk]) else w[kk, i]
        if infade[n]:
            b = 0.0 if (silent is not None and silent[kk - 1]) else w[kk - 1, n - st[kk - 1]]
            out[n] = t[i] * a + (1.0 - t[i]) * b
            bound[n] = abs(a) + abs(b)
        else:
            out[n] = a
    return out, bound
