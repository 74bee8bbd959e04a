"""Recordings of any length: the window plan of ScoreModel.enhance_batch(window_frames=...) (host code: nothing here
calls into the library or touches a device).

A recording of L samples at 16 kHz is cut into overlapping windows, every window runs as an ordinary row of the
batched enhancers -- its own max|y|, its own SNR estimate, its own noise seed -- and the results are joined by a
cross-fade (ops.window_gather / ops.window_merge, csrc/window.hip).  With window_frames and overlap_frames:

    W = (window_frames - 1) 128 samples   a full window has exactly window_frames STFT frames = its Tpad
    V = overlap_frames 128 samples        the cross-fade
    H = W - V                             the largest distance between two window starts

    L <= W:    one window [0, L): the recording runs as it would without windows
    otherwise: K = ceil((L - V) / H) windows of W samples, evenly spaced from 0 to L - W:
               s_k = (k (L - W) + (K - 1) // 2) // (K - 1)

so s_0 = 0, s_{K-1} = L - W, the starts ascend strictly, every gap is <= H (window k - 1 covers window k's fade
region [s_k, s_k + V)) and, for K >= 3, every gap is >= V (fade regions never overlap): at most two windows touch a
sample.  Every window of a long recording is full-size, the last one included.

The merge: with k(n) the last window whose s_k <= n,
    k > 0 and n < s_k + V:  out[n] = t[n - s_k] x_k[n - s_k] + (1 - t[n - s_k]) x_{k-1}[n - s_{k-1}]
    otherwise:              out[n] = x_k[n - s_k]
with the fade table t[i] = sin^2(pi (i + 1/2) / (2 V)), t[i] + t[V - 1 - i] = 1.

Seeds: window 0 keeps the recording's seed; window k >= 1 runs under window_seed(seed, k).
"""
from __future__ import annotations

import numpy as np

HOP = 128  # the STFT's hop: a window of (frames - 1) HOP samples has exactly `frames` centred frames
_M64 = (1 << 64) - 1


def geometry(window_frames, overlap_frames):
    """(W, V, H) in samples of the two arguments, which are checked here -- before any device work."""
    wf, of = int(window_frames), int(overlap_frames)
    if wf != window_frames or wf < 64 or wf % 64:
        raise ValueError(f"window_frames must be a positive multiple of 64 (the network's frame bucket), "
                         f"got {window_frames!r}")
    if of != overlap_frames or of < 2:
        raise ValueError(f"overlap_frames must be an integer of at least 2, got {overlap_frames!r}")
    W, V = (wf - 1) * HOP, of * HOP
    if 4 * V > W:
        raise ValueError(f"overlap_frames = {of} is too long for window_frames = {wf}: the cross-fade may take a "
                         f"quarter of a window at the most (4 x {V} > {W} samples)")
    return W, V, W - V


def window_starts(L, W, V):
    """Starts of the windows of a recording of L samples -> list of ints (one window, [0], when L <= W)."""
    L, W, V = int(L), int(W), int(V)
    if L <= W:
        return [0]
    H = W - V
    K = -((V - L) // H)  # ceil((L - V) / H) >= 2
    return [(k * (L - W) + (K - 1) // 2) // (K - 1) for k in range(K)]


def fade_table(V):
    """t[i] = sin^2(pi (i + 1/2) / (2 V)), i < V, float64."""
    return np.sin(np.pi * (np.arange(int(V), dtype=np.float64) + 0.5) / (2.0 * int(V))) ** 2


def window_seed(seed, k):
    """Noise seed of window k of a recording whose seed is `seed`: the seed itself for k = 0, else the top 62 bits
    of splitmix64's output function at seed + k * 0x9E3779B97F4A7C15 (mod 2^64) -- an integer function of
    (seed, k) alone with values in [0, 2^62)."""
    seed, k = int(seed), int(k)
    if k == 0:
        return seed
    z = (seed + k * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) >> 2


class Plan:
    """The windows of a list of recordings, in recording order then window order.

    W, V                     the geometry in samples
    lengths  [R]             the recordings' lengths
    first    [R + 1]         recording r owns windows first[r] .. first[r + 1] - 1
    utt, k   [nwin]          each window's recording and its index inside it
    starts, win_lengths [nwin]
    table    [nwin, 3] int32 (recording, start, length): ops.window_gather's table"""

    def __init__(self, lengths, window_frames, overlap_frames):
        self.W, self.V, _ = geometry(window_frames, overlap_frames)
        self.lengths = [int(L) for L in lengths]
        if any(L < 1 or L >= 2 ** 31 for L in self.lengths):
            raise ValueError("snrse: a recording has no samples, or 2^31 of them or more (the device tables are int32)")
        self.first, self.utt, self.k, self.starts, self.win_lengths = [0], [], [], [], []
        for r, L in enumerate(self.lengths):
            st = window_starts(L, self.W, self.V)
            self.utt += [r] * len(st)
            self.k += list(range(len(st)))
            self.starts += st
            self.win_lengths += [min(L, self.W)] * len(st)
            self.first.append(len(self.starts))
        self.table = np.stack([np.asarray(self.utt, np.int64), np.asarray(self.starts, np.int64),
                               np.asarray(self.win_lengths, np.int64)], 1).astype(np.int32).reshape(-1, 3)

    def __len__(self):
        return len(self.starts)

    def counts(self):
        """Windows per recording."""
        return [b - a for a, b in zip(self.first[:-1], self.first[1:])]

    def seeds(self, seeds):
        """Per-window seeds of per-recording seeds."""
        return [window_seed(seeds[r], k) for r, k in zip(self.utt, self.k)]
