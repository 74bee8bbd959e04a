"""Batch planner and row packer for utterances of different lengths (host code: no call into the library).

Utterances whose spectrograms pad to the same frame count Tpad = pad_frames(1 + L // 128, 64) have identical
network shapes, and no kernel of the enhancement path mixes batch rows, so they can share one
ragged batch (ops.stft(lengths=...), PCEnhancer / SNRAlignedEnhancer(lengths=...)) and each reproduces its own
run up to GEMM summation order.  plan_batches groups a file list that way; utterances are never padded into a
larger bucket, which would change their results.
"""
from __future__ import annotations

import torch

from .enhance import pad_frames

MIN_LENGTH = 256  # a shorter clip cannot be reflect-padded by n_fft // 2 = 255 samples (torch.stft refuses it too)


def pack_rows(sigs):
    """1-D signals of different lengths (numpy arrays or tensors, all on one device) -> (buf [B, max(max L, 1)]
    float32 where the signals are, row b holding signal b and zeros after it, [L_b]).  An empty signal is a row
    of zeros with L_b = 0."""
    rows = [torch.as_tensor(s).reshape(-1) for s in sigs]
    lens = [int(r.numel()) for r in rows]
    buf = torch.zeros(len(rows), max(max(lens), 1), dtype=torch.float32, device=rows[0].device)
    for b, r in enumerate(rows):
        buf[b, :lens[b]] = r
    return buf, lens


def frames(length):
    """Frame count of the centred STFT (hop 128) of `length` samples."""
    return 1 + int(length) // 128


def plan_batches(lengths, batch_size, max_frames=16384):
    """Indices of `lengths` grouped into batches -> list[list[int]].

    Rows of one batch share Tpad; inside a batch the indices ascend; a batch holds at most `batch_size` rows and
    at most max(1, max_frames // Tpad) rows (16384 frames = 32 x 512, the footprint of the flagship batch); the
    batches are ordered by their first index.  Every index appears exactly once and the plan depends on nothing
    but its arguments.  A length below MIN_LENGTH raises ValueError naming the index."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"plan_batches: batch_size must be at least 1, got {batch_size}")
    groups = {}
    for i, L in enumerate(lengths):
        if int(L) < MIN_LENGTH:
            raise ValueError(f"plan_batches: utterance {i} has {int(L)} samples; the STFT's reflect padding needs "
                             f"at least {MIN_LENGTH}")
        groups.setdefault(pad_frames(frames(L)), []).append(i)
    batches = []
    for tpad, idx in groups.items():
        cap = min(batch_size, max(1, int(max_frames) // tpad))
        batches += [idx[k:k + cap] for k in range(0, len(idx), cap)]
    return sorted(batches, key=lambda b: b[0])


def snr_groups(lengths):
    """The rows of ONE batch grouped by pad_frames(T, 16) -> [(T16, [rows])], ascending T16, rows ascending.
    SNRNet reads a spectrogram padded to a multiple of 16 frames (pad_spec_16) and works on 16-frame chunks, so
    inside one 64-frame bucket the estimator's input shape still differs; it runs once per group."""
    groups = {}
    for r, L in enumerate(lengths):
        groups.setdefault(pad_frames(frames(L), 16), []).append(r)
    return sorted(groups.items())
