"""WAV decoding for the Specs front-end (the reference reads clips with `torchaudio.load`,
data_module.py:48-49; torchaudio is not part of this build).

`load(path)` -> (float32 tensor [channels, frames], sample_rate) with torchaudio's default
normalisation (`normalize=True`): signed 16/24/32-bit PCM divided by 2^(bits-1), unsigned
8-bit PCM as (v - 128) / 128, IEEE float 32/64 passed through (as float32).  RIFF/RIFX-free
little-endian WAVE only (PCM = 1, IEEE_FLOAT = 3, EXTENSIBLE = 0xFFFE with either sub-format);
anything else raises ValueError.  The file is memory-mapped and decoded with one numpy view.
"""
from __future__ import annotations

import math
import struct

import numpy as np
import torch

_PCM, _FLOAT, _EXT = 1, 3, 0xFFFE


def _chunks(buf: memoryview):
    off = 12
    while off + 8 <= len(buf):
        cid, size = struct.unpack_from("<4sI", buf, off)
        yield cid, off + 8, size
        off += 8 + size + (size & 1)


def _layout(path: str):
    """-> (memory map, fmt tuple, data offset, frame count) of a RIFF/WAVE file (chunk headers only are read)."""
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    buf = memoryview(raw)
    if len(buf) < 12 or bytes(buf[0:4]) != b"RIFF" or bytes(buf[8:12]) != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = data = None
    for cid, off, size in _chunks(buf):
        if cid == b"fmt ":
            fmt = struct.unpack_from("<HHIIHH", buf, off)
            if fmt[0] == _EXT and size >= 40:
                sub = struct.unpack_from("<H", buf, off + 24)[0]
                fmt = (sub,) + fmt[1:]
        elif cid == b"data":
            data = (off, min(size, len(buf) - off))
    if fmt is None or data is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    _, ch, _, _, align, bits = fmt
    if ch < 1 or align != ch * ((bits + 7) // 8):
        raise ValueError(f"{path}: inconsistent fmt chunk")
    return raw, fmt, data[0], data[1] // align


FORMATS = {(_PCM, 8), (_PCM, 16), (_PCM, 24), (_PCM, 32), (_FLOAT, 32), (_FLOAT, 64)}  # (tag, bits) read_wav decodes


def info(path: str):
    """-> (frames, channels, sample_rate) from the headers alone: what load(path)'s tensor shape will be."""
    _, fmt, _, n = _layout(path)
    return n, fmt[1], fmt[2]


def readable(path: str) -> bool:
    """Whether load(path) can decode the file, from its headers alone."""
    try:
        fmt = _layout(path)[1]
    except (ValueError, OSError, struct.error):
        return False
    return (fmt[0], fmt[5]) in FORMATS


def read_wav(path: str):
    """-> (numpy float32 [frames, channels], sample_rate)."""
    raw, fmt, off, n = _layout(path)
    tag, ch, sr, _, align, bits = fmt
    b = raw[off:off + n * align]
    if tag == _PCM and bits == 16:
        x = b.view("<i2").astype(np.float32) / 32768.0
    elif tag == _PCM and bits == 32:
        x = (b.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif tag == _PCM and bits == 24:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) / 8388608.0
    elif tag == _PCM and bits == 8:
        x = (b.astype(np.float32) - 128.0) / 128.0
    elif tag == _FLOAT and bits == 32:
        x = b.view("<f4").astype(np.float32)
    elif tag == _FLOAT and bits == 64:
        x = b.view("<f8").astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported WAVE format tag {tag} / {bits} bit")
    return x.reshape(n, ch), sr


def load(path: str):
    """torchaudio.load(path) equivalent -> (float32 tensor [channels, frames], sample_rate)."""
    x, sr = read_wav(path)
    return torch.from_numpy(np.ascontiguousarray(x.T)), sr


MODEL_RATE = 16000  # the sample rate the networks were trained at


def rational(sr_in: int, sr_out: int):
    """-> (up, down), sr_out / sr_in in lowest terms: what ops.resample_poly takes to go from sr_in to sr_out."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError(f"sample rates must be positive, got {sr_in} -> {sr_out}")
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def resampled_length(L: int, sr_in: int, sr_out: int) -> int:
    """Samples ops.resample_poly returns for L samples at sr_in brought to sr_out: ceil(L up / down), as
    scipy.signal.resample_poly.  From the numbers alone, so a batch can be planned from WAV headers (info)."""
    up, down = rational(sr_in, sr_out)
    return -((-int(L) * up) // down)


def resample_taps(up: int, down: int) -> np.ndarray:
    """scipy.signal.resample_poly's default filter w for coprime (up, down), float64 [2 half + 1] with
    half = 10 max(up, down): firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) restated in numpy
    (fc sinc(fc n) times the Kaiser window, normalised to sum 1).  The resampler applies h = up w."""
    mx = max(int(up), int(down))
    half = 10 * mx
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = 1.0 / mx
    w = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, 5.0)
    return w / w.sum()


STOI_RATE = 10000  # the sample rate ESTOI is defined at


def stoi_resample_taps(up: int, down: int) -> np.ndarray:
    """The filter w ESTOI resamples with (pystoi's restatement of Octave's resample), float64 [2 Lh + 1], to be
    applied as resample_poly(sig, up, down, window=w): cutoff fc = 1 / (2 max(up, down)), roll-off width fc / 10,
    60 dB rejection, Lh = ceil((60 - 8) / (28.714 width)), a Kaiser window of beta 0.1102 (60 - 8.7) on
    2 up fc sinc(2 fc t), t = -Lh..Lh, normalised to sum 1.  (5, 8), 16 kHz -> 10 kHz: 581 taps."""
    rej = 60.0
    fc = 1.0 / (2 * max(int(up), int(down)))
    width = fc / 10.0
    Lh = int(np.ceil((rej - 8.0) / (28.714 * width)))
    t = np.arange(-Lh, Lh + 1, dtype=np.float64)
    h = np.kaiser(2 * Lh + 1, 0.1102 * (rej - 8.7)) * (2 * int(up) * fc * np.sinc(2 * fc * t))
    return h / h.sum()


def write_wav(path: str, x: np.ndarray, sr: int = 16000, bits: int = 16):
    """Write [frames] or [frames, channels] float audio as PCM16 or float32 (test fixtures, outputs).  An int16
    array with bits = 16 is written as it is: samples already converted (ops.scale_to_pcm16)."""
    x = np.asarray(x)
    x = x[:, None] if x.ndim == 1 else x
    ch = x.shape[1]
    if bits == 16 and x.dtype == np.int16:
        data = x.astype("<i2").tobytes()
        tag = _PCM
    elif bits == 16:
        data = np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2").tobytes()
        tag = _PCM
    elif bits == 32:
        data = x.astype("<f4").tobytes()
        tag = _FLOAT
    else:
        raise ValueError("bits must be 16 (PCM) or 32 (float)")
    align = ch * bits // 8
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, tag, ch, sr, sr * align,
                      align, bits, b"data", len(data))
    with open(path, "wb") as f:
        f.write(hdr + data)
