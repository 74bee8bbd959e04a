"""Float64 numpy restatement of the fixed-SNR dataset preparation (the yardstick of snrse.snrize / csrc/snrize.hip),
written from its definition:

  windows     W = int(fs * 0.1) samples, non-overlapping from sample 0; the last one may be partial and its mean is
              taken over its true length
  activity    window k is active iff sqrt(mean(n_k^2)) > 10^(-50/20) * (max|n| + eps), eps = float64 eps: decided
              by the NOISE alone
  active RMS  clean_rms = sqrt(sum_active c^2 / sum_active count), noise_rms likewise over n; both eps when no
              window is active
  remix       g = clean_rms / noise_rms * 10^(-S/20), n' = g n, y = c + n'
  clip guard  max|y| > 0.99: all three signals divided by max|y| / (0.99 - eps)
  output      16-bit PCM: clip(round(x * 32768), -32768, 32767)

Vectorised (np.add.reduceat over the window starts), everything in float64.
"""
import numpy as np

EPS = 2.220446049250313e-16
THR = 10 ** (-50 / 20)
CLIP = 0.99


def window_length(fs):
    return int(fs * 0.1)


def analyse(clean, noise, fs=16000):
    """-> dict: clean_rms, noise_rms, active (bool [nW]), counts [nW], win_rms [nW] (of the noise), threshold,
    margin [nW] = win_rms / threshold, max_noise, corr (Pearson, 0 where a signal has no variance)."""
    c = np.asarray(clean, np.float64).reshape(-1)
    n = np.asarray(noise, np.float64).reshape(-1)
    if c.shape != n.shape or c.size == 0:
        raise ValueError("analyse: clean and noise must be 1-D, non-empty and of one length")
    W = window_length(fs)
    L = c.size
    starts = np.arange(0, L, W)
    counts = np.minimum(W, L - starts).astype(np.int64)
    cc = np.add.reduceat(c * c, starts)
    nn = np.add.reduceat(n * n, starts)
    win_rms = np.sqrt(nn / counts)
    mx = float(np.max(np.abs(n)))
    threshold = THR * (mx + EPS)
    active = win_rms > threshold
    if active.any():
        cnt = counts[active].sum()
        clean_rms = float(np.sqrt(cc[active].sum() / cnt))
        noise_rms = float(np.sqrt(nn[active].sum() / cnt))
    else:
        clean_rms = noise_rms = EPS
    dc, dn = c - c.mean(), n - n.mean()
    den = np.sqrt((dc * dc).sum()) * np.sqrt((dn * dn).sum())
    corr = float((dc * dn).sum() / den) if den > 0 else 0.0
    return dict(clean_rms=clean_rms, noise_rms=noise_rms, active=active, counts=counts, win_rms=win_rms,
                threshold=threshold, margin=win_rms / threshold, max_noise=mx, corr=corr)


def gain(clean_rms, noise_rms, snr_db):
    return (clean_rms / noise_rms) * 10 ** (-snr_db / 20)


def remix(clean, noise, fs=16000, snr_db=-5.0):
    """-> (clean', noise', noisy float64, info): info is analyse()'s dict plus gain, clip_scale (the factor all
    three were multiplied by: 1, or 1 / (max|y| / (0.99 - eps))) and peak (max|y| before the guard)."""
    c = np.asarray(clean, np.float64).reshape(-1)
    n = np.asarray(noise, np.float64).reshape(-1)
    info = analyse(c, n, fs)
    g = gain(info["clean_rms"], info["noise_rms"], snr_db)
    n1 = g * n
    y = c + n1
    peak = float(np.max(np.abs(y)))
    scale = 1.0
    if peak > CLIP:
        d = peak / (CLIP - EPS)
        c, n1, y = c / d, n1 / d, y / d
        scale = 1.0 / d
    info.update(gain=g, clip_scale=scale, peak=peak)
    return c, n1, y, info


def to_pcm16(x):
    return np.clip(np.round(np.asarray(x) * 32768.0), -32768, 32767).astype(np.int16)


def active_snr_db(clean, noise, fs=16000):
    a = analyse(clean, noise, fs)
    return 20 * np.log10(a["clean_rms"] / a["noise_rms"])


# ---- the synthetic inputs the tests share (deterministic; test_snrize_host.py checks their window margins) ----

def synth_pair(L, seed, fs=16000, silent=True, noise_level=0.05, clean_level=0.1):
    """A (clean, noise) float32 pair of L samples: a modulated tone mixture and band-limited noise whose windows
    cycle loud / exactly zero / 60 dB down (silent=True), so that some windows are inactive."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / fs
    c = clean_level * (np.sin(2 * np.pi * 220 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
                       + 0.3 * rng.standard_normal(L))
    n = noise_level * rng.standard_normal(L)
    if silent:
        W = window_length(fs)
        k = np.arange(L) // W
        n = np.where(k % 4 == 1, 0.0, n)
        n = np.where(k % 4 == 3, n * 1e-3, n)
    return c.astype(np.float32), n.astype(np.float32)


def gpu_case_lengths(fs=16000, windows_per_block=8):
    W = window_length(fs)
    return [W - 1, W, 2 * W + 1, 5000, (windows_per_block + 1) * W + 37, 27861]


def gpu_cases(fs=16000, windows_per_block=8):
    """The rows of the GPU kernel test: the lengths the issue lists with silent stretches in the noise, plus one
    all-zero-noise row.  -> list of (clean, noise) float32."""
    out = [synth_pair(L, 100 + i, fs) for i, L in enumerate(gpu_case_lengths(fs, windows_per_block))]
    c, n = synth_pair(4321, 99, fs)
    out.append((c, np.zeros_like(n)))
    return out


CLIP_PEAKS = (1.2, 0.9899)  # max|y| of the two clip-guard rows before the guard: far above, just below 0.99


def clip_cases(fs=16000, snr_db=-5.0):
    """Two (clean, noise) float32 pairs of 7003 samples whose remix to snr_db peaks at CLIP_PEAKS: one pair scaled
    as a whole (which changes neither the gain nor the mask) so that the guard fires, one so that it just does not."""
    out = []
    for k, peak in enumerate(CLIP_PEAKS):
        c, n = synth_pair(7003, 200 + k, fs, silent=(k == 0))
        p = remix(c, n, fs, snr_db)[3]["peak"]
        f = peak / p
        out.append(((c.astype(np.float64) * f).astype(np.float32), (n.astype(np.float64) * f).astype(np.float32)))
    return out


def quantise_pair(c, n):
    """Float signals -> int16 (clean, noise) with clean + noise inside the int16 range, so that a noisy file
    clean + noise is exact in 16-bit PCM and noisy - clean gives the noise file's samples back."""
    cq, nq = to_pcm16(c).astype(np.int32), to_pcm16(n).astype(np.int32)
    if np.abs(cq + nq).max() > 32767:
        raise ValueError("quantise_pair: clean + noise leaves the int16 range")
    return cq.astype(np.int16), nq.astype(np.int16)


def pcm_to_float(q):
    """What snrse.audio.read_wav returns for 16-bit PCM samples."""
    return q.astype(np.float32) / 32768.0


def e2e_synth():
    """The two synthetic clips of the end-to-end test, as int16 (clean, noise) at 16 kHz."""
    return {"syn_a.wav": quantise_pair(*synth_pair(20000, 7)), "syn_b.wav": quantise_pair(*synth_pair(33333, 8))}


def rate_pair():
    """The 48 kHz pair of the --rate test, int16 (clean, noise): 1.3 s."""
    return quantise_pair(*synth_pair(62411, 9, fs=48000))
