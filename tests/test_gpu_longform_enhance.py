"""Recordings longer than one network input (GPU): ScoreModel.enhance_batch(window_frames=..., overlap_frames=...),
enhance_long and snrse.enhance_files --window_frames.  Formula weights, a 'bbed' / 'ouve' fp32 model, the PC sampler
with N = 2, windows of 64 frames (W = 8064 samples) cross-faded over 12 (V = 1536), clips from
test_gpu_enhance_files.clip()."""
import os

import numpy as np
import pytest
import torch

import window_ref
from test_gpu_dropin import score_model
from test_gpu_enhance_files import clip, pcm16

pytestmark = pytest.mark.gpu

WF, OF = 64, 12
W, V = (WF - 1) * 128, OF * 128
U = 2.0 ** -24
WIN = dict(window_frames=WF, overlap_frames=OF)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


@pytest.fixture(scope="module")
def model(gpu):
    return score_model("bbed", dtype="fp32")


@pytest.fixture(scope="module")
def long_run(model):
    """L = 20000 (3 windows) under seed 77, batch_size 32: computed once, shared, left unchanged."""
    y = clip(20000, 16000, 3)
    return y, model.enhance_batch([y], seeds=[77], N=2, **WIN)[0]


def test_one_window_is_the_plain_call(model):
    y = clip(7000, 16000, 1)
    plain = model.enhance_batch([y], seeds=[41], N=2)[0]
    win = model.enhance_batch([y], seeds=[41], N=2, **WIN)[0]
    assert win.shape == (7000,) and np.array_equal(plain, win)
    assert model.last_windows == [1] and model.last_guard["flagged_windows"] == []


def test_three_windows_are_the_hand_composition(model, long_run):
    """numpy windows -> enhance_batch(windows, seeds=window seeds) -> window_ref.merge: bit-equal outside the fades,
    within 4 x 2^-24 (|a| + |b|) inside."""
    from snrse import longform
    y, got = long_run
    wins, st, lens = window_ref.gather(y, W, V)
    assert st == [0, 5968, 11936] and lens == [W] * 3 and model.last_windows is not None
    seeds = [longform.window_seed(77, k) for k in range(3)]
    assert seeds[0] == 77
    res = np.stack(model.enhance_batch(list(wins), seeds=seeds, N=2))
    ref, bound = window_ref.merge(res, st, len(y), V)
    k, infade = window_ref.dominant(len(y), st, V)
    assert got.shape == (20000,) and got.dtype == np.float32 and np.isfinite(got).all()
    assert np.array_equal(got[~infade], ref[~infade].astype(np.float32)) and infade.sum() == 2 * V
    err = np.abs(got.astype(np.float64) - ref)[infade]
    print(f"hand composition: worst share of the fade bound {float((err / (4 * U * bound[infade])).max()):.3f}")
    assert (err <= 4 * U * bound[infade]).all()
    assert float(np.abs(got).max()) > 1e-3


def test_batch_size_independence(model, long_run):
    y, got32 = long_run
    got1 = model.enhance_batch([y], seeds=[77], N=2, batch_size=1, **WIN)[0]
    err = rel(got1, got32)
    print(f"windowed batch_size 1 vs 32: rel RMS {err:.2e}")
    assert err < 1e-4


def test_enhance_long_and_sample_rates(model, long_run):
    y, got = long_run
    assert np.array_equal(model.enhance_long(y, seeds=[77], N=2, **WIN), got)
    # declared as 32 kHz the same samples are a 10000-sample recording at 16 kHz: 2 windows, back at 20000 samples
    h = model.enhance_long(y, sample_rate=32000, seeds=[77], N=2, output_rate="input", **WIN)
    assert h.shape == (20000,) and np.isfinite(h).all() and model.last_windows == [2]


def test_window_of_silence(model):
    """One full window of exact zeros in the middle: finite everywhere (the unwindowed rule divides by max|y| = 0
    there), and exactly zero where the silent window is the sole contributor."""
    L = 3 * W - 2 * V  # starts 0, H, 2H: the middle window is [H, H + W)
    st = window_ref.starts(L, W, V)
    assert st == [0, W - V, 2 * (W - V)]
    y = clip(L, 16000, 5)
    y[st[1]:st[1] + W] = 0.0
    h = model.enhance_batch([y], seeds=[9], N=2, **WIN)[0]
    assert h.shape == (L,) and np.isfinite(h).all()
    assert not h[st[1] + V:st[2]].any()                  # the silent window alone
    assert h[:st[1]].any() and h[st[2] + V:].any()       # its neighbours did run
    assert h[st[1]:st[1] + V].any() and h[st[2]:st[2] + V].any()  # and fade out into it / in out of it
    # a recording that is silent altogether is zeros too, without a network call
    z = model.enhance_batch([np.zeros(9000, np.float32)], seeds=[1], N=2, **WIN)[0]
    assert z.shape == (9000,) and not z.any()


def test_row_and_frame_caps(model):
    """40 windows, batch_size 8: no enhancer call sees more than 8 rows or another Tpad than 64."""
    H = W - V
    L = 39 * H + W - 17
    assert len(window_ref.starts(L, W, V)) == 40
    seen, inner = [], model.batched_enhancer

    def wrapped(*a, **kw):
        enh = inner(*a, **kw)

        class Spy:
            last_guard = None

            def __call__(self, yb, **k):
                seen.append((tuple(yb.shape), 64 * -(-(1 + max(k["lengths"]) // 128) // 64)))
                out = enh(yb, **k)
                self.last_guard = enh.last_guard
                return out

        return Spy()

    model.batched_enhancer = wrapped
    try:
        h = model.enhance_batch([clip(L, 16000, 6)], seeds=[3], N=2, corrector="none", batch_size=8, **WIN)[0]
    finally:
        model.batched_enhancer = inner
    assert h.shape == (L,) and np.isfinite(h).all()
    assert len(seen) == 5 and all(s == ((8, W), 64) for s in seen), seen
    assert model.last_windows == [40]


def test_ode_route(model):
    y = clip(20000, 16000, 7)
    h = model.enhance_batch([y], seeds=[5], sampler_type="ode", rtol=1e-2, atol=1e-2, **WIN)[0]
    assert h.shape == (20000,) and np.isfinite(h).all() and float(np.abs(h).max()) > 1e-4
    assert sum(len(s["files"]) for s in model.last_ode_stats) == 3


def test_snr_route_with_oracle(gpu):
    m = score_model("sebridge_v3", "true", fixed_snr=0.17783)
    y = clip(20000, 16000, 8)
    h = m.enhance_batch([y], seeds=[5], oracle=True, clean_rms=[1.0], noise_rms=[0.3], **WIN)[0]
    assert h.shape == (20000,) and np.isfinite(h).all() and float(np.abs(h).max()) > 1e-4


def test_per_utterance_route(model):
    """A setting without a batched enhancer (the `langevin` corrector): every window runs through enhance(), in
    window order, and the merge is the same -- equal to that loop by hand under the same torch.manual_seed."""
    y = clip(10000, 16000, 11)
    wins, st, lens = window_ref.gather(y, W, V)
    assert len(st) == 2 and lens == [W, W]
    torch.manual_seed(3)
    got = model.enhance_batch([y], corrector="langevin", N=2, **WIN)[0]
    torch.manual_seed(3)
    res = np.stack([model.enhance(torch.from_numpy(w)[None], torch.from_numpy(w)[None], corrector="langevin", N=2)
                    for w in wins])
    ref, bound = window_ref.merge(res, st, len(y), V)
    _, infade = window_ref.dominant(len(y), st, V)
    assert got.shape == (10000,) and np.isfinite(got).all() and model.last_windows == [2]
    assert np.array_equal(got[~infade], ref[~infade].astype(np.float32))
    assert (np.abs(got.astype(np.float64) - ref)[infade] <= 4 * U * bound[infade]).all()


def test_flagged_windows(gpu):
    """Weights that leave fp16's range (test_gpu_range_guard's): every window is flagged and recomputed in the
    fallback format; `flagged` lists the utterances, `flagged_windows` the (utterance, window) pairs."""
    from conftest import formula_sd
    from snrse import guard
    from test_gpu_range_guard import SCALED
    from test_gpu_range_guard import score_model as raw_model
    sd = {k: torch.from_numpy(v) for k, v in formula_sd("ncsnpp").items()}
    for k in SCALED:
        sd[k] = sd[k] * 1e6
    m = raw_model(sd, "fp16")
    rng = np.random.default_rng(6)
    ys = [(0.3 * rng.standard_normal(L)).astype(np.float32) for L in (20000, 7000)]
    with pytest.warns(guard.RangeFallbackWarning):
        hs = m.enhance_batch(ys, seeds=[3, 4], N=2, **WIN)
    assert [h.shape for h in hs] == [(20000,), (7000,)] and all(np.isfinite(h).all() for h in hs)
    assert m.last_guard["flagged"] == [0, 1]
    assert m.last_guard["flagged_windows"] == [(0, 0), (0, 1), (0, 2), (1, 0)]


def test_arguments_fail_before_the_device(model):
    y = clip(20000, 16000, 9)
    with pytest.raises(ValueError, match="window_frames"):
        model.enhance_batch([y], window_frames=100)
    with pytest.raises(ValueError, match="overlap_frames"):
        model.enhance_batch([y], window_frames=64, overlap_frames=16)


# ---------------------------------------------------------------------------------------------------- the driver
FOLDER = {"long.wav": (48000, 2, 62400), "short.wav": (16000, 1, 7000)}  # 20800 (3 windows) and 7000 samples at 16 kHz


@pytest.fixture(scope="module")
def folder_runs(model, tmp_path_factory):
    from snrse import audio, enhance_files
    root = tmp_path_factory.mktemp("longform")
    noisy = root / "noisy"
    os.makedirs(noisy)
    k = 0
    for name, (sr, ch, L) in FOLDER.items():
        x = np.stack([clip(L, sr, 60 + k + c) for c in range(ch)], 1)
        k += ch
        audio.write_wav(str(noisy / name), x, sr, bits=32)
    for rate in ("model", "input"):
        torch.manual_seed(5)
        enhance_files.enhance_files(model, str(noisy), str(root / rate), batch_size=32, output_rate=rate, N=2, **WIN)
    torch.manual_seed(5)
    enhance_files.enhance_files(model, str(noisy), str(root / "plain"), batch_size=32, N=2)
    return noisy, root


def test_driver_files_and_csv(folder_runs):
    from snrse import audio
    noisy, root = folder_runs
    for rate in ("model", "input"):
        assert sorted(os.listdir(root / rate)) == ["_enhanced.csv", "long.wav", "short.wav"]
        for name, (sr, ch, L) in FOLDER.items():
            want = (L, ch, sr) if rate == "input" else (audio.resampled_length(L, sr, 16000), ch, 16000)
            assert audio.info(str(root / rate / name)) == want, (rate, name)
            x, _ = audio.load(str(root / rate / name))
            assert torch.isfinite(x).all() and float(x.abs().max()) > 1e-3
        rows = (root / rate / "_enhanced.csv").read_text().strip().split("\n")
        ro = {name: (sr if rate == "input" else 16000) for name, (sr, _, _) in FOLDER.items()}
        assert rows == ["filename,input_rate,channels,seconds,output_rate,windows",
                        f"long.wav,48000,2,1.3,{ro['long.wav']},3", f"short.wav,16000,1,0.4375,{ro['short.wav']},1"]
    assert (root / "plain" / "_enhanced.csv").read_text().split("\n")[0] == \
        "filename,input_rate,channels,seconds,output_rate"


def test_driver_is_plumbing_around_enhance_batch(model, folder_runs):
    """The long file's channels are enhance_batch(window_frames=64, overlap_frames=12) by hand under the seeds the
    driver drew, byte for byte; the short file is what the run without the flags writes under the same seed."""
    from snrse import audio
    noisy, root = folder_runs
    torch.manual_seed(5)
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(3)]
    x, sr = audio.load(str(noisy / "long.wav"))
    assert sr == 48000 and x.shape == (2, 62400)
    for rate in ("model", "input"):
        hand = model.enhance_batch(list(x), seeds=seeds[:2], batch_size=32, N=2, sample_rates=[48000, 48000],
                                   output_rate=rate, **WIN)
        assert model.last_windows == [3, 3]
        got, _ = audio.load(str(root / rate / "long.wav"))
        for c in range(2):
            np.testing.assert_array_equal(got[c].numpy(), pcm16(hand[c]))
        assert not torch.equal(got[0], got[1])
    assert (root / "model" / "short.wav").read_bytes() == (root / "plain" / "short.wav").read_bytes()
    assert (root / "model" / "long.wav").read_bytes() != (root / "plain" / "long.wav").read_bytes()
