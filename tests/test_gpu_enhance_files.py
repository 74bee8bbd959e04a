"""Recordings at any sample rate and channel count through the enhancement path (GPU): snrse.enhance_files on a
folder of 48 kHz stereo, 16 kHz mono and 44.1 kHz mono files, its agreement with snrse.evaluate on 16 kHz mono files,
snrse.evaluate --resample, and ScoreModel.enhance_batch(sample_rates=...).  Formula weights, a 'bbed' / 'ouve' fp32
model, the PC sampler with N = 2, clips of 0.4 - 0.5 s (every one pads to 64 frames)."""
import os

import numpy as np
import pytest
import torch

from test_gpu_dropin import score_model

pytestmark = pytest.mark.gpu

# name -> (rate, channels, frames); at 16 kHz: 7200, 7000, 6720 samples
FOLDER = {"a.wav": (48000, 2, 21600), "b.wav": (16000, 1, 7000), "c.wav": (44100, 1, 18522)}


def clip(L, sr, k):
    rng = np.random.default_rng(200 + k)
    t = np.arange(L) / float(sr)
    x = 0.2 * np.sin(2 * np.pi * (300.0 + 170.0 * k) * t) + (0.02 + 0.02 * k) * rng.standard_normal(L)
    return (0.03 * x).astype(np.float32)  # quiet: formula weights amplify, and the 16-bit files should not clip


def pcm16(h):
    return (np.clip(np.round(np.asarray(h) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


@pytest.fixture(scope="module")
def model(gpu):
    return score_model("bbed", dtype="fp32")


def recording(m):
    """m.enhance_batch wrapped to keep (keywords, results) of every call that names sample_rates (the call it makes
    to itself with the 16 kHz signals does not); -> (calls, undo)."""
    inner, calls = m.enhance_batch, []

    def rec(ys, **kw):
        r = inner(ys, **kw)
        if "sample_rates" in kw:
            calls.append((kw, [np.asarray(h).copy() for h in r]))
        return r

    m.enhance_batch = rec

    def undo():
        m.enhance_batch = inner

    return calls, undo


@pytest.fixture(scope="module")
def folder_runs(model, tmp_path_factory):
    """The folder, and snrse.enhance_files run on it at both output rates under torch.manual_seed(5)."""
    from snrse import audio, enhance_files
    root = tmp_path_factory.mktemp("mixed")
    noisy = root / "noisy"
    os.makedirs(noisy)
    k = 0
    for name, (sr, ch, L) in FOLDER.items():
        x = np.stack([clip(L, sr, k + c) for c in range(ch)], 1)
        k += ch
        audio.write_wav(str(noisy / name), x, sr, bits=32)
    calls, undo = recording(model)
    try:
        for rate in ("model", "input"):
            torch.manual_seed(5)
            enhance_files.enhance_files(model, str(noisy), str(root / rate), batch_size=32, output_rate=rate, N=2)
    finally:
        undo()
    return noisy, root, calls


def test_written_files(folder_runs):
    from snrse import audio
    noisy, root, calls = folder_runs
    assert len(calls) == 2 and all(len(r) == 4 for _, r in calls)  # the four channels share one ragged batch
    for rate in ("model", "input"):
        assert sorted(os.listdir(root / rate)) == ["_enhanced.csv", "a.wav", "b.wav", "c.wav"]
        for name, (sr, ch, L) in FOLDER.items():
            want = (L, ch, sr) if rate == "input" else (audio.resampled_length(L, sr, 16000), ch, 16000)
            assert audio.info(str(root / rate / name)) == want, (rate, name)
            x, _ = audio.load(str(root / rate / name))
            assert torch.isfinite(x).all() and float(x.abs().max()) > 1e-3
        rows = (root / rate / "_enhanced.csv").read_text().strip().split("\n")
        assert rows[0] == "filename,input_rate,channels,seconds,output_rate" and len(rows) == 4
        assert rows[1] == f"a.wav,48000,2,0.45,{48000 if rate == 'input' else 16000}"
        assert rows[3] == f"c.wav,44100,1,0.42,{44100 if rate == 'input' else 16000}"
    assert [audio.resampled_length(L, sr, 16000) for sr, _, L in FOLDER.values()] == [7200, 7000, 6720]
    # the stereo file's channels are different utterances with different seeds
    a, _ = audio.load(str(root / "model" / "a.wav"))
    assert not torch.equal(a[0], a[1])


def test_cli_is_plumbing_around_resample_and_enhance_batch(gpu, model, folder_runs):
    """The 16 kHz outputs are enhance_batch of the channels resampled with ops.resample_poly by hand under the
    seeds the driver drew, bit for bit; the input-rate outputs are those resampled back and cut to L_i."""
    from snrse import audio, ops
    noisy, root, calls = folder_runs
    torch.manual_seed(5)
    seeds = [int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(4)]
    chans, rates = [], []
    for name, (sr, ch, L) in FOLDER.items():
        x, sr_file = audio.load(str(noisy / name))
        assert sr_file == sr and x.shape == (ch, L)
        chans += list(x)
        rates += [sr] * ch
    ys16 = []
    for x, sr in zip(chans, rates):
        if sr == 16000:
            ys16.append(x.numpy())
        else:
            y, n = ops.resample_poly(x[None].to(gpu), *audio.rational(sr, 16000))
            assert int(n[0]) == audio.resampled_length(len(x), sr, 16000) == y.shape[1]
            ys16.append(y[0].cpu().numpy())
    hand = model.enhance_batch(ys16, seeds=seeds, batch_size=32, N=2)
    (kw_m, got_m), (kw_i, got_i) = calls
    assert kw_m["seeds"] == seeds == kw_i["seeds"] and kw_m["sample_rates"] == rates
    for k in range(4):
        assert np.array_equal(got_m[k], hand[k]), k
        back, _ = ops.resample_poly(torch.from_numpy(hand[k])[None].to(gpu), *audio.rational(16000, rates[k]))
        assert back.shape[1] >= len(chans[k])
        want = back[0, :len(chans[k])].cpu().numpy() if rates[k] != 16000 else hand[k]
        assert got_i[k].shape == (len(chans[k]),) and np.array_equal(got_i[k], want), k
    k = 0
    for name, (sr, ch, L) in FOLDER.items():
        for rate, got in (("model", got_m), ("input", got_i)):
            x, _ = audio.load(str(root / rate / name))
            for c in range(ch):
                np.testing.assert_array_equal(x[c].numpy(), pcm16(got[k + c]))
        k += ch


def test_same_bytes_as_evaluate_on_16k_mono(model, tmp_path):
    from snrse import audio, enhance_files, evaluate
    root = tmp_path / "test"
    for d in ("clean", "noisy"):
        os.makedirs(root / d)
    for k, L in enumerate((7000, 9000, 6500)):  # Tpad 64, 128, 64: two batches
        y = clip(L, 16000, 10 + k)
        audio.write_wav(str(root / "clean" / f"f{k}.wav"), 0.5 * y, bits=32)
        audio.write_wav(str(root / "noisy" / f"f{k}.wav"), y, bits=32)
    torch.manual_seed(7)
    evaluate.evaluate(model, str(root), str(tmp_path / "ev"), N=2, batch_size=32)
    torch.manual_seed(7)
    enhance_files.enhance_files(model, str(root / "noisy"), str(tmp_path / "ef"), N=2, batch_size=32)
    for k in range(3):
        a = (tmp_path / "ev" / "all" / f"f{k}.wav").read_bytes()
        b = (tmp_path / "ef" / f"f{k}.wav").read_bytes()
        assert len(a) >= 44 + 2 * 6500 and a == b, k


@pytest.mark.parametrize("batch_size", [4, 1])
def test_evaluate_resample(gpu, model, tmp_path, batch_size):
    """A 48 kHz test_dir with resample=True: 16 kHz files of resampled_length frames, metric rows those of
    evaluate.score_batch on the clean / noisy signals resampled by hand and the waveforms the run returned (the
    same call for batch_size 4; the per-file loop scores with the unragged kernel: 1e-5 dB)."""
    from snrse import audio, evaluate, ops
    root = tmp_path / "test"
    for d in ("clean", "noisy"):
        os.makedirs(root / d)
    lens = (21600, 22001)
    for k, L in enumerate(lens):
        c = clip(L, 48000, 20 + k)
        audio.write_wav(str(root / "clean" / f"f{k}.wav"), 0.8 * c, 48000, bits=32)
        audio.write_wav(str(root / "noisy" / f"f{k}.wav"), c + 0.03 * clip(L, 48000, 30 + k), 48000, bits=32)
    got = []
    inner_b, inner_1 = model.enhance_batch, model.enhance
    model.enhance_batch = lambda ys, **kw: got.extend(inner_b(ys, **kw)) or got[-len(ys):]
    model.enhance = lambda x, y, **kw: got.append(inner_1(x, y, **kw)) or got[-1]
    try:
        torch.manual_seed(3)
        data = evaluate.evaluate(model, str(root), str(tmp_path / "out"), N=2, batch_size=batch_size, resample=True)
    finally:
        model.enhance_batch, model.enhance = inner_b, inner_1
    assert len(got) == 2 and data["filename"] == ["f0.wav", "f1.wav"]
    xs, ys = [], []
    for k, L in enumerate(lens):
        n16 = audio.resampled_length(L, 48000, 16000)
        assert audio.info(str(tmp_path / "out" / "all" / f"f{k}.wav")) == (n16, 1, 16000)
        assert got[k].shape == (n16,)
        for d, dst in (("clean", xs), ("noisy", ys)):
            s, sr = audio.load(str(root / d / f"f{k}.wav"))
            assert sr == 48000
            dst.append(ops.resample_poly(s.to(gpu), 1, 3)[0][0].cpu().numpy())
    er, Ls = evaluate.score_batch([np.asarray(h, np.float32) for h in got], xs, ys)
    assert Ls == [7200, 7334]
    rows = np.array([[data[m][k] for m in ("si_sdr", "si_sir", "si_sar")] for k in range(2)])
    assert np.isfinite(rows).all()
    if batch_size > 1:
        np.testing.assert_array_equal(rows, er)
    else:
        np.testing.assert_allclose(rows, er, rtol=0, atol=1e-5)


def test_deep_evaluate_resample_equals_the_resampled_test_dir(gpu, model, tmp_path):
    """deep_evaluate(resample=True) on a 48 kHz pair is deep_evaluate on the pair resampled by hand and stored as
    16 kHz float files, under the same torch.manual_seed: the same SI-SDR columns and the same bytes written."""
    from snrse import audio, deep_evaluate, ops
    hi, lo = tmp_path / "hi", tmp_path / "lo"
    c = clip(21600, 48000, 50)
    pair = {"clean": 0.8 * c, "noisy": c + 0.03 * clip(21600, 48000, 51)}
    for d, s in pair.items():
        os.makedirs(hi / d)
        os.makedirs(lo / d)
        audio.write_wav(str(hi / d / "f.wav"), s, 48000, bits=32)
        s16 = ops.resample_poly(torch.from_numpy(s.astype(np.float32))[None].to(gpu), 1, 3)[0][0].cpu().numpy()
        audio.write_wav(str(lo / d / "f.wav"), s16, 16000, bits=32)
    res = []
    for root, flag in ((hi, True), (lo, False)):
        torch.manual_seed(9)
        res.append(deep_evaluate.deep_evaluate(model, str(root), str(root / "out"), N=2, si_sdr=True, verbose=False,
                                               resample=flag))
    for lab in deep_evaluate.LABELS:
        assert res[0][f"si_sdr_{lab}"] == res[1][f"si_sdr_{lab}"] and np.isfinite(res[0][f"si_sdr_{lab}"]).all()
        a = (hi / "out" / "{0:02d}".format(lab) / "f.wav").read_bytes()
        assert len(a) == 44 + 2 * 7200 and a == (lo / "out" / "{0:02d}".format(lab) / "f.wav").read_bytes()


def test_enhance_batch_all_at_16k_is_the_plain_call(model):
    ys = [clip(7000, 16000, 40), clip(6400, 16000, 41)]
    seeds = [123, 2 ** 61 + 9]
    plain = model.enhance_batch(ys, seeds=seeds, N=2)
    for rate in ("model", "input"):
        rated = model.enhance_batch(ys, seeds=seeds, N=2, sample_rates=[16000, 16000], output_rate=rate)
        assert all(np.array_equal(a, b) for a, b in zip(plain, rated)), rate
    # and a rate really changes the call: the same samples declared as 32 kHz come back half as long
    half = model.enhance_batch(ys, seeds=seeds, N=2, sample_rates=[32000, 16000])
    assert [len(h) for h in half] == [3500, 6400] and np.array_equal(half[1].shape, plain[1].shape)
