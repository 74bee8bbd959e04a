"""snrse.enhance_files --loudness / --peak_db end to end (GPU).

A stand-in model whose enhance_batch returns half its input (at the file's rate, or resampled to 16 kHz for
output_rate="model"), so that every level is known, on a folder of five files: 48 kHz stereo, 16 kHz mono, 44.1 kHz
mono, a 16 kHz file under 400 ms (no block: -inf, gain 1) and a 16 kHz file of clicks over a quiet floor, whose 4x
peak forces the ceiling.  The written files are re-read and measured by the fp64 reference (tests/loudness_ref.py).

Tolerances.  Written loudness against the target: 1e-3 LU -- 16-bit rounding noise sits at -101 dBFS, 78 dB under
the programme, under 1e-6 dB; the margin is for the gates seeing a scaled signal.  The csv's own loudness figures
against the reference on the float signals: 1e-6 LU, the kernels' bound.  A re-measured 4x peak against the csv's:
rounding to 16 bit moves a sample by at most 0.5 / 32768 and an interpolated value by at most that times the
largest sum of |taps| of a phase (S = 2.24), so 20 log10(1 + 0.5 S / (32768 p)) dB for a peak p, plus 1e-4 dB
for the fp32 resampler against fp64; for the limited file (p = 0.891) that is 4.4e-4 dB, inside the 1e-3 dB asked
of it.  The written samples themselves are exact: clip(rint(fl32(fl32(g) x) 32768)) with g = 10^(gain_db / 20)
of the csv's gain_db."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import loudness_ref as ref

pytestmark = pytest.mark.gpu

TARGET, CEILING = -23.0, -1.0
LU_TOL, PEAK_TOL_DB = 1e-3, 1e-3
COLS = "filename,input_rate,channels,seconds,output_rate,input_lufs,enhanced_lufs,gain_db,peak_db,limited"


def folder_files():
    """name -> (rate, [frames, channels] float32)."""
    rng = np.random.default_rng(77)
    t = lambda L, sr: np.arange(L) / float(sr)
    a = np.stack([0.05 * rng.standard_normal(57600), 0.03 * rng.standard_normal(57600)
                  + 0.05 * np.sin(2 * np.pi * 440.0 * t(57600, 48000))], 1)
    b = 0.1 * np.sin(2 * np.pi * 300.0 * t(16000, 16000)) + 0.01 * rng.standard_normal(16000)
    c = 0.04 * rng.standard_normal(39690)
    d = 0.1 * np.sin(2 * np.pi * 500.0 * t(4800, 16000))  # 0.3 s
    e = 0.002 * rng.standard_normal(16000)
    e[500::2000] += 0.6  # clicks: little loudness, much peak
    return {"a.wav": (48000, a.astype(np.float32)), "b.wav": (16000, b.astype(np.float32)[:, None]),
            "c.wav": (44100, c.astype(np.float32)[:, None]), "d.wav": (16000, d.astype(np.float32)[:, None]),
            "e.wav": (16000, e.astype(np.float32)[:, None])}


class _SDE:
    T = 1.0


class HalfModel:
    """enhance_batch returns 0.5 y, at the rate asked for; keeps (input, result) of every row."""
    sde = _SDE()

    def __init__(self):
        self.returned = []

    def _batch_route(self, sampler_type, corrector, kw):
        return "stub"

    def enhance_batch(self, ys, seeds=None, sample_rates=None, output_rate="model", **kw):
        from snrse import resample
        src = [np.asarray(y, np.float32) for y in ys]
        ys = src
        if output_rate == "model":
            ys = [np.asarray(v, np.float32) for v in resample.convert(src, list(sample_rates), 16000)]
        out = [(np.float32(0.5) * y).astype(np.float32) for y in ys]
        self.returned += list(zip(src, out))
        return out

    def result_for(self, channel):
        hits = [o for y, o in self.returned if len(y) == len(channel) and np.array_equal(y, channel)]
        assert len(hits) == 1
        return hits[0]


def write_folder(noisy):
    from snrse import audio
    os.makedirs(noisy, exist_ok=True)
    for name, (sr, x) in folder_files().items():
        audio.write_wav(os.path.join(noisy, name), x, sr, bits=32)


def read_csv(path):
    lines = open(path).read().strip().split("\n")
    keys = lines[0].split(",")
    return lines[0], {r.split(",")[0]: dict(zip(keys, r.split(","))) for r in lines[1:]}


def run(tmp, loudness, output_rate="input", **kw):
    from snrse import enhance_files
    noisy, out = os.path.join(tmp, "noisy"), os.path.join(tmp, f"out_{loudness}_{output_rate}")
    write_folder(noisy)
    m = HalfModel()
    enhance_files.enhance_files(m, noisy, out, batch_size=32, output_rate=output_rate, loudness=loudness,
                                peak_db=CEILING, **kw)
    # what the model returned, per file and channel (the batches follow the padded lengths, not the file order)
    enhanced = {name: [m.result_for(x[:, c]) for c in range(x.shape[1])] for name, (_, x) in folder_files().items()}
    return out, enhanced


def phase_sum():
    w = 4.0 * ref.resample_taps_4x()
    return max(float(np.abs(w[p::4]).sum()) for p in range(4))


def peak_tolerance(p):
    return 20.0 * math.log10(1.0 + 0.5 * phase_sum() / (32768.0 * p)) + 1e-4


def check_folder(out, enhanced, output_rate, policy):
    from snrse import audio
    head, rows = read_csv(os.path.join(out, "_enhanced.csv"))
    assert head == COLS and sorted(rows) == sorted(folder_files())
    flagged = []
    for name, (sr, noisy) in folder_files().items():
        row = rows[name]
        ro = sr if output_rate == "input" else 16000
        assert int(row["output_rate"]) == ro
        x = enhanced[name]
        q, sr_w = audio.read_wav(os.path.join(out, name))  # [frames, channels], int16 / 32768
        assert sr_w == ro and q.shape == (len(x[0]), len(x))
        l_in, l_enh, gain_db, peak_db = (float(row[k]) for k in ("input_lufs", "enhanced_lufs", "gain_db", "peak_db"))
        limited = row["limited"] == "1"
        # the csv's measurements are the reference's on the float signals
        r_in = ref.integrated([noisy[:, c] for c in range(noisy.shape[1])], sr)
        r_enh = ref.integrated(x, ro)
        for got, want in ((l_in, r_in["lufs"]), (l_enh, r_enh["lufs"])):
            assert got == want if want == -math.inf else abs(got - want) <= 1e-6, (name, got, want)
        # the written samples are the conversion of the float result times the csv's gain: one gain, every channel
        g = 10.0 ** (gain_db / 20.0)
        for c, xc in enumerate(x):
            want = ref.gain_pcm16(xc, g)
            assert np.array_equal(np.round(q[:, c] * 32768.0).astype(np.int16), want), (name, c)
        p_enh = max(ref.peak4(xc) for xc in x)
        assert abs(peak_db - 20 * math.log10(g * p_enh)) <= 1e-4, (name, peak_db)
        p_written = max(ref.peak4(q[:, c]) for c in range(q.shape[1]))
        assert abs(20 * math.log10(p_written) - peak_db) <= peak_tolerance(p_written), (name, p_written, peak_db)
        assert peak_db <= CEILING + 1e-9 or gain_db == 0.0, (name, peak_db)
        want_l = TARGET if policy == "number" else r_in["lufs"]
        written = ref.integrated([q[:, c] for c in range(q.shape[1])], ro)
        if l_enh == -math.inf:
            flagged.append(name)
            assert gain_db == 0.0 and not limited, name  # written with gain 1
            assert np.array_equal(np.round(q[:, 0] * 32768.0).astype(np.int16), ref.gain_pcm16(x[0], 1.0))
        elif limited:
            flagged.append(name)
            assert abs(20 * math.log10(p_written) - CEILING) <= PEAK_TOL_DB, (name, p_written)
            assert written["lufs"] < want_l and abs(written["lufs"] - (l_enh + gain_db)) <= LU_TOL
        else:
            assert abs(written["lufs"] - want_l) <= LU_TOL, (name, written["lufs"], want_l)
            assert abs(l_enh + gain_db - want_l) <= 1e-9
    return flagged, rows


@pytest.mark.parametrize("output_rate", ("input", "model"))
def test_target_loudness(gpu, tmp_path, output_rate):
    out, enhanced = run(str(tmp_path), "-23", output_rate)
    flagged, rows = check_folder(out, enhanced, output_rate, "number")
    assert sorted(flagged) == ["d.wav", "e.wav"]  # only the two files built for it
    assert rows["e.wav"]["limited"] == "1" and rows["d.wav"]["limited"] == "0"
    assert rows["d.wav"]["enhanced_lufs"] == "-inf"


def test_input_loudness(gpu, tmp_path):
    out, enhanced = run(str(tmp_path), "input")
    flagged, rows = check_folder(out, enhanced, "input", "input")
    assert flagged == ["d.wav"]
    # half the input brought back to the input's loudness: a gain of two, for both channels of the stereo file
    assert abs(float(rows["a.wav"]["gain_db"]) - 20 * math.log10(2.0)) <= 1e-6


def test_off_is_the_call_without_the_option(gpu, tmp_path):
    from snrse import enhance_files
    noisy = str(tmp_path / "noisy")
    write_folder(noisy)
    for name, kw in (("plain", {}), ("off", dict(loudness="off", peak_db=-3.0))):
        enhance_files.enhance_files(HalfModel(), noisy, str(tmp_path / name), output_rate="input", **kw)
    for f in sorted(os.listdir(tmp_path / "plain")):
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "off" / f).read_bytes(), f
    assert (tmp_path / "off" / "_enhanced.csv").read_text().startswith(
        "filename,input_rate,channels,seconds,output_rate\n")
    with pytest.raises(ValueError):
        enhance_files.enhance_files(HalfModel(), noisy, str(tmp_path / "bad"), loudness="-23", peak_db=0.5)
    with pytest.raises(ValueError):
        enhance_files.enhance_files(HalfModel(), noisy, str(tmp_path / "bad"), loudness="loud")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, noisy, out, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")  # both ranks share the one device
    from snrse import dist as sd
    from snrse import enhance_files
    r, w, _ = sd.init_from_env("gloo")
    files = enhance_files.enhance_files(HalfModel(), noisy, out, output_rate="input", loudness="-23", peak_db=CEILING,
                                        rank=r, world=w)
    q.put((r, len(files)))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_write_the_same_table(gpu, tmp_path):
    out1, _ = run(str(tmp_path), "-23")
    noisy, out2 = str(tmp_path / "noisy"), str(tmp_path / "two_ranks")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, noisy, out2, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, 5), (1, 5)]
    for f in sorted(os.listdir(out1)):
        assert open(os.path.join(out1, f), "rb").read() == open(os.path.join(out2, f), "rb").read(), f


def test_one_step_model_windowed_is_consistent(gpu, tmp_path):
    """The real one-step route (formula weights, fp32) with window_frames=64 on two files: whatever the network
    returns, the written bytes are the device conversion of that float result times the csv's gain, and the 4x
    peak stays under the ceiling."""
    from sgmse.backbones import SNRNet
    from sgmse.model import get_snr_model, set_snr_model
    from conftest import formula_sd
    from snrse import audio, enhance_files
    from test_gpu_dropin import score_model
    from test_gpu_enhance_files import clip

    net = SNRNet()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in formula_sd("snrnet", "snrnet.").items()})

    class _Est:
        def estimate_from_spec(self, spec):
            g = net.forward_complex(spec)[:, 0]
            return g / (1 - g)

    noisy = tmp_path / "noisy"
    os.makedirs(noisy)
    audio.write_wav(str(noisy / "a.wav"), np.stack([clip(27000, 48000, 0), clip(27000, 48000, 1)], 1), 48000, bits=32)
    audio.write_wav(str(noisy / "b.wav"), clip(9000, 16000, 2), 16000, bits=32)
    m = score_model("sebridge_v3", "true", fixed_snr=0.17783)
    inner, returned = m.enhance_batch, []

    def spy(ys, **kw):
        r = inner(ys, **kw)
        if "sample_rates" in kw:
            returned.extend(np.asarray(h, np.float32).copy() for h in r)
        return r

    m.enhance_batch = spy
    prev = get_snr_model.__globals__["_snr_model"]
    set_snr_model(_Est())
    try:
        torch.manual_seed(5)
        enhance_files.enhance_files(m, str(noisy), str(tmp_path / "out"), output_rate="input", window_frames=64,
                                    overlap_frames=12, loudness="-23", peak_db=CEILING)
    finally:
        set_snr_model(prev)
        m.enhance_batch = inner
    head, rows = read_csv(str(tmp_path / "out" / "_enhanced.csv"))
    assert head == COLS.replace(",input_lufs", ",windows,input_lufs")
    assert len(returned) == 3
    for name, xs in (("a.wav", returned[:2]), ("b.wav", returned[2:])):
        q, _ = audio.read_wav(str(tmp_path / "out" / name))
        g = 10.0 ** (float(rows[name]["gain_db"]) / 20.0)
        for c, xc in enumerate(xs):
            assert np.isfinite(xc).all() and np.abs(xc).max() > 0
            assert np.array_equal(np.round(q[:, c] * 32768.0).astype(np.int16), ref.gain_pcm16(xc, g)), (name, c)
        assert float(rows[name]["peak_db"]) <= CEILING + 1e-9
        assert rows[name]["windows"] == "2"


def test_meter_lists_a_folder(gpu, tmp_path):
    """python -m snrse.loudness DIR --csv FILE: one row per file, the channels of a file measured together."""
    from snrse import loudness
    noisy, csv = str(tmp_path / "noisy"), str(tmp_path / "levels.csv")
    write_folder(noisy)
    loudness.main([noisy, "--csv", csv])
    lines = open(csv).read().strip().split("\n")
    assert lines[0] == "filename,rate,channels,seconds,lufs,peak_db" and len(lines) == 6
    for line, (name, (sr, x)) in zip(lines[1:], sorted(folder_files().items())):
        f = line.split(",")
        assert (f[0], int(f[1]), int(f[2]), float(f[3])) == (name, sr, x.shape[1], x.shape[0] / sr)
        chans = [x[:, c] for c in range(x.shape[1])]
        want = ref.integrated(chans, sr)["lufs"]
        assert float(f[4]) == want if want == -math.inf else abs(float(f[4]) - want) <= 1e-4  # four decimals
        assert abs(float(f[5]) - 20 * math.log10(max(ref.peak4(c) for c in chans))) <= 2e-4
