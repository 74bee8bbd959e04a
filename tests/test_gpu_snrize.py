"""GPU checks of the fixed-SNR dataset preparation (csrc/snrize.hip, ops.active_rms / ops.snr_remix, snrse.snrize)
against the float64 restatement tests/snrize_ref.py and the data files the reference ships (tests/golden/snrize).
tests/test_snrize_host.py pins that restatement and shows that no window of the synthetic inputs used here lies
within 1e-6 of the activity threshold, so a mismatch below is never a threshold flip."""
import os

import numpy as np
import pytest
import torch

import snrize_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

G = os.path.join(GOLDEN, "snrize")
FS = 16000
W = 1600


def wav(rel):
    from snrse import audio
    return audio.read_wav(os.path.join(G, rel))[0][:, 0]


def golden_pair(name):
    if name == "p226_001.wav":
        return wav("VBD/train/clean/" + name), wav("VBD/train/noise/" + name)
    c = wav("VBD_SNR-5/valid/clean/" + name)
    return c, wav("VBD_SNR-5/valid/noisy/" + name) - c


def pack(pairs, gpu, stride=None):
    """[(clean, noise)] -> (clean, noise [B, stride] f32 on the device, lengths); stride defaults to the longest
    row, which for the cases here is odd: rows start 4, 8 or 12 bytes past a 16-B boundary."""
    lens = [len(c) for c, _ in pairs]
    stride = stride or max(lens)
    c = np.zeros((len(pairs), stride), np.float32)
    n = np.zeros_like(c)
    for b, (x, z) in enumerate(pairs):
        c[b, :lens[b]], n[b, :lens[b]] = x, z
    return torch.from_numpy(c).to(gpu), torch.from_numpy(n).to(gpu), lens


@pytest.fixture(scope="module")
def cases():
    from snrse import _lib
    P = int(_lib.load().snrse_active_windows_per_block())
    pairs = R.gpu_cases(FS, P)
    assert [len(c) for c, _ in pairs][:6] == [W - 1, W, 2 * W + 1, 5000, (P + 1) * W + 37, 27861]
    refs = [R.analyse(c, n, FS) for c, n in pairs]
    return pairs, refs


TARGETS = (-5.0, 0.0, 12.5)


def targets(B):
    return np.array([TARGETS[b % 3] for b in range(B)], np.float64)


@pytest.fixture(scope="module")
def batched(cases, gpu):
    """One ragged batch of all cases through ops.active_rms and ops.snr_remix (floats and PCM), per-row targets."""
    from snrse import ops
    pairs, _ = cases
    c, n, lens = pack(pairs, gpu)
    assert c.shape[1] % 4 != 0 and any((b * c.shape[1]) % 4 for b in range(len(pairs)))
    snr = torch.from_numpy(targets(len(pairs)))
    rms, info = ops.active_rms(c, n, lengths=lens, fs=FS, snr_db=snr, return_info=True)
    fl = ops.snr_remix(c, n, lengths=lens, fs=FS, snr_db=snr)
    q = ops.snr_remix(c, n, lengths=lens, fs=FS, snr_db=snr, pcm16=True)
    torch.cuda.synchronize()
    return dict(c=c, n=n, lens=lens, snr=snr, rms=rms, info=info, fl=fl, q=q)


def test_analysis_matches_reference(cases, batched):
    pairs, refs = cases
    assert any(r["active"].any() and not r["active"].all() for r in refs)  # the mask is exercised
    assert not refs[6]["active"].any()                                     # the all-zero-noise row
    rms, info = batched["rms"].cpu().numpy(), batched["info"]
    act, corr, gain = (info[k].cpu().numpy() for k in ("active_windows", "corr", "gain"))
    assert rms.dtype == np.float64 and corr.dtype == np.float64 and gain.dtype == np.float64
    snr = targets(len(pairs))
    for b, r in enumerate(refs):
        print(b, len(pairs[b][0]), rms[b], r["clean_rms"], r["noise_rms"], act[b], int(r["active"].sum()), corr[b],
              r["corr"], gain[b])
        assert act[b] == r["active"].sum() and int(info["windows"][b]) == len(r["active"])
        assert rms[b, 0] == pytest.approx(r["clean_rms"], rel=1e-10)
        assert rms[b, 1] == pytest.approx(r["noise_rms"], rel=1e-10)
        assert abs(corr[b] - r["corr"]) <= 1e-10
        assert gain[b] == pytest.approx(R.gain(r["clean_rms"], r["noise_rms"], snr[b]), rel=1e-10)
        assert float(info["max_noise"][b]) == np.float32(r["max_noise"])
    assert rms[6, 0] == R.EPS and rms[6, 1] == R.EPS


def test_rows_do_not_depend_on_their_batch(batched, gpu):
    """Each row alone gives the same bits: as a slice of the batch (same address) and as a fresh, 16-B aligned
    buffer of its own length (another alignment, another stride)."""
    from snrse import ops
    c, n, lens, snr = batched["c"], batched["n"], batched["lens"], batched["snr"]
    for b, L in enumerate(lens):
        for cb, nb in ((c[b:b + 1], n[b:b + 1]), (c[b:b + 1, :L].clone(), n[b:b + 1, :L].clone())):
            rms, info = ops.active_rms(cb, nb, lengths=[L], fs=FS, snr_db=snr[b:b + 1], return_info=True)
            assert torch.equal(rms[0], batched["rms"][b])
            for k in ("active_windows", "corr", "gain", "max_noise"):
                assert torch.equal(info[k][0], batched["info"][k][b]), (b, k)
            q = ops.snr_remix(cb, nb, lengths=[L], fs=FS, snr_db=snr[b:b + 1], pcm16=True)
            for t in range(3):
                assert torch.equal(q[t][0, :L], batched["q"][t][b, :L]), (b, t)
            assert torch.equal(q[3]["scale"][0], batched["q"][3]["scale"][b])


def test_mix_error_bound_and_target_snr(cases, batched):
    pairs, refs = cases
    c1, n1, y, info = batched["fl"]
    c1, n1, y = c1.cpu().numpy(), n1.cpu().numpy(), y.cpu().numpy()
    assert np.array_equal(info["scale"].cpu().numpy(), np.ones(len(pairs)))  # no row of these clips
    snr = targets(len(pairs))
    for b, ((c, n), r) in enumerate(zip(pairs, refs)):
        L = len(c)
        g = R.gain(r["clean_rms"], r["noise_rms"], snr[b])
        gn = g * n.astype(np.float64)
        bound = 4 * 2.0 ** -24 * (np.abs(c.astype(np.float64)) + np.abs(gn))
        assert np.array_equal(c1[b, :L], c)
        assert (np.abs(n1[b, :L] - gn) <= bound).all()
        assert (np.abs(y[b, :L] - (c.astype(np.float64) + gn)) <= bound).all()
        assert not c1[b, L:].any() and not n1[b, L:].any() and not y[b, L:].any()
        assert float(info["peak"][b]) == np.abs(y[b, :L]).max()
        if r["active"].any():
            got = R.active_snr_db(c1[b, :L], n1[b, :L], FS)
            print(b, "target", snr[b], "measured", got)
            assert abs(got - snr[b]) <= 1e-4


def test_clip_guard(gpu):
    from snrse import ops
    pairs = R.clip_cases(FS, -5.0)
    c, n, lens = pack(pairs, gpu)
    c1, n1, y, info = ops.snr_remix(c, n, lengths=lens, fs=FS, snr_db=-5.0)
    q = ops.snr_remix(c, n, lengths=lens, fs=FS, snr_db=-5.0, pcm16=True)
    scale, peak = info["scale"].cpu().numpy(), info["peak"].cpu().numpy()
    ref = [R.remix(x, z, FS, -5.0) for x, z in pairs]
    print("peaks", peak, "scales", scale, [r[3]["clip_scale"] for r in ref])
    # the row above 0.99: peak 0.99 within 1 LSB, one scale on all three signals
    assert peak[0] > 0.99 and scale[0] == pytest.approx(ref[0][3]["clip_scale"], rel=1e-6)
    lsb = 1.0 / 32768
    assert abs(float(y[0].abs().max()) - 0.99) <= lsb
    assert abs(int(q[2][0].to(torch.int32).abs().max()) - round(0.99 * 32768)) <= 1
    s32 = np.float32(scale[0])
    g32 = np.float32(float(info["gain"][0]))
    assert np.array_equal(c1[0].cpu().numpy(), pairs[0][0] * s32)
    assert np.array_equal(n1[0].cpu().numpy(), (g32 * pairs[0][1]) * s32)
    # against the float64 remix: at most six f32 roundings (the gain, the product or fma, the peak, the scale, the
    # scaling product) of values no larger than the pre-guard peak 1.2: 6 x 1.2 x 2^-24 < 8 x 2^-24
    for k, x in enumerate((c1, n1, y)):
        assert np.abs(x[0].cpu().numpy() - ref[0][k]).max() <= 8 * 2.0 ** -24
    # the row just below: untouched
    assert 0.989 < peak[1] < 0.99 and scale[1] == 1.0
    assert np.array_equal(c1[1].cpu().numpy(), pairs[1][0])
    assert float(y[1].abs().max()) == peak[1]


@pytest.mark.parametrize("stride,peak", [(4099, 0.5), (4100, 0.5), (4099, 1.3)])
def test_pcm16_is_write_wav_rounding(gpu, stride, peak):
    """int16 = clip(round(x 32768)) of the float32 the kernel itself produces, bit for bit: ties at +-(k + 0.5) LSB
    go to even, values beyond +-1 saturate; vector and scalar paths (stride 4100 / 4099), with and without a
    scale."""
    from snrse import ops
    rng = np.random.default_rng(5)
    k = np.concatenate([np.arange(-40, 40), rng.integers(-32768, 32767, 400)]).astype(np.float64)
    ties = (k + 0.5) / 32768.0
    edge = np.array([1.0, -1.0, 1.5, -1.2, 32767.5 / 32768, -32768.5 / 32768, 32766.5 / 32768, 0.0, -0.0, 3.0, -3.0])
    x = np.concatenate([ties, edge, rng.uniform(-1.1, 1.1, 2 * stride)]).astype(np.float32)
    rows = [torch.from_numpy(np.resize(np.roll(x, 17 * t), (2, stride)).copy()).to(gpu) for t in range(3)]
    pk = torch.full((2,), peak, device=gpu, dtype=torch.float32)
    lens = [stride, stride - 5]
    fl, q, scale = ops.scale_to_pcm16(*rows, pk, lengths=lens)
    assert (scale.cpu().numpy() == (1.0 if peak <= 0.99 else (0.99 - R.EPS) / np.float64(np.float32(peak)))).all()
    for t in range(3):
        f = fl[t].cpu().numpy()
        want = np.clip(np.round(f * 32768.0), -32768, 32767).astype(np.int16)
        assert np.array_equal(q[t].cpu().numpy(), want)
        src = rows[t].cpu().numpy() * np.float32(scale[0].item())
        for b, L in enumerate(lens):
            assert np.array_equal(f[b, :L], src[b, :L]) and not f[b, L:].any()
    if peak <= 0.99:
        got = q[0][0, :len(ties)].cpu().numpy().astype(np.int64)
        assert np.array_equal(got, np.clip(np.where(k % 2 == 0, k, k + 1), -32768, 32767))
    only_q = ops.scale_to_pcm16(*rows, pk, lengths=lens, floats=False)
    assert only_q[0] is None and all(torch.equal(a, b) for a, b in zip(only_q[1], q))


def test_golden_clips(gpu):
    from snrse import ops
    names = ("p226_001.wav", "p232_001.wav")
    outs = ("VBD_SNR-5/train/", "VBD_SNR-5/valid2/")
    c, n, lens = pack([golden_pair(k) for k in names], gpu)
    cq, nq, yq, info = ops.snr_remix(c, n, lengths=lens, fs=FS, snr_db=-5.0, pcm16=True)
    for b, (name, out) in enumerate(zip(names, outs)):
        L = lens[b]
        ship = [R.to_pcm16(wav(out + sub + name)).astype(np.int64) for sub in ("clean/", "noise/", "noisy/")]
        got = [t[b, :L].cpu().numpy().astype(np.int64) for t in (cq, nq, yq)]
        d = [int(np.abs(g - s).max()) for g, s in zip(got, ship)]
        print(name, "LSB clean / noise / noisy", d)
        assert d[0] == 0 and d[1] <= 2 and d[2] <= 2
        assert int(info["active_windows"][b]) == int(info["windows"][b]) == (23, 18)[b]
    with open(os.path.join(G, "active_rms_row1.txt")) as f:
        _, s, z = f.read().rstrip("\n").split("\t")
    rms = info["rms"][1].cpu().numpy()
    assert rms[0] == pytest.approx(float(s), rel=1e-10) and rms[1] == pytest.approx(float(z), rel=1e-10)
    assert float(info["corr"][0]) == pytest.approx(0.012387331561622727, abs=1e-10)
    assert float(info["corr"][1]) == pytest.approx(-0.002335082717693087, abs=1e-10)


def write(path, q, sr=FS):
    from snrse import audio
    os.makedirs(os.path.dirname(path), exist_ok=True)
    audio.write_wav(path, q, sr, bits=16)


def read_q(path):
    from snrse import audio
    x, sr = audio.read_wav(path)
    return (x[:, 0] * 32768.0).astype(np.int16), sr


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """in/{clean,noise,noisy}: the two golden inputs and two synthetic clips, noisy = clean + noise exactly."""
    root = tmp_path_factory.mktemp("snrize")
    clips = dict(R.e2e_synth())
    for name in ("p226_001.wav", "p232_001.wav"):
        c, n = golden_pair(name)
        clips[name] = R.quantise_pair(c, n)
    for name, (cq, nq) in clips.items():
        write(str(root / "in" / "clean" / name), cq)
        write(str(root / "in" / "noise" / name), nq)
        write(str(root / "in" / "noisy" / name), (cq.astype(np.int32) + nq).astype(np.int16))
    return root, clips


def listing(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


def test_end_to_end(corpus, gpu):
    from sgmse.data_module import Specs_SNR
    from snrse import ops, snrize
    root, clips = corpus
    names = sorted(clips)
    base = ["--clean_dir", str(root / "in" / "clean"), "--batch_size", "3"]
    a, b = str(root / "out" / "a"), str(root / "out" / "b")
    assert snrize.main(base + ["--noise_dir", str(root / "in" / "noise"), "--destination_folder", a]) == 0
    assert snrize.main(base + ["--noisy_dir", str(root / "in" / "noisy"), "--destination_folder", b]) == 0
    want = sorted([f"{s}/{k}" for s in ("clean", "noise", "noisy") for k in names]
                  + ["active_rms.txt", "snrize_manifest.tsv"])
    assert listing(a) == want and listing(b) == want
    for rel in want:  # --noisy_dir and --noise_dir: the same bytes
        with open(os.path.join(a, rel), "rb") as f, open(os.path.join(b, rel), "rb") as g:
            assert f.read() == g.read(), rel
    # the files hold the device PCM (one batch here, batches of 3 there: rows do not depend on their batch)
    c, n, lens = pack([(R.pcm_to_float(clips[k][0]), R.pcm_to_float(clips[k][1])) for k in names], gpu)
    q = ops.snr_remix(c, n, lengths=lens, fs=FS, snr_db=-5.0, pcm16=True)
    ds = Specs_SNR(str(root / "out"), "a", False, False, 256)
    assert [os.path.basename(f) for f in ds.clean_files] == names and len(ds.clean_rms) == len(names)
    with open(os.path.join(a, "active_rms.txt")) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    assert [r[0] for r in rows] == names
    for i, k in enumerate(names):
        files = [read_q(os.path.join(a, sub, k)) for sub in ("clean", "noise", "noisy")]
        for t in range(3):
            assert files[t][1] == FS and np.array_equal(files[t][0], q[t][i, :lens[i]].cpu().numpy()), (k, t)
        r = R.analyse(R.pcm_to_float(files[0][0]), R.pcm_to_float(files[1][0]), FS)
        print(k, ds.clean_rms[i], r["clean_rms"], ds.noise_rms[i], r["noise_rms"])
        assert ds.clean_rms[i] == float(rows[i][1]) == pytest.approx(r["clean_rms"], rel=1e-3)
        assert ds.noise_rms[i] == float(rows[i][2]) == pytest.approx(r["noise_rms"], rel=1e-3)
        assert repr(ds.clean_rms[i]) == rows[i][1]
    with open(os.path.join(a, "snrize_manifest.tsv")) as f:
        man = [ln.rstrip("\n").split("\t") for ln in f]
    assert tuple(man[0]) == snrize.MANIFEST_COLUMNS and [m[0] for m in man[1:]] == names
    assert all(len(m) == len(snrize.MANIFEST_COLUMNS) for m in man)


def test_rms_only_and_max_corr(corpus, gpu):
    from snrse import snrize
    root, clips = corpus
    names = sorted(clips)
    base = ["--clean_dir", str(root / "in" / "clean"), "--noise_dir", str(root / "in" / "noise")]
    d = str(root / "out" / "rms")
    assert snrize.main(base + ["--destination_folder", d, "--rms_only"]) == 0
    assert listing(d) == ["active_rms.txt", "snrize_manifest.tsv"]
    with open(os.path.join(d, "active_rms.txt")) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    assert [r[0] for r in rows] == names
    for r in rows:
        ref = R.analyse(R.pcm_to_float(clips[r[0]][0]), R.pcm_to_float(clips[r[0]][1]), FS)
        assert float(r[1]) == pytest.approx(ref["clean_rms"], rel=1e-10)
        assert float(r[2]) == pytest.approx(ref["noise_rms"], rel=1e-10)
    e = str(root / "out" / "corr")
    rows = snrize.remix_files(str(root / "in" / "clean"), e, noise_dir=str(root / "in" / "noise"), max_corr=0.005)
    excluded = [r["name"] for r in rows if r["excluded"]]
    assert "p226_001.wav" in excluded and "p232_001.wav" not in excluded
    with open(os.path.join(e, "excluded.txt")) as f:
        assert f.read().split() == excluded
    kept = [k for k in names if k not in excluded]
    assert sorted(os.listdir(os.path.join(e, "noisy"))) == kept
    with open(os.path.join(e, "active_rms.txt")) as f:
        assert [ln.split("\t")[0] for ln in f] == kept


def test_rate_option_resamples_on_the_device(tmp_path, gpu):
    from snrse import ops, snrize
    cq, nq = R.rate_pair()
    write(str(tmp_path / "clean" / "r.wav"), cq, 48000)
    write(str(tmp_path / "noise" / "r.wav"), nq, 48000)
    write(str(tmp_path / "noisy" / "r.wav"), (cq.astype(np.int32) + nq).astype(np.int16), 48000)
    out = str(tmp_path / "out")
    assert snrize.main(["--clean_dir", str(tmp_path / "clean"), "--noise_dir", str(tmp_path / "noise"),
                        "--destination_folder", out, "--rate", "16000"]) == 0
    c = torch.from_numpy(R.pcm_to_float(cq)[None]).to(gpu)
    n = torch.from_numpy(R.pcm_to_float(nq)[None]).to(gpu)
    c16, ln = ops.resample_poly(c, 1, 3)
    n16, _ = ops.resample_poly(n, 1, 3)
    L = int(ln[0])
    assert L == -(-len(cq) // 3)
    q = ops.snr_remix(c16, n16, lengths=[L], fs=16000, snr_db=-5.0, pcm16=True)
    for t, sub in enumerate(("clean", "noise", "noisy")):
        got, sr = read_q(os.path.join(out, sub, "r.wav"))
        assert sr == 16000 and np.array_equal(got, q[t][0, :L].cpu().numpy()), sub
    with open(os.path.join(out, "snrize_manifest.tsv")) as f:
        row = f.read().splitlines()[1].split("\t")
    assert row[1] == "16000" and int(row[2]) == L and int(row[9]) == -(-L // 1600)
    # with --noisy_dir the difference is formed after resampling: the noise is resample(noisy) - resample(clean)
    out2 = str(tmp_path / "out2")
    assert snrize.main(["--clean_dir", str(tmp_path / "clean"), "--noisy_dir", str(tmp_path / "noisy"),
                        "--destination_folder", out2, "--rate", "16000"]) == 0
    y = torch.from_numpy(R.pcm_to_float((cq.astype(np.int32) + nq).astype(np.int16))[None]).to(gpu)
    y16, _ = ops.resample_poly(y, 1, 3)
    q2 = ops.snr_remix(c16, (y16 - c16).contiguous(), lengths=[L], fs=16000, snr_db=-5.0, pcm16=True)
    for t, sub in enumerate(("clean", "noise", "noisy")):
        assert np.array_equal(read_q(os.path.join(out2, sub, "r.wav"))[0], q2[t][0, :L].cpu().numpy()), sub
