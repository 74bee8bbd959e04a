"""ESTOI on the GPU (snrse_estoi through ops.estoi) against the fp64 numpy reference tests/estoi_ref.py.

Signals: seeded band-limited noise under a syllable-rate envelope, the second signal at SNR 0, 10 or 30 dB
(estoi_ref.speechlike).  Every compared row first asserts its precondition on the reference: every frame energy lies
at least 1e-3 dB from the keep threshold, so the fp64 keep decision of the kernel cannot differ from the reference's.

Bound (not fixed in advance): the reference's float32 mode runs in fp32 what the kernels run in fp32; the GPU result
has to stay within 4 x |float32 mode - fp64| + 2^-24 of the fp64 reference.  The measured pairs go to
profiles/estoi_errors.json.  Rows that give the 1e-5 sentinel or 0.0 are compared exactly."""
import json
import os

import numpy as np
import pytest
import torch

import estoi_ref as er
from conftest import ROOT

pytestmark = pytest.mark.gpu

ERRORS = os.path.join(ROOT, "profiles", "estoi_errors.json")
SNRS = (0.0, 10.0, 30.0)


def block():
    from snrse import _lib
    return int(_lib.load().snrse_estoi_block())


def ragged_nan(rows, gpu):
    """[B, stride] device buffer of the rows, NaN at and past each row's length."""
    buf = torch.full((len(rows), max(len(r) for r in rows)), float("nan"), dtype=torch.float32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = torch.from_numpy(np.asarray(r, np.float32))
    return buf.to(gpu)


def record(key, value):
    data = {}
    if os.path.exists(ERRORS):
        with open(ERRORS) as f:
            data = json.load(f)
    data[key] = value
    try:
        with open(ERRORS, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:  # a read-only tree: the figures are printed below, the assertions do not depend on the file
        pass


def pair(seed, L, fs=er.FS):
    return er.speechlike(seed, L, fs, SNRS[seed % 3])


def silenced(seed, L, lo, hi):
    """A pair whose samples [lo, hi) are at 1e-4 of the level."""
    x, y = (s.copy() for s in pair(seed, L))
    x[lo:hi] *= 1e-4
    y[lo:hi] *= 1e-4
    return x, y


def run(pairs, gpu, fs=er.FS):
    from snrse import ops
    lens = [len(x) for x, _ in pairs]
    d, info = ops.estoi(ragged_nan([x for x, _ in pairs], gpu), ragged_nan([y for _, y in pairs], gpu), lengths=lens,
                        fs=fs, return_info=True)
    return d.cpu().numpy(), info.cpu().numpy()


def check(name, pairs, gpu, fs=er.FS):
    """The batch against the reference, row by row; -> (d, info, reference details)."""
    d, info = run(pairs, gpu, fs)
    assert d.dtype == np.float64 and info.shape == (len(pairs), 2)
    out, dets = [], []
    for b, (x, y) in enumerate(pairs):
        ref, det = er.estoi(x, y, fs, details=True)
        dets.append(det)
        assert det["margin"] >= 1e-3, f"{name}[{b}]: a frame energy {det['margin']:.2e} dB from the keep threshold"
        assert tuple(info[b]) == (det["K"], det["S"]), (name, b, tuple(info[b]), det["K"], det["S"])
        if det["S"] == 0:
            assert d[b] == er.SENTINEL
            continue
        f32 = abs(er.estoi(x, y, fs, dtype=np.float32) - ref)
        bound = 4.0 * f32 + 2.0 ** -24
        err = abs(d[b] - ref)
        out.append([float(err), float(f32), float(bound)])
        print(f"estoi {name}[{b}] L {len(x)} K {det['K']} S {det['S']} margin {det['margin']:.2f} dB: ref {ref:.9f} "
              f"hip err {err:.2e} float32-mode err {f32:.2e} bound {bound:.2e}")
    record(name, out)
    for err, _, bound in out:
        assert err <= bound, (name, out)
    return d, info, dets


def test_frame_count_edges(gpu):
    Ls = (256, 257, 384, 385, 256 + 128 * 31 - 1, 256 + 128 * 31, 256 + 128 * 31 + 1)
    _, info, dets = check("edges", [pair(10 + k, L) for k, L in enumerate(Ls)], gpu)
    assert [det["nf"] for det in dets] == [0, 1, 1, 2, 31, 31, 32]
    assert [int(s) for s in info[:, 1]] == [0, 0, 0, 0, 1, 1, 2]


def test_thirty_and_thirty_one_kept_frames(gpu):
    L = 256 + 128 * 40  # 40 frames; a silent stretch of n + 1 hops removes the n frames that lie wholly inside it
    d, info, _ = check("k30_k31", [silenced(20, L, 128 * 12, 128 * 23), silenced(21, L, 128 * 12, 128 * 22)], gpu)
    assert [tuple(r) for r in info] == [(30, 0), (31, 1)]
    assert d[0] == er.SENTINEL and d[1] != er.SENTINEL


def test_compaction(gpu):
    eb = block()
    nf = 8 * eb + 3
    L = 256 + 128 * nf
    cases = [silenced(30, L, 128 * (eb - 2), 128 * (eb + 3)),          # frames eb-2 .. eb+1 removed: across a boundary
             silenced(31, L, 128 * (3 * eb - 1), 128 * (4 * eb + 2)),  # a whole block of frames and one on each side
             silenced(32, L, 0, 256),                                  # the first frame
             silenced(33, L, 128 * (nf - 1), L),                       # the last frame
             silenced(34, L, 128 * 5, 128 * 7)]                        # one frame alone
    _, info, dets = check("compaction", cases, gpu)
    gone = [list(np.nonzero(~det["keep"])[0]) for det in dets]
    assert gone == [list(range(eb - 2, eb + 2)), list(range(3 * eb - 1, 4 * eb + 1)), [0], [nf - 1], [5]]
    assert [int(k) for k in info[:, 0]] == [nf - len(g) for g in gone]


def test_all_zero_row(gpu):
    from snrse import ops
    z = torch.zeros(2, 8000, device=gpu)
    z[1] = torch.from_numpy(pair(40, 8000)[0]).to(gpu)
    d, info = ops.estoi(z, z.clone(), fs=er.FS, return_info=True)
    nf = er.n_frames(8000)
    assert float(d[0]) == 0.0 and tuple(info[0].tolist()) == (nf, nf - 30)
    assert abs(float(d[1]) - 1.0) < 1e-6  # a signal against itself


def test_ragged_batch_bits(gpu):
    Ls = (200, 5000, 12345, 8001, 20000)
    pairs = [pair(50 + k, L) for k, L in enumerate(Ls)]
    d, info, _ = check("ragged", pairs, gpu)
    d2, info2 = run(pairs, gpu)
    assert d.tobytes() == d2.tobytes() and (info == info2).all()
    for b in range(len(pairs)):
        ds, infos = run([pairs[b]], gpu)
        assert ds.tobytes() == d[b:b + 1].tobytes() and (infos[0] == info[b]).all(), b
    perm = [3, 0, 4, 2, 1]
    dp, infop = run([pairs[i] for i in perm], gpu)
    assert dp.tobytes() == d[perm].tobytes() and (infop == info[perm]).all()


def test_long_row(gpu):
    _, info, dets = check("long", [pair(60, 300000)], gpu)
    assert dets[0]["nf"] == 2342 and int(info[0, 0]) - 1 == 2341  # 2342 frames, all kept: 2341 after re-framing


def test_resampled_from_16k(gpu):
    Ls = (9600, 30001, 64000)
    check("fs16000", [pair(70 + k, L, 16000) for k, L in enumerate(Ls)], gpu, fs=16000)


def test_argument_errors(gpu):
    from snrse import ops
    x = torch.zeros(2, 4000, device=gpu)
    with pytest.raises(TypeError):
        ops.estoi(x, x[:, :100])
    with pytest.raises(TypeError):
        ops.estoi(x.double(), x.double())
    with pytest.raises(ValueError):
        ops.estoi(x, x, lengths=[4000, 4001])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.estoi(x.cpu(), x.cpu())
