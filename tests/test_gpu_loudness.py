"""The loudness kernels (csrc/loudness.hip) against the fp64 reference tests/loudness_ref.py.

Bounds, set before any kernel ran:
  * integrated loudness, every block loudness above -70 and every sub-block above -70: within 1e-6 LU of the
    reference.  Everything after the f32 load is fp64; rounding in a 4th-order recurrence with poles at radius
    r <= 0.9988 is amplified by about 1 / (1 - r)^2 <= 7e5, relative errors near 1e-10, 1e-9 dB: three orders of
    margin, six below the 0.1 LU a meter is allowed.
  * sub-block sums below that floor: absolute, <= 1e-12 n100 max|x|^2.
  * gate decisions: the reference shows that no block of these inputs lies within 1e-3 LU of a gate; the kept
    counts are then equal.
  * 4x peak: the bits of max |ops.resample_poly(x, 4, 1)|; against scipy inside the resampler's own bound.
  * gain and conversion: int16 equal to numpy's formula.
The worst measured figures go beside their bounds into profiles/loudness_errors.json.

Two ragged batches with NaN from every length on, rows of five rates in one launch sequence, and a third that mixes
every row of the second with rows of every rate and length of the first.  `small`: per rate
the lengths 4 n100 - 1 (no block), 4 n100, 5 n100 - 1, 5 n100, C - 1, C, C + 1, 3 C + 1 for the chunk C, and
P - 1, P, P + 1 for the P = C x block samples a workgroup stages and G + 1 for the G = C x group samples of a
scan group, each as normals at 0.1, an impulse at the first sample, one at the last, a constant 0.3 (which the
high-pass takes to nothing; fp32 state would not) and zeros.  At 8 kHz (n100 = 800 = 12.5 chunks) those lengths put
sub-block boundaries strictly inside a chunk (800) and on a chunk edge (1600); at 16 and 48 kHz every boundary is a
chunk edge.  `long`: the 997 Hz sine, the two-level signal, a row whose second half lies under -70 LUFS, rows at
11025 and 44100 Hz long enough for a boundary on a chunk edge (64 n100 and 32 n100) among those inside chunks, 3 G + 1
samples, and 2^20 + 33 samples at 48 kHz so that the per-row scan runs over many groups."""
import json
import math
import os

import numpy as np
import pytest
import torch

import loudness_ref as ref
import resample_ref as rr
from conftest import ROOT
from test_gpu_resample import ragged_nan

pytestmark = pytest.mark.gpu

ERRORS = os.path.join(ROOT, "profiles", "loudness_errors.json")
RATES = (8000, 11025, 16000, 44100, 48000)
KINDS = ("normal", "impulse_first", "impulse_last", "constant", "zeros")
LU_BOUND = 1e-6
GATE_CLEARANCE = 1e-3


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
    except OSError:  # a read-only tree: the figures are printed, the assertions do not depend on the file
        pass


def geometry():
    from snrse import ops
    return ops.kweight_geometry()


def signal(kind, L, seed):
    if kind == "normal":
        return (np.random.default_rng(seed).standard_normal(L) * 0.1).astype(np.float32)
    x = np.zeros(L, np.float32)
    if kind == "impulse_first" and L:
        x[0] = 1.0
    elif kind == "impulse_last" and L:
        x[L - 1] = 1.0
    elif kind == "constant":
        x[:] = 0.3
    return x


def small_rows():
    C, T, S = geometry()
    rows = []
    for fs in RATES:
        n = ref.n100(fs)
        for L in sorted({4 * n - 1, 4 * n, 5 * n - 1, 5 * n, C - 1, C, C + 1, 3 * C + 1, C * T - 1, C * T, C * T + 1,
                         C * S + 1}):
            for kind in KINDS:
                rows.append((f"{fs}/{L}/{kind}", fs, signal(kind, L, fs + L)))
    return rows


def long_rows():
    C, T, S = geometry()
    quiet = signal("normal", 32000, 11)
    quiet[16000:] *= 1e-4  # -100 dBFS rms: far under the absolute gate
    return [("sine997/48000", 48000, ref.sine(997.0, 48000, 5.0)),
            ("sine997/16000", 16000, ref.sine(997.0, 16000, 5.0)),
            ("two_level/48000", 48000, ref.two_level()),
            ("abs_gate/16000", 16000, quiet),
            ("edge/11025", 11025, signal("normal", 65 * ref.n100(11025) + 7, 1)),
            ("edge/44100", 44100, signal("normal", 33 * ref.n100(44100) + 5, 2)),
            ("groups3/48000", 48000, signal("normal", 3 * C * S + 1, 3)),
            ("groups3const/48000", 48000, signal("constant", 3 * C * S + 1, 0)),
            ("scan/48000", 48000, signal("normal", 2 ** 20 + 33, 4))]


class Batch:
    """One ragged batch, its reference (computed once, never changed) and its result on the device."""

    def __init__(self, rows, gpu):
        from snrse import ops
        self.names = [r[0] for r in rows]
        self.rates = [r[1] for r in rows]
        self.x = [r[2] for r in rows]
        self.lens = [len(v) for v in self.x]
        self.buf = ragged_nan(self.x, gpu)
        self.ref = [ref.integrated([v], fs) for v, fs in zip(self.x, self.rates)]
        self.ref_sums = [ref.subblock_sums(v, fs) for v, fs in zip(self.x, self.rates)]
        self.lufs, self.info = ops.loudness(self.buf, lengths=self.lens, rate=self.rates, return_info=True)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def small(gpu):
    return Batch(small_rows(), gpu)


@pytest.fixture(scope="module")
def long(gpu):
    return Batch(long_rows(), gpu)


def check_batch(bt, tag):
    lufs = bt.lufs.cpu().numpy()
    sums = bt.info["sums"].cpu().numpy()
    counts = [bt.info[k].cpu().numpy() for k in ("blocks", "kept_abs", "kept_rel")]
    margin = bt.info["margin"].cpu().numpy()
    worst = {"lufs": 0.0, "block": 0.0, "subblock": 0.0, "floor_share": 0.0, "least_gate_clearance": math.inf}
    for b, name in enumerate(bt.names):
        r, fs, x = bt.ref[b], bt.rates[b], bt.x[b]
        n = ref.n100(fs)
        nsub = len(x) // n
        assert bt.info["nsub"][b] == nsub and bt.info["n100"][b] == n
        s, sr = sums[b, :nsub], bt.ref_sums[b]
        assert np.isfinite(s).all() and (sums[b, nsub:] == 0).all(), name
        # sub-blocks: relative above the floor, absolute below it
        with np.errstate(divide="ignore", invalid="ignore"):
            lr, lg = -0.691 + 10 * np.log10(sr / n), -0.691 + 10 * np.log10(s / n)
        above = lr > -70.0
        if above.any():
            worst["subblock"] = max(worst["subblock"], float(np.abs(lg[above] - lr[above]).max()))
            assert np.abs(lg[above] - lr[above]).max() <= LU_BOUND, name
        floor = 1e-12 * n * float(np.abs(x).max(initial=0.0)) ** 2
        if (~above).any():
            d = float(np.abs(s[~above] - sr[~above]).max())
            assert d <= floor, (name, d, floor)
            if floor > 0:
                worst["floor_share"] = max(worst["floor_share"], d / floor)
        # blocks from the device's sums, as the gate kernel forms them
        if nsub >= 4:
            e = (((s[0:nsub - 3] + s[1:nsub - 2]) + s[2:nsub - 1]) + s[3:nsub]) / (4.0 * n)
            with np.errstate(divide="ignore"):
                l = -0.691 + 10 * np.log10(e)
            up = r["block_l"] > -70.0
            if up.any():
                worst["block"] = max(worst["block"], float(np.abs(l[up] - r["block_l"][up]).max()))
                assert np.abs(l[up] - r["block_l"][up]).max() <= LU_BOUND, name
        # the reference itself says that no decision of this input is a close one
        assert r["margin"] > GATE_CLEARANCE, (name, r["margin"])
        worst["least_gate_clearance"] = min(worst["least_gate_clearance"], r["margin"])
        assert (counts[0][b], counts[1][b], counts[2][b]) == (r["blocks"], r["kept_abs"], r["kept_rel"]), name
        if r["margin"] == math.inf:
            assert margin[b] == math.inf, name
        else:
            assert abs(margin[b] - r["margin"]) <= 1e-6, (name, margin[b], r["margin"])
        if r["lufs"] == -math.inf:
            assert lufs[b] == -math.inf, (name, lufs[b])
        else:
            worst["lufs"] = max(worst["lufs"], abs(lufs[b] - r["lufs"]))
            assert abs(lufs[b] - r["lufs"]) <= LU_BOUND, (name, lufs[b], r["lufs"])
    print(f"loudness {tag}: worst {worst}")
    record(tag, {"rows": len(bt.names), "bound_lu": LU_BOUND, "worst_lufs_error_lu": worst["lufs"],
                 "worst_block_error_lu": worst["block"], "worst_subblock_error_lu": worst["subblock"],
                 "worst_share_of_floor_bound": worst["floor_share"], "gate_clearance_required_lu": GATE_CLEARANCE,
                 "least_gate_clearance_lu": worst["least_gate_clearance"]})


def test_small_batch_within_the_bounds(small):
    check_batch(small, "small")


def test_long_batch_within_the_bounds(long):
    check_batch(long, "long")
    got = dict(zip(long.names, long.lufs.cpu().numpy()))
    assert abs(got["sine997/48000"] - (-3.0103)) <= 1e-3
    assert abs(got["sine997/16000"] - (-2.9700)) <= 1e-3
    assert abs(got["two_level/48000"] - (-23.2328)) <= 1e-3
    i = long.names.index("two_level/48000")
    assert int(long.info["kept_rel"][i]) == 30
    j = long.names.index("abs_gate/16000")
    assert int(long.info["kept_abs"][j]) < int(long.info["blocks"][j])  # the absolute gate dropped blocks


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("which", ("small", "long"))
def test_permuted_and_solo_rows_give_the_same_bits(which, request, gpu):
    from snrse import ops
    bt = request.getfixturevalue(which)
    B = len(bt.names)
    perm = np.random.default_rng(9).permutation(B)
    buf = ragged_nan([bt.x[p] for p in perm], gpu, stride=bt.buf.shape[1] + 3)  # another stride: other alignments
    lufs, info = ops.loudness(buf, lengths=[bt.lens[p] for p in perm], rate=[bt.rates[p] for p in perm],
                              return_info=True)
    inv = torch.from_numpy(np.argsort(perm)).to(gpu)
    assert torch.equal(bits(lufs[inv]), bits(bt.lufs))
    assert torch.equal(bits(info["sums"][inv]), bits(bt.info["sums"]))
    for b in range(B):  # every row alone: stride == L, the row's last staging group ends where the buffer ends
        L = bt.lens[b]
        solo = ragged_nan([bt.x[b]], gpu)
        l1, i1 = ops.loudness(solo, lengths=[L], rate=bt.rates[b], return_info=True)
        assert torch.equal(bits(l1), bits(bt.lufs[b:b + 1])), bt.names[b]
        k = i1["sums"].shape[1]
        assert torch.equal(bits(i1["sums"][0]), bits(bt.info["sums"][b, :k])), bt.names[b]


def test_long_and_short_rows_of_every_rate_share_one_permuted_batch(small, long, gpu):
    """Every row of `long` (the 2^20-sample row, the sine, the two-level signal ..) and the rows of `small` -- every
    rate and length, the kinds in turn -- as ONE ragged batch in a random order: the bits each row has in its own
    batch.  (All 309 rows at the long stride would be a 1.3 GB buffer; the 69 rows here are 290 MB.)"""
    from snrse import ops
    picks = [(long, b) for b in range(len(long.names))]
    picks += [(small, b) for b in range(len(small.names)) if b % len(KINDS) == (b // len(KINDS)) % len(KINDS)]
    assert len({(small.rates[b], small.lens[b]) for bt, b in picks if bt is small}) == len(small.names) // len(KINDS)
    order = np.random.default_rng(10).permutation(len(picks))
    picks = [picks[i] for i in order]
    buf = ragged_nan([bt.x[b] for bt, b in picks], gpu, stride=long.buf.shape[1] + 1)
    lufs, info = ops.loudness(buf, lengths=[bt.lens[b] for bt, b in picks], rate=[bt.rates[b] for bt, b in picks],
                              return_info=True)
    for r, (bt, b) in enumerate(picks):
        assert torch.equal(bits(lufs[r:r + 1]), bits(bt.lufs[b:b + 1])), bt.names[b]
        k = min(info["sums"].shape[1], bt.info["sums"].shape[1])
        assert torch.equal(bits(info["sums"][r, :k]), bits(bt.info["sums"][b, :k])), bt.names[b]
        assert not info["sums"][r, k:].any() and not bt.info["sums"][b, k:].any(), bt.names[b]


def test_a_stereo_and_a_mono_file_in_one_call(gpu):
    from snrse import ops
    n = ref.n100(48000)
    a, b = signal("normal", 9 * n + 17, 21), ref.sine(440.0, 48000, 1.0, 0.25)[:9 * n + 17]
    m = signal("normal", 7 * ref.n100(16000) + 3, 22) * 3.0
    buf = ragged_nan([a, b, m], gpu)
    lufs, info = ops.loudness(buf, lengths=[len(a), len(b), len(m)], rate=[48000, 48000, 16000], groups=[0, 0, 1],
                              return_info=True)
    want = [ref.integrated([a, b], 48000), ref.integrated([m], 16000)]
    got = lufs.cpu().numpy()
    assert got.shape == (2,)
    for g, w in zip(got, want):
        assert w["margin"] > GATE_CLEARANCE and abs(g - w["lufs"]) <= LU_BOUND, (g, w["lufs"])
    assert info["blocks"].tolist() == [w["blocks"] for w in want]
    assert info["kept_rel"].tolist() == [w["kept_rel"] for w in want]
    # the channel sum is not the louder channel alone
    assert got[0] > ref.integrated([a], 48000)["lufs"] + 0.1
    # a file of channels with different lengths has the fewest sub-blocks of them
    lufs2 = ops.loudness(buf, lengths=[len(a), 5 * n, len(m)], rate=[48000, 48000, 16000], groups=[0, 0, 1])
    w2 = ref.integrated([a, b[:5 * n]], 48000)
    assert abs(float(lufs2[0]) - w2["lufs"]) <= LU_BOUND and w2["blocks"] == 2


def test_peak_oversampled(small, gpu):
    from snrse import ops
    pk = ops.peak_oversampled(small.buf, lengths=small.lens)
    y, ylen = ops.resample_poly(small.buf, 4, 1, lengths=small.lens)
    assert ylen.tolist() == [4 * L for L in small.lens]
    want = torch.stack([y[b, :4 * L].abs().max() for b, L in enumerate(small.lens)])
    assert torch.equal(pk.view(torch.int32), want.view(torch.int32))
    got = pk.cpu().numpy()
    worst = 0.0
    for b in range(len(small.names)):
        x = small.x[b]
        bound = float(rr.bound(x, 4, 1).max(initial=0.0))
        err = abs(float(got[b]) - ref.peak4(x))
        assert err <= bound, (small.names[b], err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    record("peak4", {"worst_share_of_resampler_bound": worst})
    # the sine at fs / 4 with a 45 degree phase: sample peak 0.7071, 1.0017 between the samples
    s = ref.sine(12000.0, 48000, 0.05, 1.0, math.pi / 4)
    inner = ops.peak_oversampled(ragged_nan([s], gpu), lengths=[len(s)])
    assert abs(float(np.abs(s).max()) - 0.70711) < 1e-4 and 1.0016 < float(inner) < 1.0135
    # an empty row reads 0; a NaN inside a row is skipped as absmax skips it
    j = next(i for i, nm in enumerate(small.names) if nm.endswith("normal") and small.lens[i] > 200)
    z = small.buf[[0, j]].clone()
    z[1, 100] = float("nan")
    L1 = small.lens[j]
    p2 = ops.peak_oversampled(z, lengths=[0, L1])
    y2, _ = ops.resample_poly(z, 4, 1, lengths=[0, L1])
    assert float(p2[0]) == 0.0 and float(p2[1]) > 0.0
    assert torch.equal(p2[1:].view(torch.int32), ops.absmax(y2[1:, :4 * L1].contiguous()).view(torch.int32))


@pytest.mark.parametrize("stride", (4100, 4099))  # 16-byte aligned rows (vector path), misaligned rows (scalar path)
def test_gain_to_pcm16(gpu, stride):
    from snrse import ops
    rng = np.random.default_rng(stride)
    special = np.array([1.0, -1.0, 1.5, -1.5, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                        32766.5 / 32768, 0.0, 0.99996948], np.float32)
    lens = [stride, stride - 1, 4097, 13, 0, 1]
    rows = [np.concatenate([special, rng.standard_normal(max(L - len(special), 0)).astype(np.float32) * 0.5])[:L]
            for L in lens]
    gains = np.array([1.0, 0.7079457843841379, 2.5, 1.0, 3.0, 1e-3])
    buf = ragged_nan(rows, gpu, stride=stride)
    for dt in (torch.float64, torch.float32):
        g = torch.from_numpy(gains).to(dt).to(gpu)
        q, f = ops.gain_to_pcm16(buf, g, lengths=lens, floats=True)
        q_only = ops.gain_to_pcm16(buf, g, lengths=lens)
        assert q.dtype == torch.int16 and f.dtype == torch.float32 and torch.equal(q, q_only)
        qh, fh = q.cpu().numpy(), f.cpu().numpy()
        for b, (x, L) in enumerate(zip(rows, lens)):
            gb = np.float32(gains[b])
            assert np.array_equal(qh[b, :L], ref.gain_pcm16(x, gb)), (b, dt)
            assert np.array_equal(fh[b, :L], (gb * x).astype(np.float32)), (b, dt)
            assert not qh[b, L:].any() and not fh[b, L:].any(), (b, dt)
    assert list(qh[0, :11]) == [32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, 32766, 0]


def test_refusals(gpu):
    from snrse import ops
    x = torch.zeros(2, 8000)
    for fn in (lambda t: ops.loudness(t), lambda t: ops.peak_oversampled(t),
               lambda t: ops.gain_to_pcm16(t, torch.ones(2, dtype=torch.float64, device=t.device))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
        with pytest.raises(TypeError):
            fn(x.to(gpu).double())
    xg = x.to(gpu)
    with pytest.raises(TypeError):
        ops.gain_to_pcm16(xg, torch.ones(2, dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError):
        ops.loudness(xg, rate=400)  # a sub-block shorter than a chunk
    with pytest.raises(ValueError):
        ops.loudness(xg, groups=[0, 2])
    with pytest.raises(ValueError):
        ops.loudness(xg, rate=[16000, 8000], groups=[0, 0])
    with pytest.raises(ValueError):
        ops.loudness(xg, lengths=[8001, 5])


def test_measure_uploads_once_and_reads_back_once(gpu, monkeypatch):
    """measure(): the signals go up in one transfer (the few-integer tables of the ops apart) and everything comes
    back in one; counted at torch.Tensor.to / .cpu / .item / .tolist."""
    from snrse import loudness
    a = np.stack([ref.sine(997.0, 48000, 1.0, 0.5), ref.sine(997.0, 48000, 1.0, 0.25)])
    b = ref.sine(997.0, 16000, 0.3)  # under 400 ms
    loudness.measure([(a, 48000), (torch.from_numpy(b), 16000)])  # builds the cached taps and parameter tables
    n = {"up": 0, "down": 0}
    to, down = torch.Tensor.to, {k: getattr(torch.Tensor, k) for k in ("cpu", "item", "tolist")}

    def counting_to(self, *args, **kw):
        r = to(self, *args, **kw)
        if r.is_cuda and not self.is_cuda and self.numel() >= 1024:  # a signal, not a table of a few integers
            n["up"] += 1
        elif self.is_cuda and not r.is_cuda:
            n["down"] += 1
        return r

    def counting(name):
        def f(self, *args, **kw):
            n["down"] += int(self.is_cuda)
            return down[name](self, *args, **kw)
        return f

    monkeypatch.setattr(torch.Tensor, "to", counting_to)
    for k in down:
        monkeypatch.setattr(torch.Tensor, k, counting(k))
    out = loudness.measure([(a, 48000), (torch.from_numpy(b), 16000)])
    monkeypatch.undo()
    assert n == {"up": 1, "down": 1}, n
    want = ref.integrated([a[0], a[1]], 48000)["lufs"]
    assert abs(out[0][0] - want) <= LU_BOUND and out[1][0] == -math.inf
    assert abs(out[0][1] - 20 * math.log10(max(ref.peak4(a[0]), ref.peak4(a[1])))) < 1e-4
    assert abs(out[1][1] - 20 * math.log10(ref.peak4(b))) < 1e-4
