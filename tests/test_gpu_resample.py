"""The polyphase resampler on the GPU (snrse_resample_poly through ops.resample_poly) against the fp64 closed form
of tests/resample_ref.py, which tests/test_resample_host.py holds to scipy on the CPU.

Bound, per output sample and set before any kernel ran: |y[m] - ref[m]| <= (K + 3) 2^-24 sum_n |x[n]| |h[...]|,
K = ceil((2 half + 1) / up) -- one rounding for the fp32 tap, one per product, at most K - 1 additions in any
order, one spare (resample_ref.bound).  The worst measured share of it per ratio goes to
profiles/resample_errors.json.

Lengths: 0, 1, 2, down - 1, down, down + 1, 2205 and the lengths whose output counts are P - 1, P, P + 1 and
2 P + 1 (P = the kernel's outputs per block, snrse_resample_poly_block) -- where up > down skips a count, the first
count above it.  Signals: formula normals x 0.3, an impulse at sample 0, an impulse at sample L - 1, a constant 1:
the four rows of one launch.  The buffer is NaN from each row's length on: nothing there may reach a result."""
import json
import os

import numpy as np
import pytest
import torch

import resample_ref as rr
from conftest import ROOT, fnormal

pytestmark = pytest.mark.gpu

ERRORS = os.path.join(ROOT, "profiles", "resample_errors.json")


def block():
    from snrse import _lib
    return int(_lib.load().snrse_resample_poly_block())


def lengths_for(up, down, P):
    ls = {0, 1, 2, down - 1, down, down + 1, 2205}
    for t in (P - 1, P, P + 1, 2 * P + 1):
        L = t * down // up  # the longest input with at most t outputs: exactly t where down >= up
        ls.add(L if rr.n_out(L, up, down) == t else L + 1)
    return sorted(v for v in ls if v >= 0)


def signals(L, tag):
    imp0, imp1 = np.zeros(L, np.float32), np.zeros(L, np.float32)
    if L:
        imp0[0] = imp1[L - 1] = 1.0
    return [(fnormal(f"t.resample.{tag}.{L}", (L,)) * 0.3).astype(np.float32), imp0, imp1, np.ones(L, np.float32)]


def ragged_nan(rows, gpu, stride=None):
    """[B, stride] device buffer of the rows, NaN at and past each row's length (at least one column)."""
    stride = stride or max(1, max(len(r) for r in rows))
    buf = torch.full((len(rows), stride), float("nan"), dtype=torch.float32)
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
    except OSError:  # a read-only tree: the figures are printed above, the assertions do not depend on the file
        pass


@pytest.mark.parametrize("sr_in,sr_out", rr.RATIOS)
def test_every_sample_within_the_bound(gpu, sr_in, sr_out):
    from snrse import audio, ops
    up, down = audio.rational(sr_in, sr_out)
    P = block()
    worst, where = 0.0, None
    for L in lengths_for(up, down, P):
        rows = signals(L, f"{sr_in}.{sr_out}")
        y, ol = ops.resample_poly(ragged_nan(rows, gpu), up, down, lengths=[L] * 4)
        n = rr.n_out(L, up, down)
        assert n == audio.resampled_length(L, sr_in, sr_out)
        assert y.shape == (4, n) and y.dtype == torch.float32 and ol.cpu().tolist() == [n] * 4
        y = y.cpu().numpy()
        for k, x in enumerate(rows):
            if up == down:
                assert y[k].tobytes() == x.tobytes(), (L, k)  # a copy, bit for bit
                continue
            ref, bnd = rr.resample_poly(x, up, down), rr.bound(x, up, down)
            err = np.abs(y[k].astype(np.float64) - ref)
            assert np.isfinite(y[k]).all() and (err <= bnd).all(), (sr_in, sr_out, L, k, float((err - bnd).max()))
            share = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
            if share > worst:
                worst, where = share, {"length": L, "signal": k}
    print(f"resample {sr_in} -> {sr_out} ({up}/{down}): worst share of the bound {worst:.3f} at {where}")
    record(f"{sr_in}->{sr_out}", {"up": up, "down": down, "outputs_per_block": P, "worst_share_of_bound": worst,
                                  "at": where})


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (44100, 16000), (16000, 44100), (16000, 16000)])
def test_ragged_rows_equal_their_solo_launches(gpu, sr_in, sr_out):
    """Rows of lengths {0, 1, 7, 2205, 4099} in one NaN-padded buffer: finite, each row the bits of its solo
    launch, zero from n_out_b to the stride; the rows permuted give the same rows; a second launch the same bits."""
    from snrse import audio, ops
    up, down = audio.rational(sr_in, sr_out)
    lens = (0, 1, 7, 2205, 4099)
    rows = [(fnormal(f"t.resample.rag.{L}", (L,)) * 0.3).astype(np.float32) for L in lens]
    buf = ragged_nan(rows, gpu)
    assert buf.shape == (5, 4099) and torch.isnan(buf[0]).all() and torch.isnan(buf[3, 2205:]).all()
    y, ol = ops.resample_poly(buf, up, down, lengths=lens)
    nout = [rr.n_out(L, up, down) for L in lens]
    assert ol.cpu().tolist() == nout and y.shape == (5, max(nout))
    assert torch.isfinite(y).all()
    y2, _ = ops.resample_poly(buf, up, down, lengths=lens)
    assert torch.equal(y, y2)
    for b, L in enumerate(lens):
        assert (y[b, nout[b]:] == 0).all() and y[b, nout[b]:].numel() == max(nout) - nout[b]
        solo, _ = ops.resample_poly(ragged_nan([rows[b]], gpu), up, down, lengths=[L])
        assert solo.shape == (1, nout[b]) and torch.equal(y[b, :nout[b]], solo[0]), (sr_in, sr_out, L)
    perm = (3, 0, 4, 2, 1)
    yp, olp = ops.resample_poly(ragged_nan([rows[i] for i in perm], gpu), up, down, lengths=[lens[i] for i in perm])
    assert olp.cpu().tolist() == [nout[i] for i in perm]
    for r, i in enumerate(perm):
        assert torch.equal(yp[r], y[i]), (perm, r)
    # whole rows (lengths=None), another filter through taps=, an unreduced ratio: the same kernel
    full = torch.from_numpy(np.stack([rows[4], rows[4][::-1].copy()])).to(gpu)
    yf, olf = ops.resample_poly(full, sr_out, sr_in)
    assert olf.cpu().tolist() == [nout[4]] * 2 and torch.equal(yf[0], y[4])
    if up != down:
        w = np.hanning(2 * 4 * max(up, down) + 1)
        w = w / w.sum()
        yt, _ = ops.resample_poly(full, up, down, taps=w)
        yt = yt.cpu().numpy()
        for k in range(2):
            x = full[k].cpu().numpy()
            assert (np.abs(yt[k] - rr.resample_poly(x, up, down, w)) <= rr.bound(x, up, down, w)).all()


def test_empty_batch_and_refusals(gpu):
    from snrse import ops
    y, ol = ops.resample_poly(torch.full((3, 4), float("nan"), device=gpu), 1, 3, lengths=[0, 0, 0])
    assert y.shape == (3, 0) and ol.cpu().tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        ops.resample_poly(torch.zeros(2, 4, device=gpu), 1, 3, lengths=[5, 1])  # longer than the row stride
    with pytest.raises(ValueError):
        ops.resample_poly(torch.zeros(2, 4, device=gpu), 1, 3, lengths=[1])
    with pytest.raises(ValueError):
        ops.resample_poly(torch.zeros(2, 4, device=gpu), 0, 3)
    with pytest.raises(RuntimeError, match="snrse_resample_poly"):
        ops.resample_poly(torch.zeros(1, 4096, device=gpu), 1, 100)  # a block's input span would not fit LDS
