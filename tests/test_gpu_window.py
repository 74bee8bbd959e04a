"""snrse_window_gather / snrse_window_merge (csrc/window.hip) against numpy slicing and the fp64 reference
tests/window_ref.py (GPU).  Three recordings share every launch: one of a single window (L <= W), one of two
windows one sample apart (L = W + 1), and one of K >= 4 windows whose length puts window starts and the end off
every 256-sample block edge.

Inside a fade the kernel's fma(t, a, (1 - t) b) has four fp32 roundings (the table, 1 - t, the product, the fma), each
at most 2^-24 relative to a term no larger than |a| + |b|: the bound is 4 * 2^-24 (|a| + |b|).  The worst share of
it that a run sees is recorded in profiles/window_errors.json."""
import json
import os

import numpy as np
import pytest
import torch

import window_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1024, 256), (8064, 1536)]


def recordings(W, V):
    """Lengths (one window; K = 2 with gap 1; K >= 4, nothing on a block edge) and the signals."""
    H = W - V
    lens = [W - 37, W + 1, 3 * H + V + 301]
    assert len(window_ref.starts(lens[2], W, V)) >= 4
    assert all(s % 256 for s in window_ref.starts(lens[2], W, V)[1:]) and lens[2] % 256 and (lens[2] - W) % 256
    rng = np.random.default_rng(W + V)
    return lens, [rng.standard_normal(L).astype(np.float32) for L in lens]


_CACHE = {}


def case(W, V, dev):
    """One gather + one merge of the three recordings (computed once per shape and left unchanged)."""
    if (W, V) in _CACHE:
        return _CACHE[(W, V)]
    from snrse import ops
    lens, xs = recordings(W, V)
    stride = max(lens) + 19
    src = np.full((3, stride), np.nan, np.float32)  # NaN at and past every recording's length
    table, first, starts = [], [0], []
    for r, (L, x) in enumerate(zip(lens, xs)):
        src[r, :L] = x
        st = window_ref.starts(L, W, V)
        table += [(r, s, min(L, W)) for s in st]
        starts += st
        first.append(len(starts))
    wins = ops.window_gather(torch.from_numpy(src).to(dev), lens, np.asarray(table, np.int32), W)
    c = dict(lens=lens, xs=xs, src=src, table=table, first=first, starts=starts, wins=wins)
    _CACHE[(W, V)] = c
    return c


def window_results(c, W, seed=3):
    """Stand-ins for the enhancers' results: independent noise per window (so neighbours disagree in the fades)."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((len(c["starts"]), W)).astype(np.float32)


def poison_unread(res, c, W, V):
    """NaN into every region of the window results that the rule says is not read: a window past the next one's
    fade end, and what lies past a short window's length."""
    res = res.copy()
    for r in range(3):
        a, b = c["first"][r], c["first"][r + 1]
        for j in range(a, b - 1):
            res[j, c["starts"][j + 1] + V - c["starts"][j]:] = np.nan
        res[b - 1, c["lens"][r] - c["starts"][b - 1]:] = np.nan
    return res


def record(key, value):
    path = os.path.join(ROOT, "profiles", "window_errors.json")
    try:
        with open(path) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    data[key] = value
    try:
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


@pytest.mark.parametrize("W,V", SHAPES)
def test_gather_is_numpy_slicing(gpu, W, V):
    c = case(W, V, gpu)
    got = c["wins"].cpu().numpy()
    assert got.shape == (len(c["table"]), W) and np.isfinite(got).all()  # the NaN past a length is never seen
    for j, (r, s, ln) in enumerate(c["table"]):
        np.testing.assert_array_equal(got[j, :ln], c["xs"][r][s:s + ln])
        assert not got[j, ln:].any()
    ref = np.concatenate([window_ref.gather(x, W, V)[0] for x in c["xs"]])
    np.testing.assert_array_equal(got, ref.astype(np.float32))


@pytest.mark.parametrize("W,V", SHAPES)
def test_gather_clamps_a_bad_table(gpu, W, V):
    """Entries that point past a recording or at no recording give zeros (no read out of bounds)."""
    from snrse import ops
    c = case(W, V, gpu)
    L0 = c["lens"][0]
    table = np.asarray([(0, L0 - 5, W), (7, 0, W), (-1, 0, W), (1, -3, W)], np.int32)
    got = ops.window_gather(torch.from_numpy(c["src"]).to(gpu), c["lens"], table, W).cpu().numpy()
    np.testing.assert_array_equal(got[0, :5], c["xs"][0][L0 - 5:])
    assert not got[0, 5:].any() and not got[1:].any()


@pytest.mark.parametrize("W,V", SHAPES)
def test_merge_against_fp64(gpu, W, V):
    from snrse import ops
    c = case(W, V, gpu)
    res = window_results(c, W)
    silent = np.zeros(len(c["starts"]), bool)
    silent[c["first"][2] + 1] = True  # the long recording's second window: flagged, and full of NaN
    dirty = poison_unread(res, c, W, V)
    dirty[silent] = np.nan
    stride_out = max(c["lens"]) + 11
    out = ops.window_merge(torch.from_numpy(dirty).to(gpu), c["starts"], c["first"], c["lens"], V,
                           silent=torch.from_numpy(silent), stride_out=stride_out).cpu().numpy()
    assert out.shape == (3, stride_out) and np.isfinite(out).all()  # no NaN from any unread region
    worst = 0.0
    for r, L in enumerate(c["lens"]):
        a, b = c["first"][r], c["first"][r + 1]
        st = c["starts"][a:b]
        ref, bound = window_ref.merge(res[a:b], st, L, V, silent=silent[a:b])
        k, infade = window_ref.dominant(L, st, V)
        n = np.arange(L)
        dom = np.where(silent[a:b][k], np.float32(0), res[a:b][k, n - np.asarray(st)[k]])
        np.testing.assert_array_equal(out[r, :L][~infade], dom[~infade])  # outside the fades: the dominant window
        assert not out[r, L:].any()                                      # the stride past L_r is zero
        err = np.abs(out[r, :L].astype(np.float64) - ref)
        if infade.any():
            assert (err[infade] <= 4 * U * bound[infade]).all(), (r, float((err[infade] / bound[infade]).max() / U))
            worst = max(worst, float((err[infade] / np.maximum(4 * U * bound[infade], 1e-300)).max()))
        assert infade.sum() == V * (b - a - 1)  # every fade is whole, the one of the window at gap 1 too
    print(f"window_merge W={W} V={V}: worst share of the 4 x 2^-24 (|a| + |b|) bound {worst:.3f}")
    assert 0 < worst <= 1
    record(f"merge_W{W}_V{V}", {"worst_share_of_bound": round(worst, 4), "bound": "4 * 2^-24 * (|a| + |b|)",
                                "lengths": c["lens"]})


@pytest.mark.parametrize("W,V", SHAPES)
def test_merge_of_gather_is_the_recording(gpu, W, V):
    from snrse import ops
    c = case(W, V, gpu)
    out = ops.window_merge(c["wins"], c["starts"], c["first"], c["lens"], V).cpu().numpy()
    assert out.shape == (3, max(c["lens"]))
    worst = 0.0
    for r, (L, x) in enumerate(zip(c["lens"], c["xs"])):
        err = np.abs(out[r, :L].astype(np.float64) - x.astype(np.float64))
        assert (err <= 2 * U * np.abs(x)).all(), (r, float((err / np.abs(x)).max() / U))
        worst = max(worst, float((err / np.maximum(np.abs(x), 1e-30)).max() / U))
        _, infade = window_ref.dominant(L, c["starts"][c["first"][r]:c["first"][r + 1]], V)
        np.testing.assert_array_equal(out[r, :L][~infade], x[~infade])
    np.testing.assert_array_equal(out[0, :c["lens"][0]], c["xs"][0])  # a one-window recording is a copy
    record(f"roundtrip_W{W}_V{V}", {"worst_error_in_units_of_2^-24_|x|": round(worst, 4), "bound": 2})


@pytest.mark.parametrize("W,V", SHAPES)
def test_merge_bits_solo_and_repeated(gpu, W, V):
    from snrse import ops
    c = case(W, V, gpu)
    res = torch.from_numpy(window_results(c, W, seed=5)).to(gpu)
    stride_out = max(c["lens"]) + 3
    one = ops.window_merge(res, c["starts"], c["first"], c["lens"], V, stride_out=stride_out)
    two = ops.window_merge(res, c["starts"], c["first"], c["lens"], V, stride_out=stride_out)
    assert torch.equal(one, two)
    for r, L in enumerate(c["lens"]):
        a, b = c["first"][r], c["first"][r + 1]
        solo = ops.window_merge(res[a:b].contiguous(), c["starts"][a:b], [0, b - a], [L], V)
        assert solo.shape == (1, L) and torch.equal(solo[0], one[r, :L]), r


def test_einval_before_any_launch(gpu):
    """NULL pointers, non-positive sizes and 4 V > W are refused by the C entry points themselves."""
    from snrse import _lib
    lib = _lib.load()
    t = torch.zeros(4096, device=gpu)
    i = torch.zeros(16, dtype=torch.int32, device=gpu)
    p, q = t.data_ptr(), i.data_ptr()
    assert lib.snrse_window_gather(None, q, 1, 1024, q, 1, 1024, p, None) != 0
    assert lib.snrse_window_gather(p, q, 1, 1024, q, 0, 1024, p, None) != 0
    assert lib.snrse_window_gather(p, q, 1, 1024, q, 1, 0, p, None) != 0
    assert lib.snrse_window_merge(p, 1, 1024, q, q, q, q, 1, p, 257, p, 1024, None) != 0  # 4 V > W
    assert lib.snrse_window_merge(p, 1, 1024, q, None, q, q, 1, p, 256, p, 1024, None) != 0
    assert lib.snrse_window_merge(p, 1, 1024, q, q, q, q, 1, p, 256, p, 0, None) != 0
    torch.cuda.synchronize()
