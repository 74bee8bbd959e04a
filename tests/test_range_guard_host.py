"""Host side of the fp16 range guard and the range probe (no GPU): run splitting, policy resolution, the noise
of a per-run recomputation, the headroom table, the score_update dtype check and the C-ABI declaration."""
import math
import os
import re

import pytest
import torch

from conftest import ROOT


def test_runs():
    from snrse import guard
    assert guard.runs([0, 1, 2, 5, 7, 8]) == [(0, 3), (5, 6), (7, 9)]
    assert guard.runs([]) == []
    assert guard.runs([3]) == [(3, 4)]


def test_resolve():
    from snrse import guard
    assert guard.resolve("auto", torch.float16) == "fallback"
    assert guard.resolve("auto", torch.bfloat16) == "off"
    assert guard.resolve("auto", torch.float32) == "off"
    assert guard.resolve(None, torch.float16) == "off"
    for p in ("off", "warn", "raise", "fallback"):
        assert guard.resolve(p, torch.bfloat16) == p
    with pytest.raises(ValueError):
        guard.resolve("sometimes", torch.float16)


def test_errors_and_warning_types():
    from snrse import guard
    e = guard.FloatRangeError([1, 4])
    assert isinstance(e, RuntimeError) and e.rows == [1, 4]
    assert issubclass(guard.RangeFallbackWarning, UserWarning)


def test_run_noise_philox_offsets():
    """The recomputation of rows [a, b) of a batch of B draws the whole-batch run's counters: draw i of a lane of
    b - a rows of `row` elements starts at i * row * B + a * row, from the caller's draw index on."""
    from snrse import guard, sampler
    B, row = 6, 256 * 64
    src = sampler.NoiseSource(seed=77)
    src.next(B * row)  # the caller has drawn once before
    snap = guard.snapshot(src)
    assert (snap.seed, snap.tape, snap.i) == (77, None, 1)
    lanes = guard.run_noise(snap, [1, 2, 4], B)
    assert [(a, b) for a, b, _ in lanes] == [(1, 3), (4, 5)]
    for a, b, lane in lanes:
        assert lane.seed == 77
        for i in (1, 2, 3):
            z, off = lane.next((b - a) * row)
            assert z is None and off == i * row * B + a * row
    assert (src.i, snap.i) == (1, 1)  # neither the caller's source nor the snapshot moved


def test_run_noise_tape_rows():
    from snrse import guard, sampler
    B = 4

    def tape(i):
        return torch.arange(B * 3, dtype=torch.float32).reshape(B, 3) + 100 * i

    (a, b, lane), = guard.run_noise(guard.snapshot(sampler.NoiseSource(tape=tape)), [2, 3], B)
    assert (a, b) == (2, 4)
    for i in range(2):
        z, off = lane.next(6)
        assert off == 0 and torch.equal(z, tape(i)[2:4])


def test_headroom_bits():
    from snrse.range_check import headroom_bits
    assert headroom_bits(65504.0, torch.float16) == 0.0
    for k in range(1, 6):
        assert headroom_bits(65504.0 / 2 ** k, torch.float16) == pytest.approx(k, abs=1e-12)
    assert headroom_bits(2 * 65504.0, torch.float16) == pytest.approx(-1.0)
    assert headroom_bits(3.0, torch.float16, nonfinite=2) == -math.inf
    assert headroom_bits(float("inf"), torch.float16) == -math.inf
    assert headroom_bits(1.0, torch.bfloat16) == pytest.approx(math.log2(torch.finfo(torch.bfloat16).max))


def test_format_report_names_first_offender():
    from snrse import range_check
    t = torch.tensor
    rep = [("3.conv", t([1.5, 2.0]), t([0, 0])), ("4.rb.conv0", t([7.0e4, 3.0]), t([0, 0])),
           ("4.rb.conv1", t([0.0, 1.0]), t([12, 0])), ("5.rb.conv0", t([1.0, 1.0]), t([0, 0]))]
    assert range_check.first_offender(rep) == "4.rb.conv0"       # a finite peak above 65504 (a bf16 probe)
    assert range_check.first_offender(rep[2:]) == "4.rb.conv1"   # non-finite elements (an fp16 probe)
    assert range_check.first_offender(rep[:1] + rep[3:]) is None
    text = range_check.format_report(rep)
    last = text.splitlines()[-1]
    assert "4.rb.conv0" in last and "4.rb.conv1" not in last and "first" in last
    assert all(name in text for name, _, _ in rep)
    assert range_check.recommend(rep) == "bf16"
    ok = range_check.format_report(rep[:1] + rep[3:])
    assert "every tensor fits" in ok and range_check.recommend(rep[:1]) == "fp16"
    merged = range_check.merge([rep[:2], rep[1:3]])
    assert [n for n, _, _ in merged] == ["3.conv", "4.rb.conv0", "4.rb.conv1"]
    assert float(merged[1][1]) == 7.0e4 and int(merged[2][2]) == 12


def test_score_update_rejects_fp16_pyramid():
    """A float16 pyramid would be read as bf16 by the library; the dtype check comes before the device check, so
    CPU tensors suffice."""
    from snrse import ops
    x = torch.zeros(1, 4, 4, dtype=torch.complex64)
    w, b, t = torch.zeros(2, 4), torch.zeros(2), torch.ones(1)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ops.score_update(torch.zeros(1, 4, 4, 4, dtype=torch.float16), w, b, t, 0, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # an accepted dtype goes on to the device check
        ops.score_update(torch.zeros(1, 4, 4, 4, dtype=torch.float32), w, b, t, 0, x)


def test_range_stats_declared_and_bound():
    from snrse import _lib
    with open(os.path.join(ROOT, "include", "snrse.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bint\s+snrse_range_stats\s*\(([^;{]*?)\)\s*;", hdr)
    assert m, "snrse_range_stats is not declared in include/snrse.h"
    assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES["snrse_range_stats"]) == 8
    assert "snrse_range_stats" in _lib.exported_symbols()


def test_range_stats_needs_device():
    from snrse import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.range_stats(torch.zeros(2, 8))
