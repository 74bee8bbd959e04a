"""Host side of the ragged-batch evaluation (no GPU): the batch planner, the SNR estimator's sub-groups, the
row-seed bookkeeping of NoiseSource / LaneNoise / the guard snapshot, the driver's defaults, the WAV header
reader the driver plans from."""
import inspect

import numpy as np
import pytest
import torch


def _tpad(L):
    T = 1 + L // 128
    return T + (64 - T % 64) % 64


def test_plan_batches_buckets_caps_and_order():
    from snrse.batching import plan_batches
    assert (_tpad(8191), _tpad(8192)) == (64, 128)
    assert plan_batches([8191, 8192], 8) == [[0], [1]]  # one sample apart, different Tpad: never one batch
    rng = np.random.default_rng(0)
    lens = [int(v) for v in rng.integers(256, 6 * 16000, 200)]
    for bs, mf in ((1, 16384), (4, 16384), (32, 16384), (32, 1024), (7, 64)):
        plan = plan_batches(lens, bs, mf)
        assert sorted(i for b in plan for i in b) == list(range(len(lens)))  # every index exactly once
        for b in plan:
            tp = {_tpad(lens[i]) for i in b}
            assert len(tp) == 1  # one Tpad per batch
            assert len(b) <= bs and len(b) <= max(1, mf // tp.pop())  # both caps
            assert b == sorted(b)  # ascending inside a batch
        assert [b[0] for b in plan] == sorted(b[0] for b in plan)  # batches by first index
        assert plan == plan_batches(list(lens), bs, mf)  # deterministic
    # the frame cap binds before batch_size: Tpad 512 (4 s) at 1024 frames -> 2 rows
    assert [len(b) for b in plan_batches([64000] * 5, 32, 1024)] == [2, 2, 1]
    # a bucket larger than max_frames still runs, one row at a time
    assert plan_batches([64000, 64000], 32, 100) == [[0], [1]]
    # a group keeps ascending index order and is cut in order
    assert plan_batches([300, 9000, 400, 9100, 500], 2) == [[0, 2], [1, 3], [4]]


def test_plan_batches_refuses_short_clip():
    from snrse.batching import plan_batches
    assert plan_batches([256], 4) == [[0]]
    with pytest.raises(ValueError, match="utterance 2"):
        plan_batches([8000, 300, 255], 4)
    with pytest.raises(ValueError):
        plan_batches([8000], 0)


def test_snr_groups_split_a_bucket_by_16_frame_padding():
    from snrse.batching import snr_groups
    lens = [39 * 128 + 5, 49 * 128, 63 * 128 + 127, 39 * 128]  # T = 40, 50, 64, 40: all Tpad 64
    assert {_tpad(v) for v in lens} == {64}
    assert snr_groups(lens) == [(48, [0, 3]), (64, [1, 2])]  # T = 40 -> 48 frames; 50 and 64 -> 64


def test_noise_source_row_seed_bookkeeping():
    from snrse import guard, sampler
    legacy = sampler.NoiseSource(seed=5)
    assert legacy.row_seeds is None and legacy.seed == 5
    assert [legacy.next(100) for _ in range(3)] == [(None, 0), (None, 100), (None, 200)]  # counter offsets
    seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64)
    src = sampler.NoiseSource(row_seeds=seeds)
    assert src.row_seeds.dtype == torch.int64 and len(src.row_seeds) == 4
    assert [src.next(100) for _ in range(3)] == [(None, 0), (None, 1), (None, 2)]  # draw indices
    snap = guard.snapshot(src)
    assert snap is not src and snap.i == 3 and torch.equal(snap.row_seeds.cpu(), seeds)
    src.next(100)
    assert snap.i == 3  # untouched by the caller's later draws
    lanes = guard.run_noise(snap, [1, 2], 4)
    assert [(a, b) for a, b, _ in lanes] == [(1, 3)]
    lane = lanes[0][2]
    assert lane.row_seeds.cpu().tolist() == [22, 33] and lane.row_seeds.is_contiguous()
    assert lane.next(50) == (None, 3) and lane.next(50) == (None, 4)  # the parent's draw index goes on
    # a batch-keyed parent keeps its counter arithmetic
    leg_lane = sampler.LaneNoise(legacy, 1, 3, 4)
    assert leg_lane.row_seeds is None and leg_lane.next(50) == (None, 3 * 25 * 4 + 25)
    # a sequence of Python ints (62-bit seeds) is held as int64
    big = sampler.NoiseSource(row_seeds=[2 ** 62 - 1, 7])
    assert big.row_seeds.cpu().tolist() == [2 ** 62 - 1, 7]
    assert sampler.row_seed_kw(3) == {"seed": 3} and "row_seeds" in sampler.row_seed_kw(seeds)


def test_driver_defaults_to_the_per_file_loop():
    from snrse import evaluate
    sig = inspect.signature(evaluate.evaluate)
    assert sig.parameters["batch_size"].default == 1 and sig.parameters["max_frames"].default == 16384
    from sgmse.model import ScoreModel
    sig = inspect.signature(ScoreModel.enhance_batch)
    assert sig.parameters["batch_size"].default == 32 and sig.parameters["seeds"].default is None


def test_audio_info_reads_the_header(tmp_path):
    from snrse import audio
    for bits, L in ((16, 4321), (32, 777)):
        p = str(tmp_path / f"a{bits}.wav")
        audio.write_wav(p, np.zeros(L, np.float32), 16000, bits=bits)
        assert audio.info(p) == (L, 1, 16000)
        assert audio.load(p)[0].shape == (1, L)
