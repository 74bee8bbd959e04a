"""Host-only checks of data-parallel training (snrse/fit.py, snrse/dist.py): the shard schedule, the optimizer
stops it implies, per-batch seeding, the reducer's flat layout, the argument checks of snrse_grad_pack and the
parser.  No device is used."""
import numpy as np
import pytest
import torch

from conftest import has_gpu


# ----------------------------------------------------------------------------- rank_batches
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_rank_batches_equal_disjoint_and_in_global_order(world):
    from snrse.fit import rank_batches
    n = 11
    batches = [[2 * b, 2 * b + 1] for b in range(n)]
    shards = [rank_batches(batches, r, world) for r in range(world)]
    used = n // world * world
    assert all(len(s) == used // world for s in shards)
    flat = [tuple(b) for s in shards for b in s]
    assert len(set(flat)) == len(flat) == used  # disjoint
    assert sorted(flat) == sorted(tuple(b) for b in batches[:used])  # the union is the first n // W * W batches
    for r, s in enumerate(shards):
        for b, got in enumerate(s):
            assert got == batches[b * world + r]  # local batch b of rank r is global batch b W + r
    if world == 1:
        assert shards[0] == batches


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n", [6, 11, 12, 13, 17])
def test_local_stops_are_the_global_stops_of_k_times_world(n, k, world):
    """world = W with accumulation k steps where world = 1 with accumulation k W steps over the used batches;
    n = 11, 13, 17 leave a partial last group for some (k, W)."""
    from snrse.fit import accumulation_steps, rank_batches
    batches = list(range(n))
    local = rank_batches(batches, 0, world)
    n_used = len(local) * world
    stops = accumulation_steps(len(local), k)
    glob = accumulation_steps(n_used, k * world)
    assert all(g % world == 0 for g in glob)
    assert stops == [g // world for g in glob]
    # and the global batches before each stop are the same sets
    for r in range(world):
        assert rank_batches(batches, r, world) == [b * world + r for b in range(len(local))]


# ----------------------------------------------------------------------------- seed_batch
def _draws():
    return np.random.uniform(size=4), torch.rand(4)


def test_seed_batch_depends_on_seed_epoch_and_index_only():
    from snrse.fit import seed_batch
    seed_batch(7, 1, 5)
    a = _draws()
    np.random.uniform(size=9)  # whatever was drawn in between
    torch.rand(3)
    seed_batch(7, 1, 5)
    b = _draws()
    assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for other in ((7, 1, 6), (7, 2, 5), (8, 1, 5)):
        seed_batch(*other)
        c = _draws()
        assert not np.array_equal(a[0], c[0]) and not torch.equal(a[1], c[1]), other


def test_validation_seed_indices_are_apart_from_training_indices():
    """Training batch j of a rank run has index b W + r < batches per epoch; validation batch j has
    VAL_INDEX0 + j and evaluate_model EVAL_INDEX: disjoint for any epoch of fewer than 2^32 batches, and the
    streams they seed differ."""
    from snrse import fit
    n_train, n_val = 4, 2  # the batch counts of the GPU tests
    train = set(range(n_train))
    val = {fit.VAL_INDEX0 + j for j in range(n_val)}
    assert not train & val and fit.EVAL_INDEX not in train | val
    assert fit.VAL_INDEX0 >= 2 ** 32 and fit.EVAL_INDEX >= fit.VAL_INDEX0 + 2 ** 32
    seen = []
    for j in sorted(train | val | {fit.EVAL_INDEX}):
        fit.seed_batch(7, 0, j)
        seen.append(tuple(np.random.uniform(size=2)))
    assert len(set(seen)) == len(seen)


# ----------------------------------------------------------------------------- reducer layout
def test_flat_layout_offsets():
    from snrse.dist import flat_layout
    sizes = [1, 2047, 2048, 2049, 5000, 33]
    offs, total = flat_layout(sizes)
    assert len(offs) == len(sizes) and offs[0] == 0
    assert all(o % 4 == 0 for o in offs)
    for (o, n), o_next in zip(zip(offs, sizes), offs[1:]):
        assert o + n <= o_next and o_next == o + (n + 3) // 4 * 4  # in order, no overlap, padded to 4
    assert total == offs[-1] + (sizes[-1] + 3) // 4 * 4 + 1  # + the loss slot
    assert flat_layout([]) == ([], 1)


def test_grad_reducer_fixes_the_layout_on_the_host():
    """The layout part of GradReducer without a device: requires_grad parameters only, in the given order."""
    from snrse.dist import GradReducer
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (1, 2047, 2048)]
    frozen = torch.nn.Parameter(torch.zeros(7), requires_grad=False)
    r = GradReducer([("a", ps[0]), ("frozen", frozen), ("b", ps[1]), ("c", ps[2])], 2, "cpu")
    assert r.names == ["a", "b", "c"] and r.offsets == [0, 4, 2052]
    assert r.flat.numel() == 2052 + 2048 + 1 and r.loss_slot == r.flat.numel() - 1
    assert r.flat.dtype == torch.float32 and not r.flat.any()
    ps[1].grad = None
    ps[0].grad, ps[2].grad = torch.zeros(1), torch.zeros(2048)
    with pytest.raises(RuntimeError, match="parameter b has no gradient"):
        r.reduce(optimizer=None)


# ----------------------------------------------------------------------------- snrse_grad_pack arguments
EINVAL = 1  # hipErrorInvalidValue
P = 0x10000  # a placeholder non-NULL address; never dereferenced on the host, never launched with


@pytest.mark.skipif(has_gpu(), reason="placeholder device addresses: only without a HIP device")
def test_grad_pack_rejects_before_any_hip_call():
    from snrse import _lib, build
    L = _lib.load(build.build_library())

    def pack(table=P, tix=P, start=P, nchunks=4, flat_off=P, scale=0.5, flat=P):
        return L.snrse_grad_pack(table, tix, start, nchunks, flat_off, scale, flat, None)

    for bad in (dict(nchunks=-1), dict(table=None), dict(tix=None), dict(start=None), dict(flat_off=None),
                dict(flat=None), dict(scale=0.0), dict(scale=-0.5), dict(scale=float("inf")),
                dict(scale=float("nan"))):
        assert pack(**bad) == EINVAL, bad
    assert pack(nchunks=0) == 0
    assert pack(nchunks=0, table=None, tix=None, start=None, flat_off=None, flat=None) == 0


# ----------------------------------------------------------------------------- parser
def test_parser_takes_gpus_and_batch_seeding():
    from snrse import fit
    argv = ["--estimator", "--base_dir", "d", "--gpus", "4", "--batch_seeding"]
    parser, temp = fit.build_parser(argv)
    assert temp.gpus == 4
    a, _ = parser.parse_known_args(argv)
    assert a.gpus == 4 and a.batch_seeding is True
    parser, temp = fit.build_parser(["--estimator", "--base_dir", "d"])
    a, _ = parser.parse_known_args(["--estimator", "--base_dir", "d"])
    assert a.gpus == 1 and a.batch_seeding is False and temp.gpus == 1


def test_spawn_ranks_timeout_terminates_and_returns_nonzero():
    """timeout_s: ranks that are still running when the time is up are terminated and the result is non-zero.
    A limit of 0 is up at the first poll, so nothing here waits (the workers would block for an hour)."""
    import time

    from snrse import dist as sd
    t0 = time.monotonic()
    rc = sd.spawn_ranks(2, _block, (), poll_s=0.05, timeout_s=0.0)
    assert rc != 0 and time.monotonic() - t0 < 60


def _block():
    import threading
    threading.Event().wait(3600)
