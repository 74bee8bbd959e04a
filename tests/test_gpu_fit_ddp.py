"""GPU checks of data-parallel training: the multi-tensor gradient pack (snrse_grad_pack), the gradient
exchange (snrse.dist.GradReducer) and the sharded fit() loop.

The test box has one GPU, so checks that need more than one rank start fresh processes with
snrse.dist.spawn_ranks and the ranks share GPU 0 over gloo (the oversubscribed mode of init_from_env).  Every
spawn joins with a time limit (JOIN_S; a first `import torch` can take a minute), terminates its ranks when the
time is up and fails on a non-zero exit code.  The ranks leave what they measured in files under tmp_path and
assert what they can see themselves; the parent asserts the rest.

Tensor sizes and gradient magnitudes (1e-6 .. 1e3) are those of test_gpu_fit.py."""
import json
import math
import os

import pytest
import torch

from conftest import formula_sd
from test_gpu_fit import NONCONTIG, SHAPES, _bits, _log, _params, _score_model, _set_grads, _tree

pytestmark = pytest.mark.gpu

JOIN_S = 300
SENTINEL = -7.5
TINY = 2.0 ** -126  # the smallest normal fp32


# ----------------------------------------------------------------------------- 1. the pack kernel
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0], ids=["1", "0.5", "1/3"])
def test_grad_pack_is_one_fp32_multiply_and_touches_nothing_else(gpu, scale):
    """Tensors of 1, 2047, 2048, 2049 elements, a (50, 100) non-contiguous gradient, a 4097-element gradient whose
    pointer is one element past a 16-B boundary (the scalar-load path, more than one chunk, n % 4 == 1) and a
    33-element row without a gradient.  flat == g * scale in fp32 bit for bit, zeros for the null row and the
    padding, and the sentinel before the layout, behind it and in the loss slot is untouched."""
    from snrse import _lib
    from snrse.dist import flat_layout
    from snrse.train import FusedAdam
    gen = torch.Generator(device=gpu).manual_seed(11)
    shapes = SHAPES[:5] + [(4097,), (33,)]
    ps = [torch.nn.Parameter(torch.zeros(s, device=gpu)) for s in shapes]
    grads = []
    for k, s in enumerate(shapes):
        mag = 10.0 ** (torch.rand(s, device=gpu, generator=gen) * 9.0 - 6.0)
        grads.append(torch.randn(s, device=gpu, generator=gen) * mag)
    base = torch.zeros(4097 + 8, device=gpu)
    base[1:4098] = grads[5]
    grads[5] = base[1:4098]
    grads[6] = None
    _set_grads(ps[:5], grads[:5])
    ps[5].grad = grads[5]
    assert ps[5].grad.data_ptr() % 16 == 4 and not ps[NONCONTIG].grad.is_contiguous() and ps[6].grad is None
    offs, total = flat_layout([p.numel() for p in ps])
    guard = 32
    buf = torch.full((guard + total + guard,), SENTINEL, device=gpu)
    flat = buf[guard:guard + total]
    assert flat.data_ptr() % 16 == 0
    flat[:total - 1] = 0.0  # the reducer's buffer is allocated zeroed; the loss slot keeps the sentinel here
    want = buf.clone()
    sc = torch.tensor(scale, dtype=torch.float32, device=gpu)
    for g, off in zip(grads, offs):
        if g is not None:
            want[guard + off:guard + off + g.numel()] = (g.contiguous().reshape(-1) * sc)
    opt = FusedAdam(ps, lr=1e-3)
    table, tix, starts, keep = opt.grad_table(ps)
    assert int(tix.numel()) == sum((p.numel() + 2047) // 2048 for p in ps)
    off_dev = torch.tensor(offs, dtype=torch.int64, device=gpu)
    _lib.call("snrse_grad_pack", table.data_ptr(), tix.data_ptr(), starts.data_ptr(), int(tix.numel()),
              off_dev.data_ptr(), scale, flat.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want))
    null = buf[guard + offs[6]:guard + offs[6] + 36]
    assert not null.any() and float(buf[guard + total - 1]) == SENTINEL


# ----------------------------------------------------------------------------- helpers of the spawns
def _rank_grads(dev, rank):
    """Rank `rank`'s gradient for every tensor of SHAPES, |g| spread log-uniformly over 1e-6 .. 1e3."""
    gen = torch.Generator(device=dev).manual_seed(100 + rank)
    out = []
    for s in SHAPES:
        mag = 10.0 ** (torch.rand(s, device=dev, generator=gen) * 9.0 - 6.0)
        out.append(torch.randn(s, device=dev, generator=gen) * mag)
    return out


def _gather_equal(t):
    """Whether the tensor is bit-identical on every rank (gloo: host copies)."""
    import torch.distributed as dist
    mine = t.detach().cpu().contiguous().reshape(-1)
    bufs = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(bufs, mine)
    return all(torch.equal(_bits(b), _bits(bufs[0])) for b in bufs)


def _spawn(world, fn, args):
    from snrse import dist as sd
    return sd.spawn_ranks(world, fn, args, timeout_s=JOIN_S)


def _read(path):
    with open(path) as f:
        return json.load(f)


# ----------------------------------------------------------------------------- 2. the reducer, world 2 and 3
def _reducer_worker(out):
    import torch.distributed as dist

    from snrse import dist as sd
    from snrse.train import FusedAdam
    rank, world, dev = sd.init_from_env()
    assert dist.get_backend() == "gloo" and dev.type == "cuda"
    mod = _params(dev)
    named = [(f"ps.{i}", p) for i, p in enumerate(mod.ps)]
    opt = FusedAdam(mod.parameters(), lr=1e-3, clip_grad_norm=1.0)
    red = sd.GradReducer(named, world, dev)
    _set_grads(mod.ps, _rank_grads(dev, rank))
    assert not mod.ps[NONCONTIG].grad.is_contiguous()
    loss = torch.tensor(float(rank + 1), device=dev)
    avg = red.reduce(opt, loss=loss)
    torch.cuda.synchronize()
    lo, hi = red.flat.data_ptr(), red.flat.data_ptr() + 4 * red.flat.numel()
    every = [_rank_grads(dev, r) for r in range(world)]
    worst = worst2 = 0.0
    for k, (p, off) in enumerate(zip(mod.ps, red.offsets)):
        assert p.grad.data_ptr() == lo + 4 * off and p.grad.data_ptr() + 4 * p.numel() <= hi  # a view of flat
        assert p.grad.shape == p.shape
        mean64 = sum(g[k].double() for g in every) / world
        bound = 4.0 * 2.0 ** -24 * sum(g[k].double().abs() for g in every) / world
        err = (p.grad.double() - mean64).abs()
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        if world == 2:  # the scale and the products are exact: one rounding, of the sum
            b2 = 2.0 ** -24 * mean64.abs().clamp_min(TINY)
            assert bool((err <= b2).all()), (k, float((err / b2).max()))
            worst2 = max(worst2, float((err / b2).max()))
    print(f"reducer world {world} rank {rank}: worst |got - mean64| / bound = {worst:.3f}"
          + (f", / (2^-24 |mean64|) = {worst2:.3f}" if world == 2 else ""), flush=True)
    assert _gather_equal(red.flat)  # gradients (and padding, and the loss slot) bit-identical across ranks
    want_loss = sum(r + 1 for r in range(world)) / world
    assert abs(float(avg) - want_loss) <= 4.0 * 2.0 ** -24 * want_loss
    assert not red.flat[red.offsets[0] + 1:red.offsets[1]].any()  # the padding behind the 1-element tensor
    # the optimizer step on the reduced gradients keeps the replicas bit-identical
    opt.step()
    torch.cuda.synchronize()
    state = [opt.last_grad_norm.reshape(1)]
    for p in mod.ps:
        state += [p.detach().reshape(-1), opt.state[p]["exp_avg"].reshape(-1), opt.state[p]["exp_avg_sq"].reshape(-1)]
    assert _gather_equal(torch.cat(state))
    red.check_replicas()
    sd.check_replicas(mod.parameters())
    if rank == world - 1:
        with torch.no_grad():
            mod.ps[2][5] += 1.0
    try:
        sd.check_replicas(mod.parameters())
        raised = None
    except RuntimeError as e:
        raised = str(e)
    assert raised is not None and f"[{world - 1}]" in raised, raised
    # last: a requires_grad parameter without a gradient, on every rank so that none is left waiting
    opt.zero_grad()
    _set_grads(mod.ps, _rank_grads(dev, rank))
    mod.ps[3].grad = None
    try:
        red.reduce(opt)
    except RuntimeError as e:
        with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
            json.dump({"worst": worst, "worst2": worst2, "raised": str(e)}, f)
        dist.barrier()  # every rank has raised and written before the first one exits and the rest are terminated
        raise
    raise AssertionError("reduce() accepted a parameter without a gradient")


@pytest.mark.parametrize("world", [2, 3])
def test_reducer_mean_views_replicas_and_missing_gradient(gpu, tmp_path, world):
    """After reduce() the .grads are views of flat, bit-identical across ranks and within
    4 2^-24 sum_r |g_r| / W of the fp64 mean per element: fl(1/W) is one rounding, each product one, and the
    W - 1 <= 2 additions one each on partial sums bounded by sum |g_r| / W.  W = 2: the scale and the products
    are exact, a single rounding remains, so also <= 2^-24 |mean64| (up to the smallest normal).  The clipped
    FusedAdam step then leaves parameters, moments and last_grad_norm bit-identical and check_replicas passes;
    it raises after one rank perturbs one element.  Last, every rank drops one gradient: reduce() raises before
    any collective and the spawn ends non-zero."""
    rc = _spawn(world, _reducer_worker, (str(tmp_path),))
    recs = [_read(tmp_path / f"rank{r}.json") for r in range(world)]  # every rank reached the last check
    assert rc not in (0, 124), rc
    for r, rec in enumerate(recs):
        print(f"world {world} rank {r}: worst ratio to the bound {rec['worst']:.3f}, W=2 one-rounding {rec['worst2']:.3f}")
        assert "parameter ps.3 has no gradient" in rec["raised"]
        assert 0.0 < rec["worst"] <= 1.0


# ----------------------------------------------------------------------------- 3. the RCCL path, world 1
def _rccl_worker(out):
    import torch.distributed as dist

    from snrse import dist as sd
    from snrse.train import FusedAdam
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        mod = _params(dev)
        opt = FusedAdam(mod.parameters(), lr=1e-3)
        red = sd.GradReducer(mod.named_parameters(), 1, dev)
        grads = _rank_grads(dev, 0)
        _set_grads(mod.ps, grads)
        avg = red.reduce(opt, loss=torch.tensor(2.5, device=dev))
        torch.cuda.synchronize()
        same = all(torch.equal(_bits(p.grad), _bits(g)) for p, g in zip(mod.ps, grads))
        lo = red.flat.data_ptr()
        views = all(p.grad.data_ptr() == lo + 4 * off for p, off in zip(mod.ps, red.offsets))
        sd.check_replicas(mod.parameters())
        with open(os.path.join(out, "rccl.json"), "w") as f:
            json.dump({"backend": dist.get_backend(), "is_cuda": bool(red.flat.is_cuda), "same": same,
                       "views": views, "loss": float(avg)}, f)
    finally:
        dist.destroy_process_group()


def test_reducer_over_rccl_world1(gpu, tmp_path):
    """A GradReducer in an 'nccl' (RCCL) group of one rank: the all-reduce runs in place on the HIP buffer and,
    the scale being 1, the reduced gradients are the originals bit for bit."""
    rc = _spawn(1, _rccl_worker, (str(tmp_path),))
    assert rc == 0
    rec = _read(tmp_path / "rccl.json")
    assert rec == {"backend": "nccl", "is_cuda": True, "same": True, "views": True, "loss": 2.5}


# ----------------------------------------------------------------------------- 4. SNRModel, world 2 vs one rank
def _snr_model(root):
    from sgmse.data_module import SpecsDataModule
    from sgmse.snr_estimator import SNRModel
    torch.manual_seed(0)
    return SNRModel(backbone="snrnet", data_module_cls=SpecsDataModule, base_dir=root, batch_size=2,
                    num_frames=64, transform_type="none", num_eval_files=0)


def _fit_state(m, opt):
    ps = list(m.parameters())
    return {"params": [p.detach().cpu() for p in ps], "ema": [s.detach().cpu() for s in m.ema.shadow_params],
            "m": [opt.state[p]["exp_avg"].cpu() for p in ps], "v": [opt.state[p]["exp_avg_sq"].cpu() for p in ps]}


def _snr_fit_worker(root, out):
    from snrse import dist as sd
    from snrse import fit
    rank, world, _ = sd.init_from_env()
    m = _snr_model(root)
    res = fit.fit(m, max_epochs=2, accumulate_grad_batches=1, gradient_clip_val=1.0, seed=7, rank=rank, world=world,
                  ckpt_dir=os.path.join(out, f"ck{rank}"), log_path=os.path.join(out, f"log{rank}.jsonl"))
    assert (res["epoch"], res["global_step"], res["epochs_run"]) == (1, 4, 2) and m.ema.num_updates == 4
    torch.save({**_fit_state(m, res["optimizer"]), "history": res["history"]}, os.path.join(out, f"rank{rank}.pt"))


def test_fit_snr_model_world2_equals_one_rank_bit_for_bit(gpu, tmp_path):
    """Run A here: world 1, batch_seeding, accumulate 2.  Run B: world 2, accumulate 1.  Both make 2 optimizer
    steps per epoch over the same global batches.  loss / 2 scales every gradient by an exact power of two, so A
    accumulates fl(g0/2 + g1/2); B packs g0 1/2 and g1 1/2 exactly and adds them once: the same single rounding.
    SNRNet's backward has no atomics and Adam is elementwise, so parameters and EMA shadows are equal bit for bit.
    The moments are held to atol 1e-37: gradient elements in the subnormal range may round differently when
    halved early or late, which cannot move an fp32 parameter past eps = 1e-8."""
    from sgmse.snr_estimator import SNRModel
    from snrse import fit
    root = _tree(tmp_path / "data", [9000 + 400 * k for k in range(8)], (9000, 10000, 12000))
    out = tmp_path / "b"
    out.mkdir()
    m = _snr_model(root)
    lg_a = str(tmp_path / "a.jsonl")
    res = fit.fit(m, max_epochs=2, accumulate_grad_batches=2, gradient_clip_val=1.0, seed=7, batch_seeding=True,
                  ckpt_dir=str(tmp_path / "cka"), log_path=lg_a)
    assert (res["epoch"], res["global_step"]) == (1, 4)
    a = _fit_state(m, res["optimizer"])
    assert _spawn(2, _snr_fit_worker, (root, str(out))) == 0
    b0, b1 = (torch.load(out / f"rank{r}.pt") for r in (0, 1))
    for key in ("params", "ema", "m", "v"):  # B's two ranks are bit-identical to each other
        assert len(b0[key]) == len(b1[key]) == len(a[key]) > 10
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(b0[key], b1[key])), key
    names = [n for n, _ in m.named_parameters()]
    for key in ("params", "ema"):
        for n, x, y in zip(names, a[key], b0[key]):
            diff = int((_bits(x) != _bits(y)).sum())
            assert diff == 0, f"{key} {n}: {diff} of {x.numel()} elements differ, max {float((x - y).abs().max()):.3e}"
    for key in ("m", "v"):
        for n, x, y in zip(names, a[key], b0[key]):
            assert torch.allclose(x, y, rtol=0.0, atol=1e-37), (key, n, float((x - y).abs().max()))
    # the log, the checkpoints: rank 0 alone
    assert sorted(os.listdir(out)) == ["ck0", "log0.jsonl", "rank0.pt", "rank1.pt"]
    la, lb = _log(lg_a), _log(out / "log0.jsonl")
    assert all(r["world"] == 2 for r in lb) and all(r["world"] == 1 for r in la)
    sa, sb = ([r for r in l if "train_loss" in r] for l in (la, lb))
    assert [r["step"] for r in sb] == [1, 2, 3, 4] and [r["epoch"] for r in sb] == [0, 0, 1, 1]
    for ra, rb in zip(sa, sb):
        # each is within one fp32 rounding (2^-24 relative) of the exact mean
        assert abs(ra["train_loss"] - rb["train_loss"]) <= 2.0 ** -23 * abs(ra["train_loss"]), (ra, rb)
        assert rb["samples_per_s"] > 0
    va, vb = ([r for r in l if "valid_loss" in r] for l in (la, lb))
    assert len(va) == len(vb) == 2
    for ra, rb in zip(va, vb):
        assert math.isfinite(rb["valid_loss"]) and math.isfinite(rb["snr_error"])
        assert abs(ra["valid_loss"] - rb["valid_loss"]) <= 1e-12 * abs(ra["valid_loss"]), (ra, rb)
        assert abs(ra["snr_error"] - rb["snr_error"]) <= 1e-12 * abs(ra["snr_error"]), (ra, rb)
    assert [h["valid_loss"] for h in b0["history"]] == [h["valid_loss"] for h in b1["history"]]
    cks = sorted(os.listdir(out / "ck0"))
    assert cks.count("last.ckpt") == 1 and all(not n.endswith(".tmp") for n in cks)
    loaded = SNRModel.load_from_checkpoint(str(out / "ck0" / "last.ckpt"))
    assert loaded.resume == {"epoch": 1, "global_step": 4}
    assert all(torch.equal(x, y) for x, y in zip(loaded.parameters(), b0["params"]))


# ----------------------------------------------------------------------------- 5. ScoreModel smoke, world 2
def _score_fit_worker(root, out):
    import torch.distributed as dist

    from sgmse import model as smodel
    from sgmse.snr_estimator import SNRModel
    from snrse import dist as sd
    from snrse import fit
    rank, world, _ = sd.init_from_env()
    sm = SNRModel()
    sm.dnn.load_state_dict({k: torch.from_numpy(v) for k, v in formula_sd("snrnet", "snrnet.").items()})
    smodel.set_snr_model(sm.cuda().eval())
    m = _score_model(root, num_eval_files=2, batch_size=1)
    w = m.dnn.all_modules[4].Conv_0.weight
    w0 = w.detach().clone()
    res = fit.fit(m, max_epochs=1, gradient_clip_val=1.0, seed=1, rank=rank, world=world,
                  ckpt_dir=os.path.join(out, f"ck{rank}"), log_path=os.path.join(out, f"log{rank}.jsonl"))
    assert (res["epoch"], res["global_step"]) == (0, 2) and m.training and m.ema.num_updates == 2
    sd.check_replicas(m.parameters())
    same = _gather_equal(w)
    dist.barrier()
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"same": same, "moved": not torch.equal(w0, w.detach()), "history": res["history"]}, f)


def test_fit_score_model_world2_smoke(gpu, tmp_path):
    """sebridge_v3 'true', batch 1 per rank x 64 frames, 4 training clips -> 2 optimizer steps, one epoch,
    num_eval_files = 2, clip 1.0: finite losses and si_sdr, replicas bit-identical, weights moved, rank 0 alone
    wrote last.ckpt and the top-k file.  No comparison with a one-rank run: the score network's statistics and
    loss use float atomics, so its gradients are not bit-reproducible; the bound of the reducer test is the
    guarantee."""
    root = _tree(tmp_path / "data", [9000 + 500 * k for k in range(4)], (8000, 9000, 10000))
    out = tmp_path / "b"
    out.mkdir()
    assert _spawn(2, _score_fit_worker, (root, str(out))) == 0
    recs = [_read(out / f"rank{r}.json") for r in (0, 1)]
    assert all(r["same"] and r["moved"] for r in recs)
    assert sorted(os.listdir(out)) == ["ck0", "log0.jsonl", "rank0.json", "rank1.json"]
    lines = _log(out / "log0.jsonl")
    steps = [r for r in lines if "train_loss" in r]
    assert [r["step"] for r in steps] == [1, 2] and all(math.isfinite(r["train_loss"]) for r in steps)
    assert all(r["world"] == 2 for r in lines)
    (val,) = [r for r in lines if "valid_loss" in r]
    assert math.isfinite(val["valid_loss"]) and math.isfinite(val["si_sdr"])
    for rec in recs:  # every rank holds rank 0's numbers
        assert rec["history"][0]["si_sdr"] == val["si_sdr"] and rec["history"][0]["valid_loss"] == val["valid_loss"]
    assert sorted(os.listdir(out / "ck0")) == sorted(["last.ckpt", f"epoch=0-si_sdr={val['si_sdr']:.2f}.ckpt"])
