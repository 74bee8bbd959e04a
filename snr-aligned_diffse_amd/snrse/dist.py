"""Multi-GPU utterance sharding: one process per GPU, no data-path
collective.  Utterances are independent, so each rank enhances a contiguous shard; RCCL
(torch.distributed 'nccl' on ROCm) is used only to take the max wall time over ranks and
to gather the per-utterance metrics at the end.  'gloo' runs the same code on CPU (tests).

Data-parallel training (snrse.fit) adds the one collective on a data path: GradReducer averages
the gradients of all ranks once per optimizer step, beside the small ones around it (the validation sums, rank
0's evaluation numbers, the replica check, barriers around rank 0's files).
"""
from __future__ import annotations

import os

import torch
import torch.distributed as dist


def oversubscribed(world: int) -> bool:
    """More ranks than visible GPUs (a rehearsal of the N-rank launch on a smaller box): ranks then
    share devices round-robin and the collectives run on gloo (RCCL needs one rank per device).
    torch.cuda.device_count() does not initialise the GPU."""
    n = torch.cuda.device_count()
    return 0 < n < world


def init_from_env(backend: str | None = None):
    """(rank, world, device) from torchrun's env; single process skips process-group init."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_gpu = torch.cuda.is_available() and backend != "gloo"
    if use_gpu and oversubscribed(world):
        local %= torch.cuda.device_count()
        backend = backend or "gloo"
    dev = torch.device("cuda", local) if use_gpu else torch.device("cpu")
    if use_gpu:
        torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        be = backend or ("nccl" if use_gpu else "gloo")
        if be == "nccl":
            dist.init_process_group(be, device_id=dev)
        else:
            dist.init_process_group(be)
    return rank, world, dev


def shard_range(n: int, rank: int, world: int):
    """Contiguous balanced shard [start, stop) of n utterances for `rank`."""
    base, extra = divmod(n, world)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def _coll_device(device):
    """gloo collectives take host tensors."""
    return torch.device("cpu") if dist.get_backend() == "gloo" else device


def max_over_ranks(value: float, device) -> float:
    if not (dist.is_available() and dist.is_initialized()):
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=_coll_device(device))
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t)


def gather_metrics(values, n_total: int, rank: int, world: int, device):
    """All ranks' per-utterance metric rows -> [n_total, k] float64 tensor on every rank,
    ordered by utterance index (rank r holds rows shard_range(n_total, r, world))."""
    vals = torch.as_tensor(values, dtype=torch.float64, device=device)
    if vals.dim() == 1:
        vals = vals[:, None]
    if not (dist.is_available() and dist.is_initialized()) or world == 1:
        return vals
    out_dev, device = device, _coll_device(device)
    vals = vals.to(device)
    k = vals.shape[1]
    cap = shard_range(n_total, 0, world)[1]  # largest shard
    pad = torch.full((cap, k), float("nan"), dtype=torch.float64, device=device)
    pad[: vals.shape[0]] = vals
    bufs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad)
    rows = []
    for r in range(world):
        a, b = shard_range(n_total, r, world)
        rows.append(bufs[r][: b - a])
    return torch.cat(rows, 0).to(out_dev)


def _active() -> bool:
    return dist.is_available() and dist.is_initialized()


def sum_over_ranks(values, device):
    """Element-wise fp64 sum of a short list of host numbers over the ranks -> list of floats."""
    if not _active():
        return [float(v) for v in values]
    t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=_coll_device(device))
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().tolist()


def broadcast_floats(values, n: int, device, src: int = 0):
    """`n` host numbers from rank `src` to every rank (the other ranks pass None) -> list of floats."""
    if not _active():
        return [float(v) for v in values]
    fill = [float(v) for v in values] if dist.get_rank() == src else [0.0] * n
    t = torch.tensor(fill, dtype=torch.float64, device=_coll_device(device))
    dist.broadcast(t, src=src)
    return t.cpu().tolist()


def barrier():
    if _active():
        dist.barrier()


def broadcast_tensors(tensors, device, src: int = 0):
    """Overwrite every tensor with rank `src`'s copy (what torch DDP does with the module state when it is
    built): the replicas start from the same weights whatever each rank's constructor drew."""
    if not _active():
        return
    host = dist.get_backend() == "gloo"
    with torch.no_grad():
        for t in tensors:
            buf = t.detach().cpu() if host else t.detach()
            dist.broadcast(buf, src=src)
            if host:
                t.copy_(buf)


# ----------------------------------------------------------------------------- data-parallel training
def flat_layout(sizes):
    """Offsets of tensors of `sizes` elements in the flat gradient buffer, each padded to 4 elements (16 B), and
    the buffer's length: the padded sizes plus one slot at the end for the loss.  -> (offsets, total)."""
    offs, off = [], 0
    for n in sizes:
        offs.append(off)
        off += (int(n) + 3) // 4 * 4
    return offs, off + 1


def check_replicas(params, device=None):
    """Every rank holds the same parameters: one fp64 checksum per rank (the sum of every parameter's
    double().sum()), gathered and compared as bits.  RuntimeError naming the ranks that differ from rank 0."""
    params = list(params)
    if not _active() or not params:
        return
    device = device if device is not None else params[0].device
    with torch.no_grad():
        s = torch.stack([p.detach().double().sum() for p in params]).sum().reshape(1)
    s = s.to(_coll_device(device))
    bufs = [torch.empty_like(s) for _ in range(dist.get_world_size())]
    dist.all_gather(bufs, s)
    bits = [int(b.cpu().view(torch.int64)) for b in bufs]
    bad = [r for r, b in enumerate(bits) if b != bits[0]]
    if bad:
        raise RuntimeError(f"snrse.dist: the parameter replicas differ: rank(s) {bad} do not match rank 0 "
                           f"(checksums {[float(b.cpu()) for b in bufs]})")


class GradReducer:
    """The gradient exchange of data-parallel training, in torch DDP's semantics (find_unused_parameters=False):
    after reduce() every parameter's .grad is the mean of the ranks' gradients, bit-identical on every rank.

    The layout is fixed at construction: every requires_grad parameter of `params` (parameters, or (name,
    parameter) pairs, in optimizer order) at an offset padded to 4 elements in one fp32 buffer `flat`, and one
    slot at the end for the loss.  `flat` is allocated zeroed and the padding is never written, so it stays zero
    through every sum.  reduce() packs g / world into `flat` in one launch (snrse_grad_pack over the optimizer's
    tensor table and chunk list), sums `flat` over the ranks with one all-reduce and points each .grad at its
    slice of `flat`: there is no unpack, the clip's norm and the Adam launch read the averaged gradients in place.
    optimizer.zero_grad() drops the views before the next backward, and everything runs on one stream, so the
    reuse of `flat` is ordered.  'nccl' (RCCL) reduces the device buffer in place; 'gloo' (ranks that share a
    device, oversubscribed()) goes through a pinned host buffer.  One all-reduce per optimizer step after the
    backward: no bucketed overlap with the backward, one node."""

    def __init__(self, params, world, device):
        items = [(pn if isinstance(pn, tuple) else (None, pn)) for pn in params]
        items = [(n, p) for n, p in items if p.requires_grad]
        if not items:
            raise ValueError("GradReducer: no parameter requires a gradient")
        self.names = [n if n is not None else f"#{i} {tuple(p.shape)}" for i, (n, p) in enumerate(items)]
        self.params = [p for _, p in items]
        self.world, self.device = int(world), torch.device(device)
        self.offsets, total = flat_layout([p.numel() for p in self.params])
        self.loss_slot = total - 1
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.flat_off = torch.tensor(self.offsets, dtype=torch.int64, device=self.device)
        # each parameter's slice of flat in its shape, made once: re-pointing a .grad is then an attribute store
        self.views = [self.flat[o:o + p.numel()].view(p.shape) for p, o in zip(self.params, self.offsets)]
        self._host = None
        self._keep = None

    def _all_reduce(self):
        if not _active():
            if self.world != 1:
                raise RuntimeError("GradReducer: world > 1 needs an initialised process group")
            return
        if dist.get_backend() == "gloo":
            if self._host is None:
                self._host = torch.empty(self.flat.numel(), dtype=torch.float32, pin_memory=True)
            self._host.copy_(self.flat)
            dist.all_reduce(self._host, op=dist.ReduceOp.SUM)
            self.flat.copy_(self._host)
        else:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)

    @torch.no_grad()
    def reduce(self, optimizer, loss=None):
        """Average the gradients over the ranks; `loss` (a device scalar) is averaged with them.  -> the averaged
        loss (a one-element view of `flat`, valid until the next reduce) or None."""
        for name, p in zip(self.names, self.params):
            if p.grad is None:
                raise RuntimeError(f"GradReducer: parameter {name} has no gradient on this rank; every "
                                   "requires_grad parameter must take part in the loss (torch DDP's rule "
                                   "with find_unused_parameters=False)")
        from .train import _call
        table, tix, starts, keep = optimizer.grad_table(self.params)
        _call("snrse_grad_pack", table.data_ptr(), tix.data_ptr(), starts.data_ptr(), int(tix.numel()),
              self.flat_off.data_ptr(), 1.0 / self.world, self.flat.data_ptr())
        slot = self.flat[self.loss_slot:]
        if loss is None:
            slot.zero_()
        else:
            torch.mul(loss.detach().reshape(1).to(self.device, torch.float32), 1.0 / self.world, out=slot)
        self._all_reduce()
        for p, view in zip(self.params, self.views):
            p.grad = view
        self._keep = keep + [tix, starts]  # the pack reads them asynchronously
        return None if loss is None else slot

    def check_replicas(self, params=None):
        check_replicas(self.params if params is None else params, self.device)


def free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_entry(rank, world, port, fn, args):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    fn(*args)


def spawn_ranks(world: int, fn, args=(), poll_s: float = 0.5, timeout_s: float | None = None) -> int:
    """Run fn(*args) in `world` fresh processes (multiprocessing 'spawn'), rank r on GPU r, with
    torchrun's environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT).
    The caller must not have initialised the GPU (children are new interpreters, nothing is exec'd
    over a GPU-initialised process).  If a rank fails, the others are terminated instead of being
    left waiting in a collective.  timeout_s (None: wait for as long as it takes): when the time is up
    every rank still running is terminated and the result is non-zero.  Returns 0 or the first failing
    rank's exit code."""
    import time

    import torch.multiprocessing as mp
    port = free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_entry, args=(r, world, port, fn, args)) for r in range(world)]
    for p in procs:
        p.start()
    rc = 0
    t_end = None if timeout_s is None else time.monotonic() + float(timeout_s)
    while any(p.is_alive() for p in procs):
        bad = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
        if not bad and t_end is not None and time.monotonic() >= t_end:
            bad = [124]  # the exit status of a run that ran out of time
        if bad:
            rc = bad[0]
            for p in procs:
                if p.is_alive():
                    p.terminate()
            break
        time.sleep(poll_s)
    for p in procs:
        p.join(30 if rc else None)
        if p.is_alive():  # terminated above and still there: a rank stuck where SIGTERM does not reach it
            p.kill()
            p.join()
        if rc == 0 and p.exitcode:
            rc = p.exitcode
    return rc
