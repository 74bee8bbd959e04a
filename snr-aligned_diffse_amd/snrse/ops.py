"""Torch-tensor wrappers over the C-ABI (device pointers + torch's current stream).

Every op requires HIP device tensors and raises otherwise — there is no CPU fallback.

Concurrency contract.  The library's stateful entries (snrse_conv2d, snrse_gn_stats, snrse_input_conv,
snrse_gn_resample) take a caller-owned launch context (snrse_ctx: switches, split-K workspace, read-backs
of the latest launch), so calls through distinct contexts are independent.  Here every host thread has
its own context per device (LaunchContext, thread-local, with its own split-K workspace), the StatsArena
stack is thread-local, and each network keeps one arena per launch stream.  So evaluations issued by
different host threads on different streams run concurrently without sharing mutable state, and one
thread interleaving several streams (snrse.sampler.pc_sample_lockstep) switches to a per-lane context
with use_workspace_lane(lane) before issuing each lane's launches.  set_option() is process-wide policy:
it edits the library's process default and every live context; get_option() reads the calling thread's
current context (so "last_kernel" etc. describe that thread's latest launch).
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
import os
import threading
import weakref

import numpy as np
import torch

from . import _lib

F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
INV_SQRT2 = 1.0 / math.sqrt(2.0)
# the 16-bit activation / weight formats of the fast path: fp16 (round 6 default) and bf16 (the same kernels)
H16 = (torch.float16, torch.bfloat16)


def conv_code(act_dtype: torch.dtype, wgt_dtype: torch.dtype) -> int:
    """snrse_conv2d dtype: fp32 activations with bf16 weights are the split-bf16 fp32 GEMM (weights from
    split_weight), else the activations' dtype (weights of the same dtype)."""
    if act_dtype == torch.float32 and wgt_dtype == torch.bfloat16:
        return _lib.F32X3
    if wgt_dtype != act_dtype:
        raise TypeError(f"snrse: conv weights {wgt_dtype} for {act_dtype} activations")
    return code(act_dtype)


def split_weight(w: torch.Tensor) -> torch.Tensor:
    """fp32 packed conv weights [N][K] (K % 32 == 0) -> the SNRSE_F32X3 layout [N][2K] bf16: per 32-element
    K-tile, 32 hi = bf16(w) then 32 lo = bf16(w - hi)."""
    n, k = w.shape
    if k % 32:
        raise ValueError(f"snrse: split weights need K % 32 == 0, got {k}")
    w = w.float().reshape(n, k // 32, 1, 32)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], 2).reshape(n, 2 * k).contiguous()


def code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.float16:
        return F16
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"snrse: unsupported dtype {dtype}")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def current_device():
    """The current HIP device with its index: what the .device of a tensor on it compares equal to."""
    return torch.device("cuda", torch.cuda.current_device())


def _ws_alloc(dev):
    mb = int(os.environ.get("SNRSE_WORKSPACE_MB", "128"))
    return (torch.empty(mb << 18, dtype=torch.float32, device=dev) if mb > 0 else None), mb


_CONTEXTS = weakref.WeakSet()  # every live LaunchContext (set_option reaches all of them)
_CTX_SEQ = itertools.count()
_TLS = threading.local()       # per thread: {device: {lane: LaunchContext}}, current lane per device, arenas


class LaunchContext:
    """A caller-owned snrse_ctx (include/snrse.h) on one device: the library's switches (copied from the
    process default at creation), a split-K workspace of SNRSE_WORKSPACE_MB (default 128; 0 disables K
    splitting) and the read-backs of the latest launch issued through it."""

    def __init__(self, device):
        lib = _lib.load()
        self.device = torch.device(device)
        self.ptr = lib.snrse_ctx_create()
        if not self.ptr:
            raise MemoryError("snrse_ctx_create failed")
        self._lib = lib
        self.ws, mb = _ws_alloc(self.device)
        _lib.call("snrse_ctx_set_workspace", self.ptr, None if self.ws is None else self.ws.data_ptr(),
                  0 if self.ws is None else mb << 20)
        # mirror of the context's "stats_zeroed" switch; snrse_ctx_create copies it from the process default
        self.zeroed = int(bool(self.get_option("stats_zeroed")))
        self.seq = next(_CTX_SEQ)  # creation order (probe_read over several threads' contexts)
        _CONTEXTS.add(self)

    def set_option(self, name, value):
        _lib.call("snrse_ctx_set_option", self.ptr, name.encode(), int(value))
        if name == "stats_zeroed":
            self.zeroed = int(bool(value))

    def get_option(self, name):
        v = C.c_int(0)
        _lib.call("snrse_ctx_get_option", self.ptr, name.encode(), C.addressof(v))
        return v.value

    def __del__(self):
        try:
            self._lib.snrse_ctx_destroy(self.ptr)
        except Exception:
            pass


def _tls_contexts(dev):
    d = getattr(_TLS, "ctx", None)
    if d is None:
        d = _TLS.ctx = {}
        _TLS.lane = {}
    return d.setdefault(torch.device(dev), {})


def context(dev=None, lane=None):
    """The calling thread's current LaunchContext on `dev` (lane: that lane's context, created on first
    use; default: the lane selected by use_workspace_lane, initially 0)."""
    dev = current_device() if dev is None else torch.device(dev)
    ctxs = _tls_contexts(dev)
    if lane is None:
        lane = _TLS.lane.get(dev, 0)
    c = ctxs.get(lane)
    if c is None:
        c = ctxs[lane] = LaunchContext(dev)
    return c


def _cx(dev):
    return context(dev).ptr


def use_workspace_lane(lane, dev):
    """Make lane `lane`'s own context (and so its own split-K workspace and read-backs) the calling
    thread's current one on `dev`.  The two-stream sampler (snrse.sampler.pc_sample_lockstep) issues each
    half-batch's launches behind its lane's context, so concurrent split-K GEMMs never share a workspace."""
    dev = torch.device(dev)
    _tls_contexts(dev)
    _TLS.lane[dev] = lane
    context(dev, lane)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("snrse: HIP device tensor required (no CPU fallback)")
        if t is not None and not t.is_contiguous():
            raise RuntimeError("snrse: contiguous tensor required")


def conv2d(src0, wgt, ksize, cout, bias=None, src1=None, sc=None, sc1=None, sc_wgt=None, temb=None,
           temb_off=0, res=None, out_scale=1.0, comb=None, comb_w=None, comb_b=None, out=None,
           out_f32=False, stats=None, gn=None, gn_act=True):
    """NHWC conv (see snrse_conv2d).  src0 [B,H,W,C0]; returns out [B,H,W,cout].
    temb: [B, R] f32 table of all Dense_0 outputs, this layer's columns start at temb_off.
    stats: optional new_stats() buffer receiving the output's per-channel (sum, sumsq).
    gn: optional (scale, shift) [B, C0+C1] f32 — consume SiLU(GN(x)) (halo path only, see halo_ok)."""
    _dev(src0, src1, wgt, sc, sc1, sc_wgt, bias, res, comb, comb_w, comb_b, temb)
    cx = context(src0.device)
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    Csc = 0 if sc is None else sc.shape[3]
    Csc1 = 0 if sc1 is None else sc1.shape[3]
    odt = torch.float32 if out_f32 else src0.dtype
    if sc_wgt is not None and sc_wgt.dtype != wgt.dtype:
        raise TypeError("snrse: conv2d wgt and sc_wgt must share one layout (both split or neither)")
    if out is None:
        out = torch.empty(B, H, W, cout, device=src0.device, dtype=odt)
    _stats_zeroed(cx, stats)
    _lib.call("snrse_conv2d", cx.ptr, _ptr(src0), C0, _ptr(src1), C1, B, H, W, ksize, _ptr(wgt), _ptr(sc), Csc,
              _ptr(sc1), Csc1, _ptr(sc_wgt), _ptr(bias), None if temb is None else temb.data_ptr() + 4 * temb_off,
              0 if temb is None else temb.shape[1], _ptr(res), 0 if res is None else res.shape[-1], float(out_scale), _ptr(comb),
              _ptr(comb_w), _ptr(comb_b), out.data_ptr(), cout, out.shape[-1], _ptr(stats),
              None if gn is None else gn[0].data_ptr(), None if gn is None else gn[1].data_ptr(), int(bool(gn_act)),
              conv_code(src0.dtype, wgt.dtype), int(out_f32), _stream())
    return out


def _opt(x, name):
    """A library switch as the launch context of x's device sees it (set_option, SNRSE_OPTS or a
    per-context setting): the shape predicates below mirror the library's own dispatch."""
    return context(x.device).get_option(name)


def get_option(name):
    """A switch or read-back of the calling thread's current context on the current device."""
    return context().get_option(name)


def _probe_contexts(dev, all_threads):
    """This thread's context first, then (all_threads) every other live context on the device by creation."""
    own = context(dev)
    if not all_threads:
        return [own]
    others = sorted((c for c in list(_CONTEXTS) if c is not own and c.device == own.device), key=lambda c: c.seq)
    return [own] + others


def probe_begin(capacity, dev=None, all_threads=False):
    """Bracket the next `capacity` conv2d calls of this thread's current context (all_threads: of every
    context on the device, e.g. the autograd engine's worker thread during a backward) with library-recorded
    HIP events (snrse_ctx_probe_begin; created without the system-scope fence).  capacity 0 stops probing."""
    for cx in _probe_contexts(dev, all_threads):
        _lib.call("snrse_ctx_probe_begin", cx.ptr, int(capacity))


def probe_read(max_calls, dev=None, all_threads=False):
    """(ms per probed conv2d call, kernel generation per call) (snrse_ctx_probe_read): in call order for one
    context; with all_threads, this thread's calls followed by each other context's (the order of a
    training step: forward on the calling thread, then the backward on the autograd worker)."""
    out_ms, out_k = [], []
    for cx in _probe_contexts(dev, all_threads):
        ms = (C.c_float * max_calls)()
        kern = (C.c_int * max_calls)()
        n = C.c_int(0)
        _lib.call("snrse_ctx_probe_read", cx.ptr, C.addressof(ms), C.addressof(kern), int(max_calls),
                  C.addressof(n))
        out_ms += list(ms[:n.value])
        out_k += list(kern[:n.value])
    return out_ms, out_k


KERNELS = {1: "conv_mfma_kernel", 2: "conv_glds_kernel", 3: "conv_x3_kernel", 4: "conv_x3h_kernel",
           5: "conv_halo5_kernel",
           10: "conv_head_kernel", 11: "conv_head_x3_kernel", 14: "conv_head_small_kernel",
           15: "conv_head_part_kernel"}


def kernel_name(gen):
    """Kernel symbol of a conv generation code (snrse_get_option "last_kernel" / "halo_kernel")."""
    return KERNELS.get(gen, f"conv_kernel_{gen}")


def conv_kernel_name():
    """Kernel symbol the halo-eligible convs dispatch to under the current setting."""
    return kernel_name(get_option("halo_kernel"))


def halo_ok(x, ksize, cout):
    """True when snrse_conv2d takes the halo path (and so accepts a fused GroupNorm).  Any batch size
    qualifies: sources beyond 2 GiB run as consecutive launches over image ranges (snrse_conv2d)."""
    B, H, W, C = x.shape
    # images tileable by 4 x 64 (the kernel then uses 8 x 32 tiles where H % 8 == 0); W = 32 alone stays on
    # the split-K GEMM (faster there: profiles/r03v_level4_halo_vs_glds.jsonl)
    return (x.dtype in H16 and ksize == 3 and cout % 128 == 0 and H % 4 == 0 and W % 64 == 0
            and _opt(x, "conv_variant") in (0, 5))


def x3h_ok(x, ksize, cout):
    """True when a split-bf16 fp32 conv (fp32 x, ops.split_weight weights) takes the halo kernel
    (conv_x3h_kernel) under the current x3_tile setting -- the one form that accepts a fused GroupNorm
    (gn=).  Mirrors snrse_conv2d's dispatch: 3x3, H % 4 == 0 and >= 256 tiles of 4 x 64 px x 128 couts
    (the last tile column cut by the image edge; x3_tile 0), or wherever legal (x3_tile 4)."""
    B, H, W, C = x.shape
    if x.dtype != torch.float32 or ksize != 3 or cout % 128 or H % 4:
        return False
    t = _opt(x, "x3_tile")
    return t == 4 or (t == 0 and B * (H // 4) * (-(-W // 64)) * (cout // 128) >= 256)


def head_ok(x, split=False):
    """True when a 3x3 conv of x with Cout = 4 and f32 output (the pyramid heads) takes a head kernel that
    accepts a fused GroupNorm (gn=): the halo-staged head (16-bit x, C <= 1024; or f32 x with split weights:
    split=True, the fp32x3 mode's conv_head_x3_kernel; H % 8 == 0, W % 32 == 0), or with C % 256 == 0 the
    wave-per-8-pixels head of the other image sizes (16-bit, or the fp32x3 form; option head_small, snrse_conv2d)."""
    B, H, W, C = x.shape
    if _opt(x, "conv_variant") == 1:
        return False
    h16 = x.dtype in H16
    dt_ok = h16 or (split and x.dtype == torch.float32)
    # channels: the C-ABI's K-tile (64 16-bit / 32 f32 channels, snrse_conv2d); the 16-bit tiled heads stage the
    # image's GroupNorm affine in an LDS table of 1024 channels
    if dt_ok and H % 8 == 0 and W % 32 == 0 and C % (64 if h16 else 32) == 0 and (not h16 or C <= 1024):
        return True
    return dt_ok and C % 256 == 0 and _opt(x, "head_small") != 0


def gn_scale_shift(sums0, gamma, beta, HW, sums1=None, groups=None, eps=1e-6):
    """Per-(b, c) GroupNorm affine [B, C] x 2 from per-channel sums."""
    _dev(sums0, sums1, gamma, beta)
    B, C0 = sums0.shape[0], sums0.shape[2]
    C1 = 0 if sums1 is None else sums1.shape[2]
    C = C0 + C1
    g = groups if groups is not None else min(C // 4, 32)
    # one [2, B, C] allocation: the persistent halo GEMM fetches scale and shift through a single
    # buffer resource (shift == scale + B*C)
    ss = torch.empty(2, B, C, device=sums0.device, dtype=torch.float32)
    scale, shift = ss[0], ss[1]
    _lib.call("snrse_gn_scale_shift", sums0.data_ptr(), C0, _ptr(sums1), C1, B, HW, gamma.data_ptr(), beta.data_ptr(),
              g, float(eps), scale.data_ptr(), shift.data_ptr(), _stream())
    return scale, shift


STAT_SLOTS = 16  # SNRSE_STAT_SLOTS (include/snrse.h)


def _arena_stack():
    """The calling thread's active StatsArena stack (innermost last)."""
    st = getattr(_TLS, "arenas", None)
    if st is None:
        st = _TLS.arenas = []
    return st


class StatsArena:
    """One f64 buffer per network evaluation, zeroed by a single fill, from which new_stats()
    carves the GroupNorm statistics buffers; the producers are told (option "stats_zeroed") to
    skip their per-call memset.  The first evaluation inside an arena only measures the size
    (its buffers come from torch.empty and are cleared by the producers as usual)."""

    ALIGN = 32  # doubles (256 B)

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf, self.off, self.need = None, 0, 0

    def __enter__(self):
        if self.buf is not None:
            self.buf.zero_()
        self.off, self.need = 0, 0
        _arena_stack().append(self)
        return self

    def __exit__(self, *exc):
        _arena_stack().remove(self)
        if self.buf is None or self.need > self.buf.numel():
            self.buf = torch.empty(self.need, dtype=torch.float64, device=self.device)
        return False

    def take(self, n):
        na = (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.need += na
        if self.buf is None or self.off + na > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n]
        self.off += na
        return t


def _stats_zeroed(cx, *bufs):
    """Set context cx's "stats_zeroed" switch for a producer writing into `bufs`."""
    bufs = [b for b in bufs if b is not None]
    if not bufs:
        return
    z = int(all(getattr(b, "_snrse_zeroed", False) for b in bufs))
    if cx.zeroed != z:
        cx.set_option("stats_zeroed", z)


def new_stats(x_or_shape, C=None):
    """[B, STAT_SLOTS, C, 2] f64 per-channel statistics buffer for an NHWC tensor (producers
    spread their atomics over the slots; consumers fold them).  Inside a StatsArena on the same
    device the buffer is a pre-zeroed arena slice."""
    if C is None:
        B, C, dev = x_or_shape.shape[0], x_or_shape.shape[-1], x_or_shape.device
    else:
        B, dev = x_or_shape, current_device()
    st = _arena_stack()
    if st and st[-1].device == torch.device(dev):
        t = st[-1].take(B * STAT_SLOTS * C * 2)
        if t is not None:
            t = t.view(B, STAT_SLOTS, C, 2)
            t._snrse_zeroed = True
            return t
    return torch.empty(B, STAT_SLOTS, C, 2, device=dev, dtype=torch.float64)


def fold_stats(st):
    """[B, STAT_SLOTS, C, 2] -> [B, C, 2] per-channel (sum, sumsq) (inspection / tests)."""
    return st.sum(1)


def gn_stats(src0, src1=None):
    """Per-channel (sum, sumsq) of each source: returns (sums0, sums1 or None)."""
    _dev(src0, src1)
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    s0 = new_stats(src0)
    s1 = None if src1 is None else new_stats(src1)
    cx = context(src0.device)
    _stats_zeroed(cx, s0, s1)
    _lib.call("snrse_gn_stats", cx.ptr, _ptr(src0), C0, _ptr(src1), C1, B, H * W, s0.data_ptr(), _ptr(s1),
              code(src0.dtype), _stream())
    return s0, s1


MODES = {"none": 0, "down": 1, "up": 2}
GN_FUSED_MAX_HW = 512  # gn_apply: images up to this many pixels take the single fold + apply launch


def gn_apply(src0, src1=None, sums=None, gamma=None, beta=None, act=True, mode="none", groups=None, eps=1e-6,
             sums1=None):
    """sums: new_stats() buffer of src0 or a (sums0, sums1) pair; None = no norm."""
    if isinstance(sums, tuple):
        sums, sums1 = sums
    _dev(src0, src1, sums, sums1, gamma, beta)
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    C = C0 + C1
    m = MODES[mode]
    # small images (the 16 x 32 .. 4 x 8 levels of C2): ONE launch that folds the statistics per block (at most
    # 4 blocks per image) and applies, instead of gn_scale_shift + gn_act -- two launch-floor kernels
    small = m == 0 and H * W <= GN_FUSED_MAX_HW
    if sums is not None and (m == 0 or resample_ok(src0)) and not small:
        # the per-(b, c) affine once (snrse_gn_scale_shift), then the elementwise / LDS-tiled apply: no
        # per-block re-fold of the slotted statistics (the fp32 gn_apply pass ran at ~0.2 of HBM peak that way)
        scale, shift = gn_scale_shift(sums, gamma, beta, H * W, sums1=sums1, groups=groups, eps=eps)
        if m == 0:
            return gn_act(src0, src1, scale, shift, act=act)
        if src1 is None and resample_ok(src0):
            return gn_resample(src0, scale, shift, act=act, mode=mode)[0]
    Ho, Wo = (H // 2, W // 2) if m == 1 else ((2 * H, 2 * W) if m == 2 else (H, W))
    out = torch.empty(B, Ho, Wo, C, device=src0.device, dtype=src0.dtype)
    g = groups if groups is not None else min(C // 4, 32)
    _lib.call("snrse_gn_apply", _ptr(src0), C0, _ptr(src1), C1, B, H, W, _ptr(sums), _ptr(sums1), _ptr(gamma),
              _ptr(beta), g, float(eps), int(bool(act)), m, out.data_ptr(), code(src0.dtype), _stream())
    return out


def resample_ok(x):
    """True when snrse_gn_resample takes x (NHWC): 16-bit with C % 16 == 0, or f32 with C / 4 dividing 64."""
    C = x.shape[3]
    if x.dtype in H16:
        return C % 16 == 0
    return x.dtype == torch.float32 and C % 4 == 0 and 64 % (C // 4) == 0


def gn_resample(x, scale=None, shift=None, act=True, mode="down", want_raw=False):
    """act(x*scale+shift) FIR-resampled x2 ('down' / 'up': upfirdn2d with [1,3,3,1]) and, with
    want_raw, the FIR of x itself (the ResBlock shortcut input) from one LDS-tiled pass over x
    (snrse_gn_resample; 16-bit: C % 8 == 0 with C / 8 dividing 64, or C % 16 == 0; f32: C / 4 dividing 64).
    Returns (activated, raw or None)."""
    _dev(x, scale, shift)
    if x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise TypeError("snrse: gn_resample takes fp16, bf16 or f32 activations")
    B, H, W, C = x.shape
    m = MODES[mode]
    if m == 0:
        raise ValueError("snrse: gn_resample mode must be 'down' or 'up'")
    Ho, Wo = (H // 2, W // 2) if m == 1 else (2 * H, 2 * W)
    oa = torch.empty(B, Ho, Wo, C, device=x.device, dtype=x.dtype)
    orw = torch.empty_like(oa) if want_raw else None
    _lib.call("snrse_gn_resample", _cx(x.device), x.data_ptr(), C, B, H, W, _ptr(scale), _ptr(shift), int(bool(act)), m,
              oa.data_ptr(), _ptr(orw), code(x.dtype), _stream())
    return oa, orw


def gn_act(src0, src1=None, scale=None, shift=None, act=True):
    """act(x*scale+shift) of the channel concatenation (src0 | src1), NHWC fp16, bf16 or f32 (snrse_gn_act)."""
    _dev(src0, src1, scale, shift)
    B, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[3]
    out = torch.empty(B, H, W, C0 + C1, device=src0.device, dtype=src0.dtype)
    _lib.call("snrse_gn_act", src0.data_ptr(), C0, _ptr(src1), C1, B, H * W, _ptr(scale), _ptr(shift),
              int(bool(act)), out.data_ptr(), code(src0.dtype), _stream())
    return out


def fir(x, mode):
    """FIR [1,3,3,1] down/up x2 of an NHWC tensor (no normalisation)."""
    return gn_apply(x, act=False, mode=mode)


def attention(qkv, C=256, split=False):
    """softmax(q k^T / sqrt(C)) v (layerspp.py:84-88) of qkv [B, L(, W), 3C]; split=True (fp32 only): the fp32x3
    mode's split-bf16 products (snrse_attention with SNRSE_F32X3) instead of exact fp32 MFMAs."""
    _dev(qkv)
    B, L = qkv.shape[0], qkv.shape[1] * (qkv.shape[2] if qkv.dim() == 4 else 1)
    out = torch.empty(*qkv.shape[:-1], C, device=qkv.device, dtype=qkv.dtype)
    if split and qkv.dtype != torch.float32:
        raise TypeError("snrse: split attention takes fp32 q, k, v")
    _lib.call("snrse_attention", qkv.data_ptr(), out.data_ptr(), B, L, C, _lib.F32X3 if split else code(qkv.dtype),
              _stream())
    return out


def temb_mlp(t, Wg, W1, b1, W2, b2, fused=False):
    """temb [B, 4 nf] (ncsnpp.py:256-275): two row-parallel launches, snrse_temb_gfp_dense (W1 gfp(t) + b1) then
    snrse_temb_dense (W2 silu(.) + b2); fused=True: the one-launch snrse_temb_mlp (a block per utterance)."""
    _dev(t, Wg, W1, b1, W2, b2)
    B = t.shape[0]
    out = torch.empty(B, W2.shape[0], device=t.device, dtype=torch.float32)
    if fused:
        _lib.call("snrse_temb_mlp", t.data_ptr(), Wg.data_ptr(), W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                  b2.data_ptr(), out.data_ptr(), B, Wg.shape[0], _stream())
        return out
    a = torch.empty(B, W1.shape[0], device=t.device, dtype=torch.float32)
    _lib.call("snrse_temb_gfp_dense", t.data_ptr(), Wg.data_ptr(), W1.data_ptr(), b1.data_ptr(), a.data_ptr(), B,
              Wg.shape[0], _stream())
    _lib.call("snrse_temb_dense", a.data_ptr(), W2.data_ptr(), b2.data_ptr(), out.data_ptr(), B, W2.shape[0],
              W2.shape[1], _stream())
    return out


def temb_dense(temb, W, bias):
    _dev(temb, W, bias)
    B, D = temb.shape
    R = W.shape[0]
    out = torch.empty(B, R, device=temb.device, dtype=torch.float32)
    _lib.call("snrse_temb_dense", temb.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), B, R, D,
              _stream())
    return out


def input_conv_ok(x):
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    return T % 64 == 0 and (F * T // 64) % 16 == 0


def input_conv(x, y, wgt, bias):
    """16-bit fused input conv: x, y complex64 [B,F,T], wgt [128][64] fp16 or bf16 -> (h [B,F,T,128] in wgt's
    format, stats, pyramid f32)."""
    _dev(x, y, wgt, bias)
    if wgt.dtype not in H16:
        raise TypeError(f"snrse: input_conv takes fp16 / bf16 weights, got {wgt.dtype}")
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    h = torch.empty(B, F, T, 128, device=x.device, dtype=wgt.dtype)
    pyr = torch.empty(B, F, T, 4, device=x.device, dtype=torch.float32)
    st = new_stats(B, 128)
    cx = context(x.device)
    _stats_zeroed(cx, st)
    _lib.call("snrse_input_conv", cx.ptr, x.data_ptr(), y.data_ptr(), B, F, T, wgt.data_ptr(), bias.data_ptr(),
              h.data_ptr(), pyr.data_ptr(), st.data_ptr(), code(wgt.dtype), _stream())
    return h, st, pyr


def input_conv_x3_ok(x):
    return input_conv_ok(x) and x.shape[-1] <= 1024


def input_conv_x3(x, y, wgt_split, bias):
    """fp32x3 fused input conv: x, y complex64 [B,F,T], split weights [128][128] bf16 -> (h [B,F,T,128] f32,
    stats, pyramid f32)."""
    _dev(x, y, wgt_split, bias)
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    h = torch.empty(B, F, T, 128, device=x.device, dtype=torch.float32)
    pyr = torch.empty(B, F, T, 4, device=x.device, dtype=torch.float32)
    st = new_stats(B, 128)
    cx = context(x.device)
    _stats_zeroed(cx, st)
    _lib.call("snrse_input_conv_x3", cx.ptr, x.data_ptr(), y.data_ptr(), B, F, T, wgt_split.data_ptr(),
              bias.data_ptr(), h.data_ptr(), pyr.data_ptr(), st.data_ptr(), _stream())
    return h, st, pyr


def input_pack(x, y, dtype):
    """x, y complex64 [B,F,T] -> (im2col [B,F,T,64] dtype, pyramid [B,F,T,4] f32)."""
    _dev(x, y)
    B, F, T = x.shape[0], x.shape[-2], x.shape[-1]
    col = torch.empty(B, F, T, 64, device=x.device, dtype=dtype)
    pyr = torch.empty(B, F, T, 4, device=x.device, dtype=torch.float32)
    _lib.call("snrse_input_pack", x.data_ptr(), y.data_ptr(), B, F, T, col.data_ptr(), pyr.data_ptr(),
              code(dtype), _stream())
    return col, pyr


def _row_seeds(row_seeds, B, dev):
    """Row seeds as the kernels read them: a contiguous int64 [B] tensor on `dev` (the bits of the uint64 keys)."""
    if not torch.is_tensor(row_seeds):
        row_seeds = torch.tensor([int(v) for v in row_seeds], dtype=torch.int64)
    if row_seeds.dtype != torch.int64 or row_seeds.numel() != B:
        raise ValueError(f"snrse: row_seeds must be {B} int64 values, one per batch row")
    return row_seeds.to(dev).contiguous()


def _noise_key(seed, row_seeds, B, dev):
    """How a noise op keys its draws -> (entry suffix, key argument, tensor to keep until the launch is issued):
    "" and the batch-keyed seed as a uint64, or "_rs" and the pointer to the row seeds.  The two entries of an op
    take the key in the same position (_lib.SIGNATURES)."""
    if row_seeds is None:
        return "", int(seed) & (2**64 - 1), None
    rs = _row_seeds(row_seeds, B, dev)
    return "_rs", rs.data_ptr(), rs


def score_update(pyr, out_w, out_b, t, score_mode, x, y=None, coef=None, noise=None, seed=0, offset=0,
                 want_score=False, x_out=None, xmean_out=None, row_seeds=None):
    """Output head + score + optional SDE step.  Returns (x_out, x_mean, score).  pyr: float32, or bfloat16 (the
    library reads any other 16-bit pattern as bf16, so a float16 pyramid is refused here).  row_seeds (int64 [B],
    device): row b draws Philox(row_seeds[b], offset * HW + e) with `offset` the draw index, instead of the
    batch-keyed Philox(seed, offset + index)."""
    if pyr.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"snrse: score_update takes a float32 or bfloat16 pyramid, got {pyr.dtype}")
    _dev(pyr, out_w, out_b, t, x, y, coef, noise)
    B = x.shape[0]
    HW = x.shape[-2] * x.shape[-1]
    score = torch.empty_like(x) if want_score else None
    if coef is not None:
        x_out = torch.empty_like(x) if x_out is None else x_out
        xmean_out = torch.empty_like(x) if xmean_out is None else xmean_out
    else:
        x_out = xmean_out = None
    sfx, key, _keep = _noise_key(seed, row_seeds, B, x.device)
    _lib.call("snrse_score_update" + sfx, pyr.data_ptr(), int(pyr.dtype == torch.float32), out_w.data_ptr(),
              out_b.data_ptr(), t.data_ptr(), int(score_mode), B, HW, x.data_ptr(), _ptr(y), _ptr(noise), key,
              int(offset), _ptr(coef), _ptr(x_out), _ptr(xmean_out), _ptr(score), _stream())
    return x_out, xmean_out, score


def sde_update(x, coef, y=None, score=None, noise=None, seed=0, offset=0, x_out=None, xmean_out=None,
               row_seeds=None):
    _dev(x, coef, y, score, noise)
    B = x.shape[0]
    HW = x.shape[-2] * x.shape[-1]
    x_out = torch.empty_like(x) if x_out is None else x_out
    xmean_out = torch.empty_like(x) if xmean_out is None else xmean_out
    sfx, key, _keep = _noise_key(seed, row_seeds, B, x.device)
    _lib.call("snrse_sde_update" + sfx, x.data_ptr(), _ptr(y), _ptr(score), _ptr(noise), key, int(offset),
              coef.data_ptr(), B, HW, x_out.data_ptr(), xmean_out.data_ptr(), _stream())
    return x_out, xmean_out


def axpby_noise(coef, x=None, y=None, noise=None, seed=0, offset=0, like=None, row_seeds=None):
    ref = x if x is not None else (y if y is not None else like)
    _dev(coef, x, y, noise)
    B = ref.shape[0]
    HW = ref.shape[-2] * ref.shape[-1]
    out = torch.empty_like(ref)
    sfx, key, _keep = _noise_key(seed, row_seeds, B, ref.device)
    _lib.call("snrse_axpby_noise" + sfx, _ptr(x), _ptr(y), _ptr(noise), key, int(offset), coef.data_ptr(), B, HW,
              out.data_ptr(), _stream())
    return out


class Lengths:
    """The valid lengths of a ragged [B, Lstride] batch: `.host` (numpy int64 [B], what the checks read) and
    `.dev` (int32 [B] on the device, what the kernels read).  Built once per batch (as_lengths) so that the ops
    of one enhancement neither upload nor read them back again."""

    def __init__(self, host, dev):
        self.host, self.dev = host, dev

    def __len__(self):
        return len(self.host)


def as_lengths(lengths, B, Lstride, dev):
    """lengths (Lengths, a sequence / numpy / CPU tensor, or an integer device tensor, which costs one read-back)
    -> Lengths; every row must fit its buffer: 0 < L_b <= Lstride."""
    if not isinstance(lengths, Lengths):
        host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int64).reshape(-1)
        lengths = Lengths(host, torch.from_numpy(host.astype(np.int32)).to(dev))
    if len(lengths) != B:
        raise ValueError(f"snrse: {len(lengths)} lengths for a batch of {B} rows")
    bad = [int(i) for i in np.nonzero((lengths.host <= 0) | (lengths.host > Lstride))[0]]
    if bad:
        raise ValueError(f"snrse: lengths of rows {bad} are outside (0, {Lstride}], the row stride of the batch")
    if lengths.dev.device != dev:
        lengths = Lengths(lengths.host, lengths.dev.to(dev))
    return lengths


def energy_ratios(s_hat, s, n=None, lengths=None):
    """[B, L] f32 device waveforms -> [B, 3] f64 (SI-SDR, SI-SIR, SI-SAR) dB (utils.py:10-35);
    without n only SI-SDR (column 0) is defined (sgmse/util/other.py:71-75).  lengths: ragged batch, row b's
    dot products run over [0, L_b) and nothing past it is read."""
    B, L = s_hat.shape
    if s.shape != s_hat.shape or (n is not None and n.shape != s_hat.shape):
        raise ValueError("energy_ratios: s_hat, s, n must share one [B, L] shape")
    a = [t.to(torch.float32).contiguous() for t in (s_hat, s)]
    nn = None if n is None else n.to(torch.float32).contiguous()
    _dev(a[0], a[1], nn)
    out = torch.empty(B, 3, device=s_hat.device, dtype=torch.float64)
    if lengths is not None:
        ln = as_lengths(lengths, B, L, s_hat.device)
        _lib.call("snrse_energy_ratios_ragged", a[0].data_ptr(), a[1].data_ptr(), _ptr(nn), ln.dev.data_ptr(), B, L,
                  out.data_ptr(), _stream())
        return out
    _lib.call("snrse_energy_ratios", a[0].data_ptr(), a[1].data_ptr(), _ptr(nn), B, L, out.data_ptr(), _stream())
    return out


def absmax(sig, lengths=None):
    """[B, L] f32 -> [B] max |sig| per row (ragged: over [0, L_b))."""
    _dev(sig)
    B, L = sig.shape
    out = torch.empty(B, device=sig.device, dtype=torch.float32)
    if lengths is not None:
        ln = as_lengths(lengths, B, L, sig.device)
        _lib.call("snrse_absmax_ragged", sig.data_ptr(), ln.dev.data_ptr(), B, L, out.data_ptr(), _stream())
        return out
    _lib.call("snrse_absmax", sig.data_ptr(), B, L, out.data_ptr(), _stream())
    return out


_TAPS = {}  # (filter design, up, down, device) -> (phase-major taps on the device, half), built once


def cached_taps(design, up, down, dev):
    """design(up, down)'s filter (snrse.audio.resample_taps, stoi_resample_taps) as resample_poly takes a caller's
    cache: (phase-major taps on `dev`, half), built on first use."""
    key = (design, up, down, dev)
    if key not in _TAPS:
        pm, half = phase_major_taps(design(up, down), up)
        _TAPS[key] = (torch.from_numpy(pm).to(dev), half)
    return _TAPS[key]


def phase_major_taps(w, up):
    """Filter w (float64 [2 half + 1], scipy's `window=` array) -> (h = up w phase-major [up, K] float32, half),
    K = ceil((2 half + 1) / up), [p, j] = h[p + j up] and 0 past the filter: snrse_resample_poly's layout.
    Computed in float64, rounded to float32 once."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if len(w) % 2 != 1:
        raise ValueError(f"snrse: resample_poly takes an odd number of taps, got {len(w)}")
    half = (len(w) - 1) // 2
    K = (2 * half + up) // up
    h = np.zeros(up * K, np.float64)
    h[:len(w)] = up * w
    return np.ascontiguousarray(h.reshape(K, up).T).astype(np.float32), half


def resample_poly(x, up, down, lengths=None, taps=None):
    """Rational polyphase FIR resampling of a ragged batch: x [B, stride_in] f32 on the device, row b valid on
    [0, L_b) (lengths: a sequence / numpy / tensor, None = whole rows; L_b = 0 is allowed) -> (y [B, stride_out]
    f32, out_lengths [B] int32), both on the device, n_out_b = ceil(L_b up / down), stride_out their maximum and
    y zero from n_out_b on.  The arithmetic of scipy.signal.resample_poly(x, up, down, window=taps,
    padtype='constant') in fp32; taps None is scipy's default filter (snrse.audio.resample_taps), cached on the
    device per ratio; taps may also be a caller's cached (phase_major_taps on the device, half) pair, used as it
    is.  up / down is reduced first; equal, the rows are copied.  One launch, no read-back (one for
    lengths given as a device tensor)."""
    _dev(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError("snrse: resample_poly takes a [B, L] float32 batch")
    B, Lin = x.shape
    up, down = int(up), int(down)
    if up <= 0 or down <= 0 or B <= 0:
        raise ValueError(f"snrse: resample_poly needs rows and up, down > 0 (got {B} rows, {up} / {down})")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if lengths is None:
        host = np.full(B, Lin, np.int64)
    else:
        host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int64).reshape(-1)
    if len(host) != B or (host < 0).any() or (host > Lin).any():
        raise ValueError(f"snrse: resample_poly needs {B} lengths inside [0, {Lin}], the row stride of the batch")
    out_host = -((-host * up) // down)
    if out_host.max(initial=0) >= 2 ** 31:
        raise ValueError("snrse: a resampled row would have 2^31 samples or more")
    out_dev = torch.from_numpy(out_host.astype(np.int32)).to(x.device)
    y = torch.empty(B, int(out_host.max()), device=x.device, dtype=torch.float32)
    if y.shape[1] == 0:
        return y, out_dev
    ln_dev = torch.from_numpy(host.astype(np.int32)).to(x.device)
    tp, half = None, 0
    if (up, down) != (1, 1):
        if taps is None:
            from .audio import resample_taps
            tp, half = cached_taps(resample_taps, up, down, x.device)
        elif isinstance(taps, tuple):  # (phase-major taps on the device, half): a caller's own cache, used as it is
            tp, half = taps
        else:
            pm, half = phase_major_taps(taps.cpu().numpy() if torch.is_tensor(taps) else taps, up)
            tp = torch.from_numpy(pm).to(x.device)
    _lib.call("snrse_resample_poly", _ptr(x) if Lin else None, ln_dev.data_ptr(), B, Lin, up, down, half, _ptr(tp),
              y.data_ptr(), y.shape[1], _stream())
    return y, out_dev


def _host_lengths(what, lengths, B, lo, hi):
    host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int64).reshape(-1)
    if len(host) != B or (host < lo).any() or (host > hi).any():
        raise ValueError(f"snrse: {what} needs {B} lengths inside [{lo}, {hi}]")
    return host


def band_gain(u, x, lengths, floor_db=30.0):
    """The "follow" policy's gain frames (snrse_band_gain; the definition stands in include/snrse.h): u the 16 kHz
    rows the network saw, x its results, [B, stride] f32 on the device, row b valid on [0, L_b), 256 <= L_b <=
    stride -> (g_s [B, Tmax] f32, frames [B] int32), both on the device, T_b = 1 + L_b // 128 and Tmax their
    maximum; g_s is zero from T_b on.  floor_db >= 0: the most the band is attenuated.  No read-back."""
    _dev(u, x)
    if u.dim() != 2 or u.dtype != torch.float32 or x.dtype != torch.float32 or u.shape != x.shape:
        raise TypeError("snrse: band_gain takes two [B, L] float32 batches of one shape")
    B, stride = u.shape
    floor_db = float(floor_db)
    if not (floor_db >= 0.0) or not math.isfinite(floor_db):
        raise ValueError(f"snrse: band_gain needs a finite floor_db >= 0, got {floor_db}")
    host = _host_lengths("band_gain (the STFT's reflect padding)", lengths, B, 256, stride)
    frames = 1 + host // 128
    Tmax = int(frames.max())
    ln = torch.from_numpy(host.astype(np.int32)).to(u.device)
    energies = torch.empty(B, 2, Tmax, device=u.device, dtype=torch.float64)
    gains = torch.empty(B, Tmax, device=u.device, dtype=torch.float32)
    _lib.call("snrse_band_gain", u.data_ptr(), x.data_ptr(), ln.data_ptr(), B, stride, Tmax,
              10.0 ** (-floor_db / 20.0), energies.data_ptr(), gains.data_ptr(), _stream())
    return gains, torch.from_numpy(frames.astype(np.int32)).to(u.device)


def resample_mix(x, u, y, len16, lenR, rate, gain, frames=None):
    """The enhanced 16 kHz rows brought to `rate` > 16000 with the band above 8 kHz of the recordings mixed back in
    (snrse_resample_mix; the definition stands in include/snrse.h): out = U(x) + g (y - U(u)).  x, u [B, stride16]
    f32 with len16 [B]; y [B, strideR] f32 with lenR [B] (lenR_b <= ceil(len16_b rate / 16000): a recording is no
    longer than its 16 kHz version brought back up), all on the device; gain: a constant in [0, 1], or the
    frames [B, Tmax] f32 on the device that band_gain returns, with frames [B] (None: 1 + len16 // 128) -> out
    [B, strideR] f32, zero from lenR_b on.  The project's default 16 k -> rate filter.  One launch, no read-back."""
    _dev(x, u, y)
    for t in (x, u, y):
        if t.dim() != 2 or t.dtype != torch.float32:
            raise TypeError("snrse: resample_mix takes [B, L] float32 batches")
    if x.shape != u.shape or y.shape[0] != x.shape[0]:
        raise ValueError(f"snrse: resample_mix takes x, u of one shape and y of as many rows, got {tuple(x.shape)}, "
                         f"{tuple(u.shape)}, {tuple(y.shape)}")
    from .audio import MODEL_RATE, rational, resample_taps
    B, s16 = x.shape
    sR = y.shape[1]
    rate = int(rate)
    if rate <= MODEL_RATE:
        raise ValueError(f"snrse: resample_mix keeps the band above {MODEL_RATE // 2} Hz of rates above {MODEL_RATE}, "
                         f"got {rate}")
    if B <= 0 or s16 <= 0 or sR <= 0:
        raise ValueError("snrse: resample_mix needs rows and samples")
    h16 = _host_lengths("resample_mix (len16)", len16, B, 0, s16)
    hR = _host_lengths("resample_mix (lenR)", lenR, B, 0, sR)
    up, down = rational(MODEL_RATE, rate)
    bad = [int(i) for i in np.nonzero(hR > -((-h16 * up) // down))[0]]
    if bad:
        raise ValueError(f"snrse: resample_mix rows {bad} are longer at {rate} Hz than their 16 kHz signals brought "
                         f"back up (lenR <= ceil(len16 {up} / {down}))")
    tp, half = cached_taps(resample_taps, up, down, x.device)
    gp, fp, Tmax, gc = None, None, 0, 0.0
    if torch.is_tensor(gain):
        _dev(gain)
        if gain.dim() != 2 or gain.dtype != torch.float32 or gain.shape[0] != B or gain.shape[1] < 1:
            raise ValueError(f"snrse: resample_mix takes gain frames [B, Tmax] float32, got {tuple(gain.shape)}")
        gp, Tmax = gain, gain.shape[1]
        fh = _host_lengths("resample_mix (frames)", 1 + h16 // 128 if frames is None else frames, B, 1, Tmax)
        fp = torch.from_numpy(fh.astype(np.int32)).to(x.device)
    else:
        gc = float(gain)
        if not 0.0 <= gc <= 1.0:
            raise ValueError(f"snrse: resample_mix takes a constant gain inside [0, 1], got {gain}")
    l16 = torch.from_numpy(h16.astype(np.int32)).to(x.device)
    lR = torch.from_numpy(hR.astype(np.int32)).to(x.device)
    out = torch.empty(B, sR, device=x.device, dtype=torch.float32)
    _lib.call("snrse_resample_mix", x.data_ptr(), u.data_ptr(), l16.data_ptr(), s16, y.data_ptr(), lR.data_ptr(), sR,
              B, up, down, half, tp.data_ptr(), _ptr(gp), _ptr(fp), Tmax, gc, out.data_ptr(), _stream())
    return out


def _i32(v, dev, shape=None):
    """A table of integers (sequence / numpy, or an int32 tensor already on `dev`) -> contiguous int32 on `dev`."""
    if torch.is_tensor(v) and v.dtype == torch.int32 and v.device == dev:
        t = v.contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(v.cpu() if torch.is_tensor(v) else v, dtype=np.int32)))
        t = t.to(dev)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"snrse: a table of shape {tuple(t.shape)} where {tuple(shape)} is expected")
    return t


def window_gather(src, lengths, table, W):
    """Cut windows out of a ragged batch of recordings: src [R, stride] f32 on the device with lengths [R]; table
    [nwin, 3] = (source row, start, length <= W) per window -> [nwin, W] f32, row j holding
    src[row_j, start_j : start_j + length_j] and zeros after it (snrse_window_gather).  Nothing at or past a
    recording's length is read.  The tables may be sequences / numpy (uploaded here) or int32 device tensors."""
    _dev(src)
    if src.dim() != 2 or src.dtype != torch.float32 or not src.is_contiguous():
        raise TypeError("snrse: window_gather takes a contiguous [R, stride] float32 batch")
    R, stride = src.shape
    tb = _i32(table, src.device)
    if tb.dim() != 2 or tb.shape[1] != 3 or tb.shape[0] < 1:
        raise ValueError(f"snrse: window_gather takes a [nwin, 3] table, got {tuple(tb.shape)}")
    ln = _i32(lengths, src.device, (R,))
    out = torch.empty(tb.shape[0], int(W), device=src.device, dtype=torch.float32)
    _lib.call("snrse_window_gather", src.data_ptr(), ln.data_ptr(), R, stride, tb.data_ptr(), tb.shape[0], int(W),
              out.data_ptr(), _stream())
    return out


def fade_table(V, dev):
    """snrse.longform.fade_table(V) on the device (fp64 on the host, rounded to fp32 once, cached per V)."""
    key = ("fade", int(V), dev)
    if key not in _TAPS:
        from .longform import fade_table as host_table
        _TAPS[key] = torch.from_numpy(host_table(V).astype(np.float32)).to(dev)
    return _TAPS[key]


def window_merge(win, starts, first, lengths, V, silent=None, stride_out=None, fade=None):
    """Join window results into their recordings (snrse_window_merge; the rule stands in include/snrse.h): win
    [nwin, W] f32 on the device, starts [nwin], first [R + 1] (recording r owns windows first[r] .. first[r + 1] - 1),
    lengths [R], silent [nwin] bool / uint8 or None (a flagged window counts as zeros and is not read), fade the
    [V] f32 table on the device (None: fade_table(V)) -> [R, stride_out] f32, stride_out default max(lengths), zero
    past each length.  One launch, no read-back."""
    _dev(win)
    if win.dim() != 2 or win.dtype != torch.float32 or not win.is_contiguous():
        raise TypeError("snrse: window_merge takes a contiguous [nwin, W] float32 batch")
    nwin, W = win.shape
    V = int(V)
    if V < 1 or 4 * V > W:
        raise ValueError(f"snrse: window_merge needs 0 < 4 V <= W, got V = {V}, W = {W}")
    dev = win.device
    fs = _i32(first, dev)
    R = fs.numel() - 1
    if R < 1:
        raise ValueError("snrse: window_merge takes first offsets of R + 1 >= 2 entries")
    st, ln = _i32(starts, dev, (nwin,)), _i32(lengths, dev, (R,))
    if silent is None:
        sl = torch.zeros(nwin, dtype=torch.uint8, device=dev)
    else:
        sl = torch.as_tensor(silent).to(dev).ne(0).to(torch.uint8).contiguous()
        if sl.shape != (nwin,):
            raise ValueError(f"snrse: {tuple(sl.shape)} silence flags for {nwin} windows")
    if fade is None:
        fade = fade_table(V, dev)
    if fade.shape != (V,) or fade.dtype != torch.float32 or fade.device != dev:
        raise ValueError(f"snrse: window_merge takes a [{V}] float32 fade table on the windows' device")
    if stride_out is None:
        stride_out = int(np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).max())
    out = torch.empty(R, max(int(stride_out), 1), device=dev, dtype=torch.float32)
    _lib.call("snrse_window_merge", win.data_ptr(), nwin, W, st.data_ptr(), sl.data_ptr(), fs.data_ptr(),
              ln.data_ptr(), R, fade.contiguous().data_ptr(), V, out.data_ptr(), out.shape[1], _stream())
    return out


def estoi(x, y, lengths=None, fs=16000, return_info=False):
    """ESTOI (Jensen & Taal 2016 with pystoi's conventions; the definition stands at snrse_estoi in
    include/snrse.h) of a ragged batch: x clean, y processed, [B, L] f32 on the device at `fs` Hz, row b valid on
    [0, L_b) (lengths None = whole rows) -> [B] f64 on the device.  fs != 10000: both signals are first resampled
    to 10 kHz by resample_poly with ESTOI's own filter (cached on the device per ratio), then one snrse_estoi call.
    Rows with fewer than 30 frames after the silent-frame removal give 1e-5.  return_info: also the [B, 2] int32
    tensor (K kept frames, S segments; S = 0 marks the 1e-5 rows).  No read-back."""
    if x.dim() != 2 or x.shape != y.shape or x.dtype != torch.float32 or y.dtype != torch.float32:
        raise TypeError("snrse: estoi takes two [B, L] float32 batches of one shape")
    B, L = x.shape
    if B <= 0 or L <= 0:
        raise ValueError(f"snrse: estoi needs a non-empty batch, got [{B}, {L}]")
    x, y = x.contiguous(), y.contiguous()
    _dev(x, y)
    if lengths is None:
        lengths = np.full(B, L, np.int64)
    ln = as_lengths(lengths, B, L, x.device)
    ln_dev = ln.dev
    from .audio import STOI_RATE, rational, stoi_resample_taps
    up, down = rational(int(fs), STOI_RATE)
    if (up, down) != (1, 1):
        taps = cached_taps(stoi_resample_taps, up, down, x.device)
        x, ln_dev = resample_poly(x, up, down, lengths=ln.host, taps=taps)
        y, _ = resample_poly(y, up, down, lengths=ln.host, taps=taps)
        L = x.shape[1]
    nbytes = int(_lib.load().snrse_estoi_workspace(B, L))
    work = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    out = torch.empty(B, device=x.device, dtype=torch.float64)
    info = torch.empty(B, 2, device=x.device, dtype=torch.int32)
    _lib.call("snrse_estoi", x.data_ptr(), y.data_ptr(), ln_dev.data_ptr(), B, L, work.data_ptr(), nbytes,
              out.data_ptr(), info.data_ptr(), _stream())
    return (out, info) if return_info else out


def _ragged_rows(what, x, lengths):
    """The checks the loudness ops share -> (B, stride, host lengths int64); L_b = 0 is allowed."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError(f"snrse: {what} takes a [B, L] float32 batch")
    _dev(x)
    B, L = x.shape
    if B <= 0 or L <= 0:
        raise ValueError(f"snrse: {what} needs a non-empty batch, got [{B}, {L}]")
    if lengths is None:
        return B, L, np.full(B, L, np.int64)
    return B, L, _host_lengths(what, lengths.host if isinstance(lengths, Lengths) else lengths, B, 0, L)


_KW_TABLES = {}  # (rates, groups, device) -> the device tables of loudness(), built once per batch layout


def kweight_geometry():
    """(chunk, block, group) of snrse_kweight_sums: samples per chunk, chunks per workgroup, chunks per scan group
    -- the lengths at which its kernels change path."""
    L = _lib.load()
    return int(L.snrse_kweight_chunk()), int(L.snrse_kweight_block()), int(L.snrse_kweight_group())


def loudness(x, lengths=None, rate=16000, groups=None, return_info=False):
    """Integrated loudness (ITU-R BS.1770-4 as stated at snrse_kweight_sums in include/snrse.h; every channel has
    weight 1) of a ragged batch: x [B, L] f32 on the device, row b valid on [0, L_b) (lengths None = whole rows,
    L_b = 0 allowed), at `rate` Hz (a scalar, or one value per row) -> [G] f64 LUFS on the device, -inf for a file
    without a block above the absolute gate.  groups: the file of each row (host integers 0, 0, 1, ..: rows of a
    file adjacent, one rate per file; a file's channels are measured together), None = every row is a file.
    return_info: also a dict: sums [B, Nmax] f64 (the sub-block energies), blocks / kept_abs / kept_rel [G] int32
    and margin [G] f64 (the least distance in LU of a block from the gate it was compared with) on the device, nsub
    and n100 [B] int64 on the host.  Seven launches, no read-back."""
    B, L, host = _ragged_rows("loudness", x, lengths)
    dev = x.device
    rates = (int(rate),) * B if np.ndim(rate) == 0 else tuple(int(r) for r in np.asarray(rate).reshape(-1))
    if len(rates) != B:
        raise ValueError(f"snrse: loudness got {len(rates)} rates for {B} rows")
    grp = tuple(range(B)) if groups is None else tuple(int(g) for g in np.asarray(groups).reshape(-1))
    Cc, _, Sg = kweight_geometry()
    key = (rates, grp, dev)
    if key not in _KW_TABLES:
        from . import loudness as _ld
        if len(grp) != B or grp[0] != 0 or any(b - a not in (0, 1) for a, b in zip(grp, grp[1:])):
            raise ValueError("snrse: loudness groups are one file index per row, 0, 0, 1, ..: ascending without gaps")
        if any(ga == gb and ra != rb for ga, gb, ra, rb in zip(grp, grp[1:], rates, rates[1:])):
            raise ValueError("snrse: the rows of a file share one rate")
        n100 = np.array([_ld.n100(r) for r in rates], np.int64)
        if (n100 < Cc).any():
            raise ValueError(f"snrse: loudness needs sample rates of at least {10 * Cc - 5} Hz")
        par = np.stack([_ld.kernel_params(r, Cc, Sg) for r in rates])
        if len(_KW_TABLES) >= 64:
            _KW_TABLES.clear()
        _KW_TABLES[key] = (torch.from_numpy(par).to(dev), n100,
                           torch.from_numpy(np.stack([n100, np.array(grp, np.int64)]).astype(np.int32)).to(dev))
    par, n100, tab = _KW_TABLES[key]
    G = grp[-1] + 1
    nsub = host // n100
    Nmax = max(int(nsub.max()), 1)
    lt = torch.from_numpy(np.stack([host, nsub]).astype(np.int32)).to(dev)
    nbytes = int(_lib.load().snrse_kweight_workspace(B, L))
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    sums = torch.empty(B, Nmax, device=dev, dtype=torch.float64)
    _lib.call("snrse_kweight_sums", x.data_ptr(), lt[0].data_ptr(), B, L, par.data_ptr(), tab[0].data_ptr(),
              work.data_ptr(), nbytes, sums.data_ptr(), Nmax, _stream())
    out = torch.empty(G, device=dev, dtype=torch.float64)
    counts = torch.empty(G, 3, device=dev, dtype=torch.int32)
    margin = torch.empty(G, device=dev, dtype=torch.float64)
    _lib.call("snrse_loudness_gate", sums.data_ptr(), Nmax, lt[1].data_ptr(), tab[0].data_ptr(), tab[1].data_ptr(), B,
              G, out.data_ptr(), counts.data_ptr(), margin.data_ptr(), _stream())
    if not return_info:
        return out
    return out, {"sums": sums, "blocks": counts[:, 0], "kept_abs": counts[:, 1], "kept_rel": counts[:, 2],
                 "margin": margin, "nsub": nsub, "n100": n100}


def peak_oversampled(x, lengths=None):
    """[B, L] f32 on the device -> [B] f32: max |.| of each row oversampled 4x by resample_poly's default filter
    (audio.resample_taps(4, 1), 81 taps), the bits of resample_poly(x, 4, 1, lengths)[0].abs() maximised over
    [0, 4 L_b) without that signal being written; a NaN is skipped as absmax skips it.  A 4x peak, not the true
    peak of BS.1770 Annex 2 (another filter).  One launch, no read-back."""
    B, L, host = _ragged_rows("peak_oversampled", x, lengths)
    from .audio import resample_taps
    tp, half = cached_taps(resample_taps, 4, 1, x.device)
    ln = torch.from_numpy(host.astype(np.int32)).to(x.device)
    out = torch.empty(B, device=x.device, dtype=torch.float32)
    _lib.call("snrse_peak_oversampled", x.data_ptr(), ln.data_ptr(), B, L, 4, half, tp.data_ptr(), out.data_ptr(),
              _stream())
    return out


def gain_to_pcm16(x, gain, lengths=None, floats=False):
    """x [B, L] f32 and gain [B] (f32 or f64), both on the device -> int16 [B, L] = clip(rint(fl32(fl32(gain_b) x)
    32768), -32768, 32767), exactly what audio.write_wav(bits=16) makes of the float32 product, zero from L_b on;
    floats: (int16, that product as f32 [B, L]).  One launch, no read-back."""
    B, L, host = _ragged_rows("gain_to_pcm16", x, lengths)
    if not torch.is_tensor(gain) or gain.dtype not in (torch.float32, torch.float64) or gain.shape != (B,):
        raise TypeError(f"snrse: gain_to_pcm16 takes a [{B}] float32 or float64 gain")
    _dev(gain)
    gain = gain.to(torch.float64)
    ln = torch.from_numpy(host.astype(np.int32)).to(x.device)
    q = torch.empty(B, L, device=x.device, dtype=torch.int16)
    f = torch.empty_like(x) if floats else None
    _lib.call("snrse_gain_to_pcm16", x.data_ptr(), ln.data_ptr(), B, L, gain.data_ptr(), q.data_ptr(), _ptr(f),
              _stream())
    return (q, f) if floats else q


def _snr_pair(what, clean, noise, lengths):
    """The checks the dataset-preparation ops share -> (B, stride, Lengths)."""
    if clean.dim() != 2 or clean.shape != noise.shape or clean.dtype != torch.float32 or noise.dtype != torch.float32:
        raise TypeError(f"snrse: {what} takes two [B, L] float32 batches of one shape")
    B, L = clean.shape
    if B <= 0 or L <= 0:
        raise ValueError(f"snrse: {what} needs a non-empty batch, got [{B}, {L}]")
    _dev(clean, noise)
    if lengths is None:
        lengths = np.full(B, L, np.int64)
    return B, L, as_lengths(lengths, B, L, clean.device)


def snr_window(fs):
    """Samples of the 100-ms analysis window at `fs` Hz: int(fs * 0.1), as the definition writes it."""
    W = int(fs * 0.1)
    if W < 1:
        raise ValueError(f"snrse: a sample rate of {fs} Hz leaves no 100-ms window")
    return W


def _snr_targets(snr_db, B, dev):
    if torch.is_tensor(snr_db):
        t = snr_db.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if t.numel() != B:
            raise ValueError(f"snrse: {t.numel()} snr_db targets for a batch of {B} rows")
        return t
    return torch.full((B,), float(snr_db), device=dev, dtype=torch.float64)


def _active_analysis(clean, noise, ln, W, snr_db):
    """-> (fin [B, 5] f64 = clean_rms, noise_rms, active windows, Pearson, gain; max |noise| [B] f32): the two
    analysis launches, no read-back."""
    B, L = clean.shape
    dev = clean.device
    nW = -(-L // W)
    P = int(_lib.load().snrse_active_windows_per_block())
    wsums = torch.empty(B, nW, 2, device=dev, dtype=torch.float64)
    partials = torch.empty(B, -(-nW // P), 5, device=dev, dtype=torch.float64)
    nmax = torch.empty(B, device=dev, dtype=torch.float32)
    fin = torch.empty(B, 5, device=dev, dtype=torch.float64)
    _lib.call("snrse_active_window_sums", clean.data_ptr(), noise.data_ptr(), ln.dev.data_ptr(), B, L, W,
              wsums.data_ptr(), partials.data_ptr(), nmax.data_ptr(), _stream())
    _lib.call("snrse_active_finalize", wsums.data_ptr(), partials.data_ptr(), nmax.data_ptr(), ln.dev.data_ptr(), B, L,
              W, _snr_targets(snr_db, B, dev).data_ptr(), fin.data_ptr(), _stream())
    return fin, nmax


def _active_info(fin, nmax, ln, W):
    return {"active_windows": fin[:, 2].to(torch.int64), "windows": torch.from_numpy(-(-ln.host // W)),
            "corr": fin[:, 3], "gain": fin[:, 4], "max_noise": nmax}


def active_rms(clean, noise, lengths=None, fs=16000, snr_db=-5.0, return_info=False):
    """Active-level analysis of clean / noise pairs (the definition stands at snrse_active_window_sums in
    include/snrse.h): [B, L] f32 on the device at `fs` Hz, row b valid on [0, L_b) (lengths None = whole rows) ->
    [B, 2] f64 on the device, (clean_rms, noise_rms) over the 100-ms windows whose NOISE is active; both are eps
    where no window is.  return_info: also a dict of device tensors: active_windows [B] int64, corr [B] f64 (the
    Pearson coefficient of the whole rows), gain [B] f64 (what brings the pair to snr_db dB active SNR; snr_db a
    scalar or a [B] tensor), max_noise [B] f32, and windows [B] int64 on the host.  Two launches, no read-back."""
    B, L, ln = _snr_pair("active_rms", clean, noise, lengths)
    W = snr_window(fs)
    fin, nmax = _active_analysis(clean, noise, ln, W, snr_db)
    rms = fin[:, :2].contiguous()
    return (rms, _active_info(fin, nmax, ln, W)) if return_info else rms


def snr_mix(clean, noise, gain, lengths=None):
    """noise' = (float)gain_b noise and noisy = fma((float)gain_b, noise, clean) per row (snrse_snr_mix): [B, L] f32
    batches and gain [B] f64, all on the device -> (noise', noisy [B, L] f32, zero past each length; max |noisy|
    [B] f32)."""
    B, L, ln = _snr_pair("snr_mix", clean, noise, lengths)
    gain = gain.to(device=clean.device, dtype=torch.float64)
    if gain.dim() != 1 or gain.numel() != B or gain.stride(0) < 1:
        raise ValueError(f"snrse: snr_mix takes a [{B}] gain")
    n1, y = torch.empty_like(clean), torch.empty_like(clean)
    ymax = torch.empty(B, device=clean.device, dtype=torch.float32)
    _lib.call("snrse_snr_mix", clean.data_ptr(), noise.data_ptr(), ln.dev.data_ptr(), B, L, gain.data_ptr(),
              int(gain.stride(0)), n1.data_ptr(), y.data_ptr(), ymax.data_ptr(), _stream())
    return n1, y, ymax


def scale_to_pcm16(clean, noise, noisy, peak, lengths=None, floats=True, pcm16=True):
    """The clip guard and the 16-bit conversion (snrse_scale_to_pcm16): three [B, L] f32 batches and peak [B] f32
    (max |noisy| per row) on the device -> (floats, pcm, scale): scale [B] f64 = peak > 0.99 ? (0.99 - eps) / peak
    : 1; floats = the three signals times (float)scale as new f32 tensors, pcm = those as int16 exactly as
    audio.write_wav(bits=16) converts them; either is None when not asked for.  One launch, no read-back."""
    B, L, ln = _snr_pair("scale_to_pcm16", clean, noise, lengths)
    _dev(noisy, peak)
    if noisy.shape != clean.shape or noisy.dtype != torch.float32 or peak.shape != (B,) or peak.dtype != torch.float32:
        raise TypeError("snrse: scale_to_pcm16 takes three [B, L] float32 batches and a [B] float32 peak")
    dev = clean.device
    of = [torch.empty_like(clean) for _ in range(3)] if floats else [None] * 3
    oq = [torch.empty(B, L, device=dev, dtype=torch.int16) for _ in range(3)] if pcm16 else [None] * 3
    scale = torch.empty(B, device=dev, dtype=torch.float64)
    _lib.call("snrse_scale_to_pcm16", clean.data_ptr(), noise.data_ptr(), noisy.data_ptr(), ln.dev.data_ptr(), B, L,
              peak.data_ptr(), *[_ptr(t) for t in of], *[_ptr(t) for t in oq], scale.data_ptr(), _stream())
    return (tuple(of) if floats else None), (tuple(oq) if pcm16 else None), scale


def snr_remix(clean, noise, lengths=None, fs=16000, snr_db=-5.0, pcm16=False):
    """Remix clean / noise pairs to snr_db dB active SNR (snr_db a scalar or a [B] tensor): the analysis of
    active_rms, noise' = gain noise, noisy = clean + noise', and the clip guard (rows whose max |noisy| exceeds 0.99
    have all three signals scaled to a peak of 0.99 - eps) -> (clean', noise', noisy, info), [B, L] on the device
    and zero past each length: float32, or with pcm16 int16 as audio.write_wav(bits=16) would write those floats.
    info: active_rms's dict plus rms [B, 2] f64 (of the INPUTS), peak [B] f32 (max |noisy| before the guard) and
    scale [B] f64 (the guard's factor; the outputs' active RMS are rms[:, 0] scale and rms[:, 1] gain scale).
    Four launches, no read-back."""
    B, L, ln = _snr_pair("snr_remix", clean, noise, lengths)
    W = snr_window(fs)
    fin, nmax = _active_analysis(clean, noise, ln, W, snr_db)
    n1, y, peak = snr_mix(clean, noise, fin[:, 4], lengths=ln)
    of, oq, scale = scale_to_pcm16(clean, n1, y, peak, lengths=ln, floats=not pcm16, pcm16=pcm16)
    info = _active_info(fin, nmax, ln, W)
    info.update(rms=fin[:, :2].contiguous(), peak=peak, scale=scale)
    return (*(oq if pcm16 else of), info)


def range_stats(t, peak=None, nonfinite=None, accumulate=False):
    """Range statistics of a contiguous device tensor whose leading dimension counts the rows (float32, float16,
    bfloat16, or complex64 read as interleaved floats): (peak [B] f32 = max |v| over the finite elements of each
    row, nonfinite [B] i32 = its number of inf / NaN elements) -- snrse_range_stats.  peak / nonfinite: slots to
    write; accumulate=True folds into their contents (max / saturating add) instead of overwriting them."""
    _dev(t, peak, nonfinite)
    if t.dim() < 1 or t.numel() == 0:
        raise ValueError("snrse: range_stats needs a non-empty tensor with a leading row dimension")
    B = t.shape[0]
    if t.dtype == torch.complex64:
        dt, per = F32, 2 * (t.numel() // B)
    else:
        dt, per = code(t.dtype), t.numel() // B
    if (peak is None or nonfinite is None) and accumulate:
        raise ValueError("snrse: range_stats(accumulate=True) folds into given peak / nonfinite slots")
    peak = torch.empty(B, device=t.device, dtype=torch.float32) if peak is None else peak
    nonfinite = torch.empty(B, device=t.device, dtype=torch.int32) if nonfinite is None else nonfinite
    if (peak.dtype, nonfinite.dtype) != (torch.float32, torch.int32) or peak.numel() != B or nonfinite.numel() != B:
        raise TypeError("snrse: range_stats slots are peak [B] float32 and nonfinite [B] int32")
    _lib.call("snrse_range_stats", t.data_ptr(), B, per, dt, peak.data_ptr(), nonfinite.data_ptr(),
              int(bool(accumulate)), _stream())
    return peak, nonfinite


_RK45_DT = {torch.float32: F32, torch.complex64: F32, torch.float64: _lib.F64, torch.complex128: _lib.F64}


def _rk45_rows(y):
    """(B, doubles per row) of a contiguous float64 / complex128 [B, ...] state."""
    if y.dtype not in (torch.float64, torch.complex128) or not y.is_contiguous() or y.dim() < 1 or y.numel() == 0:
        raise TypeError("snrse: the RK45 kernels take a contiguous, non-empty float64 / complex128 [B, ...] state")
    B = y.shape[0]
    return B, (y.numel() // B) * (2 if y.is_complex() else 1)


def _rk45_stages(ks, coefs, like):
    """Stage tensors and coefficients as snrse_rk45_* take them: zero coefficients dropped (ode._lincomb), one
    dtype, the state's shape and complexness -> (pointer array, coefficient array, ns, dtype code, kept tensors)."""
    kept = [(k, float(c)) for k, c in zip(ks, coefs) if float(c) != 0.0]
    if len(kept) > 7:
        raise ValueError("snrse: at most 7 stages")
    for k, _ in kept:
        if (k.dtype not in _RK45_DT or k.dtype != kept[0][0].dtype or k.shape != like.shape
                or k.is_complex() != like.is_complex() or not k.is_contiguous()):
            raise TypeError("snrse: RK45 stages are contiguous tensors of the state's shape, all float32 / complex64 "
                            "or all float64 / complex128")
    _dev(like, *[k for k, _ in kept])
    ns = len(kept)
    ptrs = (C.c_void_p * max(ns, 1))(*[k.data_ptr() for k, _ in kept])
    cs = (C.c_double * max(ns, 1))(*[c for _, c in kept])
    return ptrs, cs, ns, (_RK45_DT[kept[0][0].dtype] if kept else _lib.F64), [k for k, _ in kept]


def rk45_combine(y, h, ks, coefs, want32=False):
    """out[b] = y[b] + h[b] * (sum_s coefs[s] ks[s][b]) in float64, stage order, every product and sum rounded on
    its own (snrse_rk45_combine).  y: float64 / complex128 [B, ...]; h: float64 [B] on the device; ks: float32 /
    complex64 or float64 / complex128 tensors shaped like y.  Returns (out, out32): out32 is out cast to
    float32 / complex64 when want32, else None."""
    B, n = _rk45_rows(y)
    if h.dtype != torch.float64 or h.numel() != B or not h.is_contiguous():
        raise TypeError(f"snrse: rk45_combine takes h as {B} contiguous float64 values")
    ptrs, cs, ns, dt, _keep = _rk45_stages(ks, coefs, y)
    _dev(y, h)
    out = torch.empty_like(y)
    out32 = torch.empty_like(y, dtype=torch.complex64 if y.is_complex() else torch.float32) if want32 else None
    _lib.call("snrse_rk45_combine", y.data_ptr(), h.data_ptr(), ptrs, cs, ns, dt, B, n, out.data_ptr(), _ptr(out32),
              _stream())
    return out, out32


def rk45_rownorm(vs, coefs, a, b2, rtol, atol, m=None):
    """[B] float64: sqrt(mean_e |m[b] sum_s coefs[s] vs[s][b, e]|^2 / (atol + rtol max(|a|, |b2|))^2) per row, the
    modulus complex when the state is (snrse_rk45_rownorm: block partials, then a fold in a fixed order -- the same
    bits on every launch).  m: float64 [B] on the device, or None for 1."""
    B, n = _rk45_rows(a)
    if b2.dtype != a.dtype or b2.shape != a.shape or not b2.is_contiguous():
        raise TypeError("snrse: rk45_rownorm takes a and b2 of one shape and dtype")
    if m is not None and (m.dtype != torch.float64 or m.numel() != B or not m.is_contiguous()):
        raise TypeError(f"snrse: rk45_rownorm takes m as {B} contiguous float64 values")
    ptrs, cs, ns, dt, _keep = _rk45_stages(vs, coefs, a)
    _dev(a, b2, m)
    bpr = _lib.load().snrse_rk45_rownorm_blocks(B, n)
    partial = torch.empty(B, bpr, device=a.device, dtype=torch.float64)
    out = torch.empty(B, device=a.device, dtype=torch.float64)
    _lib.call("snrse_rk45_rownorm", ptrs, cs, ns, dt, _ptr(m), a.data_ptr(), b2.data_ptr(), float(rtol), float(atol),
              int(a.is_complex()), B, n, partial.data_ptr(), out.data_ptr(), _stream())
    return out


def rk45_accept(mask, y, y_new, f, f_new):
    """In place, for the rows with mask[b] != 0 (int32 [B] on the device): y[b] <- y_new[b], f[b] <- f_new[b]; the
    other rows keep their bits (snrse_rk45_accept)."""
    B, n = _rk45_rows(y)
    if y_new.dtype != y.dtype or y_new.shape != y.shape or not y_new.is_contiguous():
        raise TypeError("snrse: rk45_accept takes y and y_new of one shape and dtype")
    if (f.dtype not in _RK45_DT or f_new.dtype != f.dtype or f.shape != y.shape or f_new.shape != y.shape
            or not (f.is_contiguous() and f_new.is_contiguous())):
        raise TypeError("snrse: rk45_accept takes f and f_new of the state's shape and one dtype")
    if mask.dtype != torch.int32 or mask.numel() != B or not mask.is_contiguous():
        raise TypeError(f"snrse: rk45_accept takes the mask as {B} contiguous int32 values")
    _dev(mask, y, y_new, f, f_new)
    fwords = (f.numel() // B) * f.element_size() // 4
    _lib.call("snrse_rk45_accept", mask.data_ptr(), y.data_ptr(), y_new.data_ptr(), 2 * n, f.data_ptr(),
              f_new.data_ptr(), fwords, B, _stream())


def stft(sig, in_scale=1.0, tpad=None, mode=1, in_div=None, lengths=None):
    """sig [B, L] f32 -> complex64 [B, 256, Tpad] of sig * in_scale / in_div[b].  lengths: ragged batch, row b
    reflects at its own L_b, has 1 + L_b // 128 frames and zeros after them; a row of 255 samples or fewer (too
    short to reflect, as torch.stft refuses it) or with more frames than tpad fails as the library's EINVAL does."""
    _dev(sig, in_div)
    B, L = sig.shape
    if lengths is not None:
        if sig.dtype != torch.float32 or not sig.is_contiguous():
            raise TypeError("snrse: a ragged stft takes a contiguous float32 [B, Lstride] buffer")
        ln = as_lengths(lengths, B, L, sig.device)
        tpad = 1 + int(ln.host.max()) // 128 if tpad is None else tpad
        bad = [int(i) for i in np.nonzero((ln.host <= 255) | (1 + ln.host // 128 > tpad))[0]]
        if bad:
            _lib.check(1, f"snrse_stft_ragged (rows {bad}: 255 < L_b and 1 + L_b // 128 <= Tpad = {tpad} must hold)")
        out = torch.empty(B, 256, tpad, device=sig.device, dtype=torch.complex64)
        _lib.call("snrse_stft_ragged", sig.data_ptr(), ln.dev.data_ptr(), B, L, _ptr(in_div), float(in_scale), tpad,
                  int(mode), out.data_ptr(), _stream())
        return out
    T = 1 + L // 128
    tpad = T if tpad is None else tpad
    out = torch.empty(B, 256, tpad, device=sig.device, dtype=torch.complex64)
    _lib.call("snrse_stft", sig.data_ptr(), B, L, _ptr(in_div), float(in_scale), tpad, int(mode), out.data_ptr(),
              _stream())
    return out


def istft(spec, length, mode=1, out_scale=None):
    """spec complex64 [B, 256, T] -> [B, length] f32 (* out_scale[b])."""
    _dev(spec, out_scale)
    B, Fq, T = spec.shape
    frames = torch.empty(B, T, 510, device=spec.device, dtype=torch.float32)
    out = torch.empty(B, length, device=spec.device, dtype=torch.float32)
    _lib.call("snrse_istft", spec.data_ptr(), B, T, length, int(mode), _ptr(out_scale), frames.data_ptr(),
              out.data_ptr(), _stream())
    return out


UPFIRDN_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: _lib.F16, torch.float64: _lib.F64}


def upfirdn2d(inp, kernel, up=1, down=1, pad=(0, 0)):
    """Reference-signature upfirdn2d (op/upfirdn2d.py:145-156) on [N, C, H, W]."""
    _dev(inp, kernel)
    N, Cc, H, W = inp.shape
    out = _upfirdn_raw(inp.reshape(N * Cc, H, W, 1), kernel, up, up, down, down, pad[0], pad[1], pad[0], pad[1])
    return out.view(N, Cc, out.shape[1], out.shape[2])


def _upfirdn_raw(x4, k, upx, upy, dnx, dny, px0, px1, py0, py1):
    """snrse_upfirdn2d on [major, H, W, minor] with per-axis factors and pads."""
    major, H, W, minor = x4.shape
    kh, kw = k.shape
    oh = (H * upy + py0 + py1 - kh) // dny + 1
    ow = (W * upx + px0 + px1 - kw) // dnx + 1
    out = torch.empty(major, oh, ow, minor, device=x4.device, dtype=x4.dtype)
    dt = UPFIRDN_DTYPES.get(x4.dtype)
    if dt is None:
        raise TypeError(f"upfirdn2d: unsupported dtype {x4.dtype} (float, double, half, bfloat16)")
    _lib.call("snrse_upfirdn2d", x4.contiguous().data_ptr(), out.data_ptr(), k.to(torch.float32).contiguous().data_ptr(),
              major, H, W, minor, kh, kw, upx, upy, dnx, dny, px0, px1, py0, py1, dt, _stream())
    return out


class _UpFirDn2d(torch.autograd.Function):
    """upfirdn2d with gradients, every direction through snrse_upfirdn2d -- the call pattern of the
    reference's UpFirDn2d / UpFirDn2dBackward (op/upfirdn2d.py:19-142): the input gradient is the op on
    the output gradient with the flipped kernel, up and down swapped and the transposed pads
    (kw - pad_x0 - 1, in_w up - out_w down + pad_x0 - up + 1, likewise in y); its own gradient is the
    forward op again."""

    @staticmethod
    def forward(ctx, x, kernel, up, down, pad):
        (upx, upy), (dnx, dny), (px0, px1, py0, py1) = up, down, pad
        N, C, H, W = x.shape
        kh, kw = kernel.shape
        out = _upfirdn_raw(x.reshape(N * C, H, W, 1), kernel, upx, upy, dnx, dny, px0, px1, py0, py1)
        oh, ow = out.shape[1], out.shape[2]
        ctx.save_for_backward(kernel)
        ctx.geom = (up, down, pad, (N, C, H, W), (oh, ow),
                    (kw - px0 - 1, W * upx - ow * dnx + px0 - upx + 1, kh - py0 - 1, H * upy - oh * dny + py0 - upy + 1))
        return out.view(N, C, oh, ow)

    @staticmethod
    def backward(ctx, g):
        (kernel,) = ctx.saved_tensors
        return _UpFirDn2dGrad.apply(g, kernel, ctx.geom), None, None, None, None


class _UpFirDn2dGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, kernel, geom):
        (upx, upy), (dnx, dny), _, (N, C, H, W), (oh, ow), (gx0, gx1, gy0, gy1) = geom
        gi = _upfirdn_raw(g.contiguous().reshape(N * C, oh, ow, 1), torch.flip(kernel, [0, 1]), dnx, dny, upx, upy,
                          gx0, gx1, gy0, gy1)
        ctx.save_for_backward(kernel)
        ctx.geom = geom
        return gi.view(N, C, H, W)

    @staticmethod
    def backward(ctx, gg):
        (kernel,) = ctx.saved_tensors
        (upx, upy), (dnx, dny), (px0, px1, py0, py1), (N, C, H, W), (oh, ow), _ = ctx.geom
        go = _upfirdn_raw(gg.contiguous().reshape(N * C, H, W, 1), kernel, upx, upy, dnx, dny, px0, px1, py0, py1)
        return go.view(N, C, oh, ow), None, None


def upfirdn2d_autograd(inp, kernel, up=1, down=1, pad=(0, 0)):
    """The reference's upfirdn2d(input, kernel, up, down, pad) (op/upfirdn2d.py:145-156) with its autograd
    (first and second derivatives w.r.t. the input), on the HIP op."""
    _dev(inp, kernel)
    return _UpFirDn2d.apply(inp, kernel, (up, up), (down, down), (pad[0], pad[1], pad[0], pad[1]))


def set_option(name: str, value: int):
    """Process-wide switch: the library's process default context and every live LaunchContext."""
    _lib.call("snrse_set_option", name.encode(), int(value))
    for c in list(_CONTEXTS):
        c.set_option(name, value)


def spec_transform(spec, direction):
    """'exponent' spec_fwd (direction 0) / spec_back (1) on a complex64 device tensor."""
    _dev(spec)
    out = torch.empty_like(spec)
    _lib.call("snrse_spec_transform", spec.data_ptr(), out.data_ptr(), spec.numel(), int(direction), _stream())
    return out


SNRNET_KEYS = ["conv5x5_1.weight", "conv5x5_1.bias", "conv3x3_1.weight", "conv3x3_1.bias", "convt_1.weight",
               "convt_2.weight", "convt_3.weight", "convt_4.weight", "convt_1.bias", "convt_2.bias", "convt_3.bias",
               "convt_4.bias"]


def pack_snrnet(sd, device):
    f = lambda k: sd[k].detach().to(device, torch.float32).contiguous()  # noqa: E731
    w = [f(k) for k in SNRNET_KEYS]
    wih = torch.stack([f("blstm.weight_ih_l0"), f("blstm.weight_ih_l0_reverse")]).contiguous()
    whh = torch.stack([f("blstm.weight_hh_l0"), f("blstm.weight_hh_l0_reverse")]).contiguous()
    bsum = torch.stack([f("blstm.bias_ih_l0") + f("blstm.bias_hh_l0"),
                        f("blstm.bias_ih_l0_reverse") + f("blstm.bias_hh_l0_reverse")]).contiguous()
    return w + [wih, bsum, whh, f("fc.weight").reshape(-1).contiguous(), f("fc.bias")]


def snrnet(spec, packed):
    """SNRNet on the raw complex STFT [B, 256, T] (T % 16 == 0) -> [B] in (0, 1)."""
    _dev(spec)
    B, _, T = spec.shape
    ws = torch.empty(int(_lib.load().snrse_snrnet_workspace(B, T)) // 4 + 1, device=spec.device, dtype=torch.float32)
    out = torch.empty(B, device=spec.device, dtype=torch.float32)
    _lib.call("snrse_snrnet", spec.data_ptr(), B, T, *[p.data_ptr() for p in packed], ws.data_ptr(), out.data_ptr(),
              _stream())
    return out
