"""The halo GEMM's register epilogue (conv_halo5_kernel, 16-bit outputs): which cout a lane stores where.

The kernel loads its weight rows permuted (ring row 16 jj + lrow holds cout n0 + 8 lrow + jj), so that a lane's
accumulators are 8 adjacent couts of a pixel and leave as one 16-B store, with bias / temb / Combine weights as per-lane
constants and the GroupNorm statistics reduced over the lanes.  test_gpu_halo5_phase.py holds every element of two
epilogue configurations to the fp32 bound; here

* every epilogue flag combination the dispatcher specialises (TEMB|STATS, RES|STATS, STATS, TEMB, each with and without
  non-temporal stores; with a fused shortcut STATS and COMB|STATS) and the run-time form (h5_specialise off) is held to
  the same per-element bound: |got - ref| <= 2 K 2^-24 S + half an output ulp (+ the GroupNorm term 2^-10 S / 2^-7 S
  where the prologue is on), K = 9 Cin + Csc (+ 5 with Combine: its 4 products and its bias), Combine added to the
  fp64 reference and to S.  A wrong cout mapping puts every element outside it;
* bias = the channel index (and temb = a multiple of 512 per image) with zero weights must come back as the 16-bit
  rounding of exactly that: the permutation of the constants against the store address;
* the statistics of each (image, channel) are compared with fp64 sums of the returned output o:
  |s1 - sum o| <= 2 (u + 256 2^-24) sum |o|, |s2 - sum o^2| <= 2 (2u + u^2 + 256 2^-24) sum o^2, u = 2^-11 (fp16) /
  2^-8 (bf16): the kernel sums the fp32 values before they are rounded to o (relative u each, 2u + u^2 squared) in
  fp32 over a 256-pixel tile (256 2^-24) and then in fp64; doubled as the bound above, derived, not measured;
* three launches into fresh outputs give the same bits.

Shapes: B = 2, H = 16, W = 128 (interior tiles, all four edges, both images, for the 8 x 32 and the 4 x 64 tile);
(C0, C1, Cout) = (64, 0, 128): one cout tile, (64, 0, 256): two cout tiles (n0 = 128), (128, 128, 256): two sources.
(The smallest input depth is 64, not one 32-channel chunk: snrse_conv2d takes 16-bit channel counts in multiples of its
64-element K-tile and answers C0 = 32 with "invalid argument", so no launch of this kernel has a single chunk.)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W = 2, 16, 128
H16 = [pytest.param(torch.float16, id="fp16"), pytest.param(torch.bfloat16, id="bf16")]
CFGS = [(64, 0, 128), (64, 0, 256), (128, 128, 256)]
# mode -> (temb, res, stats, comb, GroupNorm prologue, specialised)
MODES = {
    "temb_stats": (True, False, True, False, True, True),
    "res_stats": (False, True, True, False, False, True),
    "stats": (False, False, True, False, False, True),
    "temb": (True, False, False, False, True, True),
    "rt": (True, True, True, False, False, False),
    "comb_stats": (False, False, True, True, False, True),
    "rt_comb": (False, False, True, True, False, False),
}
PLAIN = [(cfg, (0, 0), m, nt) for cfg in CFGS for m in ("temb_stats", "res_stats", "stats", "temb") for nt in (0, 1)]
PLAIN += [(cfg, (0, 0), "rt", 0) for cfg in CFGS]
SHORT = [(cfg, sc, m, nt) for cfg, sc in (((64, 0, 256), (64, 0)), ((128, 128, 256), (128, 128)))
         for m, nt in (("stats", 0), ("stats", 1), ("comb_stats", 0), ("rt_comb", 0))]


def _ids(cases):
    return [pytest.param(*c, id="c%d_%d_%d-sc%d_%d-%s-nt%d" % (c[0] + c[1] + (c[2], c[3]))) for c in cases]


ALL = _ids(PLAIN + SHORT)
WITH_STATS = _ids([c for c in PLAIN + SHORT if MODES[c[2]][2]])

_inputs, _runs = {}, {}


def conv3x3_f64(x, w):
    """x [B,H,W,C], w [Co,3,3,C], both fp64: the zero-padded 3x3 convolution as 9 shifted matmuls -> [B,H,W,Co]."""
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(*x.shape[:3], w.shape[0], dtype=torch.float64, device=x.device)
    for dy in range(3):
        for dx in range(3):
            out += xp[:, dy:dy + H, dx:dx + W, :] @ w[:, dy, dx, :].T
    return out


def make_case(gpu, h16, cfg, sc, mode):
    """The case's operands, fp64 reference, S and K: once per (format, shape, mode), shared by both tiles and +-NT."""
    key = (h16, cfg, sc, mode)
    if key in _inputs:
        return _inputs[key]
    from snrse import ops
    use_temb, use_res, _, use_comb, use_gn, _ = MODES[mode]
    C0, C1, Co = cfg
    Csc, Csc1 = sc
    Cin = C0 + C1
    g = torch.Generator(device=gpu).manual_seed(77 * Cin + Csc + Csc1 + 1000 * list(MODES).index(mode))
    rn = lambda *s: torch.randn(*s, device=gpu, generator=g)
    x0 = (rn(B, H, W, C0) * 1.3 + 0.1).to(h16)
    x1 = rn(B, H, W, C1).to(h16) if C1 else None
    xs0 = rn(B, H, W, Csc).to(h16) if Csc else None
    xs1 = rn(B, H, W, Csc1).to(h16) if Csc1 else None
    w = (rn(Co, 3, 3, Cin) / math.sqrt(9 * Cin)).to(h16)
    ws = (rn(Co, Csc + Csc1) / math.sqrt(Csc + Csc1)).to(h16) if Csc else None
    bias = rn(Co)
    temb = rn(B, Co + 40) if use_temb else None
    res = rn(B, H, W, Co).to(h16) if use_res else None
    scale = 1 / math.sqrt(2) if use_res else 1.0
    comb = rn(B, H, W, 4) if use_comb else None
    cw = rn(Co, 4) * 0.5 if use_comb else None
    cb = rn(Co) if use_comb else None
    gn = None
    a = (x0 if x1 is None else torch.cat([x0, x1], -1)).double()
    if use_gn:
        gam = torch.rand(Cin, device=gpu, generator=g) + 0.5
        bet = rn(Cin) * 0.2
        sums = ops.gn_stats(x0, x1)
        gn = ops.gn_scale_shift(sums[0], gam, bet, H * W, sums1=sums[1])
        y = a * gn[0].double()[:, None, None, :] + gn[1].double()[:, None, None, :]
        a = (y * torch.sigmoid(y)).to(h16).double()
    ref, S = conv3x3_f64(a, w.double()), conv3x3_f64(a.abs(), w.double().abs())
    ref, S = ref + bias.double(), S + bias.double().abs()
    if Csc:
        xs = (xs0 if xs1 is None else torch.cat([xs0, xs1], -1)).double()
        ref, S = ref + xs @ ws.double().T, S + xs.abs() @ ws.double().abs().T
    if temb is not None:
        t = temb[:, 40:40 + Co].double()[:, None, None, :]
        ref, S = ref + t, S + t.abs()
    if res is not None:
        ref, S = ref + res.double(), S + res.double().abs()
    ref, S = ref * scale, S * scale
    if use_comb:
        ref = ref + comb.double() @ cw.double().T + cb.double()
        S = S + comb.double().abs() @ cw.double().abs().T + cb.double().abs()
    args = dict(x0=x0, x1=x1, xs0=xs0, xs1=xs1, w=w.reshape(Co, -1).contiguous(), ws=ws, bias=bias, temb=temb, res=res,
                scale=scale, comb=comb, cw=cw, cb=cb, gn=gn)
    _inputs[key] = (args, ref, S, 9 * Cin + Csc + Csc1 + (5 if use_comb else 0))
    return _inputs[key]


def launch(a, Co, tw, nt, spec, stats, n=3):
    """n launches into fresh outputs: [(out, folded statistics or None)]."""
    from snrse import ops
    outs = []
    ops.set_option("conv_variant", 5)
    ops.set_option("h5_tw", tw)
    ops.set_option("epi_nt", nt)
    ops.set_option("h5_specialise", int(spec))
    try:
        for _ in range(n):
            st = ops.new_stats(B, Co) if stats else None
            o = ops.conv2d(a["x0"], a["w"], 3, Co, bias=a["bias"], src1=a["x1"], sc=a["xs0"], sc1=a["xs1"],
                           sc_wgt=a["ws"], temb=a["temb"], temb_off=40, res=a["res"], out_scale=a["scale"],
                           comb=a["comb"], comb_w=a["cw"], comb_b=a["cb"], stats=st, gn=a["gn"])
            assert ops.kernel_name(ops.get_option("last_kernel")) == "conv_halo5_kernel"
            assert ops.get_option("last_tw") == (64 if tw == 64 else 32)
            assert ops.get_option("last_epi_nt") == nt
            outs.append((o, ops.fold_stats(st) if stats else None))
        torch.cuda.synchronize()
    finally:
        ops.set_option("conv_variant", 0)
        ops.set_option("h5_tw", 0)
        ops.set_option("epi_nt", 2)
        ops.set_option("h5_specialise", 1)
    return outs


def run_case(gpu, h16, cfg, sc, mode, nt, tw):
    key = (h16, cfg, sc, mode, nt, tw)
    if key not in _runs:
        args, ref, S, K = make_case(gpu, h16, cfg, sc, mode)
        _runs[key] = (launch(args, cfg[2], tw, nt, MODES[mode][5], MODES[mode][2]), ref, S, K)
    return _runs[key]


@pytest.mark.parametrize("tw", [0, 64])
@pytest.mark.parametrize("cfg,sc,mode,nt", ALL)
@pytest.mark.parametrize("h16", H16)
def test_epilogue_elementwise(gpu, h16, cfg, sc, mode, nt, tw):
    """Every element within the fp32 accumulation bound of the fp64 reference (module docstring)."""
    outs, ref, S, K = run_case(gpu, h16, cfg, sc, mode, nt, tw)
    half_ulp, xform = (2.0 ** -11, 2.0 ** -10) if h16 == torch.float16 else (2.0 ** -8, 2.0 ** -7)
    floor = 2.0 ** -25 if h16 == torch.float16 else 0.0
    bound = 2 * K * 2.0 ** -24 * S + torch.clamp(half_ulp * ref.abs(), min=floor)
    if MODES[mode][4]:
        bound = bound + xform * S
    got = outs[0][0]
    err = (got.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"max |got - ref| / bound = {worst:.3f}, max err = {float(err.max()):.3e}")
    assert torch.isfinite(got).all()
    assert worst <= 1.0


@pytest.mark.parametrize("tw", [0, 64])
@pytest.mark.parametrize("cfg,sc,mode,nt", ALL)
@pytest.mark.parametrize("h16", H16)
def test_epilogue_bit_stable(gpu, h16, cfg, sc, mode, nt, tw):
    """Three launches into fresh outputs give the same bits."""
    outs = run_case(gpu, h16, cfg, sc, mode, nt, tw)[0]
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][0], outs[2][0])


@pytest.mark.parametrize("tw", [0, 64])
@pytest.mark.parametrize("cfg,sc,mode,nt", WITH_STATS)
@pytest.mark.parametrize("h16", H16)
def test_epilogue_statistics(gpu, h16, cfg, sc, mode, nt, tw):
    """Per (image, channel) sum and sum of squares against fp64 sums of the returned output (module docstring)."""
    o, st = run_case(gpu, h16, cfg, sc, mode, nt, tw)[0][0]
    o = o.double()
    u = 2.0 ** -11 if h16 == torch.float16 else 2.0 ** -8
    t = 256 * 2.0 ** -24
    s1, sa, s2 = o.sum((1, 2)), o.abs().sum((1, 2)), (o * o).sum((1, 2))
    e1, e2 = (st[..., 0] - s1).abs(), (st[..., 1] - s2).abs()
    b1, b2 = 2 * (u + t) * sa, 2 * (2 * u + u * u + t) * s2
    print(f"max |s1 - sum| / bound = {float((e1 / b1).max()):.3f}, max |s2 - sumsq| / bound = {float((e2 / b2).max()):.3f}")
    assert torch.isfinite(st).all()
    assert bool((e1 <= b1).all())
    assert bool((e2 <= b2).all())


@pytest.mark.parametrize("tw", [0, 64])
@pytest.mark.parametrize("with_temb", [False, True], ids=["bias", "bias_temb"])
@pytest.mark.parametrize("cfg", [pytest.param(c, id="c%d_%d_%d" % c) for c in CFGS])
@pytest.mark.parametrize("h16", H16)
def test_epilogue_channel_constants(gpu, h16, cfg, with_temb, tw):
    """bias = channel index (temb = 512 (image + 1), integers the formats add exactly in fp32), zero weights, no
    GroupNorm: every pixel of channel c of image b is exactly the 16-bit rounding of c (+ 512 (b + 1)), and its
    statistics are 2048 times that value and its square."""
    C0, C1, Co = cfg
    z = lambda *s: torch.zeros(*s, device=gpu, dtype=h16)
    bias = torch.arange(Co, device=gpu, dtype=torch.float32)
    temb = None
    want = bias[None, :].expand(B, Co)
    if with_temb:
        temb = torch.zeros(B, Co + 40, device=gpu)
        temb[:, 40:] = 512.0 * (torch.arange(B, device=gpu, dtype=torch.float32)[:, None] + 1)
        want = want + temb[:, 40:]
    args = dict(x0=z(B, H, W, C0) + 1, x1=z(B, H, W, C1) + 1 if C1 else None, xs0=None, xs1=None, w=z(Co, 9 * (C0 + C1)),
                ws=None, bias=bias, temb=temb, res=None, scale=1.0, comb=None, cw=None, cb=None, gn=None)
    (o, st), = launch(args, Co, tw, 0, True, True, n=1)
    want16 = want.to(h16)
    assert torch.equal(o, want16[:, None, None, :].expand(B, H, W, Co))
    # the fp32 values before rounding are the integers themselves; a tile's fp32 partial sums are exact while they
    # stay below 2^24: 256 px x 1279 always, 256 px x 255^2 with the bias alone
    assert torch.equal(st[..., 0], want.double() * (H * W))
    if not with_temb:
        assert torch.equal(st[..., 1], want.double() ** 2 * (H * W))
