"""Every element of the halo GEMM's output (conv_halo5_kernel), on shapes small enough to run in well under a second.

The whole-tensor relative RMS of the other halo tests (1e-2) does not move when one 16-B vector is wrong: an LDS-DMA
piece that lands in a ring slot still being read, or a halo vector consumed before it arrived.  Here

* each case is launched three times into fresh outputs, which must be bit-identical (the per-channel statistics go
  through atomics and are left out), and
* every output element is held to the fp32 accumulation bound against an fp64 reference of the same 16-bit-rounded
  operands: |got - ref| <= 2 K 2^-24 S + r, with S the same expression over absolute values (convolution, shortcut,
  bias, temb, residual), K = 9 Cin + Csc the summed depth and r half an output ulp of |ref| (2^-11 relative for
  fp16, 2^-8 for bf16, and not below half the spacing of fp16's subnormals, 2^-25).  K 2^-24 S bounds fp32
  accumulation in any order; it is doubled, so the bound is derived, not measured.
* With the fused GroupNorm+SiLU the kernel's transformed operand (exp2 / rcp in f32, rounded to 16 bits) may differ
  from the reference's by one ulp, so 2^-10 S (fp16) / 2^-7 S (bf16) is added.  That bound is loose on purpose:
  with the prologue it is the run-to-run check that catches a race.

Shapes: B = 2, H = 16, W = 128 = 8 x 32 tiles of 8 x 32 px (h5_tw = 64: 4 x 64 tiles of 4 x 64 px), so both tile forms
have interior tiles, all four image edges and, with Cin >= 64, at least two 32-channel chunks.  The shortcut depths give
0, 0/1, 1, 1/2, 2, 3 and 5 shortcut phases per main chunk (as test_conv_halo_large lists them), with one and two
shortcut sources.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W = 2, 16, 128
H16 = [pytest.param(torch.float16, id="fp16"), pytest.param(torch.bfloat16, id="bf16")]
# (C0, C1, Cout): the shortcut channels (Csc, Csc1) it runs with -- all multiples of the ABI's 64
SHAPES = {
    (64, 0, 128): [(0, 0), (64, 0), (128, 0), (192, 0), (320, 0)],                      # 0 1 2 3 5 per chunk
    (128, 0, 128): [(0, 0), (64, 0), (128, 0), (192, 0), (256, 0), (384, 0), (640, 0)],  # 0 0/1 1 1/2 2 3 5
    (128, 128, 256): [(0, 0), (128, 0), (128, 128), (256, 256), (384, 384), (640, 640)],  # 0 0/1 1 2 3 5
}
CASES = [pytest.param(cfg, sc, id="c%d_%d_%d-sc%d_%d" % (cfg + sc)) for cfg, scs in SHAPES.items() for sc in scs]

_cache = {}


def conv3x3_f64(x, w):
    """x [B,H,W,C], w [Co,3,3,C], both fp64: the zero-padded 3x3 convolution as 9 shifted matmuls -> [B,H,W,Co]."""
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(*x.shape[:3], w.shape[0], dtype=torch.float64, device=x.device)
    for dy in range(3):
        for dx in range(3):
            out += xp[:, dy:dy + H, dx:dx + W, :] @ w[:, dy, dx, :].T
    return out


def run_case(gpu, h16, cfg, sc, tw, use_gn):
    """The case's three outputs, its fp64 reference, S and K (computed once per case and shared by the tests)."""
    key = (h16, cfg, sc, tw, use_gn)
    if key in _cache:
        return _cache[key]
    from snrse import ops
    C0, C1, Co = cfg
    Csc, Csc1 = sc
    Cin = C0 + C1
    g = torch.Generator(device=gpu).manual_seed(1000 * Cin + Csc + Csc1 + (7 if use_gn else 0))
    rn = lambda *s: torch.randn(*s, device=gpu, generator=g)
    x0 = (rn(B, H, W, C0) * 1.3 + 0.1).to(h16)
    x1 = rn(B, H, W, C1).to(h16) if C1 else None
    xs0 = rn(B, H, W, Csc).to(h16) if Csc else None
    xs1 = rn(B, H, W, Csc1).to(h16) if Csc1 else None
    w = (rn(Co, 3, 3, Cin) / math.sqrt(9 * Cin)).to(h16)
    ws = (rn(Co, Csc + Csc1) / math.sqrt(Csc + Csc1)).to(h16) if Csc else None
    bias = rn(Co)
    # as in the network: Conv_0 (GroupNorm prologue here) adds temb, Conv_1 adds the residual or has the shortcut
    temb = rn(B, Co + 40) if (use_gn and not Csc) else None
    res = rn(B, H, W, Co).to(h16) if (not use_gn and not Csc) else None
    scale = 1 / math.sqrt(2) if res is not None else 1.0
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
    outs = []
    ops.set_option("conv_variant", 5)
    ops.set_option("h5_tw", tw)
    try:
        for _ in range(3):
            st = ops.new_stats(B, Co)
            outs.append(ops.conv2d(x0, w.reshape(Co, -1).contiguous(), 3, Co, bias=bias, src1=x1, sc=xs0, sc1=xs1,
                                   sc_wgt=ws, temb=temb, temb_off=40, res=res, out_scale=scale, stats=st, gn=gn))
            assert ops.kernel_name(ops.get_option("last_kernel")) == "conv_halo5_kernel"
            assert ops.get_option("last_tw") == (64 if tw == 64 else 32)
        torch.cuda.synchronize()
    finally:
        ops.set_option("conv_variant", 0)
        ops.set_option("h5_tw", 0)
    _cache[key] = (outs, ref, S, 9 * Cin + Csc + Csc1)
    return _cache[key]


@pytest.mark.parametrize("use_gn", [False, True], ids=["plain", "gn"])
@pytest.mark.parametrize("tw", [0, 64])
@pytest.mark.parametrize("cfg,sc", CASES)
@pytest.mark.parametrize("h16", H16)
def test_halo5_bit_stable(gpu, h16, cfg, sc, tw, use_gn):
    """Three launches of one case give the same bits."""
    outs = run_case(gpu, h16, cfg, sc, tw, use_gn)[0]
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("use_gn", [False, True], ids=["plain", "gn"])
@pytest.mark.parametrize("tw", [0, 64])
@pytest.mark.parametrize("cfg,sc", CASES)
@pytest.mark.parametrize("h16", H16)
def test_halo5_elementwise(gpu, h16, cfg, sc, tw, use_gn):
    """Every element within the fp32 accumulation bound of the fp64 reference (see the module docstring; with the
    GroupNorm+SiLU prologue the bound is loose on purpose and test_halo5_bit_stable is what catches a race)."""
    outs, ref, S, K = run_case(gpu, h16, cfg, sc, tw, use_gn)
    half_ulp, xform = (2.0 ** -11, 2.0 ** -10) if h16 == torch.float16 else (2.0 ** -8, 2.0 ** -7)
    floor = 2.0 ** -25 if h16 == torch.float16 else 0.0
    bound = 2 * K * 2.0 ** -24 * S + torch.clamp(half_ulp * ref.abs(), min=floor)
    if use_gn:
        bound = bound + xform * S
    err = (outs[0].double() - ref).abs()
    worst = float((err / bound).max())
    print(f"max |got - ref| / bound = {worst:.3f}, max err = {float(err.max()):.3e}")
    assert torch.isfinite(outs[0]).all()
    assert worst <= 1.0
