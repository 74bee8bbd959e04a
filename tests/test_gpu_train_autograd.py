"""Each torch.autograd.Function of snrse/train.py, and the two blocks built from them, against float64 torch
autograd of the same operation on the CPU (NCHW; oracle/ncsnpp_ref.py where it has the op): the HIP forward
and backward run with a random upstream gradient, and the output, every input gradient and every parameter
gradient are compared in full.

Bounds.  Exact GEMM mode: the measured rule of tests/train_unit.py, err(HIP) <= 4 err(torch fp32) + one fp32
ulp.  The fp32x3 mode (split-bf16 products, ~2^-16 per product) keeps the project's bounds: a single conv
3e-5 relative RMS (tests/test_gpu_x3.py), a whole block 1e-4 on its output (the bound of the whole fp32x3
network there) and 1e-3 on its gradients (tests/test_gpu_train.py).  Attention: 1e-5 relative norm
(tests/test_gpu_train.py).  The measured pairs go to train_unit_errors.json.

Largest measured HIP / torch-fp32 error ratio per Function in the exact mode (one MI355X,
profiles/train_unit_errors.json; bound 4): _Conv 3.1 (dx of the padded 4 -> 32 input conv), _GroupNorm 2.2, _Fir 1.3,
_Dense 2.3, _SiLU / _AddScale / _ScaleRows 1.00, resblock 1.5, attn_block 1.7.  fp32x3 mode against the fixed
bounds: _Conv 4.6e-6 (3e-5), resblock 7.9e-6 (1e-4 / 1e-3), attn_block 7.7e-7.
"""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import formula_attn_sd, formula_block_sd
from oracle import ncsnpp_ref
from train_unit import check, check_fixed, gen

pytestmark = pytest.mark.gpu

X3_CONV, X3_BLOCK_OUT, X3_BLOCK_GRAD = 3e-5, 1e-4, 1e-3


@pytest.fixture(params=["exact", "x3"])
def gemm(request):
    from snrse import train as tr
    tr.set_gemm(request.param)
    try:
        yield request.param
    finally:
        tr.set_gemm("exact")


def nhwc(t):  # NCHW (CPU) -> NHWC
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def _leaf(t, gpu):
    return t.detach().float().to(gpu).requires_grad_(True)


def _var(t, dt):  # a fresh leaf of dtype dt (t.to(float32) alone would be t itself)
    return t.detach().to(dt).clone().requires_grad_(True)


def _cmp(kernel, case, name, got, f32, ref, fixed=None):
    got = got.detach().cpu()
    if fixed is None:
        check(f"{kernel}.{name}", case, got, f32, ref)
    else:
        check_fixed(f"{kernel}.{name}", case, got, ref, fixed)


def _both(fn):
    """fn(dtype) -> dict of named tensors; run in float64 (reference) and float32 (yardstick)."""
    return fn(torch.float64), fn(torch.float32)


# ------------------------------------------------------------------------------------------ _Conv
CONV_CASES = [
    # name, C0, C1, Cout, k, bias, temb, res, scale, sizes
    ("input 4->128", 4, 0, 128, 3, True, False, False, 1.0, [(8, 16), (5, 7)]),       # padded 4 -> 32
    ("head 128->4 +res", 128, 0, 4, 3, True, False, True, 1.0, [(8, 16)]),            # 16 rows; dgrad pads 4 -> 32
    ("Conv_2 128|128->256 1x1", 128, 128, 256, 1, True, False, False, 1.0, [(8, 16), (5, 7)]),
    ("128->128 all", 128, 0, 128, 3, True, True, True, ncsnpp_ref.INV_SQRT2, [(8, 16)]),
    ("128->128 bare", 128, 0, 128, 3, False, False, False, ncsnpp_ref.INV_SQRT2, [(8, 16)]),
]


@pytest.mark.parametrize("case", [c[:9] + (hw,) for c in CONV_CASES for hw in c[9]],
                         ids=lambda c: f"{c[0]} {c[9][0]}x{c[9][1]}".replace(" ", "_"))
def test_conv_function_vs_fp64(gpu, gemm, case):
    """out = (conv(x0 | x1, w) + b + temb[b] + res) * scale: output, dx0, dx1, dw, db, dres, dtemb."""
    from snrse import train as tr
    name, C0, C1, Co, k, has_b, has_t, has_r, scale, (H, W) = case
    B = 2
    g = gen(100 + C0 + C1 + Co + k + H)
    t = {"x0": torch.randn(B, C0, H, W, generator=g), "w": torch.randn(Co, C0 + C1, k, k, generator=g) * 0.05}
    if C1:
        t["x1"] = torch.randn(B, C1, H, W, generator=g)
    if has_b:
        t["b"] = torch.randn(Co, generator=g)
    if has_t:
        t["temb"] = torch.randn(B, Co, generator=g)
    if has_r:
        t["res"] = torch.randn(B, Co, H, W, generator=g)
    dy = torch.randn(B, Co, H, W, generator=g)

    def ref(dt):
        v = {n: _var(a, dt) for n, a in t.items()}
        x = v["x0"] if not C1 else torch.cat([v["x0"], v["x1"]], 1)
        out = F.conv2d(x, v["w"], v.get("b"), padding=k // 2)
        if has_t:
            out = out + v["temb"][:, :, None, None]
        if has_r:
            out = out + v["res"]
        out = out * scale
        out.backward(dy.to(dt))
        return {"out": out.detach(), **{"d" + n: a.grad for n, a in v.items()}}
    r64, r32 = _both(ref)
    h = {n: _leaf(nhwc(a) if a.dim() == 4 and n != "w" else a, gpu) for n, a in t.items()}
    out = tr.conv(h["x0"], h["w"], h.get("b"), x1=h.get("x1"), res=h.get("res"), temb=h.get("temb"), scale=scale)
    out.backward(nhwc(dy).to(gpu))
    torch.cuda.synchronize()
    got = {"out": nchw(out)}
    for n, a in h.items():
        assert a.grad is not None, n
        got["d" + n] = nchw(a.grad) if a.dim() == 4 and n != "w" else a.grad
    tag = f"{name} {H}x{W} {gemm}"
    for n in r64:
        _cmp("_Conv", tag, n, got[n], r32[n], r64[n], X3_CONV if gemm == "x3" else None)


# ------------------------------------------------------------------------------------------ _GroupNorm
@pytest.mark.parametrize("H,W", [(3, 5), (8, 16)])
@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("C0,C1", [(128, 0), (256, 128)])
def test_groupnorm_function_vs_fp64(gpu, C0, C1, act, H, W):
    from snrse import train as tr
    B, C = 2, C0 + C1
    g = gen(200 + C + H + act)
    x = 1.0 + torch.randn(B, C, H, W, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    dy = torch.randn(B, C, H, W, generator=g)

    def ref(dt):
        xr, ga, be = (_var(a, dt) for a in (x, gamma, beta))
        out = F.group_norm(xr, min(C // 4, 32), ga, be, eps=1e-6)
        out = F.silu(out) if act else out
        out.backward(dy.to(dt))
        return {"out": out.detach(), "dx": xr.grad, "dgamma": ga.grad, "dbeta": be.grad}
    r64, r32 = _both(ref)
    x0 = _leaf(nhwc(x[:, :C0]), gpu)
    x1 = _leaf(nhwc(x[:, C0:]), gpu) if C1 else None
    ga, be = _leaf(gamma, gpu), _leaf(beta, gpu)
    out = tr.group_norm(x0, ga, be, act, x1=x1)
    out.backward(nhwc(dy).to(gpu))
    torch.cuda.synchronize()
    dx = x0.grad if x1 is None else torch.cat([x0.grad, x1.grad], -1)
    got = {"out": nchw(out), "dx": nchw(dx), "dgamma": ga.grad, "dbeta": be.grad}
    for n in r64:
        _cmp("_GroupNorm", f"{C0}|{C1} act{int(act)} {H}x{W}", n, got[n], r32[n], r64[n])


# ------------------------------------------------------------------------------------------ _Fir
@pytest.mark.parametrize("C", [4, 128])
@pytest.mark.parametrize("mode,H,W", [("down", 4, 6), ("down", 8, 16), ("up", 3, 5), ("up", 8, 16)])
def test_fir_function_vs_fp64(gpu, mode, H, W, C):
    """FIR [1,3,3,1] resampling and its adjoint (down^T = up / 4, up^T = 4 down) against autograd of
    fir_down2 / fir_up2, and the adjoint identity <fir(x), y> = <x, fir^T(y)> on the HIP results in fp64."""
    from snrse import train as tr
    B = 2
    g = gen(300 + H + W + C)
    x = torch.randn(B, C, H, W, generator=g)
    op = ncsnpp_ref.fir_down2 if mode == "down" else ncsnpp_ref.fir_up2
    dy = torch.randn(*op(x).shape, generator=g)

    def ref(dt):
        xr = _var(x, dt)
        out = op(xr)
        out.backward(dy.to(dt))
        return {"out": out.detach(), "dx": xr.grad}
    r64, r32 = _both(ref)
    xh = _leaf(nhwc(x), gpu)
    out = tr.fir(xh, mode)
    out.backward(nhwc(dy).to(gpu))
    torch.cuda.synchronize()
    got = {"out": nchw(out).detach().cpu(), "dx": nchw(xh.grad).cpu()}
    for n in r64:
        _cmp("_Fir", f"{mode} {H}x{W} C{C}", n, got[n], r32[n], r64[n])
    # every output is a 16-tap (down) or 4-tap (up) fp32 sum, then one scaling: <= 18 roundings of 2^-24 on
    # the sum of magnitudes; by Cauchy-Schwarz the two inner products differ by at most
    # 32 x 2^-24 (|fir x| |y| + |x| |fir^T y|)
    fx, gx, xd, yd = got["out"].double(), got["dx"].double(), x.double(), dy.double()
    lhs, rhs = float((fx * yd).sum()), float((xd * gx).sum())
    assert abs(lhs - rhs) <= 32 * 2.0 ** -24 * float(fx.norm() * yd.norm() + xd.norm() * gx.norm()), (lhs, rhs)


# ------------------------------------------------------------------------------------------ _Dense
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape,dout", [((3, 512), 128), ((2, 37, 256), 128)])
@pytest.mark.parametrize("kind", ["linear", "nin"])
def test_dense_function_vs_fp64(gpu, gemm, kind, shape, dout, bias):
    """nn.Linear (W [out, in]) and NIN (W [in, out]) over the last dim: y, dx, dW, db."""
    from snrse import train as tr
    din = shape[-1]
    g = gen(400 + din + len(shape) + bias)
    x = torch.randn(*shape, generator=g)
    Wt = torch.randn(*((dout, din) if kind == "linear" else (din, dout)), generator=g) / math.sqrt(din)
    b = torch.randn(dout, generator=g) if bias else None
    dy = torch.randn(*shape[:-1], dout, generator=g)

    def ref(dt):
        xr, Wr = _var(x, dt), _var(Wt, dt)
        br = None if b is None else _var(b, dt)
        out = xr @ (Wr.t() if kind == "linear" else Wr)
        out = out if br is None else out + br
        out.backward(dy.to(dt))
        r = {"out": out.detach(), "dx": xr.grad, "dW": Wr.grad}
        if br is not None:
            r["db"] = br.grad
        return r
    r64, r32 = _both(ref)
    xh, Wh = _leaf(x, gpu), _leaf(Wt, gpu)
    bh = None if b is None else _leaf(b, gpu)
    out = (tr.linear if kind == "linear" else tr.nin)(xh, Wh, bh)
    out.backward(dy.to(gpu))
    torch.cuda.synchronize()
    got = {"out": out, "dx": xh.grad, "dW": Wh.grad}
    if bh is not None:
        got["db"] = bh.grad
    for n in r64:
        _cmp("_Dense", f"{kind} {'x'.join(map(str, shape))}->{dout} bias{int(bias)} {gemm}", n, got[n], r32[n], r64[n])


# ------------------------------------------------------------------------------------------ small Functions
def test_silu_function_vs_fp64(gpu):
    from snrse import train as tr
    g = gen(500)
    x, dy = torch.randn(3, 130, generator=g) * 3, torch.randn(3, 130, generator=g)

    def ref(dt):
        xr = _var(x, dt)
        out = F.silu(xr)
        out.backward(dy.to(dt))
        return {"out": out.detach(), "dx": xr.grad}
    r64, r32 = _both(ref)
    xh = _leaf(x, gpu)
    out = tr.silu(xh)
    out.backward(dy.to(gpu))
    for n, v in (("out", out), ("dx", xh.grad)):
        _cmp("_SiLU", "3x130", n, v, r32[n], r64[n])


def test_addscale_function_vs_fp64(gpu):
    from snrse import train as tr
    g = gen(501)
    a, b, dy = (torch.randn(2, 5, 7, 12, generator=g) for _ in range(3))
    s = ncsnpp_ref.INV_SQRT2

    def ref(dt):
        ar, br = _var(a, dt), _var(b, dt)
        out = (ar + br) * torch.tensor(s, dtype=torch.float32).to(dt)
        out.backward(dy.to(dt))
        return {"out": out.detach(), "da": ar.grad, "db": br.grad}
    r64, r32 = _both(ref)
    ah, bh = _leaf(a, gpu), _leaf(b, gpu)
    out = tr._AddScale.apply(ah, bh, s)
    out.backward(dy.to(gpu))
    for n, v in (("out", out), ("da", ah.grad), ("db", bh.grad)):
        _cmp("_AddScale", "2x5x7x12", n, v, r32[n], r64[n])


def test_scalerows_function_vs_fp64(gpu):
    from snrse import train as tr
    g = gen(502)
    x, dy = torch.randn(3, 5, 7, 4, generator=g), torch.randn(3, 5, 7, 4, generator=g)
    s = torch.tensor([0.03, 0.5, 1.0])

    def ref(dt):
        xr = _var(x, dt)
        out = xr / s.to(dt)[:, None, None, None]
        out.backward(dy.to(dt))
        return {"out": out.detach(), "dx": xr.grad}
    r64, r32 = _both(ref)
    xh = _leaf(x, gpu)
    out = tr._ScaleRows.apply(xh, s.to(gpu))
    out.backward(dy.to(gpu))
    for n, v in (("out", out), ("dx", xh.grad)):
        _cmp("_ScaleRows", "3x5x7x4", n, v, r32[n], r64[n])


# ------------------------------------------------------------------------------------------ _Attention
@pytest.mark.parametrize("B,L,C", [(2, 37, 256), (1, 1, 64), (2, 130, 256)])
def test_attention_function_vs_fp64(gpu, B, L, C):
    """As test_training_attention_vs_torch (1e-5 relative norm), at L off the 64-tile, L = 1 and the network's
    C = 256.  At L = 1 the softmax is the constant 1, so dq and dk are exactly zero on both sides."""
    from snrse import train as tr
    g = gen(600 + B + L + C)
    q, k, v, do = (torch.randn(B, L, C, generator=g) for _ in range(4))
    qa, ka, va = (_leaf(t, gpu) for t in (q, k, v))
    o = tr._Attention.apply(qa, ka, va)
    o.backward(do.to(gpu))
    torch.cuda.synchronize()
    qr, kr, vr = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    orf = torch.softmax(qr @ kr.transpose(1, 2) / math.sqrt(C), -1) @ vr
    orf.backward(do.double())
    for n, got, ref in (("o", o, orf), ("dq", qa.grad, qr.grad), ("dk", ka.grad, kr.grad), ("dv", va.grad, vr.grad)):
        got = got.detach().double().cpu()
        ref = ref.detach()
        if float(ref.norm()) == 0.0:
            assert L == 1 and float(got.norm()) == 0.0, (n, float(got.norm()))
            continue
        err = float((got - ref).norm() / ref.norm())
        print(f"_Attention.{n} [B{B} L{L} C{C}]: {err:.3e}")
        assert err < 1e-5, (n, err)


# ------------------------------------------------------------------------------------------ blocks
def _module(sd, gpu):
    """A namespace of nn.Parameters shaped like the reference block (m.Conv_0.weight, m.NIN_0.W, ...)."""
    root, params = types.SimpleNamespace(), {}
    for key, val in sd.items():
        mod, attr = key.rsplit(".", 1)
        if not hasattr(root, mod):
            setattr(root, mod, types.SimpleNamespace())
        p = torch.nn.Parameter(torch.from_numpy(val).float().to(gpu))
        setattr(getattr(root, mod), attr, p)
        params[key] = p
    return root, params


RES_CASES = [
    # name, C0, C1, Cout, up, down
    ("plain128", 128, 0, 128, False, False),
    ("conv2_128to256", 128, 0, 256, False, False),
    ("down128", 128, 0, 128, False, True),
    ("up256", 256, 0, 256, True, False),
    ("cat256_128to256", 256, 128, 256, False, False),
]


@pytest.mark.parametrize("case", RES_CASES, ids=lambda c: c[0])
def test_resblock_vs_fp64(gpu, gemm, case):
    """snrse.train.resblock vs oracle.ncsnpp_ref.resblock: output, d input(s), d temb activation and every
    parameter gradient.  The oracle takes temb and applies SiLU itself, the HIP block takes a = SiLU(temb):
    d temb = d a * silu'(temb), so the HIP d a is compared after that (exact, fp64) factor."""
    from snrse import train as tr
    name, C0, C1, Co, up, down = case
    B, H, W = 2, 8, 16
    sd = formula_block_sd(f"unit_{name}.", C0 + C1, Co, up, down)
    g = gen(700 + C0 + C1 + Co + up + 2 * down)
    x = torch.randn(B, C0 + C1, H, W, generator=g)
    temb = torch.randn(B, 512, generator=g)

    def ref(dt, dy=None):
        p = {"b." + k: _var(torch.from_numpy(v), dt) for k, v in sd.items()}
        xr, tr_ = _var(x, dt), _var(temb, dt)
        out = ncsnpp_ref.resblock(xr, tr_, p, "b", up=up, down=down)
        if dy is None:
            return out.shape
        out.backward(dy.to(dt))
        return {"out": out.detach(), "dx": xr.grad, "dtemb": tr_.grad, **{"d" + k[2:]: v.grad for k, v in p.items()}}
    dy = torch.randn(*ref(torch.float32), generator=g)
    r64, r32 = ref(torch.float64, dy), ref(torch.float32, dy)
    m, params = _module(sd, gpu)
    x0 = _leaf(nhwc(x[:, :C0]), gpu)
    x1 = _leaf(nhwc(x[:, C0:]), gpu) if C1 else None
    act = _leaf(F.silu(temb.double()), gpu)
    out = tr.resblock(m, x0, act, x1=x1, up=up, down=down)
    out.backward(nhwc(dy).to(gpu))
    torch.cuda.synchronize()
    t64 = temb.double()
    sg = torch.sigmoid(t64)
    dx = x0.grad if x1 is None else torch.cat([x0.grad, x1.grad], -1)
    got = {"out": nchw(out), "dx": nchw(dx), "dtemb": act.grad.double().cpu() * (sg * (1 + t64 * (1 - sg)))}
    for k, p in params.items():
        assert p.grad is not None, k
        got["d" + k] = p.grad
    assert set(got) == set(r64)
    for n in r64:
        fixed = None if gemm == "exact" else (X3_BLOCK_OUT if n == "out" else X3_BLOCK_GRAD)
        _cmp("resblock", f"{name} {gemm}", n, got[n], r32[n], r64[n], fixed)


def test_attn_block_vs_fp64(gpu, gemm):
    """snrse.train.attn_block vs oracle.ncsnpp_ref.attn_block at C = 256, 4 x 8.  The key bias (NIN_1.b) shifts
    every logit of a query alike, so its exact gradient is zero and both sides hold rounding noise: as in
    test_gpu_train.py it must be small (1e-5) relative to the query-bias gradient, not relatively accurate."""
    from snrse import train as tr
    B, C, H, W = 2, 256, 4, 8
    sd = formula_attn_sd("unit_attn.", C)
    g = gen(800)
    x, dy = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)

    def ref(dt):
        p = {"a." + k: _var(torch.from_numpy(v), dt) for k, v in sd.items()}
        xr = _var(x, dt)
        out = ncsnpp_ref.attn_block(xr, p, "a")
        out.backward(dy.to(dt))
        return {"out": out.detach(), "dx": xr.grad, **{"d" + k[2:]: v.grad for k, v in p.items()}}
    r64, r32 = _both(ref)
    m, params = _module(sd, gpu)
    xh = _leaf(nhwc(x), gpu)
    out = tr.attn_block(m, xh)
    out.backward(nhwc(dy).to(gpu))
    torch.cuda.synchronize()
    got = {"out": nchw(out), "dx": nchw(xh.grad), **{"d" + k: p.grad for k, p in params.items()}}
    assert set(got) == set(r64)
    for n in r64:
        if n == "dNIN_1.b":
            ratio = float(got[n].double().cpu().norm() / r64["dNIN_0.b"].norm())
            print(f"attn_block key-bias gradient / query-bias gradient: {ratio:.3e}")
            assert ratio < 1e-5, ratio
            continue
        fixed = None if gemm == "exact" else (X3_BLOCK_OUT if n == "out" else X3_BLOCK_GRAD)
        _cmp("attn_block", gemm, n, got[n], r32[n], r64[n], fixed)
