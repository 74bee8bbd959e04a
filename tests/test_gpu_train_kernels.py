"""Each training kernel of csrc/train.hip, called through its C entry, against a float64 torch reference on
the CPU written here from the formula in the entry's header comment (never another kernel of the library).

Shapes are the smallest that reach the edge named beside them.  Bounds: the weight gradients keep the
project's (exact 1e-5, split-bf16 3e-5 relative RMS, tests/test_gpu_train.py); everything else is held to
the measured rule of tests/train_unit.py, err(HIP) <= 4 err(torch fp32) + one fp32 ulp, whose pairs are
written to train_unit_errors.json (the committed copy is profiles/train_unit_errors.json).

Largest measured HIP / torch-fp32 error ratio per kernel (one MI355X, profiles/train_unit_errors.json; bound 4):
snrse_gn_moments 0.75 on exact statistics (rstd 13 .. 17 over runs through the forward's fp32 block sums, whose
atomics change order; see the allowance in
test_gn_moments_and_backward_vs_fp64), snrse_gn_backward 2.5 on exact moments (dx 14 .. 21 through the forward's),
snrse_chan_sum 3.2, snrse_bgemm 1.01, snrse_softmax_rows 1.6, snrse_softmax_bwd_rows 4.5 (a nearly one-hot row:
the result is a cancelled difference, so its floor is an ulp of the operands; 7.7e-6 against a bound of 2.6e-5),
snrse_silu / snrse_silu_bwd / snrse_axpby / snrse_scale_rows 1.00 (the same roundings as torch), snrse_gfp 3.0,
snrse_ct_perturb 1.2, snrse_ct_loss 1.5.  Weight gradients against their fixed bounds: exact 1.1e-7 (1e-5),
split-bf16 4.5e-6 (3e-5).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from train_unit import check, check_fixed, gen, rel_rms

pytestmark = pytest.mark.gpu


def _call(name, *args):
    """The C entry `name` on the current stream, then a sync.  Tensors are passed as such (None = NULL): they
    stay referenced, and so allocated, until the kernel has run."""
    from snrse import train as tr
    assert all(a.is_cuda and a.is_contiguous() for a in args if torch.is_tensor(a)), name
    tr._call(name, *[a.data_ptr() if torch.is_tensor(a) else a for a in args])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ conv wgrad
WGRAD_CASES = [
    # B, C0, C1, Cout, H, W, ksize, kernels
    # nci * nco = 16 -> at most 129 splits for 160 segments: 2 segments per block (LDS re-staged behind the
    # top-of-loop barrier, accumulators carried over), the last segment of every row 8 px wide
    (2, 256, 0, 256, 16, 136, 3, "both"),
    (1, 64, 0, 64, 1, 5, 3, "both"),     # one segment in all; H = 1: both halo rows out of range; W < 32
    (1, 64, 0, 64, 2, 33, 3, "both"),    # a full segment + a 1-px segment
    (1, 64, 0, 64, 2, 33, 1, "both"),
    (2, 96, 32, 128, 4, 40, 3, "both"),  # the second 64-channel block straddles the two sources
    (1, 32, 96, 68, 3, 32, 3, "both"),   # the first one does; Cout = 64 + 4
    (2, 5, 3, 7, 3, 9, 3, "exact"),      # no multiple-of-4 rule in the exact kernel
]


def _wgrad_inputs(case, gpu):
    B, C0, C1, Co, H, W, k, _ = case
    g = gen(sum(case[:7]))
    x0 = torch.randn(B, H, W, C0, generator=g)
    x1 = torch.randn(B, H, W, C1, generator=g) if C1 else None
    dy = torch.randn(B, H, W, Co, generator=g)
    x = x0 if x1 is None else torch.cat([x0, x1], -1)
    ref = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2).double(), (Co, C0 + C1, k, k),
                                      dy.permute(0, 3, 1, 2).double(), padding=k // 2)
    return x0.to(gpu), None if x1 is None else x1.to(gpu), dy.to(gpu), ref


def _wgrad_run(name, case, x0, x1, dy, dw):
    B, C0, C1, Co, H, W, k, _ = case
    _call(name, dy, Co, x0, C0, x1, C1, B, H, W, k, dw)
    return dw.reshape(Co, k, k, C0 + C1).permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_vs_fp64(gpu, case):
    """dW[co][ky][kx][ci] = sum_p dY[p][co] X[p + (ky-1, kx-1)][ci] over the concatenated input, full tensor."""
    B, C0, C1, Co, H, W, k, which = case
    x0, x1, dy, ref = _wgrad_inputs(case, gpu)
    for name, tol in (("snrse_conv_wgrad", 1e-5), ("snrse_conv_wgrad_x3", 3e-5)):
        if which == "exact" and name.endswith("x3"):
            continue
        dw = torch.zeros(Co, k * k, C0 + C1, device=gpu)
        check_fixed(name, "x".join(map(str, case[:7])), _wgrad_run(name, case, x0, x1, dy, dw), ref, tol)


@pytest.mark.parametrize("name,tol", [("snrse_conv_wgrad", 1e-5), ("snrse_conv_wgrad_x3", 3e-5)])
def test_conv_wgrad_accumulates_into_dw(gpu, name, tol):
    """dw is added to (+=): starting from a non-zero dw the result is dw + the gradient."""
    case = (1, 64, 0, 64, 2, 33, 3, "both")
    x0, x1, dy, ref = _wgrad_inputs(case, gpu)
    dw0 = torch.randn(64, 9, 64, generator=gen(5)) * 4.0
    out = _wgrad_run(name, case, x0, x1, dy, dw0.to(gpu))
    want = dw0.reshape(64, 3, 3, 64).permute(0, 3, 1, 2).double() + ref
    check_fixed(name, "accumulate 1x64x0x64x2x33x3", out, want, tol)
    assert rel_rms(out, ref) > 0.1  # and it is not the bare gradient


# ------------------------------------------------------------------------------------------ GroupNorm
GN_CASES = [
    # B, C0, C1, G, HW
    (2, 128, 0, 32, 130),   # HW not a multiple of the 128-pixel block of the reduce pass
    (3, 256, 128, 32, 15),  # cg = 12: group 21 straddles the sources; C > 256: the channel loop runs twice
    (1, 512, 0, 32, 1),
    (2, 8, 8, 4, 257),
]


def _gn_inputs(case, seed=0):
    B, C0, C1, G, HW = case
    C = C0 + C1
    g = gen(1000 + sum(case) + seed)
    mu = 2.0 + 0.3 * torch.randn(C, generator=g)
    sd = 0.5 * (0.5 + torch.rand(C, generator=g))
    x = mu + sd * torch.randn(B, HW, C, generator=g)  # non-zero mean, another one per channel
    gamma = torch.randn(C, generator=g)
    gamma[0], gamma[1], gamma[C - 1] = -1.3, 0.0, -0.4  # negative entries and one exact zero
    beta = 0.5 * torch.randn(C, generator=g)
    dy = torch.randn(B, HW, C, generator=g)
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)  # accumulated into: start non-zero
    return x, gamma, beta, dy, dg0, db0


def _gn_reference(x, gamma, beta, dy, G, act, dtype):
    """autograd of F.group_norm(cat(x0, x1), G, gamma, beta, eps=1e-6) (+ F.silu): dx, dgamma, dbeta, and the
    per-(b, group) mean / rstd, all in `dtype` on the CPU."""
    B, HW, C = x.shape
    xr = x.to(dtype).permute(0, 2, 1).contiguous().requires_grad_(True)  # [B, C, HW]
    ga, be = (t.detach().to(dtype).clone().requires_grad_(True) for t in (gamma, beta))
    out = F.group_norm(xr, G, ga, be, eps=1e-6)
    if act:
        out = F.silu(out)
    out.backward(dy.to(dtype).permute(0, 2, 1))
    xg = xr.detach().reshape(B, G, -1)
    mean = xg.mean(-1)
    rstd = 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-6)
    return xr.grad.permute(0, 2, 1), ga.grad, be.grad, mean, rstd


def _gn_run(gpu, case, x, gamma, beta, dy, dg0, db0, act, moments=None):
    """gn_stats -> snrse_gn_moments -> snrse_gn_backward; dg0 / db0 None passes NULL.  With `moments`
    (mean, rstd [B, G], CPU) those go to snrse_gn_backward instead of the first two steps' result."""
    from snrse import ops
    B, C0, C1, G, HW = case
    C = C0 + C1
    x0 = x[..., :C0].contiguous().to(gpu)
    x1 = x[..., C0:].contiguous().to(gpu) if C1 else None
    s0, s1 = ops.gn_stats(x0.reshape(B, 1, HW, C0), None if x1 is None else x1.reshape(B, 1, HW, C1))
    mean = torch.full((B * G,), float("nan"), device=gpu)
    rstd = torch.full((B * G,), float("nan"), device=gpu)
    _call("snrse_gn_moments", s0, C0, s1, C1, B, HW, G, 1e-6, mean, rstd)
    if moments is not None:
        mean, rstd = (m.float().reshape(-1).contiguous().to(gpu) for m in moments)
    R = torch.full((B, C, 2), float("nan"), device=gpu)  # workspace: the entry zeroes it
    dx0 = torch.full((B, HW, C0), float("nan"), device=gpu)
    dx1 = torch.full((B, HW, C1), float("nan"), device=gpu) if C1 else None
    dg = None if dg0 is None else dg0.to(gpu)
    db = None if db0 is None else db0.to(gpu)
    _call("snrse_gn_backward", x0, C0, x1, C1, dy.to(gpu), B, HW, G,
          gamma.to(gpu), beta.to(gpu), mean, rstd, int(act),
          R, dx0, dx1, dg, db)
    dx = dx0 if dx1 is None else torch.cat([dx0, dx1], -1)
    return dx.cpu(), dg if dg is None else dg.cpu(), db if db is None else db.cpu(), mean.cpu(), rstd.cpu()


@pytest.mark.parametrize("moments", ["forward", "exact"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gn_moments_and_backward_vs_fp64(gpu, case, act, moments):
    """'forward': the chain the training step runs, snrse_gn_stats -> snrse_gn_moments -> snrse_gn_backward.
    'exact': snrse_gn_backward alone, on the fp64 mean / rstd rounded to fp32, held to the plain rule."""
    B, C0, C1, G, HW = case
    x, gamma, beta, dy, dg0, db0 = _gn_inputs(case)
    r64 = _gn_reference(x, gamma, beta, dy, G, act, torch.float64)
    r32 = _gn_reference(x, gamma, beta, dy, G, act, torch.float32)
    tag = "x".join(map(str, case)) + f" act{act} {moments}"
    if moments == "exact":
        dx, dg, db, _, _ = _gn_run(gpu, case, x, gamma, beta, dy, dg0, db0, act, moments=(r64[3], r64[4]))
        check("snrse_gn_backward.dx0", tag, dx[..., :C0], r32[0][..., :C0], r64[0][..., :C0])
        if C1:
            check("snrse_gn_backward.dx1", tag, dx[..., C0:], r32[0][..., C0:], r64[0][..., C0:])
        check("snrse_gn_backward.dgamma", tag, dg, dg0 + r32[1], dg0.double() + r64[1])
        check("snrse_gn_backward.dbeta", tag, db, db0 + r32[2], db0.double() + r64[2])
        return
    dx, dg, db, mean, rstd = _gn_run(gpu, case, x, gamma, beta, dy, dg0, db0, act)
    check("snrse_gn_moments.mean", tag, mean.reshape(B, G), r32[3], r64[3])
    # The statistics come from the forward's snrse_gn_stats, which adds x and x^2 in fp32 within a block (f64
    # only across blocks), and the variance is E[x^2] - mean^2: an error eps_s of the sums reaches rstd as
    # 1.5 kappa eps_s, kappa = E[x^2] / (var + eps) (here ~15: mean 2, std 0.5).  torch's fp32 group_norm
    # takes the variance about the mean and has no such factor, so the 4x rule alone is missed (measured 5e-7
    # .. 1.1e-6 against 5e-8); eps_s is taken as one fp32 ulp.  snrse_gn_moments itself is held to the plain
    # rule on exact statistics in test_gn_moments_on_exact_statistics.  dx is proportional to rstd and inherits
    # the same relative error (measured 7e-7 .. 1.2e-6), so it gets the same allowance here and the plain rule
    # in the 'exact' variant.
    xg = x.double().reshape(B, HW, G, -1).permute(0, 2, 1, 3).reshape(B, G, -1)
    kappa = float((xg.pow(2).mean(-1) / (xg.var(-1, unbiased=False) + 1e-6)).max())
    allow = 1.5 * kappa * 2.0 ** -23
    check("snrse_gn_moments.rstd", tag, rstd.reshape(B, G), r32[4], r64[4], allow=allow)
    check("snrse_gn_backward.dx0", tag, dx[..., :C0], r32[0][..., :C0], r64[0][..., :C0], allow=allow)
    if C1:
        check("snrse_gn_backward.dx1", tag, dx[..., C0:], r32[0][..., C0:], r64[0][..., C0:], allow=allow)
    check("snrse_gn_backward.dgamma", tag, dg, dg0 + r32[1], dg0.double() + r64[1])
    check("snrse_gn_backward.dbeta", tag, db, db0 + r32[2], db0.double() + r64[2])


def test_gn_backward_without_dgamma(gpu):
    """dgamma = NULL with dbeta set: dbeta and dx are still computed."""
    case, act = (3, 256, 128, 32, 15), 1
    x, gamma, beta, dy, _, db0 = _gn_inputs(case)
    dx, dg, db, _, _ = _gn_run(gpu, case, x, gamma, beta, dy, None, db0, act)
    r64 = _gn_reference(x, gamma, beta, dy, 32, act, torch.float64)
    r32 = _gn_reference(x, gamma, beta, dy, 32, act, torch.float32)
    assert dg is None
    check("snrse_gn_backward.dx", "dgamma NULL", dx, r32[0], r64[0])
    check("snrse_gn_backward.dbeta", "dgamma NULL", db, db0 + r32[2], db0.double() + r64[2])


def _exact_stats(x, gpu):
    """[B, HW, C] -> the slotted f64 (sum, sumsq) buffer [B, SLOTS, C, 2] of snrse_gn_stats, computed here in
    f64 and spread over two slots (the consumer folds all of them)."""
    from snrse import ops
    B, HW, C = x.shape
    st = torch.zeros(B, ops.STAT_SLOTS, C, 2, dtype=torch.float64)
    h = HW // 2
    for slot, part in ((3, x[:, :h].double()), (ops.STAT_SLOTS - 1, x[:, h:].double())):
        st[:, slot, :, 0] = part.sum(1)
        st[:, slot, :, 1] = (part * part).sum(1)
    return st.to(gpu)


RSTD_EPS0 = 1.0 / math.sqrt(float(torch.tensor(1e-6, dtype=torch.float32)))  # 1/sqrt(eps), eps as the float passed


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gn_moments_on_exact_statistics(gpu, case):
    """snrse_gn_moments alone, on f64 statistics computed here: mean and rstd to the plain rule; groups of one
    constant (1.5: exact sums; 2.1f: its square sum rounds in f64, the residue of either sign is clamped) give
    rstd = 1/sqrt(eps) to fp32 rounding."""
    B, C0, C1, G, HW = case
    cg = (C0 + C1) // G
    x = _gn_inputs(case, seed=3)[0]
    x[:, :, 0:cg] = 1.5
    x[:, :, (G - 1) * cg:] = 2.1
    s0 = _exact_stats(x[..., :C0].contiguous(), gpu)
    s1 = _exact_stats(x[..., C0:].contiguous(), gpu) if C1 else None
    mean = torch.full((B * G,), float("nan"), device=gpu)
    rstd = torch.full((B * G,), float("nan"), device=gpu)
    _call("snrse_gn_moments", s0, C0, s1, C1, B, HW, G, 1e-6, mean, rstd)
    mean, rstd = mean.cpu().reshape(B, G), rstd.cpu().reshape(B, G)

    def ref(dt):
        xg = x.to(dt).reshape(B, HW, G, cg).permute(0, 2, 1, 3).reshape(B, G, -1)
        return xg.mean(-1), 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + 1e-6)
    (m64, r64), (m32, r32) = ref(torch.float64), ref(torch.float32)
    tag = "x".join(map(str, case)) + " exact stats"
    check("snrse_gn_moments.mean", tag, mean, m32, m64)
    check("snrse_gn_moments.rstd", tag, rstd[:, 1:G - 1], r32[:, 1:G - 1], r64[:, 1:G - 1])
    assert (rstd[:, [0, G - 1]].double() - RSTD_EPS0).abs().max() <= 2.0 ** -23 * RSTD_EPS0, rstd
    assert torch.equal(mean[:, 0], torch.full((B,), 1.5))


@pytest.mark.parametrize("act", [0, 1])
def test_gn_constant_groups_clamped_variance(gpu, act):
    """Groups whose every element is the same constant, through snrse_gn_stats: the variance is 0, the fmax
    clamp applies, rstd = 1/sqrt(eps) to fp32 rounding and dx stays finite and right.  The constants are ones
    whose fp32 block sums are exact.  (Finding, not asserted: for a constant such as 2.1 the fp32 block sums
    of snrse_gn_stats leave var ~ 1e-6 x mean^2 instead of 0, so rstd comes out near 460 instead of 1000 --
    the statistics' limit for |mean| >> std, see the rstd allowance above; snrse_gn_moments itself returns
    1/sqrt(eps) for it, test_gn_moments_on_exact_statistics.)"""
    case = (2, 8, 8, 4, 257)
    B, C0, C1, G, HW = case
    x, gamma, beta, dy, dg0, db0 = _gn_inputs(case, seed=7)
    x[:, :, 0:4] = 1.5     # group 0
    x[:, :, 8:12] = -0.75  # group 2, in the second source
    dx, dg, db, mean, rstd = _gn_run(gpu, case, x, gamma, beta, dy, dg0, db0, act)
    assert all(torch.isfinite(t).all() for t in (dx, dg, db, mean, rstd))
    rs = rstd.reshape(B, G).double()
    assert (rs[:, [0, 2]] - RSTD_EPS0).abs().max() <= 2.0 ** -23 * RSTD_EPS0, rs
    assert torch.equal(mean.reshape(B, G)[:, [0, 2]], torch.tensor([[1.5, -0.75]] * B))
    r64 = _gn_reference(x, gamma, beta, dy, G, act, torch.float64)
    r32 = _gn_reference(x, gamma, beta, dy, G, act, torch.float32)
    check("snrse_gn_backward.dx", f"constant groups act{act}", dx, r32[0], r64[0])


# ------------------------------------------------------------------------------------------ channel sums
@pytest.mark.parametrize("mode", ["both", "bc", "c"])
@pytest.mark.parametrize("case", [(3, 257, 300), (1, 1, 1), (2, 256, 128)], ids=lambda c: "x".join(map(str, c)))
def test_chan_sum_vs_fp64(gpu, case, mode):
    """out_bc[b][c] += scale sum_p x[b][p][c], out_c[c] += scale sum_{b, p} x[b][p][c]."""
    B, HW, C = case
    g = gen(2000 + sum(case))
    x = torch.randn(B, HW, C, generator=g) + 0.3
    bc0, c0 = torch.randn(B, C, generator=g), torch.randn(C, generator=g)
    scale = -0.5
    bc = bc0.to(gpu) if mode in ("both", "bc") else None
    c = c0.to(gpu) if mode in ("both", "c") else None
    _call("snrse_chan_sum", x.to(gpu), B, HW, C, bc, c, scale)
    tag = "x".join(map(str, case)) + " " + mode
    if bc is not None:
        check("snrse_chan_sum.out_bc", tag, bc.cpu(), bc0 + scale * x.sum(1), bc0.double() + scale * x.double().sum(1))
    if c is not None:
        check("snrse_chan_sum.out_c", tag, c.cpu(), c0 + scale * x.sum((0, 1)),
              c0.double() + scale * x.double().sum((0, 1)))


# ------------------------------------------------------------------------------------------ batched GEMM
BGEMM_CASES = [
    # batch, M, N, K, A^T, B^T, C^T, shared B, alpha, beta, bias
    (1, 1, 1, 1, False, False, False, False, 0.37, 0.0, False),
    (1, 1, 1, 1, True, True, True, False, 1.0, 1.0, True),
    (2, 65, 63, 17, True, False, True, True, 1.0, 1.0, True),     # sAm = 1, sCn != 1, sBb = 0, bias + beta
    (2, 65, 63, 17, False, True, False, False, 0.37, 0.0, True),  # bias without beta
    (1, 64, 64, 16, False, False, False, False, 1.0, 1.0, False),  # exactly one tile and one K step
    (1, 64, 64, 16, True, True, False, False, 0.37, 0.0, False),
    (3, 37, 256, 15, False, True, False, True, 1.0, 0.0, True),   # nn.Linear: a shared W^T, K < 16
    (3, 37, 256, 15, True, False, True, False, 0.37, 1.0, False),
    (2, 130, 70, 100, True, True, True, False, 0.37, 1.0, True),  # three row tiles, K = 6 x 16 + 4
    (2, 130, 70, 100, False, False, False, True, 1.0, 0.0, False),
    (2, 130, 70, 100, False, True, True, False, 1.0, 0.5, False),  # any beta is supported
]


@pytest.mark.parametrize("case", BGEMM_CASES, ids=lambda c: "-".join(str(int(v) if isinstance(v, bool) else v) for v in c))
def test_bgemm_vs_fp64(gpu, case):
    """C[b](m, n) = alpha sum_k A[b](m, k) B[b](k, n) + beta C[b](m, n) + bias[n] on strided operands."""
    batch, M, N, K, at, bt, ct, shared, alpha, beta, has_bias = case
    g = gen(3000 + batch + M + N + K + at + 2 * bt + 4 * ct)
    nb = 1 if shared else batch
    A_st = torch.randn(*((batch, K, M) if at else (batch, M, K)), generator=g)
    B_st = torch.randn(*((nb, N, K) if bt else (nb, K, N)), generator=g)
    C0 = torch.randn(*((batch, N, M) if ct else (batch, M, N)), generator=g)
    bias = torch.randn(N, generator=g) if has_bias else None
    sA = (M * K, 1, M) if at else (M * K, K, 1)
    sB = (0 if shared else K * N,) + ((1, K) if bt else (N, 1))
    sC = (M * N, 1, M) if ct else (M * N, N, 1)
    Cd = C0.to(gpu) if beta != 0.0 else torch.full(C0.shape, float("nan"), device=gpu)
    Ad, Bd = A_st.to(gpu), B_st.to(gpu)
    _call("snrse_bgemm", Ad, *sA, Bd, *sB, Cd, *sC,
          None if bias is None else bias.to(gpu), batch, M, N, K, alpha, beta)

    def ref(dt):
        A = A_st.to(dt).transpose(1, 2) if at else A_st.to(dt)
        Bm = B_st.to(dt).transpose(1, 2) if bt else B_st.to(dt)
        out = alpha * torch.einsum("bmk,bkn->bmn", A, Bm.expand(batch, K, N))
        if beta != 0.0:
            out = out + beta * (C0.to(dt).transpose(1, 2) if ct else C0.to(dt))
        return out if bias is None else out + bias.to(dt)
    got = Cd.cpu().transpose(1, 2) if ct else Cd.cpu()
    check("snrse_bgemm", "-".join(str(int(v) if isinstance(v, bool) else v) for v in case), got,
          ref(torch.float32), ref(torch.float64))


# ------------------------------------------------------------------------------------------ softmax rows
def _logits(rows, L, scale, g):
    """Row 0: logits up to +-80 after scaling; row 1: one entry 60 above the rest; row 2: all equal; others
    normal.  (rows = 1 gets the +-80 row.)"""
    S = torch.randn(rows, L, generator=g) * 3.0
    S[0] = (torch.rand(L, generator=g) * 2 - 1) * 80.0
    S[0, 0], S[0, L - 1] = 80.0, -80.0 if L > 1 else 80.0
    if rows > 2:
        S[1, L // 2] = S[1].max() + 60.0
        S[2] = 3.7
    return S / scale


@pytest.mark.parametrize("scale", [1.0 / 16, 1.0])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("L", [1, 63, 64, 65, 192, 1000])
def test_softmax_rows_and_backward_vs_fp64(gpu, L, rows, scale):
    """P = softmax(scale S) over rows; dS = scale P (dP - <dP, P>) from the fp64 P."""
    g = gen(4000 + L + rows)
    S = _logits(rows, L, scale, g)
    dP = torch.randn(rows, L, generator=g)
    P = torch.full((rows, L), float("nan"), device=gpu)
    _call("snrse_softmax_rows", S.to(gpu), P, rows, L, scale)
    P = P.cpu()
    P64 = torch.softmax(S.double() * scale, -1)
    tag = f"L{L} rows{rows} scale{scale:g}"
    check("snrse_softmax_rows", tag, P, torch.softmax(S * scale, -1), P64)
    # every p_j is a few ulp off and the kernel's row sum carries the rounding of L/64 serial adds per lane
    # plus a 6-step tree: |sum_j p_j - 1| <= (L/64 + 10) 2^-23
    assert (P.double().sum(-1) - 1.0).abs().max() <= (L / 64 + 10) * 2.0 ** -23
    Pin = P64.float()  # the backward's input: the fp64 probabilities rounded, not the forward kernel's
    dS = torch.full((rows, L), float("nan"), device=gpu)
    _call("snrse_softmax_bwd_rows", Pin.to(gpu), dP.to(gpu), dS, rows, L, scale)
    ref = scale * P64 * (dP.double() - (dP.double() * P64).sum(-1, keepdim=True))
    f32 = scale * Pin * (dP - (dP * Pin).sum(-1, keepdim=True))
    if L == 1:  # dS is exactly 0 (p = 1, dP - <dP, P> = 0): no relative error to take
        assert torch.equal(dS.cpu(), torch.zeros(rows, 1))
        return
    # p (dP - <dP, P>) cancels where a row is nearly one-hot (p_j ~ 1, <dP, P> ~ dP_j): the two terms are known
    # to an fp32 ulp each, so the floor is an ulp of their magnitudes, not of the (much smaller) difference
    dot = (dP.double() * P64).sum(-1, keepdim=True)
    check("snrse_softmax_bwd_rows", tag, dS.cpu(), f32, ref, floor_of=scale * P64 * (dP.double().abs() + dot.abs()))


# ------------------------------------------------------------------------------------------ elementwise
NS = [1, 257, 4099]


def _silu_x(n, g, span):
    x = (torch.rand(n, generator=g) * 2 - 1) * span
    special = torch.tensor([span, 0.0, -0.0, -span, 1.0, -1.278])
    x[:min(n, 6)] = special[:min(n, 6)]
    return x


@pytest.mark.parametrize("n", NS)
def test_silu_vs_fp64(gpu, n):
    x = _silu_x(n, gen(5000 + n), 90.0)  # [-90, 90] with +-0: expf(90) overflows to inf, the quotient must not
    y = torch.full((n,), float("nan"), device=gpu)
    _call("snrse_silu", x.to(gpu), y, n)
    check("snrse_silu", f"n{n}", y.cpu(), F.silu(x), F.silu(x.double()), kind="max")
    if n > 2:
        assert y[1].item() == 0.0 and y[2].item() == 0.0


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_silu_bwd_vs_fp64(gpu, n, accumulate):
    """dx (+)= dy silu'(x), silu'(x) = s (1 + x (1 - s)), s = sigmoid(x)."""
    g = gen(5100 + n)
    x = _silu_x(n, g, 90.0)
    x[6:] = x[6:] / 15.0  # most of them where silu' varies
    dy, dx0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    dx = dx0.to(gpu) if accumulate else torch.full((n,), float("nan"), device=gpu)

    def ref(dt):
        s = torch.sigmoid(x.to(dt))
        v = dy.to(dt) * s * (1 + x.to(dt) * (1 - s))
        return dx0.to(dt) + v if accumulate else v
    _call("snrse_silu_bwd", x.to(gpu), dy.to(gpu), dx, n, accumulate)
    check("snrse_silu_bwd", f"n{n} acc{accumulate}", dx.cpu(), ref(torch.float32), ref(torch.float64), kind="max")


AXPBY_FORMS = [("b0_nan", 0.37, 0.0), ("inplace", 0.25, 0.0), ("b1", -1.7, 1.0), ("ema", 0.001, 0.999)]


def _axpby(gpu, n, form, a, b, g):
    x, y0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    xd = x.to(gpu)
    if form == "inplace":  # x is y, as _Fir.backward scales its result
        yd = xd
        y0 = x
    elif form == "b0_nan":  # train.scaled() hands an uninitialised y: with b = 0 it must not be read
        yd = torch.full((n,), float("nan"), device=gpu)
    else:
        yd = y0.to(gpu)
    _call("snrse_axpby", xd, yd, n, a, b)

    def ref(dt):
        a_, b_ = torch.tensor(a, dtype=torch.float32).to(dt), torch.tensor(b, dtype=torch.float32).to(dt)
        return a_ * x.to(dt) if b == 0.0 else a_ * x.to(dt) + b_ * y0.to(dt)
    return yd.cpu(), ref(torch.float32), ref(torch.float64)


@pytest.mark.parametrize("form,a,b", AXPBY_FORMS)
@pytest.mark.parametrize("n", NS)
def test_axpby_vs_fp64(gpu, n, form, a, b):
    got, f32, ref = _axpby(gpu, n, form, a, b, gen(5200 + n))
    check("snrse_axpby", f"n{n} {form}", got, f32, ref, kind="max")


def _scale_rows(gpu, B, per, recip, g):
    x = torch.randn(B, per, generator=g)
    s = torch.tensor([0.5, 1.7, 0.03, 2.9])[:B].contiguous()
    y = torch.full((B, per), float("nan"), device=gpu)
    _call("snrse_scale_rows", x.to(gpu), s.to(gpu), y, B, per, recip)

    def ref(dt):
        return x.to(dt) / s.to(dt)[:, None] if recip else x.to(dt) * s.to(dt)[:, None]
    return y.cpu(), ref(torch.float32), ref(torch.float64)


@pytest.mark.parametrize("recip", [0, 1])
@pytest.mark.parametrize("B,per", [(1, 1), (3, 257), (3, 4099), (2, 256)])
def test_scale_rows_vs_fp64(gpu, B, per, recip):
    """y[b][i] = x[b][i] * s[b] (recip: / s[b])."""
    got, f32, ref = _scale_rows(gpu, B, per, recip, gen(5300 + B + per))
    check("snrse_scale_rows", f"B{B} per{per} recip{recip}", got, f32, ref, kind="max")


BIG = 2 ** 24 + 5  # one element more than 65536 blocks x 256 threads cover: the grid-stride loop's second trip


def test_axpby_second_grid_stride_trip(gpu):
    got, f32, ref = _axpby(gpu, BIG, "ema", 0.001, 0.999, gen(5400))
    check("snrse_axpby", f"n{BIG}", got, f32, ref, kind="max")
    assert (got.double() - ref).abs().max() <= 4 * (f32.double() - ref).abs().max() + 2.0 ** -23  # every element


def test_scale_rows_second_grid_stride_trip(gpu):
    assert BIG % 3 == 0
    got, f32, ref = _scale_rows(gpu, 3, BIG // 3, 1, gen(5500))
    check("snrse_scale_rows", f"n{BIG}", got, f32, ref, kind="max")
    assert ((got.double() - ref).abs() <= 2.0 ** -23 * ref.abs()).all()  # every element, one rounding each


# ------------------------------------------------------------------------------------------ Fourier features
@pytest.mark.parametrize("B,nf", [(1, 3), (4, 128), (2, 130)])
def test_gfp_vs_fp64(gpu, B, nf):
    """out[b] = [sin, cos](2 pi log t_b W).  The fp32 argument reaches ~2000 rad (|log 0.001| x 2 pi x |W| up
    to 3 sigma = 48), so one ulp of it is ~1e-4 rad: the yardstick is fp32 torch.sin / torch.cos of the fp32
    product, over the three rotations of t taken together."""
    g = gen(6000 + B + nf)
    W = torch.randn(nf, generator=g) * 16.0
    ts = [0.001, 0.03, 1.0]
    got, f32, ref = [], [], []
    for k in range(3):
        t = torch.tensor([ts[(i + k) % 3] for i in range(B)], dtype=torch.float32)
        out = torch.full((B, 2 * nf), float("nan"), device=gpu)
        _call("snrse_gfp", t.to(gpu), W.to(gpu), B, nf, out)
        got.append(out.cpu())
        p32 = torch.log(t)[:, None] * W[None, :] * torch.tensor(2 * math.pi, dtype=torch.float32)
        f32.append(torch.cat([torch.sin(p32), torch.cos(p32)], -1))
        p64 = torch.log(t.double())[:, None] * W.double()[None, :] * (2 * math.pi)
        ref.append(torch.cat([torch.sin(p64), torch.cos(p64)], -1))
        one = [i for i in range(B) if ts[(i + k) % 3] == 1.0]  # log 1 = 0: sin 0, cos 0 exactly
        assert torch.equal(got[-1][one, :nf], torch.zeros(len(one), nf))
        assert torch.equal(got[-1][one, nf:], torch.ones(len(one), nf))
    check("snrse_gfp", f"B{B} nf{nf}", torch.cat(got), torch.cat(f32), torch.cat(ref), kind="max")


# ------------------------------------------------------------------------------------------ perturbation
def _H(c):
    m = c.abs()
    return torch.where(m > 0, 0.15 * c / torch.sqrt(torch.where(m > 0, m, torch.ones_like(m))), torch.zeros_like(c))


def _Hinv(c):
    return (c / 0.15).abs() * (c / 0.15)


@pytest.mark.parametrize("transform", [0, 1])
@pytest.mark.parametrize("B,HW", [(3, 5), (2, 64)])
def test_ct_perturb_vs_fp64(gpu, B, HW, transform):
    """mu = H(H^-1(x)(1 - w_b) + H^-1(y) w_b), x_t = mu + s_b z; H(c) = 0.15 c |c|^-1/2 with H(0) = 0,
    H^-1(c) = |c / 0.15| c / 0.15 (identity without transform).  Zero bins, as in padded frames."""
    g = gen(7000 + B + HW)
    cn = lambda: torch.complex(torch.randn(B, HW, generator=g), torch.randn(B, HW, generator=g)) * 0.4  # noqa: E731
    x, y, z = cn(), cn(), cn() / 0.4
    q = max(1, HW // 4)
    x[:, :2 * q] = 0   # a block of zero bins in x,
    y[:, q:3 * q] = 0  # one in y, [q, 2q) zero in both
    w = torch.tensor([0.0, 1.0, 0.3])[:B].contiguous()
    s = torch.tensor([0.5, 0.05, 0.0123])[:B].contiguous()
    mu = torch.full((B, HW), float("nan"), dtype=torch.complex64, device=gpu)
    xt = torch.full((B, HW), float("nan"), dtype=torch.complex64, device=gpu)
    _call("snrse_ct_perturb", x.to(gpu), y.to(gpu), z.to(gpu), w.to(gpu),
          s.to(gpu), B, HW, transform, mu, xt)

    def ref(cdt, rdt):
        xx, yy, ww = x.to(cdt), y.to(cdt), w.to(rdt)[:, None]
        a, b = (_Hinv(xx), _Hinv(yy)) if transform else (xx, yy)
        m = a * (1 - ww) + b * ww
        if transform:
            m = _H(m)
        return torch.view_as_real(m), torch.view_as_real(m + s.to(rdt)[:, None] * z.to(cdt))
    m64, x64 = ref(torch.complex128, torch.float64)
    m32, x32 = ref(torch.complex64, torch.float32)
    mu, xt = torch.view_as_real(mu.cpu()), torch.view_as_real(xt.cpu())
    tag = f"B{B} HW{HW} transform{transform}"
    check("snrse_ct_perturb.mu", tag, mu, m32, m64, kind="max")
    check("snrse_ct_perturb.xt", tag, xt, x32, x64, kind="max")
    assert torch.equal(mu[:, q:2 * q], torch.zeros(B, q, 2))  # zero in both -> H(0) = 0


# ------------------------------------------------------------------------------------------ consistency loss
@pytest.mark.parametrize("sqrt_loss", [0, 1])
@pytest.mark.parametrize("B,HW", [(1, 64), (3, 192)])
def test_ct_loss_vs_fp64(gpu, B, HW, sqrt_loss):
    """f_k = cs_k x_k + co_k dnn_k; err = f1 - f0 (mse) or s(f1) - s(f0), s(f) = f |f|^-1/2 (sqrt_mse);
    loss_b = 0.5 sum |err|^2; g_k = d mean_b(loss_b) / d dnn_k, against autograd of the same real formula."""
    g = gen(8000 + B + HW)
    d1, d0, x1, x0 = (torch.randn(B, HW, 2, generator=g) * 0.5 for _ in range(4))
    coef = torch.tensor([[0.9, -0.4, 0.8, 0.3], [0.5, 0.7, 0.6, -0.65], [0.99, 0.02, 0.97, 0.05]])[:B].contiguous()
    zero = torch.zeros(HW, dtype=torch.bool)
    if sqrt_loss:  # exact zeros at the same bins of f1 and f0: the kernel's gradient there is 0, torch's NaN
        zero[3:7] = True
        zero[HW - 1] = True
        for t in (d1, d0, x1, x0):
            t[:, zero] = 0.0
    loss_b = torch.full((B,), float("nan"), dtype=torch.float64, device=gpu)
    g1 = torch.full((B, HW, 2), float("nan"), device=gpu)
    g0 = torch.full((B, HW, 2), float("nan"), device=gpu)
    _call("snrse_ct_loss", d1.to(gpu), d0.to(gpu), x1.to(gpu), x0.to(gpu),
          coef.to(gpu), B, HW, sqrt_loss, loss_b, g1, g0)
    keep = ~zero

    def ref(dt):
        a1 = d1[:, keep].to(dt).requires_grad_(True)
        a0 = d0[:, keep].to(dt).requires_grad_(True)
        c = coef.to(dt)
        f1 = c[:, 0, None, None] * x1[:, keep].to(dt) + c[:, 1, None, None] * a1
        f0 = c[:, 2, None, None] * x0[:, keep].to(dt) + c[:, 3, None, None] * a0
        if sqrt_loss:
            f1 = f1 * f1.pow(2).sum(-1, keepdim=True).pow(-0.25)
            f0 = f0 * f0.pow(2).sum(-1, keepdim=True).pow(-0.25)
        lb = 0.5 * (f1 - f0).pow(2).sum((1, 2))
        lb.mean().backward()
        return lb.detach(), a1.grad, a0.grad
    l64, r1, r0 = ref(torch.float64)
    l32, y1, y0 = ref(torch.float32)
    g1, g0 = g1.cpu(), g0.cpu()
    tag = f"B{B} HW{HW} sqrt{sqrt_loss}"
    assert torch.isfinite(g1).all() and torch.isfinite(g0).all()
    assert torch.equal(g1[:, zero], torch.zeros(B, int(zero.sum()), 2))
    assert torch.equal(g0[:, zero], torch.zeros(B, int(zero.sum()), 2))
    check("snrse_ct_loss.loss_b", tag, loss_b.cpu(), l32, l64)
    check("snrse_ct_loss.g1", tag, g1[:, keep], y1, r1)
    check("snrse_ct_loss.g0", tag, g0[:, keep], y0, r0)
