"""Argument checks of the training entries (csrc/train.hip): every call here passes arguments that the
header comment rules out and must come back with hipErrorInvalidValue before any HIP call, so nothing
is launched and no device is needed.

The pointers are placeholder non-NULL addresses.  Should a check be missing, the entry would go on to
launch a kernel on them; with a HIP device visible that would be a real launch on wild addresses, so the
module skips there (it is a test for the machine without a GPU, like test_lib_abi.py).  A missing check
for `groups == 0` does not return at all: `C % groups` is a host integer division by zero (SIGFPE).
"""
import pytest

from conftest import has_gpu

pytestmark = pytest.mark.skipif(has_gpu(), reason="placeholder device addresses: only without a HIP device")

EINVAL = 1  # hipErrorInvalidValue
P = 0x10000  # a placeholder non-NULL address; never dereferenced on the host, never launched with


def _lib():
    from snrse import _lib, build
    return _lib.load(build.build_library())


def _gn_backward(**kw):
    a = dict(x0=P, C0=128, x1=None, C1=0, dy=P, B=2, HW=16, groups=32, gamma=P, beta=P, mean=P, rstd=P, act=1,
             R=P, dx0=P, dx1=None, dgamma=P, dbeta=P)
    a.update(kw)
    return _lib().snrse_gn_backward(a["x0"], a["C0"], a["x1"], a["C1"], a["dy"], a["B"], a["HW"], a["groups"],
                                    a["gamma"], a["beta"], a["mean"], a["rstd"], a["act"], a["R"], a["dx0"],
                                    a["dx1"], a["dgamma"], a["dbeta"], None)


@pytest.mark.parametrize("bad", [
    dict(groups=0), dict(groups=-4), dict(groups=48),  # 0: the host division; 48 does not divide 128
    dict(gamma=None), dict(beta=None), dict(mean=None), dict(rstd=None),
    dict(C0=0), dict(C0=-128), dict(C1=-32), dict(C0=0, C1=128, x1=P, dx1=P),
    dict(C1=128), dict(C1=128, x1=P),  # a second source without x1 / without dx1
    dict(x0=None), dict(dy=None), dict(dx0=None), dict(R=None), dict(B=0), dict(HW=0), dict(HW=-1),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_gn_backward_rejects(bad):
    assert _gn_backward(**bad) == EINVAL


def _gn_moments(**kw):
    a = dict(st0=P, C0=128, st1=None, C1=0, B=2, HW=16, groups=32, eps=1e-6, mean=P, rstd=P)
    a.update(kw)
    return _lib().snrse_gn_moments(a["st0"], a["C0"], a["st1"], a["C1"], a["B"], a["HW"], a["groups"], a["eps"],
                                   a["mean"], a["rstd"], None)


@pytest.mark.parametrize("bad", [
    dict(mean=None), dict(rstd=None), dict(HW=0), dict(HW=-3), dict(C0=0), dict(C0=-4), dict(C1=-4),
    dict(C0=0, C1=128, st1=P), dict(C1=128), dict(st0=None), dict(B=0), dict(groups=0), dict(groups=-1),
    dict(groups=48),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_gn_moments_rejects(bad):
    assert _gn_moments(**bad) == EINVAL


def _wgrad(name, **kw):
    a = dict(dy=P, Cout=128, x0=P, C0=128, x1=None, C1=0, B=1, H=4, W=8, ksize=3, dw=P)
    a.update(kw)
    return getattr(_lib(), name)(a["dy"], a["Cout"], a["x0"], a["C0"], a["x1"], a["C1"], a["B"], a["H"], a["W"],
                                 a["ksize"], a["dw"], None)


@pytest.mark.parametrize("bad", [
    dict(Cout=7), dict(Cout=130), dict(C0=5), dict(C0=126), dict(C0=128, C1=3, x1=P), dict(C0=6, C1=6, x1=P),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_conv_wgrad_x3_rejects_channel_counts_not_multiples_of_4(bad):
    assert _wgrad("snrse_conv_wgrad_x3", **bad) == EINVAL


@pytest.mark.parametrize("name", ["snrse_conv_wgrad", "snrse_conv_wgrad_x3"])
@pytest.mark.parametrize("bad", [
    dict(ksize=2), dict(ksize=5), dict(ksize=0), dict(dy=None), dict(x0=None), dict(dw=None), dict(Cout=0),
    dict(C0=0), dict(C1=-4), dict(C1=64), dict(B=0), dict(H=0), dict(W=0),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_conv_wgrad_rejects(name, bad):
    assert _wgrad(name, **bad) == EINVAL


@pytest.mark.parametrize("HW", [1, 63, 65, 100, 0, -64])
def test_ct_loss_rejects_hw_not_a_multiple_of_64(HW):
    assert _lib().snrse_ct_loss(P, P, P, P, P, 2, HW, 0, P, P, P, None) == EINVAL


def test_ct_loss_and_ct_perturb_reject_null_and_empty():
    L = _lib()
    for i in (0, 1, 2, 3, 4, 8, 9, 10):
        a = [P, P, P, P, P, 2, 64, 1, P, P, P, None]
        a[i] = None
        assert L.snrse_ct_loss(*a) == EINVAL, i
    assert L.snrse_ct_loss(P, P, P, P, P, 0, 64, 1, P, P, P, None) == EINVAL
    for i in (0, 1, 2, 3, 4, 8, 9):
        a = [P, P, P, P, P, 2, 64, 1, P, P, None]
        a[i] = None
        assert L.snrse_ct_perturb(*a) == EINVAL, i
    assert L.snrse_ct_perturb(P, P, P, P, P, 2, 0, 1, P, P, None) == EINVAL
    assert L.snrse_ct_perturb(P, P, P, P, P, 0, 64, 1, P, P, None) == EINVAL


def test_bgemm_chan_sum_softmax_reject_null_and_empty():
    L = _lib()

    def bgemm(A=P, Bm=P, Cm=P, batch=1, M=4, N=4, K=4):
        return L.snrse_bgemm(A, 0, 4, 1, Bm, 0, 4, 1, Cm, 0, 4, 1, None, batch, M, N, K, 1.0, 0.0, None)
    for bad in (dict(A=None), dict(Bm=None), dict(Cm=None), dict(batch=0), dict(M=0), dict(N=0), dict(K=0),
                dict(M=-1)):
        assert bgemm(**bad) == EINVAL, bad
    assert L.snrse_chan_sum(P, 1, 4, 4, None, None, 1.0, None) == EINVAL  # no output at all
    assert L.snrse_chan_sum(None, 1, 4, 4, P, P, 1.0, None) == EINVAL
    for b, hw, c in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert L.snrse_chan_sum(P, b, hw, c, P, P, 1.0, None) == EINVAL
    assert L.snrse_softmax_rows(P, P, 0, 4, 1.0, None) == EINVAL
    assert L.snrse_softmax_rows(P, P, 4, 0, 1.0, None) == EINVAL
    assert L.snrse_softmax_rows(None, P, 4, 4, 1.0, None) == EINVAL
    assert L.snrse_softmax_rows(P, None, 4, 4, 1.0, None) == EINVAL
    assert L.snrse_softmax_bwd_rows(P, P, None, 4, 4, 1.0, None) == EINVAL
    assert L.snrse_softmax_bwd_rows(P, P, P, 4, 0, 1.0, None) == EINVAL


def test_elementwise_entries_reject_null_and_empty():
    L = _lib()
    assert L.snrse_silu(None, P, 4, None) == EINVAL
    assert L.snrse_silu(P, None, 4, None) == EINVAL
    assert L.snrse_silu(P, P, 0, None) == EINVAL
    assert L.snrse_silu_bwd(P, None, P, 4, 0, None) == EINVAL
    assert L.snrse_silu_bwd(P, P, P, 0, 0, None) == EINVAL
    assert L.snrse_axpby(None, P, 4, 1.0, 0.0, None) == EINVAL
    assert L.snrse_axpby(P, None, 4, 1.0, 0.0, None) == EINVAL
    assert L.snrse_axpby(P, P, -1, 1.0, 0.0, None) == EINVAL
    assert L.snrse_scale_rows(P, None, P, 2, 4, 1, None) == EINVAL
    assert L.snrse_scale_rows(P, P, P, 0, 4, 1, None) == EINVAL
    assert L.snrse_scale_rows(P, P, P, 2, 0, 1, None) == EINVAL
    assert L.snrse_gfp(P, None, 2, 4, P, None) == EINVAL
    assert L.snrse_gfp(P, P, 2, 0, P, None) == EINVAL
    assert L.snrse_gfp(P, P, 0, 4, P, None) == EINVAL
    assert L.snrse_adam_ema(None, P, P, 4, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 0.0, None) == EINVAL
    assert L.snrse_adam_ema(P, P, P, 0, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 0.0, None) == EINVAL
