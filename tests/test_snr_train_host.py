"""CPU checks of the SNR-estimator training path: the reference golden against the oracle's float64
autograd, the closed forms, the evaluation driver's host arithmetic and the input guards."""
import numpy as np
import pytest
import torch

from conftest import fnormal, golden
import snr_train_ref as R


def _golden_batch():
    g = golden("snr_train_step.npz")
    B, T = 2, 64
    x = torch.from_numpy(fnormal("golden.snrtrain.x", (B, 1, 256, T), complex_=True)) * 0.4
    y = torch.from_numpy(fnormal("golden.snrtrain.n", (B, 1, 256, T), complex_=True)) * 0.4 + x
    return g, x.to(torch.complex64), y.to(torch.complex64), torch.from_numpy(g["gt"])


def test_golden_vs_oracle_autograd():
    """tests/golden/snr_train_step.npz (the reference SNRNet module, fp32 autograd) against
    oracle.snrnet_ref.snrnet_forward in float64 under autograd: this pins the oracle's gradients, which the GPU
    tests use at other shapes, to the reference's."""
    g, x, y, gt = _golden_batch()
    loss, est, grads = R.oracle_step(x, y, gt)
    assert abs(loss - float(g["loss"])) / abs(float(g["loss"])) < R.LOSS_RTOL
    np.testing.assert_allclose(est.numpy(), g["est"], rtol=1e-5, atol=1e-6)
    yp = R.perturb_ref(x, y, gt)
    np.testing.assert_allclose(torch.view_as_real(yp.reshape(2, -1)[:, :64]).numpy(), g["perturbed_head"], rtol=1e-6,
                               atol=1e-7)
    names = [str(k) for k in g["names"]]
    assert names == list(grads) and len(names) == 22
    full = [str(k) for k in g["full_keys"]]
    head = int(g["head"])
    for k in full:
        assert R.rel_rms(grads[k].numpy(), g[f"full__{k}"]) < R.GRAD_RTOL, k
    rest = [k for k in names if k not in full]
    heads = g["heads"].reshape(len(rest), head)
    for i, k in enumerate(rest):
        assert grads[k].numel() > 10000
        assert R.rel_rms(grads[k].reshape(-1)[:head].numpy(), heads[i]) < R.GRAD_RTOL, k
    for i, k in enumerate(names):
        sq = float((grads[k] ** 2).sum())
        assert abs(sq - g["gsq"][i]) / g["gsq"][i] < R.SUMSQ_RTOL, k


@pytest.mark.parametrize("B,T", [(2, 32), (3, 48)])
def test_parity_case_inputs_have_resolved_pool_winners(B, T):
    """The draws the GPU parity cases use (snr_train_ref.SEED) keep every conv-pool window's float64 top-two gap
    above 4x the fp32 rounding error of the conv output, so the winner a fp32 forward picks is the oracle's."""
    x, y, gt, _ = R.case(B, T)
    for gap, err in R.pool_margins(x, y, gt):
        assert gap > 4 * err, (gap, err)


def test_normfac_closed_form():
    """calculate_normfac_direct(1, SNR, 1) = 2.040166 / sqrt(1 + SNR^2) (0.240253 + 0.759747 = 1)."""
    from sgmse.snr_estimator import SNRModel
    m = SNRModel()
    snr = torch.tensor([0.0, 0.1, 1.0, 3.5, 999.0], dtype=torch.float64)
    got = m.calculate_normfac_direct(1, snr, 1)
    np.testing.assert_allclose(got.numpy(), 2.040166 / np.sqrt(1 + snr.numpy() ** 2), rtol=1e-12)
    assert abs(m.calculate_normfac_direct(1.0, 0.0, 1.0) - 2.040166) < 1e-12


def test_loss_is_mse_over_batch():
    from sgmse.snr_estimator import SNRModel
    gt = torch.tensor([0.1, 0.5, 0.9])
    est = torch.tensor([[0.2], [0.5], [0.6]])
    assert abs(float(SNRModel()._loss(gt, est)) - (0.01 + 0.0 + 0.09) / 3) < 1e-7


@pytest.mark.parametrize("L", [40000, 32640, 32641, 20001, 20000])
def test_evaluate_driver_host_arithmetic(L):
    """mix_clip (eval_snr_est.py:71-100, 113) against numpy: the centre crop / the split zero padding bit-exact,
    the mix and the normalisation, the label SNR - 5 and the dB of an estimate."""
    from snrse.evaluate_snr_est import mix_clip
    rng = np.random.RandomState(L)
    x = rng.randn(1, L).astype(np.float32)
    n = rng.randn(1, L).astype(np.float32)
    y = x + n
    snr = 17.25
    target = 255 * 128
    if L >= target:
        st = int((L - target) / 2)
        xc, yc = x[:, st:st + target], y[:, st:st + target]
    else:
        pad = target - L
        xc = np.pad(x, ((0, 0), (pad // 2, pad // 2 + pad % 2)))
        yc = np.pad(y, ((0, 0), (pad // 2, pad // 2 + pad % 2)))
    assert xc.shape == (1, target)
    # snr_db = 0 and a unit peak leave the cropped / padded noisy signal itself: bit-exact crop
    y0, real0, none = mix_clip(x, y / np.abs(yc).max(), 0.0)
    assert none is None and real0 == -5.0
    ref0 = xc + (yc / np.abs(yc).max() - xc) * np.float32(1.0)
    ref0 = ref0 / np.abs(ref0).max()
    assert np.array_equal(y0.numpy(), ref0)
    yn, real, est_db = mix_clip(x, y, snr, est_gt=0.25)
    ref = xc + (yc - xc) * np.float32(10 ** (-snr / 20))
    ref = ref / np.abs(ref).max()
    np.testing.assert_allclose(yn.numpy(), ref, rtol=1e-6, atol=1e-7)
    assert abs(float(yn.abs().max()) - 1.0) < 1e-6 and yn.shape == (1, target)
    assert real == snr - 5
    assert abs(float(est_db) - 20 * np.log10(0.75 / 0.25)) < 1e-5


def test_step_and_forward_train_raise_on_cpu_tensors():
    from sgmse.snr_estimator import SNRModel
    m = SNRModel()
    x = torch.zeros(2, 1, 256, 32, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m._step((x, x), 0, gt=torch.tensor([0.2, 0.4]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m._step((x, x, torch.ones(2), torch.ones(2)), 0, valid=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.dnn.forward_train(torch.zeros(2, 2, 256, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.dnn.forward_train(x)


@pytest.mark.parametrize("T", [16, 40])
def test_frame_count_guard(T):
    """T = 16: one chunk, the reference's unbiased std (and loss) is NaN; T = 40: not a multiple of 16."""
    from sgmse.snr_estimator import SNRModel
    from snrse import snr_train
    m = SNRModel()
    x = torch.zeros(2, 1, 256, T, dtype=torch.complex64)
    with pytest.raises(ValueError):
        m._step((x, x), 0)
    with pytest.raises(ValueError):
        m.dnn.forward_train(torch.zeros(2, 2, 256, T))
    with pytest.raises(ValueError):
        snr_train.snrnet_train(x[:, 0], dict(m.dnn.state_dict(keep_vars=True)))


def test_training_entries_reject_short_input():
    """The C entries return an error (no launch) for T < 32 or T % 16 != 0; the workspace size is 0 there."""
    from snrse import _lib
    lib = _lib.load()
    assert lib.snrse_snrnet_train_workspace(2, 16) == 0 and lib.snrse_snrnet_train_workspace(2, 40) == 0
    assert lib.snrse_snrnet_train_workspace(2, 32) > 0
    null = [None] * 17
    assert lib.snrse_snrnet_train_fwd(None, 2, 16, *null, None, None, None) != 0
    assert lib.snrse_snrnet_backward(None, 2, 16, None, None, *([None] * 8), None, *null, None) != 0
