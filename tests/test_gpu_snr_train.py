"""GPU parity of the SNR estimator's training step (sgmse.snr_estimator.SNRModel on csrc/snrnet_train.hip)
against the reference golden (tests/golden/snr_train_step.npz, the reference SNRNet under fp32 autograd) and
against oracle.snrnet_ref.snrnet_forward in float64 under autograd (tests/snr_train_ref.py; pinned to the
golden by test_snr_train_host.py).

Bounds: loss 1e-5 relative, every gradient tensor 5e-5 relative RMS, sums of squares 2e-4 -- the project's
training bounds; the reference's own fp32-vs-float64 error at these shapes is 1.2e-7 / 6.3e-6 at worst.

Measured on an MI355X (profiles/snr_train_parity.json): golden loss exact to fp32, gradients <= 5.3e-6,
sums of squares <= 1.6e-6; oracle (2, 32) 3.3e-5 (the reference arithmetic in fp32 on the CPU: 2.0e-5 there), (3, 48)
2.1e-5, (5, 272) 2.7e-6, ties 3.6e-6; loss <= 1.8e-7; the optimiser loop 0.07827 -> 1.993e-4.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import fnormal, golden
import snr_train_ref as R

pytestmark = pytest.mark.gpu

REPORT_DIR = os.environ.get("SNRSE_REPORT_DIR")  # when set, the measured figures are also written there as JSON


def _report(name, obj):
    if not REPORT_DIR:
        return
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, name), "w") as fh:
        json.dump(obj, fh, indent=1)


def _model():
    from sgmse.snr_estimator import SNRModel
    m = SNRModel()
    m.dnn.load_state_dict(R.formula_snr_sd())
    return m.cuda().train()


def _run(m, x, y, gt, gpu):
    m.zero_grad(set_to_none=True)
    loss = m._step((x.to(gpu), y.to(gpu)), 0, gt=gt)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {k: p.grad.detach().double().cpu() for k, p in m.dnn.named_parameters()}


def _errors(loss, grads, ref_loss, ref_grads):
    err = {k: R.rel_rms(grads[k].numpy(), ref_grads[k].numpy()) for k in ref_grads}
    return abs(loss - ref_loss) / abs(ref_loss), err


def test_step_vs_reference_golden(gpu):
    """1. SNRModel._step((x, y), 0, gt) + backward at B=2, T=64 against the reference module's loss, est, stored
    full gradients, gradient heads and per-tensor sums of squares."""
    g = golden("snr_train_step.npz")
    B, T = 2, 64
    x = (torch.from_numpy(fnormal("golden.snrtrain.x", (B, 1, 256, T), complex_=True)) * 0.4).to(torch.complex64)
    y = (torch.from_numpy(fnormal("golden.snrtrain.n", (B, 1, 256, T), complex_=True)) * 0.4).to(torch.complex64) + x
    gt = torch.from_numpy(g["gt"])
    m = _model()
    loss, grads = _run(m, x, y, gt, gpu)
    from snrse import snr_train
    est = m.dnn.forward_train(snr_train.perturb(x.to(gpu), y.to(gpu), gt.to(gpu))).detach().cpu()
    names = [str(k) for k in g["names"]]
    full = [str(k) for k in g["full_keys"]]
    rest = [k for k in names if k not in full]
    head = int(g["head"])
    heads = g["heads"].reshape(len(rest), head)
    err_loss = abs(loss - float(g["loss"])) / abs(float(g["loss"]))
    err_full = {k: R.rel_rms(grads[k].numpy(), g[f"full__{k}"]) for k in full}
    err_head = {k: R.rel_rms(grads[k].reshape(-1)[:head].numpy(), heads[i]) for i, k in enumerate(rest)}
    err_sq = {k: abs(float((grads[k] ** 2).sum()) - g["gsq"][i]) / g["gsq"][i] for i, k in enumerate(names)}
    print("golden", err_loss, err_full, err_head, err_sq)
    _report("snr_train_golden.json", {"loss": loss, "ref_loss": float(g["loss"]), "rel_err_loss": err_loss,
                                      "rel_rms_full": err_full, "rel_rms_heads": err_head, "rel_err_sumsq": err_sq})
    assert sorted(grads) == sorted(names) and len(names) == 22
    assert err_loss < R.LOSS_RTOL, err_loss
    np.testing.assert_allclose(est.numpy(), g["est"], rtol=1e-4, atol=1e-6)
    assert max(err_full.values()) < R.GRAD_RTOL, err_full
    assert max(err_head.values()) < R.GRAD_RTOL, err_head
    assert max(err_sq.values()) < R.SUMSQ_RTOL, err_sq


@pytest.mark.parametrize("B,T", [(2, 32), (3, 48), (5, 272)])
def test_full_gradients_vs_oracle(gpu, B, T):
    """2. All 22 gradient tensors against the float64 oracle.  (2, 32): S = 2, the least S with a defined std,
    N = 4 < the time conv's 16-chunk block; (3, 48): odd B and S, N = 9; (5, 272): S = 17, N = 85, a partial last
    block in every stage.  The b_ih and b_hh gradients are the same numbers; forward_train's est equals
    SNRNet.forward's within test_snrnet_vs_oracle_larger's bound."""
    from snrse import snr_train
    x, y, gt, (ref_loss, ref_est, ref_grads) = R.case(B, T)
    m = _model()
    loss, grads = _run(m, x, y, gt, gpu)
    err_loss, err = _errors(loss, grads, ref_loss, ref_grads)
    print(f"oracle B={B} T={T}", err_loss, err)
    _report(f"snr_train_oracle_{B}_{T}.json", {"loss": loss, "ref_loss": ref_loss, "rel_err_loss": err_loss,
                                               "rel_rms_grads": err})
    assert len(grads) == 22 and sorted(grads) == sorted(ref_grads)
    assert err_loss < R.LOSS_RTOL, err_loss
    assert max(err.values()) < R.GRAD_RTOL, err
    for sfx in ("", "_reverse"):
        assert torch.equal(grads["blstm.bias_ih_l0" + sfx], grads["blstm.bias_hh_l0" + sfx])
    yp = snr_train.perturb(x.to(gpu), y.to(gpu), gt.to(gpu))
    est_t = m.dnn.forward_train(yp).detach().cpu()
    est_i = m.dnn.forward_complex(yp[:, 0].contiguous()).cpu()
    np.testing.assert_allclose(est_t.numpy(), est_i.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(est_t.numpy(), ref_est.numpy(), rtol=1e-4, atol=1e-6)


def test_ties_zero_padded_chunk(gpu):
    """3. (3, 48) with the last 16 frames exactly zero: one chunk per utterance whose conv outputs equal the bias,
    so every pooling window of it ties; the first maximum in row-major order wins, as in the reference."""
    x, y, gt, (ref_loss, _, ref_grads) = R.case(3, 48, 16)
    assert all(bool(torch.isfinite(v).all()) for v in ref_grads.values()) and math.isfinite(ref_loss)
    loss, grads = _run(_model(), x, y, gt, gpu)
    err_loss, err = _errors(loss, grads, ref_loss, ref_grads)
    print("ties", err_loss, err)
    _report("snr_train_ties.json", {"loss": loss, "ref_loss": ref_loss, "rel_err_loss": err_loss, "rel_rms_grads": err})
    assert err_loss < R.LOSS_RTOL, err_loss
    assert max(err.values()) < R.GRAD_RTOL, err


def test_perturb_kernel(gpu):
    """4. snrse_snr_perturb against the torch expression of snr_estimator.py:93-98 on the device."""
    from snrse import snr_train
    x, y = R.batch("t.snrperturb", 3, 48)
    gt = torch.tensor([0.0, 0.37, 0.998], device=gpu)
    got = snr_train.perturb(x.to(gpu), y.to(gpu), gt)
    ref = R.perturb_ref(x.to(gpu), y.to(gpu), gt)
    for b in range(3):
        rel = float((got[b] - ref[b]).abs().max() / ref[b].abs().max())
        assert rel <= 1e-6, (b, rel)
    assert got.shape == y.shape and got.dtype == torch.complex64


def test_validation_branch(gpu):
    """5. validation_step on a Specs_SNR batch (x, y, s, n): gt = n / (s + n), the loss and snr_error against the
    host formulas over SNRNet.forward."""
    m = _model()
    x, y = R.batch("t.snrvalid", 3, 48)
    s = torch.tensor([1.0, 0.5, 2.0])
    n = torch.tensor([0.25, 0.5, 6.0])
    loss = m.validation_step((x.to(gpu), y.to(gpu), s.to(gpu), n.to(gpu)), 0)
    gt = n / (s + n)
    est = m.dnn.forward_complex(y[:, 0].contiguous().to(gpu)).cpu()[:, 0]
    assert abs(float(loss) - float(torch.mean((gt - est) ** 2))) < 1e-7
    real = 20 * torch.log10((1 - gt) / gt)
    est_db = 20 * torch.log10((1 - est) / est)
    assert abs(m.snr_error - float(torch.mean(torch.abs(real - est_db)))) < 1e-4
    assert torch.allclose(m.real_SNRs, real, atol=1e-5)


def test_optimiser_loop_fits_fixed_batch(gpu):
    """6. 40 x (_step, backward, optimizer_step) at the reference's lr 1e-4 on one fixed batch: finite losses, the
    last at most 0.1 x the first (the reference arithmetic with torch Adam on the CPU: 0.0783 -> 2.0e-4), and
    the EMA shadows move."""
    B, T = 4, 64
    x = (torch.from_numpy(fnormal("t.snrfit.x", (B, 1, 256, T), complex_=True)) * 0.4).to(torch.complex64)
    y = x + (torch.from_numpy(fnormal("t.snrfit.n", (B, 1, 256, T), complex_=True)) * 0.4).to(torch.complex64)
    gt = torch.tensor([0.1, 0.35, 0.6, 0.85])
    m = _model()
    assert m.lr == 1e-4
    opt = m.configure_optimizers()
    w0 = [p.detach().clone() for p in m.parameters()]
    xd, yd = x.to(gpu), y.to(gpu)
    losses = []
    for it in range(40):
        opt.zero_grad()
        loss = m._step((xd, yd), it, gt=gt)
        loss.backward()
        m.optimizer_step(opt)
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print("fit", losses[0], losses[-1])
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] <= 0.1 * losses[0], (losses[0], losses[-1])
    assert m.ema.num_updates == 40 and len(m.ema.shadow_params) == 22
    assert all(not torch.equal(s, w) for s, w in zip(m.ema.shadow_params, w0))
    assert all(not torch.equal(p.detach(), w) for p, w in zip(m.parameters(), w0))


def test_repeatable(gpu):
    """7. Two runs of the (3, 48) case agree within the gradient bound."""
    x, y, gt, _ = R.case(3, 48)
    m = _model()
    l0, g0 = _run(m, x, y, gt, gpu)
    l1, g1 = _run(m, x, y, gt, gpu)
    assert abs(l0 - l1) <= R.LOSS_RTOL * abs(l0)
    for k in g0:
        assert R.rel_rms(g1[k].numpy(), g0[k].numpy()) < R.GRAD_RTOL, k
