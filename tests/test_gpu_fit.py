"""GPU checks of the training loop (snrse/fit.py) and what it stands on: the device-side global gradient norm
and clipped optimizer step (snrse_grad_sumsq / snrse_grad_clip_coef / snrse_adam_ema_scaled behind FusedAdam),
checkpoints that resume bit for bit, evaluate_model against a loop of enhance() calls, and fit() end to end
for both models on synthetic trees.

Tensor sizes of the optimizer tests are the edges of the kernels' 2048-element chunks: 1, 2047, 2048, 2049 and
5000 elements (the last with a non-contiguous gradient), beside a parameter that has no gradient.  Gradient
magnitudes span 1e-6 .. 1e3."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import formula_sd

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (2047,), (2048,), (2049,), (50, 100), (33,)]  # (50, 100): non-contiguous grad; (33,): no grad
NONCONTIG, NOGRAD = 4, 5


def _params(gpu, seed=3):
    gen = torch.Generator(device=gpu).manual_seed(seed)
    mod = torch.nn.Module()
    mod.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, device=gpu, generator=gen)) for s in SHAPES])
    return mod


def _grads(gpu, it, scale=1.0):
    """One gradient per tensor, |g| spread log-uniformly over 1e-6 .. 1e3 (times `scale`); None for NOGRAD."""
    gen = torch.Generator(device=gpu).manual_seed(100 + it)
    out = []
    for k, s in enumerate(SHAPES):
        if k == NOGRAD:
            out.append(None)
            continue
        mag = 10.0 ** (torch.rand(s, device=gpu, generator=gen) * 9.0 - 6.0)
        out.append(torch.randn(s, device=gpu, generator=gen) * mag * scale)
    return out


def _set_grads(ps, grads):
    for k, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
        elif k == NONCONTIG:
            p.grad = g.t().contiguous().t()
            assert not p.grad.is_contiguous() and torch.equal(p.grad, g)
        else:
            p.grad = g.clone()


def _true_norm(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_grad_norm_matches_fp64_and_is_bit_stable(gpu):
    """last_grad_norm vs sqrt(sum g^2) in fp64 to 2^-22 relative: the fp64 square of an fp32 is exact and the
    fp64 sums lose ~1e-16 per add, so what remains is the one rounding of the result to fp32 (2^-24) plus
    margin.  No atomics, a fixed fold order: two runs give the same bits."""
    from snrse.train import FusedAdam
    grads = _grads(gpu, 0)
    ref = _true_norm(grads)
    got = []
    for _ in range(2):
        mod = _params(gpu)
        opt = FusedAdam(mod.parameters(), lr=1e-3, clip_grad_norm=1.0)
        _set_grads(mod.ps, grads)
        opt.step()
        assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dtype == torch.float32
        got.append(opt.last_grad_norm.clone())
    torch.cuda.synchronize()
    rel = abs(float(got[0].double()) - ref) / ref
    print(f"grad norm {float(got[0]):.9e} vs fp64 {ref:.9e}: rel {rel:.2e}")
    assert rel <= 2.4e-7, rel
    assert torch.equal(_bits(got[0]), _bits(got[1]))
    # the step without clip or scale computes no norm
    opt = FusedAdam(_params(gpu).parameters(), lr=1e-3)
    assert opt.last_grad_norm is None


@pytest.mark.parametrize("clip,grad_scale", [(1.0, 1.0), (1.0, 0.5), (None, 0.5)])
def test_clipped_step_matches_torch(gpu, clip, grad_scale):
    """3 steps of FusedAdam(clip_grad_norm=c).step(grad_scale) vs clip_grad_norm_(params, c) + torch.optim.Adam +
    the torch_ema rule on a CPU copy whose gradients were multiplied by grad_scale; c = 1 is far below the norm
    (~1e4).  rtol = atol = 1e-6, the project's bound for the unclipped step (test_gpu_train.py)."""
    from sgmse.ema import EMAState
    from snrse.train import FusedAdam
    mod = _params(gpu)
    ref = [p.detach().cpu().clone().requires_grad_(True) for p in mod.ps]
    ema = EMAState(mod, 0.999)
    opt = FusedAdam(mod.parameters(), lr=1e-3, ema=ema, clip_grad_norm=clip)
    topt = torch.optim.Adam(ref, lr=1e-3)
    shadow = [p.detach().clone() for p in ref]
    for it in range(3):
        grads = _grads(gpu, it)
        _set_grads(mod.ps, grads)
        for q, g in zip(ref, grads):
            q.grad = None if g is None else (g.cpu() * grad_scale)
        opt.step(grad_scale=grad_scale)
        with_grad = [q for q in ref if q.grad is not None]
        total = _true_norm(grads) * grad_scale  # the norm of the gradients as the optimizer sees them
        assert abs(float(opt.last_grad_norm.double()) - total) <= 2.4e-7 * total
        if clip is not None:
            assert total > 100 * clip
            torch.nn.utils.clip_grad_norm_(with_grad, clip)
        topt.step()
        decay = min(0.999, (1 + it + 1) / (10 + it + 1))
        with torch.no_grad():
            for s, q in zip(shadow, ref):
                s.sub_((1.0 - decay) * (s - q))
    torch.cuda.synchronize()
    for p, q in zip(mod.ps, ref):
        assert torch.allclose(p.cpu(), q, rtol=1e-6, atol=1e-6), (p.shape, (p.cpu() - q).abs().max())
    for s, r in zip(ema.shadow_params, shadow):
        assert torch.allclose(s.cpu(), r, rtol=1e-6, atol=1e-6), (s.cpu() - r).abs().max()
    assert ema.num_updates == 3


def test_clip_above_the_norm_is_bit_identical_to_the_default_step(gpu):
    """max_norm above the norm: the coefficient is exactly 1, so the scaled launch leaves parameters, moments
    and shadows bit-identical to the default FusedAdam launch from the same state (2 steps)."""
    from sgmse.ema import EMAState
    from snrse.train import FusedAdam
    runs = []
    for clip in (None, 1e9):
        mod = _params(gpu)
        ema = EMAState(mod, 0.999)
        opt = FusedAdam(mod.parameters(), lr=1e-3, ema=ema, clip_grad_norm=clip)
        for it in range(2):
            _set_grads(mod.ps, _grads(gpu, it))
            opt.step()
        torch.cuda.synchronize()
        assert (opt.last_grad_norm is None) == (clip is None)
        have = [p for p in mod.ps if p in opt.state]
        runs.append(([p.detach().clone() for p in mod.ps], [opt.state[p]["exp_avg"] for p in have],
                     [opt.state[p]["exp_avg_sq"] for p in have], list(ema.shadow_params)))
    assert float(opt.last_grad_norm) < 1e9
    for a, b in zip(runs[0], runs[1]):
        assert len(a) == len(b) and len(a) >= 5
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))


def _hand_grads(model, it):
    gen = torch.Generator(device="cuda").manual_seed(500 + it)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device=p.device, generator=gen) * 0.1 if p.requires_grad else None


def _state_equal(m1, o1, m2, o2):
    ps1, ps2 = list(m1.parameters()), list(m2.parameters())
    assert len(ps1) == len(ps2) > 10
    for p, q in zip(ps1, ps2):
        assert torch.equal(_bits(p), _bits(q))
        s1, s2 = o1.state[p], o2.state[q]
        assert float(s1["step"]) == float(s2["step"])
        assert torch.equal(_bits(s1["exp_avg"]), _bits(s2["exp_avg"]))
        assert torch.equal(_bits(s1["exp_avg_sq"]), _bits(s2["exp_avg_sq"]))
    assert m1.ema.num_updates == m2.ema.num_updates and m1.ema.decay == m2.ema.decay
    for a, b in zip(m1.ema.shadow_params, m2.ema.shadow_params):
        assert torch.equal(_bits(a), _bits(b))


def test_checkpoint_resume_is_bit_exact(gpu, tmp_path):
    """Hand-set gradients, so only the optimizer path is involved (elementwise + the ordered reduction):
    2 steps, save, load into a fresh model and optimizer -> equal state; 2 more steps on both -> still equal."""
    from sgmse.snr_estimator import SNRModel
    torch.manual_seed(1)
    m = SNRModel().cuda().train()
    opt = m.configure_optimizers()
    opt.clip_grad_norm = 1.0
    for it in range(2):
        _hand_grads(m, it)
        m.optimizer_step(opt)
    path = str(tmp_path / "resume.ckpt")
    m.save_checkpoint(path, optimizer=opt, epoch=4, global_step=2)
    torch.manual_seed(2)  # other initial weights: everything must come from the file
    m2 = SNRModel.load_from_checkpoint(path, optimizer=True)
    opt2 = m2.resume["optimizer"]
    opt2.clip_grad_norm = 1.0
    assert m2.resume["epoch"] == 4 and m2.resume["global_step"] == 2 and next(m2.parameters()).is_cuda
    _state_equal(m, opt, m2, opt2)
    for it in range(2, 4):
        for mm, oo in ((m, opt), (m2, opt2)):
            _hand_grads(mm, it)
            mm.train()
            mm.optimizer_step(oo)
    torch.cuda.synchronize()
    _state_equal(m, opt, m2, opt2)
    assert m.ema.num_updates == 4 and float(opt.state[next(m.parameters())]["step"]) == 4
    assert torch.equal(_bits(opt.last_grad_norm), _bits(opt2.last_grad_norm))


# ----------------------------------------------------------------------------- synthetic trees
def _clip(L, k):
    rng = np.random.default_rng(300 + k)
    t = np.arange(L) / 16000.0
    c = (0.2 * np.sin(2 * np.pi * (250.0 + 90.0 * k) * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))).astype(np.float32)
    return c, (c + (0.03 + 0.02 * k) * rng.standard_normal(L)).astype(np.float32)


def _tree(root, train_lens, valid_lens):
    from snrse import audio
    for sub, lens in (("train", train_lens), ("valid", valid_lens)):
        for d in ("clean", "noisy"):
            os.makedirs(root / sub / d)
        rows = []
        for k, L in enumerate(lens):
            c, y = _clip(L, k + (0 if sub == "train" else 50))
            audio.write_wav(str(root / sub / "clean" / f"f{k}.wav"), c, bits=32)
            audio.write_wav(str(root / sub / "noisy" / f"f{k}.wav"), y, bits=32)
            rows.append(f"f{k}.wav\t{float(np.sqrt(np.mean(c ** 2))):.6f}\t{float(np.sqrt(np.mean((y - c) ** 2))):.6f}")
        if sub == "valid":
            (root / sub / "active_rms.txt").write_text("\n".join(rows) + "\n")
    return str(root)


@pytest.fixture()
def formula_snr_estimator(gpu):
    """The formula-weight SNR estimator as the enhance() paths' estimator for the duration."""
    from sgmse import model as smodel
    from sgmse.snr_estimator import SNRModel
    sm = SNRModel()
    sm.dnn.load_state_dict({k: torch.from_numpy(v) for k, v in formula_sd("snrnet", "snrnet.").items()})
    sm = sm.cuda().eval()
    old = smodel._snr_model
    smodel.set_snr_model(sm)
    yield sm
    smodel.set_snr_model(old)


def _score_model(base_dir, **kw):
    from sgmse.model import ScoreModel
    hp = dict(backbone="ncsnpp", sde="ouve", model_type="sebridge_v3", snr_conditioned="true", theta=1.5,
              sigma_min=0.05, sigma_max=0.5, N=30, compute_dtype="fp32", fixed_snr=0.17783, loss_type="mse",
              base_dir=base_dir, batch_size=2, num_frames=64)
    hp.update(kw)
    m = ScoreModel(**hp)
    m.dnn.load_state_dict({k: torch.from_numpy(v) for k, v in formula_sd("ncsnpp").items()})
    return m.cuda().train()


def test_evaluate_model_matches_a_loop_of_enhance_calls(gpu, tmp_path, formula_snr_estimator):
    """5 validation clips of 0.5 .. 1.2 s, num_eval_files = 3 -> files 0, 2, 4.  evaluate_model (ragged batches,
    EMA weights, device SI-SDR) against evaluate.score_files on a loop of enhance() calls under the same
    torch.manual_seed: waveforms <= 1e-4 relative RMS per file, the bound test_gpu_batch_eval.py holds ragged
    batches to; the mean SI-SDR within what that waveform bound allows -- a perturbation d of x_hat with
    |d| <= eps |x_hat| moves |x_hat - a x| by at most |d|, i.e. the ratio by 20 log10(1 + eps |x_hat| /
    |x_hat - a x|) dB, taken from the loop's own waveforms -- plus the kernel's 1e-5 dB.  The model is back
    in train mode with its live weights bit-equal afterwards."""
    from sgmse.util.inference import eval_indices, evaluate_model
    from snrse import audio, evaluate
    lens = (8000, 11000, 14000, 16500, 19200)
    root = _tree(tmp_path, (), lens)
    m = _score_model(root)
    m.data_module.setup(stage="fit")
    # EMA weights that differ from the live ones: the formula weights as shadows, the live ones nudged
    m.ema.shadow_params = [p.detach().clone() for p in m.ema._params()]
    m.ema.num_updates = 1
    with torch.no_grad():
        for p in m.ema._params():
            p.mul_(1.001)
    live = [p.detach().clone() for p in m.parameters()]
    live_w = m.ema._params()[0].detach().clone()
    idx = eval_indices(len(lens), 3)
    assert idx == [0, 2, 4]
    vs = m.data_module.valid_set
    torch.manual_seed(5)
    m.eval(no_ema=False)
    loop, rows = [], []
    for i in idx:
        x, sr = audio.load(vs.clean_files[i])
        y, _ = audio.load(vs.noisy_files[i])
        xh = np.asarray(m.enhance(x, y), np.float32)
        loop.append(xh)
        rows.append(evaluate.score_files(xh, x[0].numpy(), y[0].numpy(), sr))
    m.train(True)
    want = float(np.mean([r[1] for r in rows]))
    got_wave = []
    enhance_batch = m.enhance_batch

    def rec(ys, **kw):
        assert not m.training and not torch.equal(m.ema._params()[0], live_w)  # the EMA weights are in
        r = enhance_batch(ys, **kw)
        got_wave.extend(r)
        return r

    m.enhance_batch = rec
    torch.manual_seed(5)
    pesq, si_sdr, estoi = evaluate_model(m, 3)
    assert m.training and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(m.parameters(), live))
    assert math.isnan(estoi) and math.isnan(pesq) == (evaluate._pesq_fn() is None)
    tol = 1e-5
    for k, i in enumerate(idx):
        assert got_wave[k].shape == loop[k].shape == (lens[i],)
        err = float(np.sqrt(np.mean((got_wave[k].astype(np.float64) - loop[k]) ** 2)) / np.sqrt(np.mean(loop[k].astype(np.float64) ** 2)))
        ratio = 10.0 ** (rows[k][1] / 20.0)  # |a x| / |x_hat - a x|; |x_hat|^2 = |a x|^2 + |x_hat - a x|^2
        tol += 20.0 * math.log10(1.0 + 1e-4 * math.sqrt(1.0 + ratio ** 2)) / len(idx)
        print(f"evaluate_model file {i}: ragged vs enhance() rel RMS {err:.2e}, SI-SDR {rows[k][1]:.4f} dB")
        assert err <= 1e-4, (i, err)
    print(f"evaluate_model si_sdr {si_sdr:.6f} vs loop mean {want:.6f} (tolerance {tol:.2e} dB)")
    assert abs(si_sdr - want) <= tol, (si_sdr, want, tol)


def _log(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def test_fit_snr_model_end_to_end_and_resume(gpu, tmp_path, monkeypatch):
    """SNRModel, 8 training clips, batch 2, accumulate 2 -> 2 optimizer steps per epoch, 2 epochs, clip 1.0:
    finite losses, moved parameters, one log line per optimizer step (gradient norm on every 2nd here), top-2 by
    valid_loss, last.ckpt loads; resuming it with max_epochs=3 runs exactly one more epoch."""
    from sgmse.data_module import SpecsDataModule
    from sgmse.snr_estimator import SNRModel
    from snrse import fit
    monkeypatch.setattr(fit, "LOG_EVERY_N_STEPS", 2)
    root = _tree(tmp_path / "data", [9000 + 400 * k for k in range(8)], (9000, 10000, 12000))

    def make():
        return SNRModel(backbone="snrnet", data_module_cls=SpecsDataModule, base_dir=root, batch_size=2,
                        num_frames=64, transform_type="none", num_eval_files=0)

    torch.manual_seed(0)
    m = make()
    w0 = [p.detach().clone() for p in m.parameters()]
    ck, lg = str(tmp_path / "ck"), str(tmp_path / "log.jsonl")
    res = fit.fit(m, max_epochs=2, accumulate_grad_batches=2, gradient_clip_val=1.0, ckpt_dir=ck, log_path=lg, seed=7)
    assert (res["epoch"], res["global_step"], res["epochs_run"]) == (1, 4, 2)
    lines = _log(lg)
    steps = [r for r in lines if "train_loss" in r]
    vals = [r for r in lines if "valid_loss" in r]
    assert [r["step"] for r in steps] == [1, 2, 3, 4] and [r["epoch"] for r in steps] == [0, 0, 1, 1]
    assert all(math.isfinite(r["train_loss"]) and r["samples_per_s"] > 0 for r in steps)
    assert [r["grad_norm"] is not None for r in steps] == [False, True, False, True]
    assert all(math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 for r in steps if r["grad_norm"] is not None)
    assert len(vals) == 2 and all(math.isfinite(r["valid_loss"]) and math.isfinite(r["snr_error"]) for r in vals)
    assert all(not torch.equal(a.cpu(), b.detach().cpu()) for a, b in zip(w0, m.parameters()))
    assert m.training and m.ema.num_updates == 4
    names = sorted(os.listdir(ck))
    assert "last.ckpt" in names and all(not n.endswith(".tmp") for n in names)
    top = [n for n in names if n.startswith("epoch=")]
    assert sorted(top) == sorted(f"epoch={r['epoch']}-valid_loss={r['valid_loss']:.2f}.ckpt" for r in vals)
    loaded = SNRModel.load_from_checkpoint(os.path.join(ck, "last.ckpt"))
    assert loaded.resume == {"epoch": 1, "global_step": 4}
    assert all(torch.equal(a, b.detach().cpu()) for a, b in zip(loaded.parameters(), m.parameters()))
    torch.manual_seed(9)
    m2 = make()
    res2 = fit.fit(m2, max_epochs=3, accumulate_grad_batches=2, gradient_clip_val=1.0, ckpt_dir=ck, log_path=lg,
                   seed=7, resume=os.path.join(ck, "last.ckpt"))
    assert (res2["epoch"], res2["global_step"], res2["epochs_run"]) == (2, 6, 1)
    assert m2.ema.num_updates == 6
    steps2 = [r for r in _log(lg) if "train_loss" in r]
    assert [r["step"] for r in steps2] == [1, 2, 3, 4, 5, 6] and steps2[-1]["epoch"] == 2
    assert len([n for n in os.listdir(ck) if n.startswith("epoch=")]) == 2  # top 2 of 3 kept
    assert SNRModel.load_from_checkpoint(os.path.join(ck, "last.ckpt")).resume == {"epoch": 2, "global_step": 6}


def test_fit_score_model_end_to_end(gpu, tmp_path, formula_snr_estimator):
    """sebridge_v3 'true', B = 2 x 64 frames, one epoch of 2 steps, num_eval_files = 2: a finite si_sdr is logged
    and the top-k checkpoint carries train.py's name."""
    from snrse import fit
    root = _tree(tmp_path / "data", [9000 + 500 * k for k in range(4)], (8000, 9000, 10000))
    m = _score_model(root, num_eval_files=2)
    w0 = m.dnn.all_modules[4].Conv_0.weight.detach().clone()
    ck, lg = str(tmp_path / "ck"), str(tmp_path / "log.jsonl")
    res = fit.fit(m, max_epochs=1, gradient_clip_val=1.0, ckpt_dir=ck, log_path=lg, seed=1)
    assert (res["epoch"], res["global_step"]) == (0, 2)
    lines = _log(lg)
    steps = [r for r in lines if "train_loss" in r]
    assert [r["step"] for r in steps] == [1, 2] and all(math.isfinite(r["train_loss"]) for r in steps)
    (val,) = [r for r in lines if "valid_loss" in r]
    assert math.isfinite(val["valid_loss"]) and math.isfinite(val["si_sdr"]) and val["estoi"] is None  # NaN -> null
    assert not torch.equal(w0, m.dnn.all_modules[4].Conv_0.weight) and m.training and m.ema.num_updates == 2
    assert sorted(os.listdir(ck)) == sorted(["last.ckpt", f"epoch=0-si_sdr={val['si_sdr']:.2f}.ckpt"])
