"""Utterances of different lengths in one batch (GPU): the ragged STFT / absmax / energy-ratio kernels, the
row-seeded noise entries, PCEnhancer and SNRAlignedEnhancer on a ragged batch against each utterance run alone,
and the evaluation driver at batch_size 4 against its per-file loop.  fp32 compute_dtype, formula weights, F = 256.
Buffers are filled with NaN past each row's length: nothing there may reach a result."""
import os

import numpy as np
import pytest
import torch

from conftest import fnormal, formula_sd
from test_gpu_dropin import score_model

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = torch.as_tensor(a).detach().cpu()
    b = torch.as_tensor(b).detach().cpu()
    dt = torch.complex128 if (a.is_complex() or b.is_complex()) else torch.float64
    a, b = a.to(dt), b.to(dt)
    return float((a - b).abs().pow(2).mean().sqrt() / (b.abs().pow(2).mean().sqrt() + 1e-30))


def ragged(rows, gpu, fill=float("nan")):
    """[B, max L] device buffer of the rows, `fill` past each row's end."""
    buf = torch.full((len(rows), max(len(r) for r in rows)), fill, dtype=torch.float32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = torch.as_tensor(r)
    return buf.to(gpu)


def clip(L, k):
    rng = np.random.default_rng(100 + k)
    t = np.arange(L) / 16000.0
    return (0.2 * np.sin(2 * np.pi * (300.0 + 170.0 * k) * t) + (0.02 + 0.05 * k) * rng.standard_normal(L)).astype(np.float32)


def test_ragged_stft_absmax_energy_ratios(gpu):
    from oracle import spec_ref
    from snrse import ops
    lens = (256, 300, 1000, 8191)
    rows = [(fnormal(f"t.rag.{L}", (L,)) * 0.3).astype(np.float32) for L in lens]
    buf = ragged(rows, gpu)
    assert buf.shape == (4, 8191) and torch.isnan(buf[0, 256:]).all()
    div = torch.tensor([0.5, 1.25, 2.0, 0.75], device=gpu)
    for mode in (0, 1):
        out = ops.stft(buf, 1.0, tpad=64, mode=mode, in_div=div, lengths=lens)
        assert out.shape == (4, 256, 64)
        for b, L in enumerate(lens):
            alone = ops.stft(torch.from_numpy(rows[b])[None].to(gpu), 1.0, tpad=64, mode=mode, in_div=div[b:b + 1])
            assert torch.equal(out[b], alone[0]), (mode, L)
            T = 1 + L // 128
            ref = spec_ref.stft(rows[b].astype(np.float64) / float(div[b]))[0]
            ref = spec_ref.spec_fwd(ref) if mode == 1 else ref
            err = rel(out[b, :, :T], ref)
            print(f"ragged stft mode {mode} L {L}: rel RMS vs fp64 oracle {err:.2e}")
            assert err < 1e-5, (mode, L, err)
            assert (out[b, :, T:] == 0).all() and out[b, :, T:].numel() == 256 * (64 - T)
    # a clip too short to reflect, and one with more frames than tpad, are refused before any launch
    with pytest.raises(RuntimeError, match="snrse_stft_ragged"):
        ops.stft(buf, 1.0, tpad=64, mode=0, lengths=(255, 300, 1000, 8191))
    with pytest.raises(RuntimeError, match="snrse_stft_ragged"):
        ops.stft(buf, 1.0, tpad=32, mode=0, lengths=lens)
    with pytest.raises(ValueError):
        ops.stft(buf, 1.0, tpad=128, mode=0, lengths=(256, 300, 1000, 8192))  # longer than the row stride
    am = ops.absmax(buf, lengths=lens).cpu()
    for b in range(4):
        assert float(am[b]) == float(np.abs(rows[b]).max())
        assert float(am[b]) == float(ops.absmax(torch.from_numpy(rows[b])[None].to(gpu))[0])
    sh = [(0.9 * r + 0.05 * fnormal(f"t.rag.h.{len(r)}", (len(r),))).astype(np.float32) for r in rows]
    nz = [(0.3 * fnormal(f"t.rag.n.{len(r)}", (len(r),))).astype(np.float32) for r in rows]
    er = ops.energy_ratios(ragged(sh, gpu), buf, ragged(nz, gpu), lengths=lens).cpu().numpy()
    er1 = ops.energy_ratios(ragged(sh, gpu), buf, lengths=lens).cpu().numpy()
    for b in range(4):
        one = ops.energy_ratios(*(torch.from_numpy(v[b])[None].to(gpu) for v in (sh, rows, nz))).cpu().numpy()[0]
        np.testing.assert_allclose(er[b], one, rtol=0, atol=1e-6)
        np.testing.assert_allclose(er1[b, 0], one[0], rtol=0, atol=1e-6)
    assert np.isfinite(er).all() and np.isnan(er1[:, 1:]).all()


def test_row_seeded_noise_equals_legacy_single_row_calls(gpu):
    from snrse import ops
    B, F, T = 3, 256, 64
    HW = F * T
    seeds = (11, 22, 33)
    rs = torch.tensor(seeds, dtype=torch.int64, device=gpu)
    x = torch.from_numpy(fnormal("t.rs.x", (B, F, T), complex_=True)).to(gpu)
    y = torch.from_numpy(fnormal("t.rs.y", (B, F, T), complex_=True)).to(gpu)
    sc = torch.from_numpy(fnormal("t.rs.s", (B, F, T), complex_=True)).to(gpu)
    pyr = torch.from_numpy(fnormal("t.rs.pyr", (B, F, T, 4))).to(gpu)
    ow = torch.from_numpy(fnormal("t.rs.ow", (2, 4))).to(gpu).contiguous()
    ob = torch.from_numpy(fnormal("t.rs.ob", (2,))).to(gpu)
    t = torch.tensor([0.3, 0.6, 0.9], device=gpu)
    coef = torch.tensor([[1.0, 0.1, 0.02, 0.3], [0.9, 0.2, 0.03, 0.5], [1.1, -0.1, 0.01, 0.7]], device=gpu)
    # legacy calls draw what they always drew: Philox(seed, offset + index) over the whole batch
    leg = ops.axpby_noise(coef, x=x, y=y, seed=11, offset=5)
    leg0 = ops.axpby_noise(coef[:1], x=x[:1], y=y[:1], seed=11, offset=5)
    leg1 = ops.axpby_noise(coef[1:2], x=x[1:2], y=y[1:2], seed=11, offset=5 + HW)
    assert torch.equal(leg[0], leg0[0]) and torch.equal(leg[1], leg1[0])
    for draw in (0, 3):
        a = ops.axpby_noise(coef, x=x, y=y, row_seeds=rs, offset=draw)
        so, sm = ops.sde_update(x, coef, y=y, score=sc, row_seeds=rs, offset=draw)
        uo, um, us = ops.score_update(pyr, ow, ob, t, 0, x, y, coef=coef, row_seeds=rs, offset=draw, want_score=True)
        for b, s in enumerate(seeds):
            k = slice(b, b + 1)
            a1 = ops.axpby_noise(coef[k], x=x[k].contiguous(), y=y[k].contiguous(), seed=s, offset=draw * HW)
            assert torch.equal(a[b], a1[0]), ("axpby", draw, b)
            so1, sm1 = ops.sde_update(x[k].contiguous(), coef[k], y=y[k].contiguous(), score=sc[k].contiguous(),
                                      seed=s, offset=draw * HW)
            assert torch.equal(so[b], so1[0]) and torch.equal(sm[b], sm1[0]), ("sde", draw, b)
            uo1, um1, us1 = ops.score_update(pyr[k].contiguous(), ow, ob, t[k].contiguous(), 0, x[k].contiguous(),
                                             y[k].contiguous(), coef=coef[k], seed=s, offset=draw * HW,
                                             want_score=True)
            assert torch.equal(uo[b], uo1[0]) and torch.equal(um[b], um1[0]) and torch.equal(us[b], us1[0]), \
                ("score", draw, b)
        # the rows really differ (different keys) and so do the draws
        assert not torch.equal(a[0] - coef[0, 0] * x[0] - coef[0, 1] * y[0], a[1] - coef[1, 0] * x[1] - coef[1, 1] * y[1])
    d0 = ops.axpby_noise(coef, x=x, y=y, row_seeds=rs, offset=0)
    d3 = ops.axpby_noise(coef, x=x, y=y, row_seeds=rs, offset=3)
    assert not torch.equal(d0, d3)


@pytest.fixture(scope="module")
def pc_setup(gpu):
    """One fp32 bbed model, three clips of one Tpad-64 bucket, and each clip enhanced alone (the reference the
    ragged runs are held to), computed once."""
    from snrse import sampler
    from snrse.enhance import PCEnhancer
    m = score_model("bbed", dtype="fp32")
    enh = PCEnhancer(m.dnn.hip(gpu), m.sde.copy().spec(), N=2, eps=m.t_eps, snr=0.5, corrector="ald")
    lens = (5000, 6311, 8064)
    seeds = (1234567, 2 ** 61 + 5, 42)
    ys = [clip(L, k) for k, L in enumerate(lens)]
    alone = []
    for y, s in zip(ys, seeds):
        xh, nfe = enh(torch.from_numpy(y)[None].to(gpu), sampler.NoiseSource(seed=s))
        assert nfe == 4
        alone.append(xh[0].cpu().numpy())
    return enh, lens, seeds, ys, alone


@pytest.mark.parametrize("perm", [(0, 1, 2), (2, 0, 1)])
def test_pc_ragged_batch_matches_each_utterance_alone(gpu, pc_setup, perm):
    """<= 1e-4 relative RMS per utterance (the project's fp32 bound, as test_gpu_deep_eval), in input order and
    with the rows permuted: a row's result depends on neither its batch nor its place in it."""
    from snrse import sampler
    enh, lens, seeds, ys, alone = pc_setup
    rows = [ys[i] for i in perm]
    ln = [lens[i] for i in perm]
    src = sampler.NoiseSource(row_seeds=[seeds[i] for i in perm])
    xh, nfe = enh(ragged(rows, gpu), src, lengths=ln)
    assert nfe == 4 and xh.shape == (3, max(lens)) and src.i == 5  # prior + 2 x (corrector, predictor)
    xh = xh.cpu().numpy()
    assert np.isfinite(xh).all()
    for r, i in enumerate(perm):
        err = rel(xh[r, :lens[i]], alone[i])
        print(f"pc ragged perm {perm} utterance {i} (row {r}): rel RMS vs alone {err:.2e}")
        assert err < 1e-4, (perm, i, err)
        assert (xh[r, lens[i]:] == 0).all()


def test_pc_ragged_batch_refuses_mixed_tpad(gpu, pc_setup):
    enh = pc_setup[0]
    with pytest.raises(ValueError, match="Tpad"):
        enh(ragged([clip(8191, 0), clip(8192, 1)], gpu), lengths=(8191, 8192))


def test_snr_aligned_ragged_batch_matches_each_utterance_alone(gpu):
    """One Tpad-64 batch whose rows have T = 40, 50, 64 frames (SNRNet sub-groups of 48 and 64 frames): t_hat
    equal to the per-utterance values, waveforms <= 1e-4 relative RMS."""
    from sgmse.backbones import SNRNet
    from snrse.enhance import SNRAlignedEnhancer
    net = SNRNet()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in formula_sd("snrnet", "snrnet.").items()})

    def snr_fn(spec):
        g = net.forward_complex(spec)[:, 0]
        return g / (1 - g)

    m = score_model("sebridge_v3", "true", fixed_snr=0.17783)
    enh = SNRAlignedEnhancer(m.dnn.hip(gpu), snr_fn=snr_fn, fixed_snr=0.17783, sigma_max=float(m.sigma_max))
    lens = (39 * 128 + 17, 49 * 128 + 100, 63 * 128 + 127)
    assert [1 + L // 128 for L in lens] == [40, 50, 64]
    seeds = (5, 6, 2 ** 62 - 1)
    ys = [clip(L, k) for k, L in enumerate(lens)]
    # the estimator's input: rows 1 and 2 share the 64-frame sub-group, row 0 has its own 48-frame one
    from snrse import ops
    from snrse.batching import snr_groups
    assert snr_groups(lens) == [(48, [0]), (64, [1, 2])]
    pair = ops.stft(ragged(ys[1:], gpu), 1.0, tpad=64, mode=0, lengths=lens[1:])
    g = net.forward_complex(pair)[:, 0].cpu().numpy()  # SNRNet's output g in (0, 1); fp32, rows independent
    for k in (1, 2):
        one = net.forward_complex(ops.stft(torch.from_numpy(ys[k])[None].to(gpu), 1.0, tpad=64, mode=0))[:, 0]
        np.testing.assert_allclose(g[k - 1], one.cpu().numpy()[0], rtol=1e-5)
    xh, t_hat = enh(ragged(ys, gpu), lengths=lens, row_seeds=torch.tensor(seeds, dtype=torch.int64, device=gpu))
    xh = xh.cpu().numpy()
    assert t_hat.shape == (3,) and np.isfinite(xh).all()
    for k, (y, s) in enumerate(zip(ys, seeds)):
        x1, t1 = enh(torch.from_numpy(y)[None].to(gpu), seed=s)
        assert t_hat[k] == t1[0], (k, t_hat[k], t1[0])
        err = rel(xh[k, :lens[k]], x1[0].cpu())
        print(f"snr-aligned ragged utterance {k}: t_hat {t_hat[k]:.6f}, rel RMS vs alone {err:.2e}")
        assert err < 1e-4, (k, err)
        assert (xh[k, lens[k]:] == 0).all()


def test_evaluate_driver_batched_matches_per_file_loop(gpu, tmp_path):
    """Four files in two Tpad buckets (interleaved): evaluate(batch_size=4) against evaluate(batch_size=1) under
    the same torch.manual_seed -- same names and order, float waveforms <= 1e-4 per file, each mode's csv metrics
    equal to numpy on its own waveform (1e-5 dB), the wav files the PCM16 of the batch waveforms."""
    from snrse import audio, evaluate
    from test_metrics import np_energy_ratios
    root = tmp_path / "test"
    for d in ("clean", "noisy"):
        os.makedirs(root / d)
    lens = (7000, 9000, 8100, 12000)  # Tpad 64, 128, 64, 128
    rng = np.random.default_rng(3)
    for k, L in enumerate(lens):
        c = (0.2 * np.sin(np.arange(L) * (0.02 + 0.01 * k))).astype(np.float32)
        y = (c + 0.05 * rng.standard_normal(L)).astype(np.float32)
        audio.write_wav(str(root / "clean" / f"f{k}.wav"), c, bits=32)
        audio.write_wav(str(root / "noisy" / f"f{k}.wav"), y, bits=32)
    m = score_model("bbed", dtype="fp32")
    loop_out, batch_out, batch_calls = [], {}, []
    enhance, enhance_batch = m.enhance, m.enhance_batch

    def rec_enhance(x, y, **kw):
        r = enhance(x, y, **kw)
        loop_out.append(r)
        return r

    def rec_batch(ys, **kw):
        r = enhance_batch(ys, **kw)
        batch_calls.append([len(y) for y in ys])
        for y, h in zip(ys, r):
            batch_out[len(y)] = h
        return r

    m.enhance, m.enhance_batch = rec_enhance, rec_batch
    torch.manual_seed(7)
    d1 = evaluate.evaluate(m, str(root), str(tmp_path / "o1"), N=2, batch_size=1)
    assert len(loop_out) == 4 and not batch_calls
    torch.manual_seed(7)
    d4 = evaluate.evaluate(m, str(root), str(tmp_path / "o4"), N=2, batch_size=4)
    assert len(loop_out) == 4 and batch_calls == [[7000, 8100], [9000, 12000]]
    assert d1["filename"] == d4["filename"] == [f"f{k}.wav" for k in range(4)]
    for k, L in enumerate(lens):
        hb = batch_out[L]
        err = rel(hb, loop_out[k])
        print(f"driver file {k}: batch_size 4 vs per-file loop rel RMS {err:.2e}")
        assert hb.shape == loop_out[k].shape == (L,) and err < 1e-4, (k, err)
        x, _ = audio.load(str(root / "clean" / f"f{k}.wav"))
        y, _ = audio.load(str(root / "noisy" / f"f{k}.wav"))
        for data, h, out in ((d1, loop_out[k], "o1"), (d4, hb, "o4")):
            ref = np_energy_ratios(h, x[0].numpy(), (y - x)[0].numpy())
            np.testing.assert_allclose([data["si_sdr"][k], data["si_sir"][k], data["si_sar"][k]], ref, atol=1e-5)
            xh, _ = audio.load(str(tmp_path / out / "all" / f"f{k}.wav"))
            pcm = np.clip(np.round(h * 32768.0), -32768, 32767) / 32768.0
            np.testing.assert_array_equal(xh[0].numpy(), pcm.astype(np.float32))
        assert np.isnan(d4["pesq"][k]) == (evaluate._pesq_fn() is None)
    assert (tmp_path / "o4" / "_results.csv").exists()


def test_range_guard_fallback_redraws_the_row_seeded_noise(gpu):
    """A row-seeded batch whose rows overflow fp16 (module 4's weights x 1e6, as test_gpu_range_guard): the
    fallback re-run draws what the first run drew, so each row matches the bf16 run of that utterance ALONE under
    its own seed within the project's bound for a 16-bit computation under another batch split (2e-2 per row);
    noise from any other key or draw index is an O(1) difference."""
    from snrse import guard, ncsnpp, sampler
    from snrse.enhance import PCEnhancer
    sd = {k: torch.from_numpy(v) for k, v in formula_sd("ncsnpp").items()}
    for k in ("all_modules.4.Conv_1.weight", "all_modules.4.Conv_1.bias"):
        sd[k] = sd[k] * 1e6
    sde = sampler.SDESpec("ouve", theta=1.5, sigma_min=0.05, sigma_max=0.5)
    Y = (torch.from_numpy(fnormal("batch.guard.Y", (2, 256, 64), complex_=True)) * 0.5).to(gpu)
    seeds = (77, 2 ** 60 + 3)
    enh = PCEnhancer(ncsnpp.NCSNppHIP(sd, dtype=torch.float16, device=gpu), sde, N=2, guard="fallback")
    src = sampler.NoiseSource(row_seeds=seeds)
    with pytest.warns(guard.RangeFallbackWarning):
        x, _ = enh.sample(Y, src)
    assert enh.last_guard["flagged"] == [0, 1] and torch.isfinite(torch.view_as_real(x)).all() and src.i == 5
    ref = PCEnhancer(ncsnpp.NCSNppHIP(sd, dtype=torch.bfloat16, device=gpu), sde, N=2, guard=None)
    for b, s in enumerate(seeds):
        alone, _ = ref.sample(Y[b:b + 1].contiguous(), sampler.NoiseSource(seed=s))
        err = rel(x[b], alone[0])
        print(f"guard fallback row {b}: rel RMS vs the bf16 run alone {err:.2e}")
        assert err < 2e-2, (b, err)
