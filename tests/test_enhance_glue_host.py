"""Host side of the layer between the C ABI and the command lines (no GPU): the SNR branch's scalars, which
ScoreModel.enhance and SNRAlignedEnhancer share, against the reference's own formulas; the row packer every padding
site uses; the drivers' reverse-start prelude and the PESQ-or-NaN rule."""
import types

import numpy as np
import pytest
import torch

FIXED_SNRS = (0.17783, 1.0)


def test_snap_and_normfac_are_the_reference_formulas_bit_for_bit():
    """enhance.snap_t / normfac (numpy, per batch) against ScoreModel.calculate_snr_direct / calculate_normfac_direct
    (the reference API, Python floats, one utterance) as ScoreModel.enhance applied them: the nearest point of the
    reference's t_30 grid (model.py:22-23) and the norm factor there, equal in every bit of the float64 on all 30
    grid values, and the snap also half way between neighbours and outside the grid."""
    from sgmse.model import ScoreModel
    from snrse import enhance
    i_30 = np.arange(1, 30 + 1)
    t_30 = (0.001 ** (1 / 7) + (i_30 - 1) / (30 - 1) * (1 ** (1 / 7) - 0.001 ** (1 / 7))) ** 7
    assert enhance.T_30.dtype == np.float64 and np.array_equal(enhance.T_30, t_30)
    probes = np.concatenate([t_30, 0.5 * (t_30[1:] + t_30[:-1]), [0.0, 1e-6, 2.5]])
    for fs in FIXED_SNRS:
        est = probes * (10 ** 0.25 * fs)  # the estimated SNRs whose calculate_snr_direct lands on the probes
        want_t = [float(t_30[np.abs(t_30 - ScoreModel.calculate_snr_direct(None, 1.0, float(e), fs)).argmin()])
                  for e in est]
        got_t = enhance.snap_t(est, fs)
        assert got_t.dtype == np.float64 and got_t.tolist() == want_t
        assert [float(enhance.snap_t(float(e), fs)[0]) for e in est] == want_t  # one utterance at a time
        want_n = [float(ScoreModel.calculate_normfac_direct(None, 1.0, 10 ** 0.25 * fs * float(t), fs)) for t in t_30]
        got_n = enhance.normfac(t_30, fs)
        assert got_n.dtype == np.float64 and got_n.tolist() == want_n
        assert [float(enhance.normfac(float(t), fs)) for t in t_30] == want_n


def test_pack_rows_lengths_zero_fill_and_empty_rows():
    from snrse.batching import pack_rows
    sigs = [np.arange(1, 6, dtype=np.float32), torch.arange(1, 4, dtype=torch.float64), np.zeros(0, np.float32),
            np.full((1, 7), 2.0, np.float32)]
    buf, lens = pack_rows(sigs)
    assert lens == [5, 3, 0, 7] and buf.shape == (4, 7) and buf.dtype == torch.float32 and not buf.is_cuda
    assert buf.is_contiguous()
    for b, s in enumerate(sigs):
        assert torch.equal(buf[b, :lens[b]], torch.as_tensor(s).reshape(-1).float())
        assert (buf[b, lens[b]:] == 0).all()
    # nothing but empty rows still has a column: the resampler's launch takes a buffer with a row stride
    buf, lens = pack_rows([np.zeros(0, np.float32), torch.zeros(0)])
    assert lens == [0, 0] and buf.shape == (2, 1) and (buf == 0).all()
    # rows of one length: the plain stack
    buf, lens = pack_rows([np.ones(4, np.float32)] * 3)
    assert lens == [4, 4, 4] and torch.equal(buf, torch.ones(3, 4))


def test_reverse_start_sets_the_sde_and_scales_n():
    from snrse.evaluate import reverse_start

    class OUVESDE:
        T, _T = "untouched", None

    class BBEDSDE:
        T, _T = None, "untouched"

    ouve, bbed = types.SimpleNamespace(sde=OUVESDE()), types.SimpleNamespace(sde=BBEDSDE())
    assert reverse_start(ouve, 0.5, 30) == 15 and ouve.sde._T == 0.5 and ouve.sde.T == "untouched"
    assert reverse_start(bbed, 0.5, 30) == 15 and bbed.sde.T == 0.5 and bbed.sde._T == "untouched"
    assert reverse_start(bbed, 1.0, 30, 0) == 30 and bbed.sde.T == 1.0
    assert reverse_start(bbed, 0.7, 30) == int(0.7 / (1 / 30))  # the reference's own rounding (eval.py:109)
    assert reverse_start(ouve, 0.5, 30, force_N=7) == 7 and ouve.sde._T == 0.5  # force_N wins, T is still set


def test_pesq_or_nan():
    from snrse.evaluate import pesq_or_nan
    ref, deg = np.zeros(4, np.float32), np.ones(4, np.float32)
    assert np.isnan(pesq_or_nan(None, 16000, ref, deg))  # the package is not installed

    def boom(*a):
        raise RuntimeError("No utterances detected")

    assert np.isnan(pesq_or_nan(boom, 16000, ref, deg))  # the reference records NaN for any failure
    calls = []

    def fake(sr, r, d, mode):
        calls.append((sr, r is ref, d is deg, mode))
        return np.float32(2.5)

    got = pesq_or_nan(fake, 16000, ref, deg)
    assert got == 2.5 and type(got) is float and calls == [(16000, True, True, "wb")]
    with pytest.raises(KeyboardInterrupt):  # not an Exception: a run can still be interrupted
        pesq_or_nan(lambda *a: (_ for _ in ()).throw(KeyboardInterrupt()), 16000, ref, deg)
