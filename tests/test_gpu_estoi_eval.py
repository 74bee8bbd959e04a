"""ESTOI through the drivers (GPU): evaluate(estoi=True) in the per-file loop and at batch_size 4,
deep_evaluate(estoi=True) and evaluate_model(estoi=True), on formula weights and the one-step SNR-aligned model (one
NFE per file), three short synthetic files (estoi_ref.speechlike at 16 kHz: broadband, so every third-octave band
carries signal).  The columns are held to tests/estoi_ref.py on the float waveforms the drivers scored, by the
bound of test_gpu_estoi.py: 4 x |float32 mode - fp64| + 2^-24."""
import math
import os

import numpy as np
import pytest
import torch

import estoi_ref as er
from test_gpu_fit import _score_model, formula_snr_estimator  # noqa: F401  (fixture: the formula-weight estimator)

pytestmark = pytest.mark.gpu

LENS = (8000, 11000, 14000)  # 0.5 .. 0.9 s at 16 kHz: 38 .. 67 frames at 10 kHz


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """<root>/valid/{clean,noisy}/f{k}.wav + active_rms.txt (and an empty train set): a data module's base_dir whose
    valid directory is also an evaluation test_dir."""
    from snrse import audio
    root = tmp_path_factory.mktemp("estoi_tree")
    for sub in ("train", "valid"):
        for d in ("clean", "noisy"):
            os.makedirs(root / sub / d)
    rows = []
    for k, L in enumerate(LENS):
        c, y = er.speechlike(200 + k, L, 16000, (0.0, 10.0, 30.0)[k])
        audio.write_wav(str(root / "valid" / "clean" / f"f{k}.wav"), c, bits=32)
        audio.write_wav(str(root / "valid" / "noisy" / f"f{k}.wav"), y, bits=32)
        rows.append(f"f{k}.wav\t{float(np.sqrt(np.mean(c ** 2))):.6f}\t{float(np.sqrt(np.mean((y - c) ** 2))):.6f}")
    (root / "valid" / "active_rms.txt").write_text("\n".join(rows) + "\n")
    return root


def clean(tree, k):
    from snrse import audio
    return audio.load(str(tree / "valid" / "clean" / f"f{k}.wav"))[0][0].numpy()


def reference(x, h, what):
    """(fp64 ESTOI of the float waveform h against x at 16 kHz, the bound); the precondition asserted first."""
    L = min(len(x), len(h))
    ref, det = er.estoi(x[:L], np.asarray(h[:L], np.float32), 16000, details=True)
    assert det["margin"] >= 1e-3 and det["S"] > 0, (what, det["margin"], det["S"])
    return ref, 4.0 * abs(er.estoi(x[:L], np.asarray(h[:L], np.float32), 16000, dtype=np.float32) - ref) + 2.0 ** -24


def test_evaluate_estoi_column_loop_and_batched(gpu, tree, tmp_path, formula_snr_estimator):  # noqa: F811
    from snrse import evaluate
    m = _score_model(str(tree))
    loop_out, batch_out = [], {}
    enhance, enhance_batch = m.enhance, m.enhance_batch

    def rec_enhance(x, y, **kw):
        r = enhance(x, y, **kw)
        loop_out.append(np.asarray(r, np.float32))
        return r

    def rec_batch(ys, **kw):
        r = enhance_batch(ys, **kw)
        for y, h in zip(ys, r):
            batch_out[len(y)] = np.asarray(h, np.float32)
        return r

    m.enhance, m.enhance_batch = rec_enhance, rec_batch
    test_dir = str(tree / "valid")
    torch.manual_seed(7)
    d0 = evaluate.evaluate(m, test_dir, str(tmp_path / "o0"), batch_size=1)
    assert "estoi" not in d0 and len(loop_out) == 3
    assert open(tmp_path / "o0" / "_results.csv").readline().strip() == "filename,pesq,si_sdr,si_sir,si_sar"
    assert len(open(tmp_path / "o0" / "_avg_results.txt").read().splitlines()) == 4
    del loop_out[:]
    torch.manual_seed(7)
    d1 = evaluate.evaluate(m, test_dir, str(tmp_path / "o1"), batch_size=1, estoi=True)
    torch.manual_seed(7)
    d4 = evaluate.evaluate(m, test_dir, str(tmp_path / "o4"), batch_size=4, estoi=True)
    assert len(loop_out) == 3 and sorted(batch_out) == sorted(LENS)
    for d in (d1, d4):
        assert d["filename"] == [f"f{k}.wav" for k in range(3)] and len(d["estoi"]) == 3
        assert d["si_sdr"] != d["estoi"] and all(-1.0 <= v <= 1.0 for v in d["estoi"])
    np.testing.assert_allclose(d1["si_sdr"], d0["si_sdr"], atol=1e-3)  # the other columns: as without the option
    for out, d in (("o1", d1), ("o4", d4)):
        lines = open(tmp_path / out / "_results.csv").read().splitlines()
        assert lines[0] == "filename,pesq,si_sdr,si_sir,si_sar,estoi" and len(lines) == 4
        assert [float(ln.split(",")[5]) for ln in lines[1:]] == d["estoi"]
        avg = open(tmp_path / out / "_avg_results.txt").read().splitlines()
        assert len(avg) == 5 and avg[4].startswith("ESTOI: ") and "±" in avg[4]
        assert avg[4] == f"ESTOI: {evaluate.print_mean_std(d['estoi'])} "
    for k, L in enumerate(LENS):
        x = clean(tree, k)
        r1, b1 = reference(x, loop_out[k], ("loop", k))
        r4, b4 = reference(x, batch_out[L], ("batch", k))
        wave = float(np.sqrt(np.mean((batch_out[L].astype(np.float64) - loop_out[k]) ** 2) /
                             np.mean(loop_out[k].astype(np.float64) ** 2)))
        print(f"evaluate estoi file {k}: loop {d1['estoi'][k]:.9f} (ref {r1:.9f}, bound {b1:.2e}), batch_size 4 "
              f"{d4['estoi'][k]:.9f} (ref {r4:.9f}, bound {b4:.2e}); waveforms differ by {wave:.2e} relative RMS")
        assert abs(d1["estoi"][k] - r1) <= b1 and abs(d4["estoi"][k] - r4) <= b4
        # the two routes agree as closely as their waveforms do: the reference's own difference between the two
        # waveforms, plus each column's bound
        assert wave <= 1e-4
        assert abs(d1["estoi"][k] - d4["estoi"][k]) <= abs(r1 - r4) + b1 + b4


def test_deep_evaluate_estoi_columns(gpu, tree, tmp_path, formula_snr_estimator):  # noqa: F811
    from snrse import deep_evaluate as de
    one = tmp_path / "t"
    for d in ("clean", "noisy"):
        os.makedirs(one / d)
        os.symlink(tree / "valid" / d / "f1.wav", one / d / "f1.wav")
    m = _score_model(str(tree))
    outs, orig = [], de.enhance_variants

    def rec(*a, **kw):
        r = orig(*a, **kw)
        outs.append(r)
        return r

    de.enhance_variants = rec
    try:
        data = de.deep_evaluate(m, str(one), str(tmp_path / "o"), estoi=True, verbose=False)
        plain = de.deep_evaluate(m, str(one), str(tmp_path / "p"), verbose=False)
    finally:
        de.enhance_variants = orig
    assert list(plain) == ["filename"] + [f"pesq_{s}" for s in de.LABELS]
    assert list(data) == ["filename"] + [f"pesq_{s}" for s in de.LABELS] + [f"estoi_{s}" for s in de.LABELS]
    x = clean(tree, 1)
    for j, lab in enumerate(de.LABELS):
        ref, bound = reference(x, outs[0][j], ("deep", lab))
        print(f"deep_evaluate estoi_{lab}: {data[f'estoi_{lab}'][0]:.9f} (ref {ref:.9f}, bound {bound:.2e})")
        assert abs(data[f"estoi_{lab}"][0] - ref) <= bound
    head = open(tmp_path / "o" / "_results_deep.csv").read().splitlines()[0].split(",")
    assert head == list(data)
    avg = open(tmp_path / "o" / "_avg_results_deep.txt").read().splitlines()
    assert len(avg) == 18 and [ln.split(":")[0] for ln in avg[9:]] == [f"ESTOI_{s}" for s in de.LABELS]
    assert len(open(tmp_path / "p" / "_avg_results_deep.txt").read().splitlines()) == 9


def test_evaluate_model_estoi_is_the_mean_over_its_files(gpu, tree, formula_snr_estimator):  # noqa: F811
    from sgmse.util.inference import evaluate_model
    from snrse import ops
    m = _score_model(str(tree))
    m.data_module.setup(stage="fit")
    got, enhance_batch = [], m.enhance_batch

    def rec(ys, **kw):
        r = enhance_batch(ys, **kw)
        got.extend(np.asarray(h, np.float32) for h in r)
        return r

    m.enhance_batch = rec
    torch.manual_seed(5)
    _, si_sdr, st = evaluate_model(m, 3, estoi=True)
    assert len(got) == 3 and math.isfinite(si_sdr) and m.training
    alone = []
    for k in range(3):  # each file alone: a row's bits do not depend on the batch it is in
        x = clean(tree, k)
        L = min(len(x), len(got[k]))
        d = ops.estoi(torch.from_numpy(x[None, :L]).to(gpu), torch.from_numpy(got[k][None, :L]).to(gpu), fs=16000)
        alone.append(float(d[0]))
    assert st == float(np.mean(alone)), (st, alone)
    torch.manual_seed(5)
    assert math.isnan(evaluate_model(m, 3)[2])  # off: NaN, as before
    # the training loop's validation record: the number with the option, NaN (logged as null) without
    from snrse import fit
    m.enhance_batch = enhance_batch
    m.num_eval_files = 3
    on = fit.validate(m, limit_val_batches=1, estoi=True)
    assert -1.0 <= on["estoi"] <= 1.0 and on["estoi"] != 1e-5 and math.isfinite(on["si_sdr"])
    assert math.isnan(fit.validate(m, limit_val_batches=1)["estoi"])
