"""Host checks of the long-recording window layer (snrse/longform.py): the plan's invariants by brute force, the
worked examples, the argument validation, the seed derivation, the fade table, the enhance_files flags and the
library's declarations.  No device."""
import inspect
import os

import numpy as np
import pytest

import window_ref
from conftest import ROOT

GRIDS = [(8064, 1536, 1), (8064, 256, 1), (8064, 2016, 1), (1024, 256, 1), (2048, 512, 1), (65408, 8192, 13)]


@pytest.mark.parametrize("W,V,step", GRIDS)
def test_plan_invariants(W, V, step):
    from snrse import longform
    H = W - V
    for L in range(W + 1, 7 * W + 1, step):
        s = np.asarray(longform.window_starts(L, W, V), dtype=np.int64)
        K = len(s)
        assert K == -((V - L) // H) and K >= 2, L
        assert s[0] == 0 and s[-1] == L - W, L
        gaps = np.diff(s)
        assert gaps.min() >= 1, L                  # strictly ascending
        assert gaps.max() <= H, L                  # window k - 1 covers window k's fade region
        assert K < 3 or gaps.min() >= V, L         # fade regions never overlap
    for L in (W + 1, W + 77, 2 * W, 3 * W + 5, 7 * W):
        assert longform.window_starts(L, W, V) == window_ref.starts(L, W, V)


def test_worked_examples():
    from snrse import longform
    assert longform.window_starts(20000, 8064, 1536) == [0, 5968, 11936]
    assert longform.window_starts(8065, 8064, 1536) == [0, 1]
    assert longform.window_starts(21121, 8064, 1536) == [0, 4352, 8705, 13057]
    assert longform.geometry(64, 12) == (8064, 1536, 6528)
    assert longform.geometry(512, 64) == (65408, 8192, 57216)


def test_short_recording_is_one_window():
    from snrse import longform
    for L in (256, 7000, 8063, 8064):
        assert longform.window_starts(L, 8064, 1536) == [0]
    p = longform.Plan([7000, 20000, 8064], 64, 12)
    assert p.first == [0, 1, 4, 5] and p.counts() == [1, 3, 1] and len(p) == 5
    assert p.table.dtype == np.int32
    assert p.table.tolist() == [[0, 0, 7000], [1, 0, 8064], [1, 5968, 8064], [1, 11936, 8064], [2, 0, 8064]]
    assert p.utt == [0, 1, 1, 1, 2] and p.k == [0, 0, 1, 2, 0]


def test_validation_names_the_argument():
    from snrse import longform
    for wf in (0, 63, 100, -64, 64.5):
        with pytest.raises(ValueError, match="window_frames"):
            longform.geometry(wf, 12)
    for of in (0, 1, -3, 2.5):
        with pytest.raises(ValueError, match="overlap_frames"):
            longform.geometry(64, of)
    with pytest.raises(ValueError, match="overlap_frames"):
        longform.geometry(64, 16)  # 4 V = 8192 > W = 8064
    assert longform.geometry(64, 15)[1] == 1920
    with pytest.raises(ValueError, match="overlap_frames"):
        longform.geometry(512, 128)


def test_enhance_batch_validates_before_any_device_work():
    """The windowed call checks its arguments first: these raise ValueError here, where no device exists."""
    from sgmse.model import ScoreModel
    m = ScoreModel(backbone="ncsnpp", sde="ouve", model_type="bbed", theta=1.5, sigma_min=0.05, sigma_max=0.5)
    y = np.zeros(20000, np.float32)
    with pytest.raises(ValueError, match="window_frames"):
        m.enhance_batch([y], window_frames=100)
    with pytest.raises(ValueError, match="overlap_frames"):
        m.enhance_batch([y], window_frames=64, overlap_frames=1)
    with pytest.raises(ValueError, match="overlap_frames"):
        m.enhance_long(y, window_frames=64, overlap_frames=16)
    with pytest.raises(ValueError, match="seeds"):
        m.enhance_batch([y], seeds=[1, 2], window_frames=64, overlap_frames=12)
    sig = inspect.signature(ScoreModel.enhance_batch)
    assert sig.parameters["window_frames"].default is None and sig.parameters["overlap_frames"].default == 64
    assert hasattr(ScoreModel, "enhance_long")


def test_window_seeds():
    from snrse import longform
    seeds = [0, 1, 123, 2 ** 61 + 9, 2 ** 62 - 1]
    for s in seeds:
        assert longform.window_seed(s, 0) == s
        ws = [longform.window_seed(s, k) for k in range(4096)]
        assert len(set(ws)) == len(ws)
        assert all(isinstance(v, int) and 0 <= v < 2 ** 62 for v in ws)
        assert ws == [longform.window_seed(s, k) for k in range(4096)]  # a function of (seed, k) alone
    # different utterances' windows differ too, and the plan hands out exactly these
    assert longform.window_seed(5, 1) != longform.window_seed(6, 1)
    p = longform.Plan([20000, 7000], 64, 12)
    assert p.seeds([11, 22]) == [11, longform.window_seed(11, 1), longform.window_seed(11, 2), 22]
    # pinned values: the derivation is part of the interface (results under a seed must not move)
    assert longform.window_seed(0, 1) == 0xE220A8397B1DCDAF >> 2


def test_fade_table():
    from snrse import longform
    for V in (256, 1536, 8192, 2016):
        t = longform.fade_table(V)
        assert t.dtype == np.float64 and t.shape == (V,)
        assert np.abs(t + t[::-1] - 1.0).max() <= 1e-15
        assert (np.diff(t) > 0).all() and 0 < t[0] < t[-1] < 1
        assert np.abs(t - window_ref.fade(V)).max() <= 1e-15


def test_reference_merge_of_gather_is_identity():
    """window_ref itself: cutting a signal and merging the untouched windows gives the signal back."""
    x = np.random.default_rng(0).standard_normal(5000)
    wins, st, lens = window_ref.gather(x, 1024, 256)
    out, _ = window_ref.merge(wins, st, len(x), 256)
    assert len(st) == 7 and np.abs(out - x).max() < 1e-14


def test_enhance_files_flags_default_off():
    from snrse import enhance_files
    base = ["--noisy_dir", "a", "--ckpt", "b", "--destination_folder", "c"]
    a = enhance_files.parser().parse_args(base)
    assert a.window_frames is None and a.overlap_frames == 64
    a = enhance_files.parser().parse_args(base + ["--window_frames", "512", "--overlap_frames", "32"])
    assert a.window_frames == 512 and a.overlap_frames == 32
    sig = inspect.signature(enhance_files.enhance_files)
    assert sig.parameters["window_frames"].default is None
    assert "windows" not in enhance_files.CSV_COLUMNS
    assert "--window_frames" in enhance_files.__doc__


def test_csv_windows_column_only_with_the_flag(tmp_path):
    from snrse import enhance_files
    files = [("x/long.wav", 62400, 2, 48000), ("x/short.wav", 7000, 1, 16000)]
    enhance_files.write_csv(files, "model", str(tmp_path))
    rows = (tmp_path / "_enhanced.csv").read_text().strip().split("\n")
    assert rows[0] == "filename,input_rate,channels,seconds,output_rate" and rows[1] == "long.wav,48000,2,1.3,16000"
    enhance_files.write_csv(files, "model", str(tmp_path), (64, 12))
    rows = (tmp_path / "_enhanced.csv").read_text().strip().split("\n")
    assert rows[0] == "filename,input_rate,channels,seconds,output_rate,windows"
    assert rows[1] == "long.wav,48000,2,1.3,16000,3" and rows[2] == "short.wav,16000,1,0.4375,16000,1"


def test_header_declares_the_window_kernels():
    """test_lib_abi's rule (header declarations == bindings == exports) covers the new entries because the header
    declares them."""
    from snrse import _lib
    with open(os.path.join(ROOT, "include", "snrse.h")) as f:
        hdr = f.read()
    for name in ("snrse_window_gather", "snrse_window_merge"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES
