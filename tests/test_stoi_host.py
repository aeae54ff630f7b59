"""CPU tests of STOI's host side: the float64 restatement (tests/stoi_np.py) answers its own known questions -- the band
table, the resampler's length, stoi(x, x) = 1, 1e-5 below 30 spectral frames, the frame-count formulas, a score that
falls as noise rises -- and rced_stoi is declared, exported, bound and refuses bad arguments without a device."""

import ctypes
import os
import re

import numpy as np
import pytest

import stoi_np as sn
from conftest import ROOT

BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219)]


def test_band_table():
    obm, edges = sn.thirdoct()
    assert edges == BANDS
    assert obm.shape == (15, 257) and obm.sum() == sum(hi - lo for lo, hi in BANDS) == 212
    assert not obm[:, :7].any() and not obm[:, 219:].any()       # only bins 7..218 are ever needed


def test_resampler_taps_and_length():
    h = sn.resample_window(10000, 8000)
    assert len(h) == 365 and np.array_equal(h, h[::-1]) and h.argmax() == 182
    for L in (1, 4, 5, 204, 205, 1001, 24000):
        assert len(sn.resample(np.ones(L), 8000)) == -(-5 * L // 4)
    # unit gain in the pass band: a constant stays a constant away from the edges
    assert np.abs(sn.resample(np.ones(4000), 8000)[400:-400] - 1).max() < 1e-3


def test_identity_scores_one():
    x = sn.speechlike(24000, 0)
    d, (F, K, M), e = sn.stoi_detail(x, x, 8000)
    assert abs(d - 1) <= 1e-12
    assert (F, K, M) == (233, 128, 98) and len(e) == F         # silent-frame removal really removes frames
    assert abs(sn.stoi(x, 0.5 * x, 8000) - 1) <= 1e-12           # the per-segment normalisation takes a gain out


def test_too_short_gives_1e_5():
    rng = np.random.default_rng(2)
    for L, fs, counts in ((0, 8000, (0, 0, 0)), (204, 8000, (0, 0, 0)), (256, 10000, (0, 0, 0)), (4096, 10000, (30, 30, 0))):
        x = rng.standard_normal(L)
        d, det, _ = sn.stoi_detail(x, x + 0.1 * rng.standard_normal(L), fs)
        assert d == 1e-5 and det == counts, (L, fs, d, det)
    x = rng.standard_normal(4097)                                # one more sample: 31 frames, 30 spectra, one segment
    d, det, _ = sn.stoi_detail(x, x, 10000)
    assert det == (31, 31, 1) and abs(d - 1) <= 1e-12


def test_frame_counts():
    rng = np.random.default_rng(3)
    for L10 in (257, 384, 385, 5000, 12345):
        x = rng.standard_normal(L10)                             # stationary: every frame is kept
        F = -(-(L10 - 256) // 128)
        _, (f, k, m), e = sn.stoi_detail(x, x, 10000)
        assert (f, k, m) == (F, F, F - 30 if F - 1 >= 30 else 0) and len(e) == F
    x = sn.speechlike(9000, 4)
    L10 = -(-5 * 9000 // 4)
    _, (f, k, m), _ = sn.stoi_detail(x, x, 8000)
    assert f == -(-(L10 - 256) // 128) and 30 < k < f and m == k - 30


def test_all_zero_clean_scores_zero():
    y = np.random.default_rng(5).standard_normal(8000)
    d, (F, K, M), _ = sn.stoi_detail(np.zeros(8000), y, 10000)
    assert d == 0 and F == K == 61 and M == 31


def test_score_falls_as_noise_rises():
    rng = np.random.default_rng(0)
    x = sn.speechlike(24000, rng)
    scores = [sn.stoi(x, sn.add_white(x, snr, rng), 8000) for snr in (20, 10, 0, -5)]
    print("STOI at 20, 10, 0, -5 dB:", scores)
    assert all(a > b for a, b in zip(scores, scores[1:]))
    assert np.abs(np.array(scores) - [0.947, 0.777, 0.580, 0.458]).max() < 1e-3
    xr = sn.resample(x, 8000)
    e = sn.frame_energies(xr)
    assert np.abs(e - (e.max() - 40)).min() > 0.5                # no frame sits at the threshold


def test_entry_is_declared_exported_and_bound(built):
    from fullycnnspeechenhancement_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rced.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.SO_PATH)
    assert re.search(r"\bint\s+rced_stoi\s*\(", src)
    assert hasattr(lib, "rced_stoi")
    assert "rced_stoi" in _lib.SYMBOLS and _lib.load().rced_stoi.restype is ctypes.c_int
    assert len(_lib.SYMBOLS["rced_stoi"][1]) == 11


def test_bad_arguments_are_refused_before_any_device_is_touched(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = 4096                      # never dereferenced on the host
    ARG = _lib.RCED_ERR_ARG
    assert lib.rced_stoi(None, 8, p, 8, None, 1, 8000, p, None, 0, None) == ARG
    assert lib.rced_stoi(p, 8, None, 8, None, 1, 8000, p, None, 0, None) == ARG
    assert lib.rced_stoi(p, 8, p, 8, None, 1, 8000, None, None, 0, None) == ARG
    assert b"null pointer" in lib.rced_last_error()
    assert lib.rced_stoi(p, 8, p, 8, None, -1, 8000, p, None, 0, None) == ARG
    assert lib.rced_stoi(p, -8, p, 8, None, 1, 8000, p, None, 0, None) == ARG
    assert lib.rced_stoi(p, 8, p, -8, None, 1, 8000, p, None, 0, None) == ARG
    for fs in (16000, 0, 44100, -8000):
        assert lib.rced_stoi(p, 8, p, 8, None, 1, fs, p, None, 0, None) == ARG
        assert b"fs_sig" in lib.rced_last_error()
    assert lib.rced_stoi(p, 8, p, 8, None, 70000, 8000, p, None, 0, None) == ARG
    assert lib.rced_stoi(p, 8, p, 8, None, 0, 8000, p, None, 0, None) == 0           # nothing to do
    assert lib.rced_stoi(p, 8, p, 8, None, 0, 10000, p, p, 0, None) == 0


def test_entry_fails_loudly_without_gpu(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    if torch.cuda.is_available():
        return                    # with a device this call would run: tests/test_stoi_gpu.py
    lib, p = _lib.load(), 4096
    assert lib.rced_stoi(p, 8, p, 8, None, 1, 8000, p, None, 0, None) == _lib.RCED_ERR_HIP
    assert b"no CPU fallback" in lib.rced_last_error()


def test_python_surface_and_argument_checks():
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd.metrics import STOI
    assert hasattr(pkg.audio, "stoi_batch") and hasattr(pkg.metrics, "STOI")
    with pytest.raises(ValueError):
        STOI()(np.zeros((2, 8)), np.zeros((2, 8)))
    with pytest.raises(ValueError):
        STOI()(np.zeros(8), np.zeros(9))
    with pytest.raises(ValueError):
        STOI(sr=16000)
    with pytest.raises(ValueError):
        pkg.audio.stoi_batch(np.zeros((1, 8)), np.zeros((1, 8)))                     # not device tensors
    import inspect
    for fn in (pkg.audio.denoise_and_score, pkg.engine.evaluate_pcm, pkg.FullyCNNTester.evaluate_pcm, pkg.FullyCNNTester.test,
               pkg.FullyCNNTrainer.valid):
        assert inspect.signature(fn).parameters["stoi"].default is False
