"""CPU tests of the three further scores of the evaluation loop: the float64 restatements (tests/estoi_np.py,
tests/td_metrics_np.py) answer the known questions of their definitions (DESIGN.md "ESTOI", "SI-SDR", "Segmental SNR"), and
rced_stoi_ex / rced_si_sdr / rced_seg_snr are declared, exported, bound and refuse bad arguments without a device."""

import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import estoi_np as en
import stoi_np as sn
import td_metrics_np as td
from conftest import ROOT

NEW = {"rced_stoi_ex": 13, "rced_si_sdr": 10, "rced_seg_snr": 11}


# ---- ESTOI ---------------------------------------------------------------------------------------------------------

def test_estoi_zero_rows_score_exactly_zero():
    y = np.random.default_rng(5).standard_normal(8000)
    d, counts, _ = en.estoi_detail(np.zeros(8000), y, 10000)
    assert d == 0 and counts == (61, 61, 31)
    assert en.estoi(y, np.zeros(8000), 10000) == 0


def test_estoi_identity_scores_one():
    """A column of unit-norm rows with norm q contributes (q / (q + EPS))^2 = 1 - 2 EPS / q by definition: 1 to 1e-15 where
    q is of the order of 1 (white noise: independent bands), 1 to a few 1e-15 where the bands move together and q is small
    (the gated harmonics)."""
    x = np.random.default_rng(1).standard_normal(8000)
    d, counts, _ = en.estoi_detail(x, x, 10000)
    assert abs(d - 1) <= 1e-15 and counts == (61, 61, 31)
    x = sn.speechlike(24000, 0)
    d, counts, _ = en.estoi_detail(x, x, 8000)
    assert abs(d - 1) <= 1e-14 and counts == (233, 128, 98)


def test_estoi_power_of_two_gain_leaves_the_bits():
    """Every step scales exactly under a power of two except `norm + EPS` of the rows: the bits are the same where EPS is
    under a quarter of an ulp of both norms, i.e. both are at least 4.  The test signals are scaled to make it so."""
    x = sn.speechlike(24000, 7)
    y = 8 * sn.add_white(x, 5, 8)
    for gain in (0.25, 4.0):
        assert min(en.min_row_norm(y, x, 8000), en.min_row_norm(gain * y, x, 8000)) >= 4
        assert en.estoi(x, gain * y, 8000) == en.estoi(x, y, 8000)


def test_estoi_rises_with_snr():
    x = sn.speechlike(24000, 7)
    snrs = (-10, 0, 10, 20, 40)
    scores = [en.estoi(x, sn.add_white(x, snr, 8), 8000) for snr in snrs]
    print("ESTOI at -10, 0, 10, 20, 40 dB:", scores)
    assert all(a < b for a, b in zip(scores, scores[1:]))
    assert abs(scores[0] - 0.087) < 1e-3 and abs(scores[-1] - 0.996) < 1e-3


def test_estoi_counts_are_stoi_np_s():
    rng = np.random.default_rng(2)
    for L, fs in ((0, 8000), (204, 8000), (256, 10000), (4096, 10000), (4097, 10000), (6017, 10000), (6145, 10000)):
        x = rng.standard_normal(L)
        y = x + 0.1 * rng.standard_normal(L)
        d, counts, e = en.estoi_detail(x, y, fs)
        _, ref_counts, ref_e = sn.stoi_detail(x, y, fs)
        assert counts == ref_counts and np.array_equal(e, ref_e)
        assert (d == 1e-5) == (counts[2] == 0)
    for seed, L in ((3, 9000), (4, 24001)):
        x = sn.speechlike(L, seed)
        y = sn.add_white(x, 3, seed + 10)
        for f32 in (False, True):
            assert en.estoi_detail(x, y, 8000, f32_dft=f32)[1] == sn.stoi_detail(x, y, 8000)[1]


def test_f32_emulation_is_close_to_the_restatement_and_not_equal_to_it():
    x = sn.speechlike(12000, 9)
    y = sn.add_white(x, 0, 10)
    a, b = en.estoi(x, y, 8000), en.estoi(x, y, 8000, f32_dft=True)
    assert 0 < abs(a - b) < 1e-6


# ---- SI-SDR --------------------------------------------------------------------------------------------------------

def test_si_sdr_equals_the_closed_form_on_a_poor_estimate():
    x = sn.speechlike(24000, 7)
    y = sn.add_white(x, 5, 8)
    d = td.si_sdr(x, y)
    assert abs(d - td.si_sdr_closed_form(x, y)) <= 1e-9
    assert 4.5 < d < 5.5                                          # white noise is nearly orthogonal to the signal
    alpha, target, residual = td.si_sdr_parts(x, y)
    assert abs(alpha - 1) < 0.02 and d == 10 * math.log10(target / residual)


def test_si_sdr_special_values():
    x = sn.speechlike(4000, 1)
    for k in (-3, 0, 1, 5):
        assert td.si_sdr(x, 2.0 ** k * x) == math.inf
    assert math.isnan(td.si_sdr(np.zeros(100), x[:100])) and math.isnan(td.si_sdr(x[:100], np.zeros(100)))
    assert math.isnan(td.si_sdr(x[:0], x[:0]))
    y = sn.add_white(x, 10, 2)
    assert abs(td.si_sdr(x, 3.7 * y) - td.si_sdr(x, y)) <= 1e-9    # the scale of the estimate is taken out
    assert td.si_sdr(x, y) != td.si_sdr(x + 0.1, y + 0.1)         # no mean removal


# ---- segmental SNR -------------------------------------------------------------------------------------------------

def test_seg_snr_cases():
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(239), rng.standard_normal(239)
    d, nf = td.seg_snr_detail(x, y, 8000)
    assert math.isnan(d) and nf == 0
    x = rng.standard_normal(240)
    assert td.seg_snr_detail(x, np.zeros(240), 8000) == (10 * np.log10(1 + td.EPS), 1)
    assert td.seg_snr_detail(np.zeros(300), np.ones(300), 8000) == (-10.0, 2)
    x = sn.speechlike(24000, 3)
    assert td.seg_snr_detail(x, x, 8000) == (35.0, (24000 - 240) // 60 + 1)
    assert td.seg_window(8000) == 240 and td.seg_window(16000) == 480 and td.seg_window(117) == 4 and td.seg_window(48016) == 1440
    for L, nf in ((299, 1), (300, 2), (359, 2), (360, 3)):
        assert td.seg_snr_detail(x[:L], x[:L], 8000)[1] == nf
    y = sn.add_white(x, 10, 5)
    assert -10 < td.seg_snr(x, y, 8000) < 35


# ---- the library and the Python surface ------------------------------------------------------------------------------

def test_entries_are_declared_exported_and_bound(built):
    from fullycnnspeechenhancement_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rced.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs
        assert getattr(_lib.load(), name).restype is ctypes.c_int
    assert re.search(r"#define\s+RCED_STOI_CLASSIC\s+1\b", src) and re.search(r"#define\s+RCED_STOI_EXTENDED\s+2\b", src)
    assert (_lib.STOI_CLASSIC, _lib.STOI_EXTENDED) == (1, 2)


def test_bad_arguments_are_refused_before_any_device_is_touched(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = 4096                      # never dereferenced on the host
    ARG = _lib.RCED_ERR_ARG
    # rced_stoi_ex: a requested output that is null, a mask outside {1, 2, 3}, and rced_stoi's own refusals
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 1, 8000, 1, None, p, None, 0, None) == ARG
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 1, 8000, 2, p, None, None, 0, None) == ARG
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 1, 8000, 3, p, None, None, 0, None) == ARG
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 1, 8000, 3, None, p, None, 0, None) == ARG
    assert b"null pointer" in lib.rced_last_error()
    for which in (0, 4, 7, -1):
        assert lib.rced_stoi_ex(p, 8, p, 8, None, 1, 8000, which, p, p, None, 0, None) == ARG
        assert b"which" in lib.rced_last_error()
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 1, 16000, 3, p, p, None, 0, None) == ARG
    assert lib.rced_stoi_ex(p, 8, p, 8, None, -1, 8000, 3, p, p, None, 0, None) == ARG
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 0, 8000, 2, None, p, None, 0, None) == 0      # nothing to do
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 0, 8000, 1, p, None, None, 0, None) == 0
    # rced_si_sdr
    assert lib.rced_si_sdr(None, 8, p, 8, None, 1, p, None, 0, None) == ARG
    assert lib.rced_si_sdr(p, 8, None, 8, None, 1, p, None, 0, None) == ARG
    assert lib.rced_si_sdr(p, 8, p, 8, None, 1, None, None, 0, None) == ARG
    assert lib.rced_si_sdr(p, -8, p, 8, None, 1, p, None, 0, None) == ARG
    assert lib.rced_si_sdr(p, 8, p, 8, None, 70000, p, None, 0, None) == ARG
    assert lib.rced_si_sdr(p, 8, p, 8, None, 0, p, None, 0, None) == 0
    # rced_seg_snr: frames of 4 .. 1440 samples only
    assert lib.rced_seg_snr(None, 8, p, 8, None, 1, 8000, p, None, 0, None) == ARG
    assert lib.rced_seg_snr(p, 8, p, 8, None, 1, 8000, None, None, 0, None) == ARG
    for fs in (0, -8000, 116, 48017, 96000, 2 ** 31 - 1):
        assert lib.rced_seg_snr(p, 8, p, 8, None, 1, fs, p, None, 0, None) == ARG
        assert b"fs = " in lib.rced_last_error()
    for fs in (117, 8000, 48016):
        assert lib.rced_seg_snr(p, 8, p, 8, None, 0, fs, p, None, 0, None) == 0


def test_entries_fail_loudly_without_gpu(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    if torch.cuda.is_available():
        return                    # with a device these calls would run: the GPU tests
    lib, p = _lib.load(), 4096
    assert lib.rced_stoi_ex(p, 8, p, 8, None, 1, 8000, 3, p, p, None, 0, None) == _lib.RCED_ERR_HIP
    assert lib.rced_si_sdr(p, 8, p, 8, None, 1, p, None, 0, None) == _lib.RCED_ERR_HIP
    assert lib.rced_seg_snr(p, 8, p, 8, None, 1, 8000, p, None, 0, None) == _lib.RCED_ERR_HIP
    assert b"no CPU fallback" in lib.rced_last_error()


def test_python_surface_and_argument_checks():
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd import evaluation
    from fullycnnspeechenhancement_amd.metrics import ESTOI, SISDR, SegSNR
    for name in ("si_sdr_batch", "seg_snr_batch", "stoi_batch", "EXTRA_METRICS"):
        assert getattr(pkg.audio, name) is getattr(evaluation, name)
    assert evaluation.EXTRA_METRICS == ("estoi", "si_sdr", "seg_snr")
    assert inspect.signature(pkg.audio.stoi_batch).parameters["extended"].default is False
    assert inspect.signature(pkg.audio.seg_snr_batch).parameters["sample_rate"].default == 8000
    for fn in (pkg.audio.denoise_and_score, pkg.engine.evaluate_pcm, pkg.FullyCNNTester.evaluate_pcm, pkg.FullyCNNTester.test,
               pkg.FullyCNNTrainer.valid):
        assert inspect.signature(fn).parameters["extra"].default == ()
    # bad rates
    for bad in (16000, 0, 44100):
        with pytest.raises(ValueError):
            ESTOI(sr=bad)
    for bad in (0, -8000, 116, 48017, 8000.5):
        with pytest.raises(ValueError):
            SegSNR(sr=bad)
        with pytest.raises(ValueError):
            pkg.audio.seg_snr_batch(None, None, sample_rate=bad)
    assert SegSNR(sr=16000).window == 480 and SegSNR().window == 240 and ESTOI(sr=10000).sr == 10000
    with pytest.raises(ValueError):
        pkg.audio.stoi_batch(None, None, extended="yes")
    # bad shapes, as SDR and STOI refuse them
    for metric in (ESTOI(), SISDR(), SegSNR()):
        with pytest.raises(ValueError):
            metric(np.zeros((2, 8)), np.zeros((2, 8)))
        with pytest.raises(ValueError):
            metric(np.zeros(8), np.zeros(9))
    assert ESTOI()(np.zeros(0), np.zeros(0)) == 1e-5 and math.isnan(SISDR()(np.zeros(0), np.zeros(0)))
    assert math.isnan(SegSNR()(np.zeros(0), np.zeros(0)))
    for fn in (pkg.audio.si_sdr_batch, pkg.audio.seg_snr_batch):
        with pytest.raises(ValueError):
            fn(np.zeros((1, 8)), np.zeros((1, 8)))                                   # not device tensors


def test_bad_extra_names_raise_before_any_device_work():
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd import evaluation

    def forward(_mag):
        raise AssertionError("the network must not run")

    sig = [np.zeros(1000, np.float32)]
    for bad in (("pesq",), ("estoi", "stoi"), ("si_sdr", "si_sdr"), "sdr", (1,)):
        with pytest.raises(ValueError):
            evaluation.check_extra(bad)
        with pytest.raises(ValueError):
            pkg.engine.evaluate_pcm(forward, sig, sig, extra=bad)
        with pytest.raises(ValueError):
            pkg.audio.denoise_and_score(forward, None, None, [1000], extra=bad)
        with pytest.raises(ValueError):
            pkg.FullyCNNTester.test(None, [(None, None, sig, sig)], extra=bad)
        with pytest.raises(ValueError):
            pkg.FullyCNNTrainer.valid(None, [(None, None, sig, sig)], 0, extra=bad)
    assert evaluation.check_extra(()) == () and evaluation.check_extra(["seg_snr", "estoi"]) == ("seg_snr", "estoi")
    assert evaluation.check_extra("si_sdr") == ("si_sdr",)
    # an empty batch comes back in the promised shape without a device
    den, sdr, st, more = pkg.engine.evaluate_pcm(forward, [], [], stoi=True, extra=("estoi", "seg_snr"))
    assert den == [] and sdr.shape == st.shape == (0,) and sorted(more) == ["estoi", "seg_snr"]
    assert all(v.dtype == np.float64 and v.shape == (0,) for v in more.values())
    assert len(pkg.engine.evaluate_pcm(forward, [], [])) == 2


def test_the_score_table_is_the_truth():
    """evaluation._EXTRA names every score `extra` takes and nothing else; the public tuples keep their values; every host
    mirror keeps its named method, and calling the mirror calls it."""
    from fullycnnspeechenhancement_amd import evaluation, metrics
    assert set(evaluation._EXTRA) == set(evaluation.ALL_EXTRA) and len(evaluation._EXTRA) == len(evaluation.ALL_EXTRA) == 6
    assert evaluation.EXTRA_METRICS == ("estoi", "si_sdr", "seg_snr")
    assert evaluation.SPECTRAL_METRICS == ("llr", "wss") and evaluation.PROJECTION_METRICS == ("bss_sdr",)
    assert evaluation.ALL_EXTRA == evaluation.EXTRA_METRICS + evaluation.SPECTRAL_METRICS + evaluation.PROJECTION_METRICS
    for name, (batch, keywords) in evaluation._EXTRA.items():
        assert batch is getattr(evaluation, batch.__name__) and batch.__name__.endswith("_batch"), name
        assert set(keywords) <= set(inspect.signature(batch).parameters), name
    mirrors = {"sdr": metrics.SDR, "stoi": metrics.STOI, "estoi": metrics.ESTOI, "si_sdr": metrics.SISDR, "bss_sdr": metrics.BSSSDR,
               "seg_snr": metrics.SegSNR, "llr": metrics.LLR, "wss": metrics.WSS}
    for method, cls in mirrors.items():
        mirror, seen = cls(), []
        assert callable(getattr(mirror, method)) and mirror.device == 0
        setattr(mirror, method, lambda x, y: seen.append((x, y)) or 0.25)
        assert mirror("a", "b") == 0.25 and seen == [("a", "b")]
