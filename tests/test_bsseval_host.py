"""CPU tests of the restatement of BSS Eval's single-source SDR (tests/bsseval_np.py) -- its three forms against each other
and against the properties of the definition -- and of the Python surface over rced_bss_sdr, which refuses bad arguments
before any device work.  mir_eval is not available here: parity with it is unpinned."""

import inspect
import math

import numpy as np
import pytest

import bsseval_np as bn
import stoi_np as sn
import td_metrics_np as td


def pair(L, i, snr=5):
    x = sn.speechlike(L, 500 + i, 8000).astype(np.float32)
    return x, sn.add_white(x.astype(np.float64), snr, 600 + i).astype(np.float32)


@pytest.mark.parametrize("F", (1, 2, 16, 33, 512))
def test_the_three_forms_agree(F):
    worst = 0.0
    for i, L in enumerate((2, 17, 64, 513, 1500, 4100, 20000)):
        x, y = pair(L, i)
        assert bn.cond(x, F) < 1e7
        a, b = bn.normal(x, y, F), bn.direct(x, y, F)
        forms = [b] + ([bn.lstsq(x, y, F)] if L <= bn.LSTSQ_MAX else [])
        for other in forms:
            worst = max(worst, abs(a[0] - other[0]))
            assert abs(a[2][0] / other[2][0] - 1) <= 1e-9 and abs(a[2][1] / other[2][1] - 1) <= 1e-9
        assert a[1].shape == (F,) and math.isfinite(a[0])
    print("F = %d: the forms lie at most %.3e dB apart" % (F, worst))
    assert worst <= 1e-10


def test_one_tap_is_si_sdr_and_a_gain_changes_nothing():
    for i, L in enumerate((1000, 4097)):
        x, y = pair(L, i)
        assert abs(bn.bss_sdr(x, y, 1) - td.si_sdr(x, y)) <= 1e-12
        alpha = td.si_sdr_parts(x, y)[0]
        assert abs(bn.normal(x, y, 1)[1][0] - alpha) <= 1e-14 * abs(alpha)
        for F in (1, 16, 512):
            base = bn.bss_sdr(x, y, F)
            for g in (0.25, -3.7, 1e3):
                assert abs(bn.bss_sdr(x, g * y.astype(np.float64), F) - base) <= 1e-9
            assert bn.bss_sdr(x, y, F) >= bn.bss_sdr(x, y, 1) - 1e-9            # more taps never fit worse


@pytest.mark.parametrize("F", (16, 512))
def test_a_filtered_copy_is_forgiven(F):
    """y = (x * h)[:L], len(h) <= F, the clean signal's last F - 1 samples zero: the projection is exact up to the float32
    rounding of y (about 2^-24 relative, roughly 140 dB); SI-SDR of the same pair is low."""
    rng = np.random.default_rng(7)
    L = 6000
    x = sn.speechlike(L, 511, 8000)
    x[L - (F - 1):] = 0.0
    x = x.astype(np.float32)
    h = rng.standard_normal(F) * np.exp(-np.arange(F) / (F / 4.0))
    h[0] = 0.3
    y = np.convolve(x.astype(np.float64), h)[:L].astype(np.float32)
    score, plain = bn.bss_sdr(x, y, F), td.si_sdr(x, y)
    print("F = %d: BSS Eval SDR %.1f dB, SI-SDR %.2f dB" % (F, score, plain))
    assert score > 120.0 and plain < 10.0
    assert abs(bn.bss_sdr(x, y, F) - bn.direct(x, y, F)[0]) <= 1e-3             # both far beyond the float32 floor


def test_a_delayed_noisy_copy_scores_near_its_noise_level():
    L, delay = 16000, 37
    x = sn.speechlike(L, 512, 8000)
    x[L - 600:] = 0.0
    for snr in (0, 10, 20):
        y = sn.add_white(np.concatenate([np.zeros(delay), x[:L - delay]]), snr, 613)
        x32, y32 = x.astype(np.float32), y.astype(np.float32)
        score = bn.bss_sdr(x32, y32, 512)
        print("snr %d dB, delay %d: BSS Eval SDR %.2f dB, SI-SDR %.2f dB" % (snr, delay, score, td.si_sdr(x32, y32)))
        assert abs(score - snr) <= 1.5 and td.si_sdr(x32, y32) < snr - 3        # 512 taps soak up a little of the noise
        short = bn.bss_sdr(x32, y32, 16)                                        # a filter shorter than the delay cannot reach it
        assert short < score and (snr < 10 or short < score - 5)


def test_edge_rules():
    x, y = pair(300, 3)
    empty = np.zeros(0, np.float32)
    for form in (bn.normal, bn.direct, bn.lstsq):
        for F in (1, 16, 512):
            assert math.isnan(form(empty, empty, F)[0])                           # L = 0
            assert math.isnan(form(np.zeros(300, np.float32), y, F)[0])           # x = 0
            assert math.isnan(form(x, np.zeros(300, np.float32), F)[0])           # y = 0: 0 / 0
    bad = y.copy()
    bad[100] = np.nan
    assert math.isnan(bn.normal(x, bad, 16)[0])                                   # non-finite samples propagate
    one = bn.normal(np.float32([0.3]), np.float32([-0.7]), 512)
    assert one[0] > 250.0 and abs(one[1][0] + 0.7 / 0.3) <= 1e-6 and not one[1][1:].any()
    for F in (0, 513, -1, 1.5):
        with pytest.raises(ValueError):
            bn.normal(x, y, F)
    with pytest.raises(ValueError):
        bn.normal(x, y[:-1], 16)
    assert bn.cond(np.zeros(10), 4) == float("inf") and bn.cond(np.float32([1.0]), 8) == 1.0


def test_python_surface_refuses_before_any_device_work(built):
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd import _lib, evaluation
    from fullycnnspeechenhancement_amd.metrics import BSSSDR
    assert evaluation.PROJECTION_METRICS == ("bss_sdr",)
    assert evaluation.EXTRA_METRICS == ("estoi", "si_sdr", "seg_snr") and evaluation.SPECTRAL_METRICS == ("llr", "wss")
    for name in ("bss_sdr_batch", "PROJECTION_METRICS"):
        assert getattr(pkg.audio, name) is getattr(evaluation, name)
    sig = inspect.signature(pkg.audio.bss_sdr_batch).parameters
    assert list(sig) == ["clean", "estimate", "lengths", "filter_length", "detail"]
    assert [sig[k].default for k in ("lengths", "filter_length", "detail")] == [None, 512, False]
    assert inspect.signature(BSSSDR).parameters["filter_length"].default == 512 and BSSSDR().filter_length == 512
    assert "unpinned" in evaluation.bss_sdr_batch.__doc__ and "unpinned" in BSSSDR.__doc__
    assert evaluation.check_extra(("bss_sdr", "si_sdr")) == ("bss_sdr", "si_sdr") and evaluation.check_extra("bss_sdr") == ("bss_sdr",)
    assert evaluation.check_extra(("llr", "bss_sdr", "estoi")) == ("llr", "bss_sdr", "estoi")
    for bad in (("bss_sdr", "bss_sdr"), ("bss",), "sdr", ("bss_sdr", "pesq")):
        with pytest.raises(ValueError):
            evaluation.check_extra(bad)
    for bad in (0, 513, -4, 1.5, 512.0, "16", None, True):
        with pytest.raises(ValueError):
            pkg.audio.bss_sdr_batch(None, None, filter_length=bad)
        with pytest.raises(ValueError):
            BSSSDR(filter_length=bad)
    assert BSSSDR(np.int64(7)).filter_length == 7
    assert len(_lib.SYMBOLS["rced_bss_sdr"][1]) == 12
    for cls in (pkg.FullyCNNTester, pkg.FullyCNNTrainer):
        assert "PROJECTION_METRICS" in (cls.test if cls is pkg.FullyCNNTester else cls.valid).__doc__


def test_symbol_refuses_bad_arguments(built):
    import ctypes
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    buf = np.zeros(8, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    ARG = _lib.RCED_ERR_ARG
    for F in (0, 513, -1):
        assert lib.rced_bss_sdr(p, 8, p, 8, None, 1, F, p, None, None, 0, None) == ARG and b"filter_length" in lib.rced_last_error()
        assert lib.rced_bss_sdr(p, 8, p, 8, None, 0, F, p, None, None, 0, None) == ARG      # checked before N = 0 passes
    assert lib.rced_bss_sdr(None, 8, p, 8, None, 1, 16, p, None, None, 0, None) == ARG
    assert lib.rced_bss_sdr(p, 8, p, 8, None, 1, 16, None, None, None, 0, None) == ARG
    assert lib.rced_bss_sdr(p, 8, p, -8, None, 1, 16, p, None, None, 0, None) == ARG
    assert lib.rced_bss_sdr(p, 8, p, 8, None, 70000, 16, p, None, None, 0, None) == ARG
    assert lib.rced_bss_sdr(p, 8, p, 8, None, 0, 512, p, None, None, 0, None) == 0
