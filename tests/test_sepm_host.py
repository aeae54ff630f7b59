"""CPU tests of the LLR / WSS restatement (tests/sepm_np.py), of metrics.composite and of the surface around rced_llr /
rced_wss: declared, exported, bound, and refusing bad arguments without a device."""

import inspect
import math

import numpy as np
import pytest

import sepm_np as sp
import stoi_np as sn

SNRS = (-10, 0, 10, 20, 30, 40)


def pair(snr, length=12000, seed=3):
    x = sn.speechlike(length, seed)
    return x, sn.add_white(x, snr, seed + 100)


def test_identity_is_exactly_zero():
    for fs in sp.RATES:
        x = sn.speechlike(6000, 1, fs)
        assert sp.llr(x, x, fs) == 0.0 and sp.llr(x, x, fs, limit=None) == 0.0
        d, _ = sp.wss_frames(x, x, fs)
        assert len(d) == sp.num_frames(6000, fs) and not d.any() and sp.wss(x, x, fs) == 0.0
    z = np.zeros(600)                              # digital silence: the + EPS keeps LLR finite
    assert sp.llr(z, z, 8000) == 0.0


def test_scores_fall_as_the_snr_rises_and_the_limit_bites_only_at_the_bottom():
    llr, wss = [], []
    for snr in SNRS:
        x, y = pair(snr)
        d = sp.llr_frames(x, y, 8000)
        llr.append((sp.llr_from_frames(d, 2.0), sp.llr_from_frames(d, None), float(d.max())))
        wss.append(sp.wss(x, y, 8000))
    print("LLR (limited, unlimited, largest frame):", llr)
    print("WSS:", wss)
    assert all(a[0] > b[0] and a[1] > b[1] for a, b in zip(llr, llr[1:]))
    assert all(a > b for a, b in zip(wss, wss[1:]))
    assert all(math.isfinite(v) and v > 0 for v in wss) and all(0 < a[0] <= a[1] for a in llr)
    assert llr[0][2] > 2 and llr[0][0] < llr[0][1]          # -10 dB: frames above 2, the limit changes the score
    assert llr[-1][2] < 2 and llr[-1][0] == llr[-1][1]      # 40 dB: none


def test_aggregation_takes_the_lowest_95_percent():
    assert [sp.lowest_count(nf) for nf in (0, 1, 10, 11, 30, 1000)] == [0, 1, 10, 10, 29, 950]
    assert math.isnan(sp.lowest_mean([]))
    assert sp.lowest_mean([7.0]) == 7.0
    assert sp.lowest_mean(np.arange(10.0)[::-1]) == 4.5                       # nf = 10: all ten
    assert sp.lowest_mean([5.0] + list(np.arange(10.0))) == 4.5 + 0.5 - 9 / 10  # nf = 11: the largest leaves: (45 + 5 - 9) / 10
    d = np.random.default_rng(0).standard_normal(1000)
    assert abs(sp.lowest_mean(d) - np.sort(d)[:950].mean()) <= 1e-13
    assert sp.lowest_mean([1.0, float("nan")] + [0.0] * 18) == 1 / 19          # nan sorts last and is the one left out
    assert math.isnan(sp.lowest_mean([float("nan"), 1.0]))


def test_llr_ignores_a_gain_on_the_estimate_up_to_the_eps_term():
    """A gain of 4 scales y exactly; what is left is EPS against 4 EPS on every sample, a relative change of the lags of
    about EPS / rms(y) = 2e-15 here.  The Levinson recursion amplifies it by at most the condition number of the
    estimate's Toeplitz matrix, the ratio of its spectrum's extremes: white noise at 5 dB under harmonics 40 dB above the
    clean floor keeps that under 1e5.  1e-9 leaves a factor of five."""
    x, y = pair(5)
    a, b = sp.llr_frames(x, y, 8000), sp.llr_frames(x, 4 * y, 8000)
    print("largest change of a frame's LLR under a gain of 4: %.3e" % np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-9
    assert abs(sp.llr_from_frames(a) - sp.llr_from_frames(b)) <= 1e-9


def test_filter_bank_shape_and_ranges():
    for fs in sp.RATES:
        F, ranges = sp.filter_bank(fs)
        nfft, nb = sp.dft_size(fs)
        assert (nfft, nb) == {8000: (512, 256), 16000: (1024, 512)}[fs] and F.shape == (25, nb)
        for i, (lo, hi) in enumerate(ranges):
            centre = int(np.floor(sp.CENTRE[i] * nb / (fs / 2)))
            assert (F[i, lo:hi] > 0).all() and not F[i, :lo].any() and not F[i, hi:].any()       # one run of nonzero bins
            assert lo <= centre < hi and F[i].argmax() == centre and abs(F[i, centre] - 70 / sp.WIDTH[i]) <= 1e-15
            assert F[i, lo:hi].min() > math.exp(-30 / (2 * 2.303))
        # both rates place the centres on the same bins: 4000 / 256 = 8000 / 512 Hz per bin
        assert ranges[0] == (0, 7) and ranges[24][1] <= 249 and all(hi - lo <= 31 for lo, hi in ranges)
    assert sp.filter_bank(8000)[1] == sp.filter_bank(16000)[1]


def test_peak_search_on_hand_made_slopes():
    rising = np.arange(25.0)                       # every slope > 0: each walk runs to n = 24, the peak is e[23]
    assert (sp.nearest_peaks(rising, np.diff(rising)) == 23.0).all()
    falling = -np.arange(25.0)                     # every slope <= 0: each walk runs to n = -1, the peak is e[0]
    assert (sp.nearest_peaks(falling, np.diff(falling)) == 0.0).all()
    flat = np.full(25, 3.0)                        # a slope of 0 counts as falling
    assert (sp.nearest_peaks(flat, np.diff(flat)) == 3.0).all()
    e = np.array([0.0, 2, 5, 4, 1, 3] + [3.0] * 19)     # up up down down up flat...: peaks e[1] (n stops at 2), e[3], e[4] ...
    assert sp.nearest_peaks(e, np.diff(e))[:6].tolist() == [2.0, 2.0, 5.0, 5.0, 1.0, 3.0]
    s, wt = sp.slope_weights(rising)
    assert np.allclose(wt, 20 / (20 + 24 - np.arange(24.0)) / (1 + 23 - np.arange(24.0)))


def test_order_and_framing_per_rate():
    assert sp.lpc_order(8000) == 10 and sp.lpc_order(16000) == 16
    assert sp.framing(8000) == (240, 60) and sp.framing(16000) == (480, 120)
    assert [sp.num_frames(L, 8000) for L in (0, 239, 240, 299, 300)] == [0, 0, 1, 1, 2]
    x = sn.speechlike(2000, 5, 16000)
    R = sp.autocorr(sp.frames(x + sp.EPS, 16000)[0], 16)
    A = sp.levinson(R, 16)
    assert len(R) == 17 and len(A) == 17 and A[0] == 1.0
    # the model solves the normal equations: sum_j T[i][j] a[j] = R[i + 1]
    T = np.array([[R[abs(i - j)] for j in range(16)] for i in range(16)])
    assert np.abs(T @ (-A[1:]) - R[1:]).max() <= 1e-6 * R[0]
    for bad in (10000, 44100, 0, 8000.5):
        with pytest.raises(ValueError):
            sp.framing(bad)
    assert math.isnan(sp.llr(np.zeros(239), np.zeros(239), 8000)) and math.isnan(sp.wss(np.zeros(100), np.zeros(100), 16000))


def test_the_two_dfts_and_the_two_summation_orders_agree():
    x, y = pair(5, 3000)
    fr = sp.frames(x, 8000)
    a, b = sp.power_matrix(fr, 8000), sp.power_rfft(fr, 8000)
    assert np.abs(a - b).max() <= 1e-12 * a.max()
    d1, d2 = sp.llr_frames(x, y, 8000), sp.llr_frames(x, y, 8000, reverse=True)
    assert 0 < np.abs(d1 - d2).max() <= 1e-9
    w1, w2 = sp.wss_frames(x, y, 8000)[0], sp.wss_frames(x, y, 8000, "rfft")[0]
    assert np.abs(w1 / w2 - 1).max() <= 1e-9


def test_composite_formulas_and_clipping(built):
    from fullycnnspeechenhancement_amd.metrics import composite
    csig, cbak, covl = composite(2.0, 0.5, 40.0, 5.0)
    assert abs(csig - (3.093 - 0.5145 + 1.206 - 0.36)) <= 1e-12        # 3.4245
    assert abs(cbak - (1.634 + 0.956 - 0.28 + 0.315)) <= 1e-12         # 2.625
    assert abs(covl - (1.594 + 1.61 - 0.256 - 0.28)) <= 1e-12          # 2.668
    csig, cbak, covl = composite([4.5, 1.0, 2.0], [0.0, 3.0, 0.5], [0.0, 150.0, 40.0], [35.0, -10.0, 5.0])
    assert csig.tolist()[:2] == [5.0, 1.0] and cbak.tolist()[:2] == [5.0, 1.0] and covl.tolist()[:2] == [5.0, 1.0]
    assert abs(csig[2] - 3.4245) <= 1e-12 and csig.dtype == np.float64 and csig.shape == (3,)
    assert "unlimited" in composite.__doc__ and "does not compute" in composite.__doc__


def test_symbols_are_declared_bound_and_refuse_bad_arguments(built):
    import ctypes
    from fullycnnspeechenhancement_amd import _lib
    assert len(_lib.SYMBOLS["rced_llr"][1]) == 14 and len(_lib.SYMBOLS["rced_wss"][1]) == 13
    lib = _lib.load()
    buf = np.zeros(8, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    ARG = _lib.RCED_ERR_ARG
    for fs in (0, 10000, 44100, -8000):
        assert lib.rced_llr(p, 8, p, 8, None, 1, fs, 2.0, p, None, 0, None, 0, None) == ARG
        assert lib.rced_wss(p, 8, p, 8, None, 1, fs, p, None, 0, None, 0, None) == ARG
        assert lib.rced_wss(p, 8, p, 8, None, 0, fs, p, None, 0, None, 0, None) == ARG       # the rate is checked before N = 0 passes
    assert lib.rced_llr(None, 8, p, 8, None, 1, 8000, 2.0, p, None, 0, None, 0, None) == ARG
    assert lib.rced_wss(p, 8, p, 8, None, 1, 8000, None, None, 0, None, 0, None) == ARG
    assert lib.rced_llr(p, 8, p, 8, None, 1, 8000, float("nan"), p, None, 0, None, 0, None) == ARG
    assert lib.rced_llr(p, -1, p, 8, None, 1, 8000, 2.0, p, None, 0, None, 0, None) == ARG
    # rows of 300 samples can carry two frames: a per-frame buffer of one column is refused
    assert lib.rced_llr(p, 300, p, 301, None, 1, 8000, 2.0, p, p, 1, None, 0, None) == ARG
    assert lib.rced_wss(p, 300, p, 301, None, 1, 8000, p, p, 1, None, 0, None) == ARG and b"frames_stride" in lib.rced_last_error()
    assert lib.rced_llr(p, 8, p, 8, None, 0, 16000, 2.0, p, None, 0, None, 0, None) == 0
    assert lib.rced_wss(p, 8, p, 8, None, 0, 8000, p, None, 0, None, 0, None) == 0


def test_python_surface_refuses_before_any_device_work(built):
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd import evaluation
    from fullycnnspeechenhancement_amd.metrics import LLR, WSS
    assert evaluation.EXTRA_METRICS == ("estoi", "si_sdr", "seg_snr") and evaluation.SPECTRAL_METRICS == ("llr", "wss")
    for name in ("llr_batch", "wss_batch", "SPECTRAL_METRICS"):
        assert getattr(pkg.audio, name) is getattr(evaluation, name)
    sig = inspect.signature(pkg.audio.llr_batch).parameters
    assert [sig[k].default for k in ("lengths", "sample_rate", "limit", "detail")] == [None, 8000, 2.0, False]
    sig = inspect.signature(pkg.audio.wss_batch).parameters
    assert [sig[k].default for k in ("lengths", "sample_rate", "detail")] == [None, 8000, False] and "limit" not in sig
    assert evaluation.check_extra(("llr", "wss", "seg_snr")) == ("llr", "wss", "seg_snr") and evaluation.check_extra("wss") == ("wss",)
    for bad in (("pesq",), ("sdr",), ("stoi",), ("llr", "llr"), ("wss", "estoi", "wss"), "csig"):
        with pytest.raises(ValueError):
            evaluation.check_extra(bad)
    for bad in (10000, 44100, 0, 8000.5, None):
        with pytest.raises(ValueError):
            LLR(sr=bad)
        with pytest.raises(ValueError):
            WSS(sr=bad)
        with pytest.raises(ValueError):
            pkg.audio.llr_batch(None, None, sample_rate=bad)
        with pytest.raises(ValueError):
            pkg.audio.wss_batch(None, None, sample_rate=bad)
    with pytest.raises(ValueError):
        pkg.audio.llr_batch(None, None, limit=float("nan"))
    with pytest.raises(ValueError):
        LLR(limit=float("nan"))
    assert (LLR().sr, LLR().limit, LLR(16000, None).limit, WSS(sr=16000).sr) == (8000, 2.0, None, 16000)
    for metric in (LLR(), WSS()):
        with pytest.raises(ValueError):
            metric(np.zeros((2, 300)), np.zeros((2, 300)))
        with pytest.raises(ValueError):
            metric(np.zeros(300), np.zeros(301))
        assert math.isnan(metric(np.zeros(0), np.zeros(0)))
    for fn in (pkg.audio.llr_batch, pkg.audio.wss_batch):
        with pytest.raises((ValueError, TypeError)):
            fn(np.zeros((2, 300), np.float32), np.zeros((2, 300), np.float32))       # host arrays are not device rows
    forward = lambda m: m      # noqa: E731
    den, sdr, more = pkg.engine.evaluate_pcm(forward, [], [], extra=("llr", "wss"))
    assert den == [] and sorted(more) == ["llr", "wss"] and more["llr"].shape == (0,)
