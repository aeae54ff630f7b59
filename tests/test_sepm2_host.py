"""CPU tests of the fwSNRseg / CD restatement (tests/sepm2_np.py) and of the surface around rced_fwseg / rced_cepd: declared,
exported, bound, and refusing bad arguments without a device."""

import inspect
import math

import numpy as np
import pytest

import sepm2_np as s2
import sepm_np as sp
import stoi_np as sn


def pair(snr, length=6000, seed=3, fs=8000):
    x = sn.speechlike(length, seed, fs).astype(np.float32)
    return x, sn.add_white(x.astype(np.float64), snr, seed + 100).astype(np.float32)


def test_the_two_evaluations_of_each_measure_agree():
    """The DFT as a matrix product against np.fft.rfft; the autocorrelation sums from either end.  A band's SNR is
    20 log10(E_x / |E_x - E_y|) and is limited at 35 dB, so a relative error r of the band values reaches the frame value as
    at most (20 / ln 10) 10^(35 / 20) r = 490 r dB: 1e-13 relative between the two DFTs stays under 1e-10 dB.  CD: the bound
    of the LLR restatement's own test, 1e-9."""
    for fs in sp.RATES:
        x, y = pair(5, 25 * fs // 40, fs=fs)
        a, b = s2.fwseg_frames(x, y, fs), s2.fwseg_frames(x, y, fs, "rfft")
        c, d = s2.cd_frames(x, y, fs), s2.cd_frames(x, y, fs, reverse=True)
        print("%d Hz: fwSNRseg frames %.3e dB apart, CD frames %.3e apart" % (fs, np.abs(a - b).max(), np.abs(c - d).max()))
        assert len(a) == len(c) == sp.num_frames(len(x), fs) > 0
        assert np.abs(a - b).max() <= 1e-10 and abs(s2.fwseg(x, y, fs) - s2.fwseg(x, y, fs, "rfft")) <= 1e-10
        assert 0 < np.abs(c - d).max() <= 1e-9 and abs(s2.cd(x, y, fs) - s2.cd(x, y, fs, reverse=True)) <= 1e-9
        m1, m2 = s2.magnitude_matrix(sp.frames(x, fs), fs), s2.magnitude_rfft(sp.frames(x, fs), fs)
        assert m1.shape == (len(a), sp.dft_size(fs)[1]) and np.abs(m1 - m2).max() <= 1e-12 * m1.max()


U = 2.0 ** -53                                       # the unit roundoff


def weighted_mean_slack(bands=sp.BANDS, value=s2.SNR_MAX):
    """How far sum(Wt v) / sum(Wt) can lie from v when every band's value is v: each product rounds once, each sum adds 24
    times, the quotient rounds once -- (1 + 24 + 24 + 1) U relative, to first order."""
    return (2 * bands) * U * abs(value)


def eps_term_bound(x, fs):
    """Per frame, the first-order bound on CD(x, g x) for a gain g that is a power of two (see the test below)."""
    P = sp.lpc_order(fs)
    w = sp.window(sp.framing(fs)[0])
    out = []
    for fr in sp.frames(np.asarray(x, float) + sp.EPS, fs):
        R = sp.autocorr(fr, P)
        A = sp.levinson(R, P)
        T = np.array([[R[abs(i - j)] for j in range(P)] for i in range(P)])
        delta = 2 * sp.EPS * math.sqrt(float(w @ w) / R[0])
        h = np.zeros(P + 1)
        h[0] = 1.0
        for n in range(1, P + 1):
            h[n] = -sum(A[k] * h[n - k] for k in range(1, n + 1))
        out.append(s2.CD_SCALE * math.sqrt(2.0) * 2 * np.linalg.cond(T) * delta * np.linalg.norm(A[1:]) * np.abs(h).sum())
    return np.array(out)


def test_half_the_clean_signal_is_the_best_score():
    """0.5 x scales every magnitude exactly, the normalised magnitudes and the band values are the clean ones bit for bit, and
    every band's SNR is exactly 35.0, in either evaluation.  A frame's value is then the weighted mean of 25 equal numbers,
    35.0 up to that mean's own rounding (weighted_mean_slack: 1.9e-13; 2.1e-14 is met), and the score the mean of nf such
    values, (nf - 1) U more.
    CD of x against itself is exactly 0.0.  CD of x against 0.5 x is not: the definition frames x + EPS and 0.5 x + EPS, which
    are not multiples of each other; 0.5 x + EPS = 0.5 (x + 2 EPS), so the estimate's model is that of x + 2 EPS.  To first
    order (eps_term_bound): the lags move by at most delta = 2 EPS sqrt(sum w^2 / sum (w x)^2) of R[0]; the solution of
    T a = r by at most 2 cond(T) delta |a|; the cepstrum of 1 / A by that convolved with the model's impulse response h, at
    most |delta a| sum |h[0 .. P]|; the distance is (10 / ln 10) sqrt(2) times that norm.  The test computes the bound per
    frame and holds the frame against it."""
    slack = weighted_mean_slack()
    for fs in sp.RATES:
        x = sn.speechlike(6000, 1, fs).astype(np.float32)
        half = (0.5 * x).astype(np.float32)
        nf = sp.num_frames(6000, fs)
        for dft in ("matrix", "rfft"):
            ex, ey = s2.fwseg_bands(x, fs, dft), s2.fwseg_bands(half, fs, dft)
            assert ex.shape == (nf, sp.BANDS) and np.array_equal(ex, ey) and (s2.band_snr(ex, ey) == 35.0).all()
            d = s2.fwseg_frames(x, half, fs, dft)
            print("%d Hz, %s: frames within %.3e of 35, the score within %.3e" % (fs, dft, np.abs(d - 35).max(), abs(s2.fwseg(x, half, fs, dft) - 35)))
            assert np.abs(d - 35.0).max() <= slack and abs(s2.fwseg(x, half, fs, dft) - 35.0) <= slack + nf * U * 35.0
        assert abs(s2.fwseg(x, x, fs) - 35.0) <= slack + nf * U * 35.0
        assert not s2.cd_frames(x, x, fs).any() and s2.cd(x, x, fs) == 0.0
        d = s2.cd_frames(x, half, fs)
        bound = eps_term_bound(x, fs)
        print("%d Hz: CD of x against 0.5 x, largest frame %.3e (its bound %.3e), score %.3e; largest frame / bound %.3e"
              % (fs, d.max(), bound[d.argmax()], s2.cd(x, half, fs), (d / bound).max()))
        assert 0.0 <= d.min() and (d <= bound).all() and s2.cd(x, half, fs) <= bound.max()


def test_a_gain_on_the_estimate_changes_neither_score_beyond_rounding():
    """fwSNRseg normalises each signal by its own magnitude sum: a gain of 4 is exact and leaves every bit; a gain of 3
    rounds every sample product once (1.1e-16 relative), which reaches a frame value as at most 490 times that (see above)
    times the few hundred additions behind a band value: 1e-10 dB leaves a factor of ten.  CD: the EPS term, as in the test above."""
    x, y = pair(5)
    a = s2.fwseg_frames(x, y, 8000)
    assert np.array_equal(a, s2.fwseg_frames(x, 4 * y, 8000))
    b = s2.fwseg_frames(x, 3 * y.astype(np.float64), 8000)
    print("largest change of a frame's fwSNRseg under a gain of 3: %.3e dB" % np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-10
    c, d = s2.cd_frames(x, y, 8000), s2.cd_frames(x, 4 * y, 8000)
    print("largest change of a frame's CD under a gain of 4: %.3e" % np.abs(c - d).max())
    bound = eps_term_bound(y, 8000)                       # 4 y + EPS = 4 (y + EPS / 4): the estimate's eps term moves by less than EPS
    assert (np.abs(c - d) <= bound).all() and abs(sp.lowest_mean(c) - sp.lowest_mean(d)) <= bound.max()


def test_the_limits_are_reached():
    x = sn.speechlike(6000, 3).astype(np.float32)
    noise = (0.1 * np.random.default_rng(0).standard_normal(6000)).astype(np.float32)
    snr = s2.band_snr(s2.fwseg_bands(x, 8000), s2.fwseg_bands(noise, 8000))
    low, high = float((snr == s2.SNR_MIN).mean()), float((snr == s2.SNR_MAX).mean())
    values, counts = np.unique(snr, return_counts=True)
    print("pure noise as the estimate: %.1f %% of the band values at -10 dB, %.1f %% at 35 dB" % (100 * low, 100 * high))
    assert snr.min() == s2.SNR_MIN and snr.max() <= s2.SNR_MAX
    assert low >= 0.25 and values[counts.argmax()] == s2.SNR_MIN             # no other value is as common as the lower limit
    score = s2.fwseg(x, noise, 8000)
    assert s2.SNR_MIN < score < 5.0
    d = s2.cd_frames(x, noise, 8000)
    at_limit = int((d == s2.CD_MAX).sum())
    print("CD of speech against white noise: %d of %d frames at the limit of 10, score %.4f" % (at_limit, len(d), sp.lowest_mean(d)))
    assert at_limit >= 3 and d.max() == s2.CD_MAX and d.min() > 0.0
    # the limited frames still rank: they tie at 10 and leave by frame index, last first
    k = sp.lowest_count(len(d))
    assert sp.lowest_mean(d) == sp.ordered_sum(np.sort(d, kind="stable")[:k]) / k and sp.lowest_mean(d) < s2.CD_MAX
    all_ten = np.full(40, 10.0)
    assert sp.lowest_mean(all_ten) == 10.0


def test_digital_silence_and_short_signals():
    x, y = pair(5, 3000)
    x = x.copy()
    x[600:1100] = 0.0                                    # frames 10 .. 14 (samples 600 .. 1079) are all zero in the clean signal
    d = s2.fwseg_frames(x, y, 8000)
    silent = [t for t in range(len(d)) if not x[60 * t:60 * t + 240].any()]
    assert silent == [10, 11, 12, 13, 14]
    assert np.flatnonzero(np.isnan(d)).tolist() == silent and math.isnan(s2.fwseg(x, y, 8000))
    assert np.array_equal(np.isnan(d), np.isnan(s2.fwseg_frames(x, y, 8000, "rfft")))
    e = s2.fwseg_frames(y, x, 8000)                      # silence in the estimate: the same frames
    assert np.flatnonzero(np.isnan(e)).tolist() == silent
    c = s2.cd_frames(x, y, 8000)                         # the + EPS keeps CD finite
    assert np.isfinite(c).all() and math.isfinite(s2.cd(x, y, 8000))
    for fs in sp.RATES:
        w, _ = sp.framing(fs)
        short = np.ones(w - 1)
        assert len(s2.fwseg_frames(short, short, fs)) == 0 and math.isnan(s2.fwseg(short, short, fs)) and math.isnan(s2.cd(short, short, fs))
        one = sn.speechlike(w, 2, fs)
        assert len(s2.cd_frames(one, one, fs)) == 1 and abs(s2.fwseg(one, one, fs) - 35.0) <= weighted_mean_slack()


def test_order_argument():
    x, y = pair(10, 3000)
    assert s2.check_order(None, 8000) == 10 and s2.check_order(None, 16000) == 16
    assert np.array_equal(s2.cd_frames(x, y, 8000), s2.cd_frames(x, y, 8000, order=10))
    scores = {P: s2.cd(x, y, 8000, order=P) for P in (1, 10, 16)}
    print("CD at orders 1, 10, 16:", scores)
    assert all(math.isfinite(v) and 0 < v < 10 for v in scores.values()) and len(set(scores.values())) == 3
    # order 1: c[1] = a[0] = R[1] / R[0] of each signal
    fx, fy = sp.frames(x + sp.EPS, 8000)[4], sp.frames(y + sp.EPS, 8000)[4]
    rx, ry = sp.autocorr(fx, 1), sp.autocorr(fy, 1)
    want = s2.CD_SCALE * math.sqrt(2 * (rx[1] / rx[0] - ry[1] / ry[0]) ** 2)
    assert abs(s2.cd_frames(x, y, 8000, order=1)[4] - want) <= 1e-12
    for bad in (0, 17, -1, 10.0, True, "10"):
        with pytest.raises(ValueError):
            s2.check_order(bad, 8000)


def test_cepstrum_recursion_against_the_log_spectrum():
    """The model 1 / A(z) of a Levinson solution is minimum phase: its complex cepstrum is causal, c[n] = sum_i p_i^n / n over
    the poles, and the real cepstrum of log|1 / A| holds c[n] / 2 at n and at -n.  On an N-point grid the inverse FFT of the
    log spectrum aliases: it returns sum_m c_real[n + m N], so the first P coefficients are off by at most
    sum_{m >= 1} (|c[m N + n]| + |c[m N - n]|) / 2 <= P rho^(N - P) / ((N - P) (1 - rho^N)), rho the largest pole radius.
    The test computes that truncation bound; 1e-12 is added for the FFT's own rounding (N log2 N eps on values under 10)."""
    N = 1 << 14
    for fs, seed in ((8000, 5), (16000, 6)):
        P = sp.lpc_order(fs)
        x = sn.speechlike(4 * fs // 10, seed, fs)
        fr = sp.frames(x + sp.EPS, fs)
        worst = worst_bound = 0.0
        for t in range(0, len(fr), 3):
            A = sp.levinson(sp.autocorr(fr[t], P), P)
            rho = float(np.abs(np.roots(A)).max())
            assert rho < 1.0
            bound = P * rho ** (N - P) / ((N - P) * (1 - rho ** N)) + 1e-12
            spec = -np.log(np.abs(np.fft.fft(A, N)))         # log |1 / A| on the unit circle
            real = np.fft.ifft(spec).real
            got = s2.cepstrum(A)
            err = np.abs(got - 2 * real[1:P + 1]).max()
            worst, worst_bound = max(worst, err), max(worst_bound, bound)
            assert err <= bound, (fs, t, err, bound, rho)
            # and the impulse response itself: h = 1 / A by the recursion, exp of the cepstral series gives it back
            h = np.zeros(P + 1)
            h[0] = 1.0
            for n in range(1, P + 1):
                h[n] = -sum(A[k] * h[n - k] for k in range(1, n + 1))
            g = np.zeros(P + 1)
            g[0] = 1.0
            for n in range(1, P + 1):
                g[n] = sum(k * got[k - 1] * g[n - k] for k in range(1, n + 1)) / n
            assert np.abs(g - h).max() <= 1e-9 * np.abs(h).max()
        print("%d Hz, order %d: worst |recursion - log spectrum| %.3e, truncation bound up to %.3e" % (fs, P, worst, worst_bound))
    assert s2.cepstrum(np.array([1.0, -0.5])).tolist() == [0.5]
    assert np.allclose(s2.cepstrum(np.array([1.0, -0.5, 0.0, 0.0])), [0.5, 0.5 ** 2 / 2, 0.5 ** 3 / 3], rtol=0, atol=1e-16)


def test_symbols_are_declared_bound_and_refuse_bad_arguments(built):
    import ctypes
    from fullycnnspeechenhancement_amd import _lib
    assert len(_lib.SYMBOLS["rced_fwseg"][1]) == 13 and len(_lib.SYMBOLS["rced_cepd"][1]) == 14
    assert _lib.SYMBOLS["rced_fwseg"] == _lib.SYMBOLS["rced_wss"]
    lib = _lib.load()
    buf = np.zeros(8, np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    ARG = _lib.RCED_ERR_ARG
    for fs in (0, 10000, 44100, -8000):
        assert lib.rced_fwseg(p, 8, p, 8, None, 1, fs, p, None, 0, None, 0, None) == ARG
        assert lib.rced_cepd(p, 8, p, 8, None, 1, fs, 10, p, None, 0, None, 0, None) == ARG
        assert lib.rced_fwseg(p, 8, p, 8, None, 0, fs, p, None, 0, None, 0, None) == ARG     # the rate is checked before N = 0 passes
    for order in (0, 17, -3, 1 << 20):
        assert lib.rced_cepd(p, 8, p, 8, None, 1, 8000, order, p, None, 0, None, 0, None) == ARG and b"order" in lib.rced_last_error()
        assert lib.rced_cepd(p, 8, p, 8, None, 0, 16000, order, p, None, 0, None, 0, None) == ARG
    assert lib.rced_fwseg(None, 8, p, 8, None, 1, 8000, p, None, 0, None, 0, None) == ARG
    assert lib.rced_cepd(p, 8, p, 8, None, 1, 8000, 10, None, None, 0, None, 0, None) == ARG
    assert lib.rced_fwseg(p, -1, p, 8, None, 1, 8000, p, None, 0, None, 0, None) == ARG
    # rows of 300 samples can carry two frames: a per-frame buffer of one column is refused
    assert lib.rced_fwseg(p, 300, p, 301, None, 1, 8000, p, p, 1, None, 0, None) == ARG and b"frames_stride" in lib.rced_last_error()
    assert lib.rced_cepd(p, 300, p, 301, None, 1, 8000, 10, p, p, 1, None, 0, None) == ARG
    assert lib.rced_fwseg(p, 8, p, 8, None, 0, 16000, p, None, 0, None, 0, None) == 0
    for order in (1, 10, 16):
        assert lib.rced_cepd(p, 8, p, 8, None, 0, 8000, order, p, None, 0, None, 0, None) == 0


def test_python_surface_refuses_before_any_device_work(built):
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd import evaluation
    from fullycnnspeechenhancement_amd.metrics import CepDist, FwSegSNR
    assert evaluation.SEPM_METRICS == ("fw_seg_snr", "cd") and evaluation.EVERY_EXTRA == evaluation.ALL_EXTRA + evaluation.SEPM_METRICS
    for name in ("fw_seg_snr_batch", "cep_dist_batch", "SEPM_METRICS"):
        assert getattr(pkg.audio, name) is getattr(evaluation, name)
    for name, (batch, keywords) in evaluation._EXTRA_SEPM.items():
        assert batch is getattr(evaluation, batch.__name__) and set(keywords) <= set(inspect.signature(batch).parameters), name
    sig = inspect.signature(pkg.audio.fw_seg_snr_batch).parameters
    assert [sig[k].default for k in ("lengths", "sample_rate", "detail")] == [None, 8000, False] and list(sig)[:2] == ["clean", "estimate"]
    sig = inspect.signature(pkg.audio.cep_dist_batch).parameters
    assert [sig[k].default for k in ("lengths", "sample_rate", "order", "detail")] == [None, 8000, None, False]
    assert evaluation.check_extra(("fw_seg_snr", "cd")) == ("fw_seg_snr", "cd") and evaluation.check_extra("cd") == ("cd",)
    assert evaluation.check_extra(("cd", "llr", "fw_seg_snr", "wss")) == ("cd", "llr", "fw_seg_snr", "wss")
    forward = lambda m: m      # noqa: E731
    sig1 = [np.zeros(1000, np.float32)]
    for bad in (("fwsnrseg",), ("cd", "cd"), ("fw_seg_snr", "pesq"), "cepd"):
        with pytest.raises(ValueError):
            evaluation.check_extra(bad)
        with pytest.raises(ValueError):
            pkg.engine.evaluate_pcm(forward, sig1, sig1, extra=bad)
        with pytest.raises(ValueError):
            pkg.audio.denoise_and_score(forward, None, None, [1000], extra=bad)
        with pytest.raises(ValueError):
            pkg.FullyCNNTester.test(None, [(None, None, sig1, sig1)], extra=bad)
        with pytest.raises(ValueError):
            pkg.FullyCNNTrainer.valid(None, [(None, None, sig1, sig1)], 0, extra=bad)
    for bad in (10000, 44100, 0, 8000.5, None):
        with pytest.raises(ValueError):
            FwSegSNR(sr=bad)
        with pytest.raises(ValueError):
            CepDist(sr=bad)
        with pytest.raises(ValueError):
            pkg.audio.fw_seg_snr_batch(None, None, sample_rate=bad)
        with pytest.raises(ValueError):
            pkg.audio.cep_dist_batch(None, None, sample_rate=bad)
    for bad in (0, 17, -1, 10.5, True, "10"):
        with pytest.raises(ValueError):
            pkg.audio.cep_dist_batch(None, None, order=bad)
        with pytest.raises(ValueError):
            CepDist(order=bad)
    assert (FwSegSNR().sr, FwSegSNR(sr=16000).sr, CepDist().order, CepDist(16000).order, CepDist(8000, 16).order) == (8000, 16000, 10, 16, 16)
    for metric, method in ((FwSegSNR(), "fw_seg_snr"), (CepDist(), "cd")):
        with pytest.raises(ValueError):
            metric(np.zeros((2, 300)), np.zeros((2, 300)))
        with pytest.raises(ValueError):
            metric(np.zeros(300), np.zeros(301))
        assert math.isnan(metric(np.zeros(0), np.zeros(0))) and metric.device == 0
        seen = []
        setattr(metric, method, lambda x, y: seen.append((x, y)) or 0.25)
        assert metric("a", "b") == 0.25 and seen == [("a", "b")]
    for fn in (pkg.audio.fw_seg_snr_batch, pkg.audio.cep_dist_batch):
        with pytest.raises((ValueError, TypeError)):
            fn(np.zeros((2, 300), np.float32), np.zeros((2, 300), np.float32))       # host arrays are not device rows
    den, sdr, more = pkg.engine.evaluate_pcm(forward, [], [], extra=("fw_seg_snr", "cd", "llr"))
    assert den == [] and list(more) == ["fw_seg_snr", "cd", "llr"] and more["cd"].shape == (0,)
