"""SI-SDR and the segmental SNR restated in numpy float64 as DESIGN.md "SI-SDR" / "Segmental SNR" define them: the pins of
rced_si_sdr and rced_seg_snr (pysepm is not available to this project; parity with it is unpinned).
Not a test module: tests/test_metrics_ext_host.py and tests/test_td_metrics_gpu.py import it."""

import numpy as np

EPS = np.finfo(float).eps
SEG_MIN, SEG_MAX = -10.0, 35.0


def si_sdr_parts(x, y):
    """(alpha, sum((alpha x)^2), sum((y - alpha x)^2)): two passes, no mean removal.  x clean, y estimate."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D signals of one length")
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.sum(y * x) / np.sum(x * x)
        t = alpha * x
        return float(alpha), float(np.sum(t * t)), float(np.sum((y - t) ** 2))


def si_sdr(x, y):
    _, target, residual = si_sdr_parts(x, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10 * np.log10(np.float64(target) / np.float64(residual)))


def si_sdr_closed_form(x, y):
    """The one-pass form from the three sums: fine for a poor estimate, cancels for a good one -- the test's cross-check only."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    sxx, sxy, syy = np.sum(x * x), np.sum(x * y), np.sum(y * y)
    return float(10 * np.log10((sxy * sxy / sxx) / (syy - sxy * sxy / sxx)))


def seg_window(fs):
    """Samples per frame, (3 fs + 50) // 100; ValueError outside [4, 1440]."""
    w = (3 * int(fs) + 50) // 100 if fs > 0 else 0
    if int(fs) != fs or not 4 <= w <= 1440:
        raise ValueError("fs = %r gives frames of %d samples: outside [4, 1440]" % (fs, w))
    return w


def seg_snr_detail(x, y, fs):
    """(score, nf)."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D signals of one length")
    W = seg_window(fs)
    H = W // 4
    L = len(x)
    nf = (L - W) // H + 1 if L >= W else 0
    if nf == 0:
        return float("nan"), 0
    w = 0.5 * (1 - np.cos(2 * np.pi * (np.arange(W) + 1) / (W + 1)))
    s = np.empty(nf)
    for i in range(nf):
        xs, ys = x[i * H:i * H + W], y[i * H:i * H + W]
        s[i] = 10 * np.log10(np.sum((w * xs) ** 2) / (np.sum((w * (xs - ys)) ** 2) + EPS) + EPS)
    return float(np.mean(np.clip(s, SEG_MIN, SEG_MAX))), nf


def seg_snr(x, y, fs):
    return seg_snr_detail(x, y, fs)[0]
