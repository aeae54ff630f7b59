"""The frequency-weighted segmental SNR (fwSNRseg) and the cepstral distance (CD) restated in numpy float64 as DESIGN.md
"fwSNRseg" / "CD" define them: the pins of rced_fwseg and rced_cepd (pysepm is not available to this project; parity with
it, or with the MATLAB originals, is unpinned).  Framing, window, filters, DFT, Levinson and the lowest-95 % mean are
tests/sepm_np.py's; every sum here is a plain ordered loop.  Each measure has a second evaluation -- the DFT by np.fft.rfft
for fwSNRseg, the autocorrelation sums from the other end for CD -- that measures how far two correct evaluations of one
definition lie apart: the bar of tests/test_sepm2_gpu.py.
Not a test module: tests/test_sepm2_host.py and tests/test_sepm2_gpu.py import it."""

import math

import numpy as np

import sepm_np as sp

EPS = sp.EPS
SNR_MIN, SNR_MAX = -10.0, 35.0
GAMMA = 0.2
CD_MAX = 10.0
CD_SCALE = 10.0 / math.log(10.0)
MAX_ORDER = 16


# ---- fwSNRseg --------------------------------------------------------------------------------------------------------


def magnitude_matrix(fr, fs):
    """|DFT_nfft(frame)| on the nb bins as an explicit matrix product."""
    c, s = sp.dft_matrix(fs)
    re, im = fr @ c, fr @ s
    return np.sqrt(re * re + im * im)


def magnitude_rfft(fr, fs):
    nfft, nb = sp.dft_size(fs)
    z = np.fft.rfft(fr, nfft, axis=1)[:, :nb]
    return np.sqrt(z.real ** 2 + z.imag ** 2)


def normalised(mag):
    """Every frame's magnitudes over their sum, the sum added in bin order; a frame of zeros gives 0 / 0 = nan."""
    total = np.cumsum(mag, axis=1)[:, -1] if mag.shape[0] else np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return mag / total[:, None]


def band_values(norm, fs):
    """[nf, 25] linear: each filter's sum over its nonzero bins in bin order, on normalised magnitudes."""
    F, ranges = sp.filter_bank(fs)
    e = np.empty((len(norm), sp.BANDS))
    for i, (lo, hi) in enumerate(ranges):
        e[:, i] = np.cumsum(norm[:, lo:hi] * F[i, lo:hi], axis=1)[:, -1]
    return e


def band_snr(ex, ey):
    """[..., 25] dB: 10 log10(E_x^2 / max((E_x - E_y)^2, eps)) limited to [-10, 35]; nan stays nan."""
    diff = ex - ey
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = 10 * np.log10(ex * ex / np.maximum(diff * diff, EPS))
    return np.minimum(np.maximum(snr, SNR_MIN), SNR_MAX)


def fwseg_from_bands(ex, ey):
    """[nf]: sum(Wt snr) / sum(Wt), Wt = E_x ** 0.2, both sums in band order."""
    d = np.empty(len(ex))
    with np.errstate(invalid="ignore"):
        wt, snr = ex ** GAMMA, band_snr(ex, ey)
    for t in range(len(ex)):
        num = den = 0.0
        for b in range(sp.BANDS):
            num += wt[t, b] * snr[t, b]
            den += wt[t, b]
        with np.errstate(invalid="ignore"):
            d[t] = np.float64(num) / np.float64(den)
    return d


def fwseg_bands(x, fs, dft="matrix"):
    mag = {"matrix": magnitude_matrix, "rfft": magnitude_rfft}[dft]
    return band_values(normalised(mag(sp.frames(x, fs), fs)), fs)


def fwseg_frames(x, y, fs, dft="matrix"):
    """Every frame's value.  dft: "matrix" or "rfft" (the second evaluation)."""
    x, y = sp._pair(x, y)
    return fwseg_from_bands(fwseg_bands(x, fs, dft), fwseg_bands(y, fs, dft))


def plain_mean(d):
    """The mean of all frames, added in frame order; nan for none."""
    d = np.asarray(d, float)
    return sp.ordered_sum(d) / d.size if d.size else float("nan")


def fwseg(x, y, fs, dft="matrix"):
    return plain_mean(fwseg_frames(x, y, fs, dft))


# ---- CD --------------------------------------------------------------------------------------------------------------


def check_order(order, fs):
    """The LPC order of CD: None = sepm_np.lpc_order(fs), else an integer in 1 .. 16."""
    if order is None:
        return sp.lpc_order(fs)
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= MAX_ORDER:
        raise ValueError("order must be an integer in [1, %d], got %r" % (MAX_ORDER, order))
    return int(order)


def cepstrum(A):
    """c[1 .. P] of 1 / A(z), A = [1, A[1], ..., A[P]]: c[1] = -A[1], c[k] = -(A[k] + (sum_{i < k} i c[i] A[k - i]) / k),
    the sum in ascending i."""
    P = len(A) - 1
    c = [0.0] * (P + 1)
    for k in range(1, P + 1):
        s = 0.0
        for i in range(1, k):
            s += (i * c[i]) * A[k - i]
        c[k] = -(A[k] + s / k)
    return np.array(c[1:])


def cd_frames(x, y, fs, order=None, reverse=False):
    """Every frame's value, limited to [0, 10].  reverse: the autocorrelation sums from the other end (the second evaluation)."""
    x, y = sp._pair(x, y)
    P = check_order(order, fs)
    fx, fy = sp.frames(x + EPS, fs), sp.frames(y + EPS, fs)
    d = np.empty(len(fx))
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(len(fx)):
            cx = cepstrum(sp.levinson(sp.autocorr(fx[t], P, reverse), P))
            cy = cepstrum(sp.levinson(sp.autocorr(fy[t], P, reverse), P))
            s = 0.0
            for k in range(P):
                diff = cx[k] - cy[k]
                s += diff * diff
            d[t] = CD_SCALE * np.sqrt(np.float64(2.0 * s))
        return np.minimum(np.maximum(d, 0.0), CD_MAX)


def cd(x, y, fs, order=None, reverse=False):
    return sp.lowest_mean(cd_frames(x, y, fs, order, reverse))
