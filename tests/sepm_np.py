"""LLR and WSS restated in numpy float64 as DESIGN.md "LLR" / "WSS" define them: the pins of rced_llr and rced_wss (pysepm
is not available to this project; parity with it, or with the MATLAB originals, is unpinned).
Every sum is a plain ordered loop (np.cumsum(...)[-1] adds left to right) so that a second evaluation in another order --
autocorrelation sums reversed, the DFT by np.fft.rfft instead of the matrix product -- measures how far two correct
evaluations of the same definition lie apart: the bar of tests/test_sepm_gpu.py.
Not a test module: tests/test_sepm_host.py and tests/test_sepm_gpu.py import it."""

import functools

import numpy as np

EPS = np.finfo(float).eps
RATES = (8000, 16000)
BANDS = 25
CENTRE = np.array([50, 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
                   1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63])
WIDTH = np.array([70] * 7 + [77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776,
                             217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136])


def ordered_sum(v, reverse=False):
    """v[0] + v[1] + ... in that order (or from the other end), one rounding per addition."""
    v = np.asarray(v, float)
    if v.size == 0:
        return 0.0
    return float(np.cumsum(v[::-1] if reverse else v)[-1])


def framing(fs):
    """(W, H): samples per frame and hop; ValueError for a rate other than 8000 or 16000."""
    if fs not in RATES:
        raise ValueError("fs must be 8000 or 16000, got %r" % (fs,))
    w = (3 * int(fs) + 50) // 100
    return w, w // 4


def num_frames(length, fs):
    w, h = framing(fs)
    return (length - w) // h + 1 if length >= w else 0


def window(w):
    return 0.5 * (1 - np.cos(2 * np.pi * (np.arange(w) + 1) / (w + 1)))


def frames(x, fs):
    """[nf, W]: frame i = x[i H : i H + W] under the window."""
    x = np.asarray(x, float)
    w, h = framing(fs)
    nf = num_frames(len(x), fs)
    idx = np.arange(w)[None, :] + h * np.arange(nf)[:, None]
    return x[idx] * window(w)


def lowest_count(nf):
    return (95 * nf + 50) // 100


def lowest_mean(d):
    """The mean of the k = (95 nf + 50) // 100 smallest values, ties by index, nan last, added in rank order; nan for none."""
    d = np.asarray(d, float)
    if d.size == 0:
        return float("nan")
    k = lowest_count(d.size)
    order = sorted(range(d.size), key=lambda i: (bool(np.isnan(d[i])), d[i] if not np.isnan(d[i]) else 0.0, i))
    with np.errstate(invalid="ignore"):
        return ordered_sum(d[order[:k]]) / k


def _pair(x, y):
    x, y = np.asarray(x, float), np.asarray(y, float)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D signals of one length")
    return x, y


# ---- LLR -------------------------------------------------------------------------------------------------------------


def lpc_order(fs):
    return 10 if fs < 10000 else 16


def autocorr(s, order, reverse=False):
    """R[m] = sum_{n = 0}^{W - 1 - m} s[n] s[n + m], m = 0 .. order."""
    n = len(s)
    return np.array([ordered_sum(s[:n - m] * s[m:], reverse) for m in range(order + 1)])


def levinson(R, order):
    """A = [1, -a[0], ..., -a[order - 1]] by Levinson-Durbin, as DESIGN.md writes the recursion."""
    a = [0.0] * order
    E = R[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(order):
            prev = list(a)
            s = 0.0
            for j in range(i):
                s += prev[j] * R[i - j]
            rc = (R[i + 1] - s) / E
            a[i] = rc
            for j in range(i):
                a[j] = prev[j] - rc * prev[i - 1 - j]
            E = (1 - rc * rc) * E
    return np.array([1.0] + [-v for v in a])


def toeplitz_form(A, R):
    """A T A^T, T[i][j] = R[|i - j|]: rows in order, each row's sum in column order."""
    q = 0.0
    n = len(A)
    for i in range(n):
        row = 0.0
        for j in range(n):
            row += R[abs(i - j)] * A[j]
        q += A[i] * row
    return q


def llr_frames(x, y, fs, reverse=False):
    """Every frame's value, before any limit.  reverse: the autocorrelation sums from the other end (the second evaluation)."""
    x, y = _pair(x, y)
    order = lpc_order(fs)
    fx, fy = frames(x + EPS, fs), frames(y + EPS, fs)
    d = np.empty(len(fx))
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(len(fx)):
            Rx, Ry = autocorr(fx[t], order, reverse), autocorr(fy[t], order, reverse)
            Ax, Ay = levinson(Rx, order), levinson(Ry, order)
            d[t] = np.log(np.float64(toeplitz_form(Ay, Rx)) / np.float64(toeplitz_form(Ax, Rx)))
    return d


def llr_from_frames(d, limit=2.0):
    if limit is not None:
        d = np.minimum(d, limit)
    return lowest_mean(d)


def llr(x, y, fs, limit=2.0, reverse=False):
    return llr_from_frames(llr_frames(x, y, fs, reverse), limit)


# ---- WSS -------------------------------------------------------------------------------------------------------------


def dft_size(fs):
    """(nfft, nb): the power of two at or above 2 W, and nfft / 2 bins."""
    w, _ = framing(fs)
    nfft = 1
    while nfft < 2 * w:
        nfft *= 2
    return nfft, nfft // 2


@functools.lru_cache(maxsize=None)
def filter_bank(fs):
    """(F [25, nb], ranges [25][2]): the critical-band filters, 0 where at or under exp(-30 / (2 2.303)), and each filter's
    nonzero bins [lo, hi)."""
    _, nb = dft_size(fs)
    fmax = fs / 2
    F = np.zeros((BANDS, nb))
    j = np.arange(nb)
    ranges = []
    for i in range(BANDS):
        g = np.exp(-11 * ((j - np.floor(CENTRE[i] * nb / fmax)) / (WIDTH[i] * nb / fmax)) ** 2 + np.log(70.0) - np.log(WIDTH[i]))
        g[g <= np.exp(-30 / (2 * 2.303))] = 0
        F[i] = g
        nz = np.nonzero(g)[0]
        ranges.append((int(nz[0]), int(nz[-1]) + 1))
    return F, ranges


@functools.lru_cache(maxsize=None)
def dft_matrix(fs):
    w, _ = framing(fs)
    nfft, nb = dft_size(fs)
    th = 2 * np.pi * ((np.arange(w)[:, None] * np.arange(nb)[None, :]) % nfft) / nfft
    return np.cos(th), -np.sin(th)


def power_matrix(fr, fs):
    """|DFT_nfft(frame)|^2 on the nb bins as an explicit matrix product."""
    c, s = dft_matrix(fs)
    re, im = fr @ c, fr @ s
    return re * re + im * im


def power_rfft(fr, fs):
    nfft, nb = dft_size(fs)
    z = np.fft.rfft(fr, nfft, axis=1)[:, :nb]
    return z.real ** 2 + z.imag ** 2


def band_energies(power, fs):
    """[nf, 25] dB: each filter's sum over its nonzero bins in bin order."""
    F, ranges = filter_bank(fs)
    e = np.empty((len(power), BANDS))
    for i, (lo, hi) in enumerate(ranges):
        e[:, i] = np.cumsum(power[:, lo:hi] * F[i, lo:hi], axis=1)[:, -1]
    return 10 * np.log10(np.maximum(e, 1e-10))


def nearest_peaks(e, s):
    """p[i] for the 24 slopes of one frame's 25 energies, the two walks as DESIGN.md writes them."""
    p = np.empty(BANDS - 1)
    for i in range(BANDS - 1):
        n = i
        if s[i] > 0:
            while n < BANDS - 1 and s[n] > 0:
                n += 1
            p[i] = e[n - 1]
        else:
            while n >= 0 and s[n] <= 0:
                n -= 1
            p[i] = e[n + 1]
    return p


def slope_weights(e):
    """(s [24], Wt [24]) of one frame's energies."""
    s = e[1:] - e[:-1]
    p = nearest_peaks(e, s)
    return s, 20 / (20 + e.max() - e[:-1]) * (1 / (1 + p - e[:-1]))


def wss_from_energies(ex, ey):
    """(d [nf], the smallest |slope| of either signal) from two [nf, 25] energy arrays."""
    d = np.empty(len(ex))
    clearance = np.inf
    for t in range(len(ex)):
        sx, wx = slope_weights(ex[t])
        sy, wy = slope_weights(ey[t])
        clearance = min(clearance, np.abs(sx).min(), np.abs(sy).min())
        num = den = 0.0
        for i in range(BANDS - 1):
            w = (wx[i] + wy[i]) / 2
            diff = sx[i] - sy[i]
            num += w * (diff * diff)
            den += w
        d[t] = num / den
    return d, float(clearance)


def wss_frames(x, y, fs, dft="matrix"):
    """(every frame's value, the smallest |slope| in dB met on the way).  dft: "matrix" or "rfft" (the second evaluation)."""
    x, y = _pair(x, y)
    power = {"matrix": power_matrix, "rfft": power_rfft}[dft]
    return wss_from_energies(band_energies(power(frames(x, fs), fs), fs), band_energies(power(frames(y, fs), fs), fs))


def wss(x, y, fs, dft="matrix"):
    return lowest_mean(wss_frames(x, y, fs, dft)[0])
