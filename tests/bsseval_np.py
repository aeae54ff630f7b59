"""The SDR of BSS Eval for a single source (Vincent, Gribonval, Fevotte 2006) restated in numpy float64 as DESIGN.md "BSS Eval
SDR" defines it: the pin of rced_bss_sdr.  mir_eval and museval are not available to this project: parity with
mir_eval.separation.bss_eval_sources is unpinned.

    r[t] = sum_n x[n] x[n + t],  d[t] = sum_n x[n] y[n + t],  t = 0 .. F - 1  (samples at or past L count as 0)
    toeplitz(r) c = d;  s = x * c,  e = [y, 0 .. 0] - s over L + F - 1 samples;  10 log10(sum s^2 / sum e^2)

Three forms: (a) `normal` -- correlations by FFT, np.linalg.solve, np.convolve -- is the yardstick; (b) `direct` -- direct
correlation sums, scipy.linalg.solve_toeplitz -- and (c) `lstsq` -- the definition as a least-squares problem on the explicit
matrix of delayed copies, short signals only -- are second evaluations.  Each returns (score, c, (sum s^2, sum e^2)).
Nothing is regularised: a singular toeplitz(r) raises or gives what the solver gives.
Not a test module: tests/test_bsseval_host.py and tests/test_bsseval_gpu.py import it."""

import numpy as np

MAX_FILTER = 512
NAN = float("nan")


def _signals(x, y, F):
    x, y = np.asarray(x, float), np.asarray(y, float)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D signals of one length")
    if int(F) != F or not 1 <= F <= MAX_FILTER:
        raise ValueError("filter_length must be an integer in [1, %d], got %r" % (MAX_FILTER, F))
    return x, y, int(F)


def correlations_fft(x, y, F):
    """(r, d) at lags 0 .. F - 1 through one real FFT long enough for the linear correlation."""
    L = len(x)
    n = 1
    while n < L + F:
        n *= 2
    X, Y = np.fft.rfft(x, n), np.fft.rfft(y, n)
    return np.fft.irfft(np.conj(X) * X, n)[:F], np.fft.irfft(np.conj(X) * Y, n)[:F]


def correlations_direct(x, y, F):
    L = len(x)
    r, d = np.zeros(F), np.zeros(F)
    for t in range(min(F, L)):
        r[t] = np.dot(x[:L - t], x[t:])
        d[t] = np.dot(x[:L - t], y[t:])
    return r, d


def toeplitz(r):
    i = np.arange(len(r))
    return r[np.abs(i[:, None] - i[None, :])]


def cond(x, F):
    """The 2-norm condition number of toeplitz(r) of a clean signal (inf for a singular one)."""
    x = np.asarray(x, float)
    if not len(x) or not np.any(x):
        return float("inf")
    return float(np.linalg.cond(toeplitz(correlations_direct(x, x, int(F))[0])))


def _finish(x, y, c):
    F, L = len(c), len(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.convolve(x, c)                                  # L + F - 1 samples
        e = np.concatenate([y, np.zeros(F - 1)]) - s
        ss, se = float(np.sum(s * s)), float(np.sum(e * e))
        return float(10 * np.log10(np.float64(ss) / np.float64(se))), c, (ss, se)


def _degenerate(x, y, F):
    """L = 0, x = 0: nan, with the filter 0 / 0 gives."""
    if len(x) == 0 or not np.any(x):
        return NAN, np.full(F, NAN), (NAN, NAN) if len(x) else (0.0, 0.0)
    return None


def normal(x, y, filter_length=512):
    """(a): the normal equations."""
    x, y, F = _signals(x, y, filter_length)
    out = _degenerate(x, y, F)
    if out is not None:
        return out
    r, d = correlations_fft(x, y, F)
    return _finish(x, y, np.linalg.solve(toeplitz(r), d))


def direct(x, y, filter_length=512):
    """(b): direct correlation sums, Levinson's recursion by scipy."""
    from scipy.linalg import solve_toeplitz
    x, y, F = _signals(x, y, filter_length)
    out = _degenerate(x, y, F)
    if out is not None:
        return out
    r, d = correlations_direct(x, y, F)
    return _finish(x, y, solve_toeplitz(r, d))


LSTSQ_MAX = 4100


def lstsq(x, y, filter_length=512):
    """(c): min || [y, 0 ..] - A c ||, column k of A the clean signal delayed by k samples.  len(x) <= about 4,100."""
    x, y, F = _signals(x, y, filter_length)
    out = _degenerate(x, y, F)
    if out is not None:
        return out
    L = len(x)
    A = np.zeros((L + F - 1, F))
    for k in range(F):
        A[k:k + L, k] = x
    c = np.linalg.lstsq(A, np.concatenate([y, np.zeros(F - 1)]), rcond=None)[0]
    return _finish(x, y, c)


def bss_sdr(x, y, filter_length=512):
    return normal(x, y, filter_length)[0]
