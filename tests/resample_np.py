"""The sample-rate conversion of DESIGN.md 3.4f in float64 numpy, as the direct sum -- no phase table --, and the same
filter handed to scipy.signal.resample_poly.  The parameters are those of resampy's kaiser_best; the kernel is evaluated
exactly, not through resampy's interpolated table.

    ratio = float(sr_new) / sr_orig,  s = min(1, ratio),  p / q = sr_new / sr_orig in lowest terms
    M = int(n_orig * ratio)
    y[n] = sum_j x[j] s h(s ((j - n0) - r / p)),  (n0, r) = divmod(n q, p),  x = 0 outside [0, n_orig)
    h(t) = rho sinc(rho t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta)  for |t| < Z (strictly), else 0
"""

from math import gcd

import numpy as np
from scipy.special import i0

Z = 64
RHO = 0.9475937167399596
BETA = 14.769656459379492


def h(tau):
    tau = np.asarray(tau, np.float64)
    inside = np.abs(tau) < Z
    t = np.where(inside, tau, 0.0)
    return np.where(inside, RHO * np.sinc(RHO * t) * i0(BETA * np.sqrt(1.0 - (t / Z) ** 2)) / i0(BETA), 0.0)


def terms(sr_orig, sr_new):
    ratio = float(sr_new) / sr_orig
    g = gcd(int(sr_new), int(sr_orig))
    return ratio, min(1.0, ratio), int(sr_new) // g, int(sr_orig) // g


def length(n, sr_orig, sr_new):
    return int(n * (float(sr_new) / sr_orig))


def to_mono(x):
    """Stored samples -> float64 mono: int16 / 32768, float as it is; [frames, channels]: (c0 + c1 + ..) / C in channel order."""
    x = np.asarray(x)
    v = x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
    if v.ndim == 1:
        return v
    acc = v[:, 0].copy()
    for c in range(1, v.shape[1]):
        acc += v[:, c]
    return acc / v.shape[1] if v.shape[1] > 1 else acc


def resample(x, sr_orig, sr_new):
    """The direct sum over every input frame a kernel of half-width Z / s can reach."""
    x = to_mono(x)
    if int(sr_orig) == int(sr_new):
        return x.copy()
    ratio, s, p, q = terms(sr_orig, sr_new)
    M = length(x.size, sr_orig, sr_new)
    reach = int(np.ceil(Z / s)) + 1
    n0, r = np.divmod(np.arange(M, dtype=np.int64) * q, p)
    d = np.arange(-reach, reach + 1, dtype=np.int64)
    y = np.zeros(M, np.float64)
    for lo in range(0, M, 512):                                   # [512, 2 reach + 1] at a time
        hi = min(M, lo + 512)
        j = n0[lo:hi, None] + d[None, :]
        tau = s * (d[None, :].astype(np.float64) - (r[lo:hi, None].astype(np.float64) / p))
        xs = np.where((j >= 0) & (j < x.size), x[np.clip(j, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
        y[lo:hi] = (xs * (s * h(tau))).sum(axis=1)
    return y


def taps(sr_orig, sr_new):
    """(p, q, left, table [p, width]): table[r, c] = s h(s ((c - left) - r / p)) over the columns d = c - left that some phase
    reaches: phase 0 reaches furthest back, phase p - 1 furthest on."""
    if int(sr_orig) == int(sr_new):
        return 1, 1, 0, np.ones((1, 1))
    ratio, s, p, q = terms(sr_orig, sr_new)
    reach = int(np.ceil(Z / s)) + 1
    left = max(d for d in range(1, reach + 1) if abs(s * (float(-d) - 0.0 / p)) < Z)
    right = max(d for d in range(1, reach + 1) if abs(s * (float(d) - float(p - 1) / p)) < Z)
    d = np.arange(-left, right + 1, dtype=np.float64)
    r = np.arange(p, dtype=np.float64)
    return p, q, left, s * h(s * (d[None, :] - r[:, None] / p))


def scipy_form(x, sr_orig, sr_new):
    """resample_poly(x, p, q, window=g / p)[:M] with g[m] = s h(s m / p), |m| <= ceil(Z p / s): resample_poly scales the window
    by p and centres it, which is this sum."""
    from scipy.signal import resample_poly
    x = to_mono(x)
    ratio, s, p, q = terms(sr_orig, sr_new)
    half = int(np.ceil(Z * p / s))
    m = np.arange(-half, half + 1, dtype=np.float64)
    g = s * h(s * m / p)
    return resample_poly(x, p, q, window=g / p)[:length(x.size, sr_orig, sr_new)]


def to_int16(y):
    return np.clip(np.rint(np.asarray(y, np.float64) * 32768.0), -32768, 32767).astype(np.int16)
