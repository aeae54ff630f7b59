"""Test infrastructure, not product code: the float64 restatement of the overlap-add rebuild (rced.h, rced_istft_ola), written
from its definition.  8 kHz, 256-sample hamming window w, stride 128, rfft(256).  For F frames:

    x_t  = irfft(mag[t] * phase[t], 256),  t < F        (numpy's irfft drops the imaginary parts of bins 0 and 128)
    e[i] = sum_t w[i - 128t] x_t[i - 128t] / sum_t w[i - 128t]^2,  i < 128 (F + 1), over the frames t < F that cover i
    y[0] = e[0],  y[i] = e[i] + 0.97 y[i-1]

Hops 0 and F are covered by one frame, so their denominator is that frame's w^2 alone: the sums take care of it."""

import numpy as np

FRAME, STEP = 256, 128
PRE_EMPHASIS = 0.97


def deemphasis(e):
    y = np.empty_like(e)
    acc = 0.0
    for i, v in enumerate(e):
        acc = v + PRE_EMPHASIS * acc if i else v
        y[i] = acc
    return y


def ola(mag, phase, frames=None, length=None):
    """mag [T, 129], phase [T, 129] complex -> y [(T + 1) * 128] float64 (or its first `length` samples).  frames: F in [0, T]
    (None = T): frames t >= F are not read, columns from 128 (F + 1) on are 0 (every column for F = 0)."""
    mag, phase = np.asarray(mag), np.asarray(phase)
    T = mag.shape[0]
    F = T if frames is None else min(max(int(frames), 0), T)
    out = np.zeros((T + 1) * STEP)
    if F:
        w = np.hamming(FRAME)
        x = np.fft.irfft(mag[:F].astype(np.float64) * phase[:F].astype(np.complex128), FRAME)
        num, den = np.zeros((F + 1) * STEP), np.zeros((F + 1) * STEP)
        for t in range(F):
            num[STEP * t:STEP * t + FRAME] += w * x[t]
            den[STEP * t:STEP * t + FRAME] += w * w
        out[:(F + 1) * STEP] = deemphasis(num / den)
    return out if length is None else out[:length]
