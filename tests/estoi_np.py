"""ESTOI (Jensen, Taal 2016) restated in numpy float64 as DESIGN.md "ESTOI" specifies it: the pin of rced_stoi_ex's extended
half.  Stages 1-4 (resampling, silent-frame removal, spectra, one-third-octave bands) are tests/stoi_np.py's; only the
segment stage is new.  The guards of the divisions are the deterministic `+ EPS` of the classic path, not the EPS-scaled
random numbers of pystoi's row_col_normalize; parity with pystoi is unpinned, as STOI's is.
`f32_dft=True` emulates the one place where the device is below float64: frames rounded to fp32, an fp32 DFT matrix, fp32
dot products of 256 terms; everything else stays float64.
Not a test module: tests/test_metrics_ext_host.py and tests/test_estoi_gpu.py import it."""

import numpy as np

import stoi_np as sn

N, J = sn.N, sn.NUMBAND


def spectra_f32(x):
    """sn.spectra with the device's arithmetic: the windowed DFT as a matrix product, fp32 operands, fp32 accumulation.
    Only the 256 samples of a frame meet the matrix (the zero-padded half drops out)."""
    w = sn.window()
    k = np.arange(sn.N_FRAME)
    b = np.arange(sn.NFFT // 2 + 1)[:, None]
    th = 2 * np.pi * ((b * k) % sn.NFFT) / sn.NFFT
    re, im = (w * np.cos(th)).astype(np.float32), (-w * np.sin(th)).astype(np.float32)
    frames = np.array([x[i:i + sn.N_FRAME] for i in sn.frame_starts(len(x))]).reshape(-1, sn.N_FRAME).astype(np.float32)
    return (re @ frames.T).astype(np.float64) + 1j * (im @ frames.T).astype(np.float64)


def bands(x, y, fs_sig, f32_dft=False):
    """Stages 1-4: (xt, yt [15, K - 1] band amplitudes or None where the score is TOO_SHORT, (F, K, M), e)."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D signals of one length")
    if fs_sig != sn.FS:
        x, y = (sn.resample(x, fs_sig), sn.resample(y, fs_sig)) if len(x) else (x, y)
    F = len(sn.frame_starts(len(x)))
    if F == 0:
        return None, None, (0, 0, 0), np.zeros(0)
    x, y, mask, e = sn.remove_silent(x, y)
    K = int(mask.sum())
    if K - 1 < N:
        return None, None, (F, K, 0), e
    spectra = spectra_f32 if f32_dft else sn.spectra
    X, Y = spectra(x), spectra(y)
    obm, _ = sn.thirdoct()
    return np.sqrt(obm @ np.abs(X) ** 2), np.sqrt(obm @ np.abs(Y) ** 2), (F, K, K - N), e


def segments(t):
    """[M, 15, 30]: the 30 frames [m - 30, m) of every band, m = 30 .. K - 1."""
    return np.array([t[:, m - N:m] for m in range(N, t.shape[1] + 1)])


def row_col_normalize(s):
    """Rows (a band over the 30 frames), then columns (a frame over the 15 bands): subtract the mean, divide by (the
    2-norm + EPS)."""
    s = s - s.mean(axis=2, keepdims=True)
    s = s / (np.linalg.norm(s, axis=2, keepdims=True) + sn.EPS)
    s = s - s.mean(axis=1, keepdims=True)
    return s / (np.linalg.norm(s, axis=1, keepdims=True) + sn.EPS)


def estoi_detail(x, y, fs_sig, f32_dft=False):
    """(d, (F, K, M), e), as sn.stoi_detail."""
    xt, yt, counts, e = bands(x, y, fs_sig, f32_dft)
    if xt is None:
        return sn.TOO_SHORT, counts, e
    xn, yn = row_col_normalize(segments(xt)), row_col_normalize(segments(yt))
    M = xn.shape[0]
    assert (M, xn.shape[1], xn.shape[2]) == (counts[2], J, N)
    return float(np.sum(xn * yn) / (N * M)), counts, e


def estoi(x, y, fs_sig, f32_dft=False):
    return estoi_detail(x, y, fs_sig, f32_dft)[0]


def min_row_norm(y, x, fs_sig):
    """The smallest 2-norm of a mean-free band row of y's segments (the first division's guard is EPS against this)."""
    _, yt, _, _ = bands(x, y, fs_sig)
    s = segments(yt)
    return float(np.linalg.norm(s - s.mean(axis=2, keepdims=True), axis=2).min())
