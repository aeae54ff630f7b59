"""STOI (Taal, Hendriks, Heusdens, Jensen 2011) restated in numpy / scipy float64, stage by stage as DESIGN.md "STOI"
specifies it: the pin of rced_stoi.  The reference takes the metric from pystoi, which is not available to this project;
parity is therefore with this restatement and with the analytic properties tests/test_stoi_host.py checks, not with pystoi.
Not a test module: tests/test_stoi_host.py and tests/test_stoi_gpu.py import it."""

import math

import numpy as np
from scipy.signal import resample_poly

FS, N_FRAME, NFFT, NUMBAND, MINFREQ, N, BETA, DYN_RANGE = 10000, 256, 512, 15, 150, 30, -15.0, 40
HOP = N_FRAME // 2
EPS = np.finfo(float).eps
TOO_SHORT = 1e-5


def thirdoct():
    """(band matrix [15, 257], [(lo, hi)] half-open bin ranges)."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND).astype(float)
    fl, fh = MINFREQ * 2.0 ** ((2 * k - 1) / 6), MINFREQ * 2.0 ** ((2 * k + 1) / 6)
    obm, edges = np.zeros((NUMBAND, len(f))), []
    for i in range(NUMBAND):
        lo, hi = int(np.argmin((f - fl[i]) ** 2)), int(np.argmin((f - fh[i]) ** 2))
        obm[i, lo:hi] = 1
        edges.append((lo, hi))
    return obm, edges


def resample_window(p, q):
    g = math.gcd(p, q)
    p, q = p // g, q // g
    fc = 1.0 / (2 * max(p, q))
    rolloff, rejection = fc / 10, 60.0
    half = int(np.ceil((rejection - 8) / (28.714 * rolloff)))
    t = np.arange(-half, half + 1)
    return np.kaiser(2 * half + 1, 0.1102 * (rejection - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)


def resample(x, fs_sig):
    h = resample_window(FS, fs_sig)
    g = math.gcd(FS, fs_sig)
    return resample_poly(x, FS // g, fs_sig // g, window=h / np.sum(h))


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_starts(length):
    return range(0, length - N_FRAME, HOP)


def frame_energies(x):
    """20 log10(|| w * frame || + EPS) of every frame of the (10 kHz) clean signal."""
    w = window()
    if not len(frame_starts(len(x))):
        return np.zeros(0)
    xf = np.array([w * x[i:i + N_FRAME] for i in frame_starts(len(x))])
    return 20 * np.log10(np.linalg.norm(xf, axis=1) + EPS)


def remove_silent(x, y):
    w = window()
    e = frame_energies(x)
    mask = (np.max(e) - DYN_RANGE - e) < 0
    starts = [s for s, keep in zip(frame_starts(len(x)), mask) if keep]
    n = (len(starts) - 1) * HOP + N_FRAME
    xs, ys = np.zeros(n), np.zeros(n)
    for i, s in enumerate(starts):
        xs[i * HOP:i * HOP + N_FRAME] += w * x[s:s + N_FRAME]
        ys[i * HOP:i * HOP + N_FRAME] += w * y[s:s + N_FRAME]
    return xs, ys, mask, e


def spectra(x):
    w = window()
    return np.array([np.fft.rfft(w * x[i:i + N_FRAME], n=NFFT) for i in frame_starts(len(x))]).reshape(-1, NFFT // 2 + 1).T


def stoi_detail(x, y, fs_sig):
    """(d, (F, K, M), e): the score, the counts of frames at 10 kHz / frames kept / segments, the per-frame energies."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError("x and y must be 1-D signals of one length")
    if fs_sig != FS:
        x, y = (resample(x, fs_sig), resample(y, fs_sig)) if len(x) else (x, y)
    F = len(frame_starts(len(x)))
    if F == 0:
        return TOO_SHORT, (0, 0, 0), np.zeros(0)
    x, y, mask, e = remove_silent(x, y)
    K = int(mask.sum())
    X, Y = spectra(x), spectra(y)
    if X.shape[-1] < N:
        return TOO_SHORT, (F, K, 0), e
    obm, _ = thirdoct()
    xt, yt = np.sqrt(obm @ np.abs(X) ** 2), np.sqrt(obm @ np.abs(Y) ** 2)
    xs = np.array([xt[:, m - N:m] for m in range(N, xt.shape[1] + 1)])
    ys = np.array([yt[:, m - N:m] for m in range(N, xt.shape[1] + 1)])
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yp = np.minimum(ys * c, xs * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xs = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xs = xs / (np.linalg.norm(xs, axis=2, keepdims=True) + EPS)
    M, J = xs.shape[0], xs.shape[1]
    assert (M, J) == (K - N, NUMBAND)
    return float(np.sum(yp * xs) / (J * M)), (F, K, M), e


def stoi(x, y, fs_sig):
    return stoi_detail(x, y, fs_sig)[0]


def speechlike(length, seed, fs=8000):
    """(seed: an int or a numpy Generator.)  A seeded gated-harmonic signal: a 3 Hz on/off gate over seven harmonics, with a -80 dB noise floor, so that
    silent-frame removal really removes frames."""
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    t = np.arange(length) / float(fs)
    env = (np.sin(2 * np.pi * 3 * t) > 0) * (0.3 + 0.7 * np.abs(np.sin(2 * np.pi * 0.7 * t)))
    tone = sum(np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) / (i + 1) for i, f in enumerate([180, 360, 540, 900, 1400, 2200, 3100]))
    return env * tone + 1e-4 * rng.standard_normal(length)


def add_white(x, snr_db, seed):
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    n = rng.standard_normal(len(x))
    return x + n * np.sqrt((x ** 2).sum() / 10 ** (snr_db / 10) / (n ** 2).sum())
