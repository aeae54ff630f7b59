"""Float64 restatement of the three transforms at a framing (W, S, window name) under rfft(256): the STFT
(data_utils/audio_feature.py:22-115), the reference rebuild (model_utils/utils.py:171-183) and the weighted overlap-add rebuild
(DESIGN.md 3.4i).  Pinned to the reference's own code by tests/golden/framing_ref.npz and to scipy.signal.istft
(tests/test_framing_host.py).  numpy only; nothing here is product code."""

import numpy as np

NFFT = 256
BINS = 129
PRE = 0.97
DEN_FLOOR = 1e-10      # scipy.signal.istft: samples whose sum of squared windows is at most this stay zero

WINDOWS = {"hamming": np.hamming, "hanning": np.hanning, "blackman": np.blackman, "bartlett": np.bartlett}
CODES = {"hamming": 0, "hanning": 1, "blackman": 2, "bartlett": 3}

# the framings every framing test runs at
FRAMINGS = [(160, 80, "hamming"), (256, 64, "hanning"), (256, 128, "hanning"), (200, 80, "blackman"), (256, 256, "bartlett"),
            (64, 16, "hamming"), (255, 100, "hanning")]
HAMMING_FRAMINGS = [(160, 80, "hamming"), (64, 16, "hamming"), (256, 128, "hamming")]
FRAMING_IDS = ["%d-%d-%s" % f for f in FRAMINGS]


def tag(W, S, name):
    return "%d_%d_%s" % (W, S, name)


def window(name, W):
    return np.asarray(WINDOWS[name](W), np.float64)


def num_frames(L, W, S):
    return int(np.ceil(float(abs(L - W)) / S + 1))


def width(T, W, S):
    return (W - S) + T * S


def stft(sig, W, S, name):
    """sig: 1-D float32 -> (mag [T, 129], unit phase [T, 129] complex128).  The pre-emphasis runs in the signal's own precision,
    as the reference's does (audio_feature.py:54); everything after it in float64."""
    sig = np.asarray(sig)
    e = np.append(sig[0], sig[1:] - PRE * sig[:-1]).astype(np.float64)
    T = num_frames(len(sig), W, S)
    pad = np.zeros(T * S + W)
    pad[:len(e)] = e
    frames = np.stack([pad[t * S:t * S + W] for t in range(T)]) * window(name, W)
    spec = np.fft.rfft(frames, NFFT)
    return np.abs(spec), np.exp(1j * np.angle(spec))


def de_emphasis(x):
    y = np.array(x, dtype=x.dtype)
    for i in range(1, y.shape[-1]):
        y[..., i] = y[..., i] + PRE * y[..., i - 1]
    return y


def rebuild_reference(mag, phase, W, S, nfft, name="hamming"):
    """mag [T, 129], phase [T, 129] complex -> [(W - S) + T S]: irfft(n = nfft)[:W] / w, the first W - S samples of frame 0 and
    the last S samples of every frame, de-emphasis."""
    x = np.fft.irfft(np.asarray(mag, np.float64) * np.asarray(phase, np.complex128), nfft)[:, :W] / window(name, W)
    return de_emphasis(np.append(x[0, :W - S], x[:, W - S:].reshape(-1)))


def ola_sums(F, W, S, name, dtype=np.float64):
    """(sum of |w|, sum of w^2) per sample of an utterance of F frames, [(F - 1) S + W]."""
    w = window(name, W).astype(dtype)
    a = np.zeros((F - 1) * S + W if F > 0 else 0, dtype)
    d = np.zeros_like(a)
    for t in range(F):
        a[t * S:t * S + W] += np.abs(w)
        d[t * S:t * S + W] += w * w
    return a, d


def rebuild_ola(mag, phase, F, W, S, name, dtype=np.float64):
    """mag [T, 129], phase [T, 129] complex, F <= T frames of them used -> [(W - S) + T S]; frames at or past F are not read."""
    T = mag.shape[0]
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    w = window(name, W).astype(dtype)
    num = np.zeros(width(T, W, S), dtype)
    if F > 0:
        x = np.fft.irfft(np.asarray(mag[:F], dtype) * np.asarray(phase[:F], cdt), NFFT)[:, :W].astype(dtype)
        for t in range(F):
            num[t * S:t * S + W] += w * x[t]
        _, den = ola_sums(F, W, S, name, dtype)
        n = len(den)
        ok = den > DEN_FLOOR
        e = np.zeros(n, dtype)
        e[ok] = num[:n][ok] / den[ok]
        num[:n] = de_emphasis(e)
    return num


def ola_conditioning(F, W, S, name):
    """A[n] = sum_{m <= n} 0.97^(n - m) G[m], G = sum |w| / sum w^2 (0 where the rebuild is zero): how far an error of one unit per
    frame sample can grow in the rebuilt, de-emphasised sample n."""
    a, d = ola_sums(F, W, S, name)
    g = np.zeros_like(a)
    ok = d > DEN_FLOOR
    g[ok] = a[ok] / d[ok]
    return de_emphasis(g)
