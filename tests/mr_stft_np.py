"""Test infrastructure, not product code: the multi-resolution STFT term and its gradient with respect to the signal (rced.h,
rced_mr_stft), written from the definition in float64, two float32 restatements of the same chain (the yardsticks of the device's
bar, as wave_loss_np.MODES: plain order; the device's association) and a torch-float64 autograd form.

Per utterance: y the signal, c the clean one, [lo, hi) the scored range, K resolutions (W, S, name):
    J = floor((hi - lo - W) / S) + 1 whole frames inside the range (0 if hi - lo < W);  X_j = rfft_256(w x[lo + j S : lo + j S + W]);
    |X|_eps = sqrt(re^2 + im^2 + 1e-8);  A = sum (|C| - |Y|)^2, B = sum |C|^2, sc = sqrt(A / B);
    lsd = sum (ln|C| - ln|Y|)^2 / (129 J);  term = sum_{J > 0} (sc + lsd) / K;  valid = any J > 0.
Gradient of scale * term:  g = -(|C| - |Y|) / (sqrt(A) sqrt(B)) - 2 d / (129 J |Y|), the first part 0 where A = 0;  G = g Y / |Y|;
    d/dy[lo + j S + k] += w[k] sum_b (G_re cos(2 pi b k / 256) - G_im sin(2 pi b k / 256)), times scale / K; frames in ascending j,
    then resolutions in ascending r."""

import numpy as np

import framing_np as fn
from wave_loss_fr_np import _matmul32
from wave_loss_np import MODES, _f32, _forward_matrix  # noqa: F401

BINS, NFFT = 129, 256
EPS = 1e-8


def frames_in(lo, hi, W, S):
    return (hi - lo - W) // S + 1 if hi - lo >= W else 0


def _cut(x, lo, J, W, S):
    return np.stack([np.asarray(x[lo + j * S:lo + j * S + W]) for j in range(J)])


def _synth_matrix():
    """[258 slots (2b + c), 256 samples] float64: slot (b, re) -> cos(2 pi b k / 256), slot (b, im) -> -sin: the transpose of
    _forward_matrix, no 1 / 256 and no kappa."""
    return _forward_matrix().T.copy()


def _spectra(x, lo, J, W, S, name, mode):
    """(re, im) [J, 129] of the frames of x in the mode's arithmetic; the imaginary parts of bins 0 and 128 are exactly zero."""
    w = fn.window(name, W)
    seg = _cut(x, lo, J, W, S)
    if mode == "f64":
        X = np.fft.rfft(seg.astype(np.float64) * w, NFFT)
        return X.real.copy(), X.imag.copy()
    if mode == "f32_plain":
        X = _matmul32(_f32(seg) * _f32(w), _forward_matrix()[:W])
    else:
        X = _matmul32(_f32(seg), _forward_matrix()[:W] * w[:, None])
    re, im = X[:, 0::2].copy(), X[:, 1::2].copy()
    im[:, 0] = im[:, 128] = 0
    return re, im


def _mag(re, im, mode):
    if mode == "f64":
        return np.sqrt(re * re + im * im + EPS)
    if mode == "f32_plain":
        return np.sqrt(re * re + im * im + np.float32(EPS))
    return _f32(np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2 + EPS))      # fp64 under the root, rounded once


def magnitudes(x, lo, hi, W, S, name, mode="f64"):
    """|X|_eps [J, 129] of the whole frames of x inside [lo, hi) in one mode, as float64 values; [0, 129] where there is none."""
    J = frames_in(lo, hi, W, S)
    if J == 0:
        return np.zeros((0, BINS))
    return _mag(*_spectra(x, lo, J, W, S, name, mode), mode).astype(np.float64)


def mr_stft(y, c, lo, hi, resolutions, scale=1.0, mode="f64", grad=True):
    """((term, valid, [(sc, lsd, J)] per resolution), d(scale * term) / dy [len(y)] or None) of one utterance in one mode.  The sums
    are float64 sums of the mode's magnitudes in every mode (the definition says so)."""
    dt = np.float64 if mode == "f64" else np.float32
    K = len(resolutions)
    g_y = np.zeros(len(y), dt) if grad else None
    term, valid, detail = 0.0, 0.0, []
    for W, S, name in resolutions:
        J = frames_in(lo, hi, W, S)
        if J == 0:
            detail.append((0.0, 0.0, 0))
            continue
        yre, yim = _spectra(y, lo, J, W, S, name, mode)
        cre, cim = _spectra(c, lo, J, W, S, name, mode)
        ym, cm = _mag(yre, yim, mode), _mag(cre, cim, mode)
        ym64, cm64 = ym.astype(np.float64), cm.astype(np.float64)
        A, B = float(np.sum((cm64 - ym64) ** 2)), float(np.sum(cm64 ** 2))
        d64 = np.log(cm64) - np.log(ym64)
        sc, lsd = float(np.sqrt(A / B)), float(np.sum(d64 ** 2)) / (BINS * J)
        term, valid = term + sc + lsd, 1.0
        detail.append((sc, lsd, J))
        if not grad:
            continue
        c1 = scale / K / (np.sqrt(A) * np.sqrt(B)) if A > 0 else 0.0
        c2 = scale / K * 2.0 / (BINS * J)
        w = fn.window(name, W)
        if mode == "f32_plain":
            g = -(cm - ym) * np.float32(c1) - np.float32(c2) * np.log(cm / ym) / ym      # (one logarithm: two would cancel in float32)
            q = g / ym
            G = np.empty((J, 2 * BINS), np.float32)
            G[:, 0::2], G[:, 1::2] = q * yre, q * yim
            x = _matmul32(G, _synth_matrix()[:, :W]) * _f32(w)
        else:      # float64 from the mode's magnitudes, G rounded once in f32_device
            q = (-(cm64 - ym64) * c1 - c2 * d64 / ym64) / ym64
            G = np.empty((J, 2 * BINS), dt)
            G[:, 0::2], G[:, 1::2] = q * yre, q * yim
            if mode == "f64":
                x = (G @ _synth_matrix()[:, :W]) * w
            else:
                x = _matmul32(G, _synth_matrix()[:, :W] * w[None, :])
        for j in range(J):      # ascending frames, then ascending resolutions: one chain per sample
            g_y[lo + j * S:lo + j * S + W] += x[j]
    return (term / K, valid, detail), g_y


def torch_term(y, c, lo, hi, resolutions):
    """(term, valid) with term a torch float64 scalar differentiable in y (a float64 tensor): the definition in torch operations."""
    import torch
    K = len(resolutions)
    term, valid = y.sum() * 0, 0.0
    cc = torch.as_tensor(np.asarray(c, np.float64))
    for W, S, name in resolutions:
        J = frames_in(lo, hi, W, S)
        if J == 0:
            continue
        at = torch.as_tensor(lo + np.arange(J)[:, None] * S + np.arange(W)[None, :])
        w = torch.as_tensor(fn.window(name, W))
        Y, C = torch.fft.rfft(y[at] * w, n=NFFT), torch.fft.rfft(cc[at] * w, n=NFFT)
        keep = torch.ones(BINS, dtype=torch.float64)
        keep[0] = keep[128] = 0                                   # rfft of a real frame: these two imaginary parts are zero
        ym = torch.sqrt(Y.real ** 2 + (Y.imag * keep) ** 2 + EPS)
        cm = torch.sqrt(C.real ** 2 + (C.imag * keep) ** 2 + EPS)
        term = term + torch.sqrt(((cm - ym) ** 2).sum() / (cm ** 2).sum()) + ((torch.log(cm) - torch.log(ym)) ** 2).sum() / (BINS * J)
        valid = 1.0
    return term / K, valid


# ---------------------------------------------------------------------------------------- the wave objective with the term

def wave_loss_mr(mag, phase, clean, length, F, a_sse, a_si, a_mr, skip_edges, W, S, name, resolutions, mode="f64", y=None):
    """rced_wave_loss_mr of one utterance in one mode: ((wave_sse, si_sdr, valid, mr_stft, mr_valid), dM [T, 129], the term's detail).
    a_x = weight / B.  wave_loss_fr_np's chain with the term's gradient with respect to y added to g_y on R, in float64 before the one
    rounding (f32_device) or in float32 (f32_plain); with a_mr = 0 it is wave_loss_fr_np.gradient (test_mr_stft_host.py)."""
    import wave_loss_fr_np as wf
    from wave_loss_np import K_DB, _fma32
    phase = np.asarray(phase)
    T = phase.shape[0]
    if y is None:
        y = wf.rebuild(mag, phase, F, W, S, name, mode)
    dt = np.float64 if mode == "f64" else np.float32
    lo, hi = wf.scored_range(length, F, skip_edges, W, S)
    sse, si, valid, alpha, target, resid = wf.terms(y, clean, length, F, skip_edges, W, S)
    n = wf.n_out(F, W, S)
    (term, mr_valid, detail), g_mr = mr_stft(y[:n], np.asarray(clean)[:max(hi, 0)] if hi > lo else np.zeros(0), lo, hi, resolutions, a_mr, mode)
    grad = np.zeros((T, BINS), dt)
    terms = (sse, si, valid, term, mr_valid)
    if F <= 0:
        return terms, grad, detail
    q1 = a_si * K_DB * 2 * alpha / (target + wf.EPS) if valid else 0.0
    q2 = a_si * K_DB * 2 / (resid + wf.EPS) if valid else 0.0
    gy = np.zeros(n, dt)
    if hi > lo:
        if mode == "f32_plain":
            yy, c = _f32(y[lo:hi]), _f32(clean[lo:hi])
            r = yy - np.float32(alpha) * c
            gy[lo:hi] = (np.float32(2 * a_sse) * (yy - c) - (np.float32(q1) * c - np.float32(q2) * r)) + g_mr[lo:hi]
        else:   # float64, rounded once in f32_device
            yy, c = np.asarray(y[lo:hi], np.float64), np.asarray(clean[lo:hi], np.float64)
            gy[lo:hi] = (2 * a_sse * (yy - c) + (q2 * (yy - alpha * c) - q1 * c)) + g_mr[lo:hi].astype(np.float64)
    ge = wf._scan(gy, mode, reverse=True)
    w = fn.window(name, W)
    kap = np.where((np.arange(BINS) == 0) | (np.arange(BINS) == 128), 1.0, 2.0) / NFFT
    den = wf.denominator(F, W, S, name, mode)
    ok = den > dt(wf.FLOOR)
    u = np.zeros(n, dt)
    if mode == "f32_device":
        u[ok] = ge[ok] * (np.float32(1) / den[ok])
    else:
        u[ok] = ge[ok] / den[ok]
    seg = np.stack([u[t * S:t * S + W] for t in range(F)])
    pr, pi = phase[:F].real.astype(dt), phase[:F].imag.astype(dt)
    if mode == "f64":
        G = np.fft.rfft(seg * w, NFFT)
        grad[:F] = kap * (pr * G.real + pi * G.imag)
    elif mode == "f32_plain":
        G = _matmul32(seg * _f32(w), _forward_matrix()[:W])
        im = pi * G[:, 1::2]
        im[:, 0] = im[:, 128] = 0
        grad[:F] = _f32(kap) * (pr * G[:, 0::2] + im)
    else:
        G = _matmul32(seg, _forward_matrix()[:W] * w[:, None] * np.repeat(kap, 2)[None, :])
        grad[:F] = _fma32(pr, G[:, 0::2], _f32(pi * G[:, 1::2]))
        grad[:F, 0], grad[:F, 128] = pr[:, 0] * G[:, 0], pr[:, 128] * G[:, 256]
    return terms, grad, detail


def torch_rebuild(mag, phase, F, W, S, name):
    """y [n_out] of one utterance as a torch float64 tensor differentiable in `mag` [T, 129]: wave_loss_fr_np.torch_terms' rebuild,
    for the term to be taken of it."""
    import torch
    import wave_loss_fr_np as wf
    ph = torch.as_tensor(np.asarray(phase[:F], np.complex128))
    keep = torch.ones(BINS, dtype=torch.float64)
    keep[0] = keep[128] = 0
    spec = torch.complex(mag[:F] * ph.real, mag[:F] * ph.imag * keep)
    x = torch.fft.irfft(spec, n=NFFT)[:, :W] * torch.as_tensor(fn.window(name, W))
    n = wf.n_out(F, W, S)
    at = torch.as_tensor((np.arange(F)[:, None] * S + np.arange(W)[None, :]).reshape(-1))
    num = torch.zeros(n, dtype=torch.float64).index_add(0, at, x.reshape(-1))
    den = fn.ola_sums(F, W, S, name)[1]
    ok = den > wf.FLOOR
    e = num * torch.as_tensor(np.where(ok, 1.0 / np.where(ok, den, 1.0), 0.0))
    B = 128
    pw = wf.PRE ** np.arange(B + 1)
    tri = torch.as_tensor(np.tril(pw[np.subtract.outer(np.arange(B), np.arange(B)).clip(0)]))
    e = torch.cat([e, torch.zeros(-n % B, dtype=torch.float64)])
    blocks, carry = [], mag.sum() * 0
    for h in range(len(e) // B):
        yb = tri @ e[B * h:B * (h + 1)] + torch.as_tensor(pw[1:]) * carry
        blocks.append(yb)
        carry = yb[-1]
    return torch.cat(blocks)[:n]
