"""Test infrastructure, not product code: the float64 restatement of the waveform terms of the training objective and of their
gradient (rced.h, rced_wave_loss), written from the definition over ola_np.ola, two float32 restatements of the same chain
(the yardsticks of the device's bar) and a torch-float64 autograd form of the terms.

Per utterance: M [T, 129] the prediction, P [T, 129] complex the mixture's unit phase, F frames, c the clean signal, l samples.
    y = ola(M, P, F);   R = [128, min(l, 128 F)) with skip_edges, else [0, min(l, 128 (F + 1)));
    wave_sse = sum_R (y - c)^2;   alpha = <y,c> / <c,c>;   si_sdr = 10 log10((|alpha c|^2 + eps) / (|y - alpha c|^2 + eps)), eps = 1e-8;
    <c,c> = 0 or R empty: the SI-SDR term is invalid (counts 0, gradient 0).
Gradient of  a_sse * sum wave_sse - a_si * sum_valid si_sdr  (a_x = weight / B), k = 10 / ln 10, r = y - alpha c:
    g_y = a_sse 2 (y - c) - a_si k (2 alpha c / (|alpha c|^2 + eps) - 2 r / (|r|^2 + eps)) on R, 0 outside;
    g_e[i] = g_y[i] + 0.97 g_e[i+1];   u = g_e / sum w^2;   G_t = rfft(w u[128t : 128t + 256]);
    dM_t[b] = (kappa_b / 256)(P_re G_re + P_im G_im), kappa = 1 at bins 0 and 128, 2 elsewhere; 0 for t >= F."""

import numpy as np

import ola_np
import td_metrics_np

FRAME, STEP, BINS = ola_np.FRAME, ola_np.STEP, 129
PRE = ola_np.PRE_EMPHASIS
EPS = 1e-8
K_DB = 10.0 / np.log(10.0)
MODES = ("f64", "f32_plain", "f32_device")


def num_frames(length):
    """rced_stft_num_frames: ceil(|l - 256| / 128 + 1), 0 for an empty signal."""
    return 0 if length <= 0 else (abs(length - FRAME) + STEP - 1) // STEP + 1


def scored_range(length, frames, skip_edges):
    lo = STEP if skip_edges else 0
    hi = min(int(length), STEP * (frames if skip_edges else frames + 1))
    return (lo, hi) if frames > 0 and hi > lo else (0, 0)


def denominator(frames):
    w = np.hamming(FRAME)
    den = np.zeros((frames + 1) * STEP)
    for t in range(frames):
        den[STEP * t:STEP * t + FRAME] += w * w
    return den


# ------------------------------------------------------------------------------------------------------------- float32 helpers

def _f32(x):
    return np.asarray(x, np.float32)


def _fma32(a, b, c):
    """fmaf on float32 values: the product of two float32 is exact in float64, one rounding of the sum to float64 and one to float32."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _inverse_matrix():
    """[258 slots (2b + c), 256 samples] float64: irfft(256) as a real matrix; the imaginary parts of bins 0 and 128 have zero rows."""
    n, b = np.arange(FRAME)[None, :], np.arange(BINS)[:, None]
    th = 2 * np.pi * ((b * n) % FRAME) / FRAME
    kap = np.where((b == 0) | (b == 128), 1.0, 2.0) / FRAME
    m = np.zeros((2 * BINS, FRAME))
    m[0::2] = kap * np.cos(th)
    m[1::2] = -kap * np.sin(th)
    m[1] = m[2 * 128 + 1] = 0.0
    return m


def _forward_matrix():
    """[256 samples, 258 slots]: rfft(256) as a real matrix, (re, im) of bin b in slots 2b, 2b + 1."""
    n, b = np.arange(FRAME)[:, None], np.arange(BINS)[None, :]
    th = 2 * np.pi * ((b * n) % FRAME) / FRAME
    m = np.zeros((FRAME, 2 * BINS))
    m[:, 0::2] = np.cos(th)
    m[:, 1::2] = -np.sin(th)
    return m


# ------------------------------------------------------------------------------------------------------------------ the rebuild

def rebuild(mag, phase, frames, mode="f64"):
    """y [(T + 1) * 128] of one utterance.  f64: ola_np.ola.  f32_plain: the definition in float32, one step at a time (irfft as a
    float32 matrix product, numerator and denominator summed apart, a division, the recursion).  f32_device: the device's
    association -- w and the interior denominator folded into the coefficients, the sum of the two halves, the two single-frame
    hops put right by one factor, the recursion with fused multiply-adds."""
    mag, phase = np.asarray(mag), np.asarray(phase)
    T, F = mag.shape[0], frames
    if mode == "f64":
        return ola_np.ola(mag, phase, F)
    out = np.zeros((T + 1) * STEP, np.float32)
    if F == 0:
        return out
    w = np.hamming(FRAME)
    spec = np.empty((F, 2 * BINS), np.float32)
    spec[:, 0::2] = _f32(mag[:F]) * _f32(phase[:F].real)
    spec[:, 1::2] = _f32(mag[:F]) * _f32(phase[:F].imag)
    if mode == "f32_plain":
        x = spec @ _f32(_inverse_matrix())
        num, den, w32 = np.zeros((F + 1) * STEP, np.float32), np.zeros((F + 1) * STEP, np.float32), _f32(w)
        for t in range(F):
            num[STEP * t:STEP * t + FRAME] += w32 * x[t]
            den[STEP * t:STEP * t + FRAME] += w32 * w32
        e = num / den
        acc = np.float32(0)
        for i in range(len(e)):
            acc = e[i] + np.float32(PRE) * acc
            out[i] = acc
        return out
    d = w[:STEP] ** 2 + w[STEP:] ** 2
    x = spec @ _f32(_inverse_matrix() * (w / np.tile(d, 2))[None, :])
    e = np.zeros((F + 1) * STEP, np.float32)
    e[:F * STEP] = x[:, :STEP].reshape(-1)
    e[STEP:] += x[:, STEP:].reshape(-1)
    e[:STEP] *= _f32(d / w[:STEP] ** 2)
    e[F * STEP:] *= _f32(d / w[STEP:] ** 2)
    acc = np.float32(0)
    for i in range(len(e)):
        acc = _fma32(np.float32(PRE), acc, e[i])
        out[i] = acc
    return out


# -------------------------------------------------------------------------------------------------------- terms and gradient

def terms(y, clean, length, frames, skip_edges):
    """(wave_sse, si_sdr, valid, alpha, |alpha c|^2, |r|^2) in float64 from y and the clean signal as they are."""
    lo, hi = scored_range(length, frames, skip_edges)
    yr, c = np.asarray(y[lo:hi], np.float64), np.asarray(clean[lo:hi], np.float64)
    sse = float(np.sum((yr - c) ** 2))
    if hi <= lo or not np.sum(c * c) > 0:
        return sse, 0.0, 0.0, 0.0, 0.0, 0.0
    alpha, target, resid = td_metrics_np.si_sdr_parts(c, yr)
    return sse, float(10 * np.log10((target + EPS) / (resid + EPS))), 1.0, alpha, target, resid


def gradient(y, phase, clean, length, frames, a_sse, a_si, skip_edges, mode="f64"):
    """dM [T, 129] from the rebuilt y (of the same mode), a_sse = w_sse / B, a_si = w_si_sdr / B.  The scalars are float64 sums
    of the signals as they are in every mode (the definition says so); what follows them is the mode's arithmetic."""
    phase = np.asarray(phase)
    T, F = phase.shape[0], frames
    dt = np.float64 if mode == "f64" else np.float32
    grad = np.zeros((T, BINS), dt)
    lo, hi = scored_range(length, F, skip_edges)
    if F == 0:
        return grad
    _, _, valid, alpha, target, resid = terms(y, clean, length, F, skip_edges)
    q1 = a_si * K_DB * 2 * alpha / (target + EPS) if valid else 0.0
    q2 = a_si * K_DB * 2 / (resid + EPS) if valid else 0.0
    n = (F + 1) * STEP
    gy = np.zeros(n, dt)
    if hi > lo:
        if mode == "f32_plain":
            yy, c = _f32(y[lo:hi]), _f32(clean[lo:hi])
            r = yy - np.float32(alpha) * c
            gy[lo:hi] = np.float32(2 * a_sse) * (yy - c) - (np.float32(q1) * c - np.float32(q2) * r)
        else:   # float64, rounded once in f32_device
            yy, c = np.asarray(y[lo:hi], np.float64), np.asarray(clean[lo:hi], np.float64)
            gy[lo:hi] = 2 * a_sse * (yy - c) + (q2 * (yy - alpha * c) - q1 * c)
    ge = np.zeros(n, dt)
    acc = dt(0)
    for i in range(n - 1, -1, -1):
        acc = _fma32(np.float32(PRE), acc, gy[i]) if mode == "f32_device" else gy[i] + dt(PRE) * acc
        ge[i] = acc
    w = np.hamming(FRAME)
    kap = np.where((np.arange(BINS) == 0) | (np.arange(BINS) == 128), 1.0, 2.0) / FRAME
    if mode == "f32_device":
        inv = np.tile(_f32(1.0 / (w[:STEP] ** 2 + w[STEP:] ** 2)), F + 1)
        inv[:STEP] = _f32(1.0 / w[:STEP] ** 2)
        inv[F * STEP:] = _f32(1.0 / w[STEP:] ** 2)
        u = ge * inv
        seg = np.stack([u[STEP * t:STEP * t + FRAME] for t in range(F)])
        G = seg @ _f32(_forward_matrix() * w[:, None] * np.repeat(kap, 2)[None, :])
        pr, pi = _f32(phase[:F].real), _f32(phase[:F].imag)
        grad[:F] = _fma32(pr, G[:, 0::2], _f32(pi * G[:, 1::2]))
        grad[:F, 0], grad[:F, 128] = pr[:, 0] * G[:, 0], pr[:, 128] * G[:, 256]
        return grad
    den = denominator(F).astype(dt) if mode == "f64" else None
    if mode == "f32_plain":
        den, w32 = np.zeros(n, np.float32), _f32(w)
        for t in range(F):
            den[STEP * t:STEP * t + FRAME] += w32 * w32
    u = ge / den
    seg = np.stack([u[STEP * t:STEP * t + FRAME] for t in range(F)]) * w.astype(dt)
    if mode == "f64":
        G = np.fft.rfft(seg, FRAME)
        grad[:F] = kap * (phase[:F].real * G.real + phase[:F].imag * G.imag)
    else:
        G = seg @ _f32(_forward_matrix())
        pr, pi = _f32(phase[:F].real), _f32(phase[:F].imag)
        im = pi * G[:, 1::2]
        im[:, 0] = im[:, 128] = 0
        grad[:F] = _f32(kap) * (pr * G[:, 0::2] + im)
    return grad


def wave_loss(mag, phase, clean, length, frames, a_sse, a_si, skip_edges, mode="f64", y=None):
    """((wave_sse, si_sdr, valid), dM [T, 129], y) of one utterance in one mode; y: the mode's rebuild if the caller has it."""
    if y is None:
        y = rebuild(mag, phase, frames, mode)
    return terms(y, clean, length, frames, skip_edges)[:3], gradient(y, phase, clean, length, frames, a_sse, a_si, skip_edges, mode), y


def objective(mag, phase, clean, length, frames, a_sse, a_si, skip_edges):
    """a_sse wave_sse - a_si si_sdr (0 for an invalid row), float64: what `gradient` differentiates."""
    sse, si, valid = terms(ola_np.ola(mag, phase, frames), clean, length, frames, skip_edges)[:3]
    return a_sse * sse - a_si * valid * si


# ------------------------------------------------------------------------------------------------------------------ torch form

def torch_terms(mag, phase, clean, length, frames, skip_edges):
    """(wave_sse, si_sdr, valid) as torch float64 scalars, differentiable in `mag` [T, 129] (a float64 tensor); the same chain
    written with torch operations, so that it composes with a float64 network whose output is `mag`."""
    import torch
    F = frames
    lo, hi = scored_range(length, F, skip_edges)
    zero = mag.sum() * 0
    if hi <= lo:
        return zero, zero, 0.0
    ph = torch.as_tensor(np.asarray(phase[:F], np.complex128))
    keep = torch.ones(BINS, dtype=torch.float64)
    keep[0] = keep[128] = 0                                  # irfft ignores these two imaginary parts: made explicit
    spec = torch.complex(mag[:F] * ph.real, mag[:F] * ph.imag * keep)
    x = torch.fft.irfft(spec, n=FRAME) * torch.as_tensor(np.hamming(FRAME))
    pad = torch.zeros(STEP, dtype=torch.float64)
    e = (torch.cat([x[:, :STEP].reshape(-1), pad]) + torch.cat([pad, x[:, STEP:].reshape(-1)])) / torch.as_tensor(denominator(F))
    pw = PRE ** np.arange(STEP + 1)
    tri = torch.as_tensor(np.tril(pw[np.subtract.outer(np.arange(STEP), np.arange(STEP)).clip(0)]))   # one hop of the recursion
    hops, carry = [], zero
    for h in range(F + 1):
        yb = tri @ e[STEP * h:STEP * (h + 1)] + torch.as_tensor(pw[1:]) * carry
        hops.append(yb)
        carry = yb[-1]
    y = torch.cat(hops)[lo:hi]
    c = torch.as_tensor(np.asarray(clean[lo:hi], np.float64))
    sse = ((y - c) ** 2).sum()
    cc = (c * c).sum()
    if not float(cc) > 0:
        return sse, zero, 0.0
    alpha = (y * c).sum() / cc
    t = alpha * c
    return sse, 10 * torch.log10(((t * t).sum() + EPS) / (((y - t) ** 2).sum() + EPS)), 1.0
