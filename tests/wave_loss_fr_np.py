"""Test infrastructure, not product code: the waveform terms of the training objective and their gradient at any framing
(W, S, window name) -- rced.h, rced_wave_loss_fr -- restated over framing_np: the float64 chain, the two float32 chains
wave_loss_np has (plain order; the device's association) and a torch-float64 autograd form.  wave_loss_np, the default framing's
restatement, is left as it is; at 256 / 128 / hamming the float64 chain here equals it (tests/test_wave_loss_fr_host.py).

Per utterance: M [T, 129] the prediction, P [T, 129] complex the mixture's unit phase, F frames, c the clean signal, l samples,
w = numpy's window of the name at length W.
    y = framing_np.rebuild_ola(M, P, F): x_t = irfft(M_t P_t, 256)[:W]; D[i] = sum_t w[i - tS]^2, e[i] = sum_t w[i - tS] x_t[i - tS] / D[i]
        over the frames t < F that cover i, e[i] = 0 where D[i] <= 1e-10; y[i] = e[i] + 0.97 y[i-1]; n_out = (F - 1) S + W;
    R = [W - S, min(l, F S)) with skip_edges, else [0, min(l, n_out)); F <= 0 or an empty R: no contribution, SI-SDR invalid;
    terms, validity, eps, the objective and g_y: wave_loss_np's;
    g_e[i] = g_y[i] + 0.97 g_e[i+1];  u = g_e / D (0 where D <= 1e-10);  G_t = rfft_256(w u[tS : tS + W]);
    dM_t[b] = (kappa_b / 256)(P_re G_re + P_im G_im) for t < F, 0 for t >= F."""

import numpy as np

import framing_np as fn
import td_metrics_np
from wave_loss_np import EPS, K_DB, MODES, _f32, _fma32, _forward_matrix, _inverse_matrix  # noqa: F401

BINS, NFFT, PRE = fn.BINS, fn.NFFT, fn.PRE
FLOOR = fn.DEN_FLOOR


def num_frames(length, W, S):
    """rced_stft_num_frames_fr: 0 for an empty signal."""
    return 0 if length <= 0 else fn.num_frames(length, W, S)


def n_out(F, W, S):
    return (F - 1) * S + W if F > 0 else 0


def scored_range(length, F, skip_edges, W, S):
    lo = W - S if skip_edges else 0
    hi = min(int(length), F * S if skip_edges else n_out(F, W, S))
    return (lo, hi) if F > 0 and hi > lo else (0, 0)


def denominator(F, W, S, name, mode="f64"):
    """D [n_out].  f64: the definition.  f32_plain: float32 w * w, summed in float32.  f32_device: the device's table, w^2 formed in
    double and rounded once, summed in float32.  Both float32 sums run in ascending frame order per sample."""
    w = fn.window(name, W)
    if mode == "f64":
        return fn.ola_sums(F, W, S, name)[1]
    w2 = _f32(w) * _f32(w) if mode == "f32_plain" else _f32(w * w)
    d = np.zeros(n_out(F, W, S), np.float32)
    for t in range(F):
        d[t * S:t * S + W] += w2
    return d


def _matmul32(a, b):
    """a [m, k] @ b [k, n] in float32, the k products of an element rounded and added in ascending k: one summation order on every
    machine (a BLAS picks its blocking by the CPU it runs on, and the bars are made of these errors)."""
    a, b = _f32(a), _f32(b)
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * b[k]
    return acc


def _scan(x, mode, reverse=False):
    """acc = x[i] + 0.97 acc along the array (from the end with reverse) in the mode's arithmetic: float64; float32 with a rounded
    product and a rounded sum; float32 with a fused multiply-add (the product of two float32 is exact in float64)."""
    v = np.asarray(x).tolist()
    if reverse:
        v = v[::-1]
    out, acc = [], 0.0
    if mode == "f64":
        for s in v:
            acc = s + PRE * acc
            out.append(acc)
    else:
        pre, f32 = float(np.float32(PRE)), np.float32
        for s in v:
            acc = float(f32(pre * acc + s)) if mode == "f32_device" else float(f32(s + float(f32(pre * acc))))
            out.append(acc)
    if reverse:
        out = out[::-1]
    return np.asarray(out, np.float64 if mode == "f64" else np.float32)


# ------------------------------------------------------------------------------------------------------------------ the rebuild

def rebuild(mag, phase, F, W, S, name, mode="f64"):
    """y [(W - S) + T S] of one utterance.  f64: framing_np.rebuild_ola.  f32_plain: the definition in float32, one step at a
    time (irfft as a float32 matrix product in ascending order, the window, numerator and denominator summed apart, a division,
    the recursion).  f32_device: the device's association -- w folded into the coefficients, the addends and the table of w^2 summed in ascending
    frame order, a division, the recursion with fused multiply-adds."""
    mag, phase = np.asarray(mag), np.asarray(phase)
    T = mag.shape[0]
    if mode == "f64":
        return fn.rebuild_ola(mag, phase, F, W, S, name)
    out = np.zeros(fn.width(T, W, S), np.float32)
    if F <= 0:
        return out
    w = fn.window(name, W)
    spec = np.empty((F, 2 * BINS), np.float32)
    spec[:, 0::2] = _f32(mag[:F]) * _f32(phase[:F].real)
    spec[:, 1::2] = _f32(mag[:F]) * _f32(phase[:F].imag)
    n = n_out(F, W, S)
    num = np.zeros(n, np.float32)
    if mode == "f32_plain":
        x = _matmul32(spec, _inverse_matrix()[:, :W]) * _f32(w)
    else:
        x = _matmul32(spec, _inverse_matrix()[:, :W] * w[None, :])
    for t in range(F):
        num[t * S:t * S + W] += x[t]
    den = denominator(F, W, S, name, mode)
    ok = den > np.float32(FLOOR)
    e = np.zeros(n, np.float32)
    e[ok] = num[ok] / den[ok]
    out[:n] = _scan(e, mode)
    return out


# -------------------------------------------------------------------------------------------------------- terms and gradient

def terms(y, clean, length, F, skip_edges, W, S):
    """(wave_sse, si_sdr, valid, alpha, |alpha c|^2, |r|^2) in float64 from y and the clean signal as they are."""
    lo, hi = scored_range(length, F, skip_edges, W, S)
    yr, c = np.asarray(y[lo:hi], np.float64), np.asarray(clean[lo:hi], np.float64)
    sse = float(np.sum((yr - c) ** 2))
    if hi <= lo or not np.sum(c * c) > 0:
        return sse, 0.0, 0.0, 0.0, 0.0, 0.0
    alpha, target, resid = td_metrics_np.si_sdr_parts(c, yr)
    return sse, float(10 * np.log10((target + EPS) / (resid + EPS))), 1.0, alpha, target, resid


def gradient(y, phase, clean, length, F, a_sse, a_si, skip_edges, W, S, name, mode="f64"):
    """dM [T, 129] from the rebuilt y (of the same mode), a_sse = w_sse / B, a_si = w_si_sdr / B.  The scalars are float64 sums of
    the signals as they are in every mode; what follows them is the mode's arithmetic."""
    phase = np.asarray(phase)
    T = phase.shape[0]
    dt = np.float64 if mode == "f64" else np.float32
    grad = np.zeros((T, BINS), dt)
    lo, hi = scored_range(length, F, skip_edges, W, S)
    if F <= 0:
        return grad
    _, _, valid, alpha, target, resid = terms(y, clean, length, F, skip_edges, W, S)
    q1 = a_si * K_DB * 2 * alpha / (target + EPS) if valid else 0.0
    q2 = a_si * K_DB * 2 / (resid + EPS) if valid else 0.0
    n = n_out(F, W, S)
    gy = np.zeros(n, dt)
    if hi > lo:
        if mode == "f32_plain":
            yy, c = _f32(y[lo:hi]), _f32(clean[lo:hi])
            r = yy - np.float32(alpha) * c
            gy[lo:hi] = np.float32(2 * a_sse) * (yy - c) - (np.float32(q1) * c - np.float32(q2) * r)
        else:   # float64, rounded once in f32_device
            yy, c = np.asarray(y[lo:hi], np.float64), np.asarray(clean[lo:hi], np.float64)
            gy[lo:hi] = 2 * a_sse * (yy - c) + (q2 * (yy - alpha * c) - q1 * c)
    ge = _scan(gy, mode, reverse=True)
    w = fn.window(name, W)
    kap = np.where((np.arange(BINS) == 0) | (np.arange(BINS) == 128), 1.0, 2.0) / NFFT
    den = denominator(F, W, S, name, mode)
    ok = den > dt(FLOOR)
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
    return grad


def wave_loss(mag, phase, clean, length, F, a_sse, a_si, skip_edges, W, S, name, mode="f64", y=None):
    """((wave_sse, si_sdr, valid), dM [T, 129], y) of one utterance in one mode; y: the mode's rebuild if the caller has it."""
    if y is None:
        y = rebuild(mag, phase, F, W, S, name, mode)
    return (terms(y, clean, length, F, skip_edges, W, S)[:3],
            gradient(y, phase, clean, length, F, a_sse, a_si, skip_edges, W, S, name, mode), y)


def objective(mag, phase, clean, length, F, a_sse, a_si, skip_edges, W, S, name):
    """a_sse wave_sse - a_si si_sdr (0 for an invalid row), float64: what `gradient` differentiates."""
    sse, si, valid = terms(fn.rebuild_ola(mag, phase, F, W, S, name), clean, length, F, skip_edges, W, S)[:3]
    return a_sse * sse - a_si * valid * si


# ------------------------------------------------------------------------------------------------------------------ torch form

def torch_terms(mag, phase, clean, length, F, skip_edges, W, S, name):
    """(wave_sse, si_sdr, valid) as torch float64 scalars, differentiable in `mag` [T, 129] (a float64 tensor): the same chain
    written with torch operations, so that it composes with a float64 network whose output is `mag`."""
    import torch
    lo, hi = scored_range(length, F, skip_edges, W, S)
    zero = mag.sum() * 0
    if hi <= lo:
        return zero, zero, 0.0
    ph = torch.as_tensor(np.asarray(phase[:F], np.complex128))
    keep = torch.ones(BINS, dtype=torch.float64)
    keep[0] = keep[128] = 0                                  # irfft ignores these two imaginary parts: made explicit
    spec = torch.complex(mag[:F] * ph.real, mag[:F] * ph.imag * keep)
    x = torch.fft.irfft(spec, n=NFFT)[:, :W] * torch.as_tensor(fn.window(name, W))
    n = n_out(F, W, S)
    at = torch.as_tensor((np.arange(F)[:, None] * S + np.arange(W)[None, :]).reshape(-1))
    num = torch.zeros(n, dtype=torch.float64).index_add(0, at, x.reshape(-1))
    den = fn.ola_sums(F, W, S, name)[1]
    ok = den > FLOOR
    e = num * torch.as_tensor(np.where(ok, 1.0 / np.where(ok, den, 1.0), 0.0))
    B = 128                                                  # the recursion a block at a time
    pw = PRE ** np.arange(B + 1)
    tri = torch.as_tensor(np.tril(pw[np.subtract.outer(np.arange(B), np.arange(B)).clip(0)]))
    e = torch.cat([e, torch.zeros(-n % B, dtype=torch.float64)])
    blocks, carry = [], zero
    for h in range(len(e) // B):
        yb = tri @ e[B * h:B * (h + 1)] + torch.as_tensor(pw[1:]) * carry
        blocks.append(yb)
        carry = yb[-1]
    y = torch.cat(blocks)[lo:hi]
    c = torch.as_tensor(np.asarray(clean[lo:hi], np.float64))
    sse = ((y - c) ** 2).sum()
    cc = (c * c).sum()
    if not float(cc) > 0:
        return sse, zero, 0.0
    alpha = (y * c).sum() / cc
    t = alpha * c
    return sse, 10 * torch.log10(((t * t).sum() + EPS) / (((y - t) ** 2).sum() + EPS)), 1.0
