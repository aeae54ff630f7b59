"""Test infrastructure: the one ragged batch that test_wave_loss_host.py (the guard on the bars) and test_wave_loss_gpu.py (the
device held to them) share, with its float64 reference and the bars.  Computed once, left unchanged.

The bar on a gradient is the rule of forward_bars.py: MARGIN = 4 times the error of float32 restatements of the same chain
(wave_loss_np: one in plain order, one in the device's association), the larger of the two, per row and case, every error
taken as the largest element's over the largest entry of the row's float64 gradient."""

import functools

import numpy as np

import wave_loss_np as wl

MARGIN = 4
T, BATCH = 67, 4
# 65 frames: across the 64-frame block, ends inside a hop | 64 frames: the block that holds hop F alone | 3 frames | 1 frame: an empty
# range under skip_edges | 2 frames, 2 scored samples | nothing | a silent clean signal: the SI-SDR term is invalid
LENGTHS = (8327, 8320, 385, 256, 130, 0, 1000)
SILENT = 6
N = len(LENGTHS)
FRAMES = tuple(wl.num_frames(v) for v in LENGTHS)
CLEAN_WIDTH, CLEAN_STRIDE = 8327, 8401          # rows of a wider buffer, at no alignment
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.5, 1.0))   # (wave_sse, si_sdr): each alone, both
CASES = tuple((w, s) for w in WEIGHTS for s in (True, False))


@functools.lru_cache(maxsize=None)
def batch():
    """(mag [N, T, 129] float32, every frame non-zero; phase [N, T, 129] complex64, bins 0 and 128 non-real; clean [N, width]
    float32: 0.7 of the float64 rebuild plus noise at half its rms, zeros past the length)."""
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((N, T, 129)) + 1j * rng.standard_normal((N, T, 129))
    mag, ph = np.abs(X).astype(np.float32) + np.float32(0.01), np.exp(1j * np.angle(X)).astype(np.complex64)
    clean = np.zeros((N, CLEAN_WIDTH), np.float32)
    for i, (l, F) in enumerate(zip(LENGTHS, FRAMES)):
        if l and i != SILENT:
            y = wl.rebuild(mag[i], ph[i], F)[:l]
            clean[i, :l] = 0.7 * y + 0.5 * np.sqrt(np.mean(y * y)) * rng.standard_normal(l)
    for a in (mag, ph, clean):
        a.setflags(write=False)
    return mag, ph, clean


@functools.lru_cache(maxsize=None)
def rebuilt(row, mode):
    mag, ph, _ = batch()
    y = wl.rebuild(mag[row], ph[row], FRAMES[row], mode)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(weights, skip_edges):
    """Per row: (terms (wave_sse, si_sdr, valid), float64 gradient, the two yardstick errors, the bar)."""
    mag, ph, clean = batch()
    out = []
    for i in range(N):
        res = {m: wl.wave_loss(mag[i], ph[i], clean[i], LENGTHS[i], FRAMES[i], weights[0] / BATCH, weights[1] / BATCH, skip_edges, m,
                               y=rebuilt(i, m)) for m in wl.MODES}
        terms, g = res["f64"][0], res["f64"][1]
        scale = float(np.abs(g).max())
        yard = tuple(float(np.abs(res[m][1] - g).max()) / scale if scale else 0.0 for m in wl.MODES[1:])
        g.setflags(write=False)
        out.append((terms, g, yard, MARGIN * max(yard)))
    return out
