"""Test infrastructure: the ragged batch per framing that test_wave_loss_fr_host.py (the guard on the bars) and
test_wave_loss_fr_gpu.py (the device held to them) share, with its float64 reference and the bars.  Computed once per framing,
left unchanged.

The bar on a gradient is the rule of forward_bars.py and wave_loss_cases.py: MARGIN = 4 times the error of float32 restatements of
the same chain (wave_loss_fr_np: plain order, and the device's association), the larger of the two, per row and case, every error
taken as the largest element's over the largest entry of the row's float64 gradient.  The rule is applied a second time to frames
1 .. F - 2 alone, relative to their own largest entry: under a window that ends in zero, 1 / D at the utterance's edge can dominate
a row and hide an interior error."""

import functools

import numpy as np

import framing_np as fn
import wave_loss_fr_np as wf
from wave_loss_cases import MARGIN  # noqa: F401  (4: the project's)

# 20 / 10 ms hamming, the reference's | four frames per sample, the window ends in zero: D = 0 at sample 0 | W no multiple of S |
# S no multiple of 8, row widths no multiple of four | no overlap: lo = 0, the 1e-10 rule fires at every seam inside R | the default,
# through the general kernels
FRAMINGS = [(160, 80, "hamming"), (256, 64, "hanning"), (200, 80, "blackman"), (255, 100, "hanning"), (256, 256, "bartlett"),
            (256, 128, "hamming")]
assert all(f in fn.FRAMINGS or f == (256, 128, "hamming") for f in FRAMINGS)
IDS = ["%d-%d-%s" % f for f in FRAMINGS]
DEFAULT = (256, 128, "hamming")
BATCH = 4
CHUNK = 8192                                     # samples per step of the reverse pass
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.5, 1.0))   # (wave_sse, si_sdr): each alone, both
CASES = tuple((w, s) for w in WEIGHTS for s in (True, False))
SILENT = 7


def big_count(W, S):
    """A frame count whose n_out is past one chunk of the reverse pass and ends inside a later one, and past the 64-frame block."""
    F = max((CHUNK + 700 - W) // S + 1, 67)
    assert wf.n_out(F, W, S) > CHUNK and wf.n_out(F, W, S) % CHUNK
    return F


def counts(W, S):
    """65: across the 64-frame block | 64 | n_out > 8192, ends inside a chunk | 3 | 2 | 1: an empty range under skip_edges wherever
    S <= W - S | no samples | a silent clean row (5 frames)."""
    return (65, 64, big_count(W, S), 3, 2, 1, 0, 5)


def length_of(F, W, S):
    """A length of F frames that ends inside a hop (F >= 2), the window itself (F = 1), nothing (F = 0)."""
    return 0 if F == 0 else W if F == 1 else W + (F - 1) * S - S // 3


class Batch(object):
    def __init__(self, W, S, name):
        self.framing = (W, S, name)
        self.frames = counts(W, S)
        self.lengths = tuple(length_of(F, W, S) for F in self.frames)
        assert tuple(wf.num_frames(v, W, S) for v in self.lengths) == self.frames
        self.N, self.T = len(self.frames), max(self.frames) + 2
        self.clean_width = max(self.lengths)
        self.clean_stride = (self.clean_width + 74) | 1      # rows of a wider buffer at an odd stride
        rng = np.random.default_rng(2025 + 1000 * W + S)
        X = rng.standard_normal((self.N, self.T, 129)) + 1j * rng.standard_normal((self.N, self.T, 129))
        self.mag = np.abs(X).astype(np.float32) + np.float32(0.01)     # every frame non-zero
        self.ph = np.exp(1j * np.angle(X)).astype(np.complex64)        # bins 0 and 128 non-real
        self.clean = np.zeros((self.N, self.clean_width), np.float32)
        for i, (l, F) in enumerate(zip(self.lengths, self.frames)):
            if l and i != SILENT:     # 0.7 of the float64 rebuild plus noise at half its rms
                y = self.rebuilt(i, "f64")[:l]
                self.clean[i, :l] = 0.7 * y + 0.5 * np.sqrt(np.mean(y * y)) * rng.standard_normal(l)
        for a in (self.mag, self.ph, self.clean):
            a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def rebuilt(self, row, mode):
        y = wf.rebuild(self.mag[row], self.ph[row], self.frames[row], *self.framing, mode=mode)
        y.setflags(write=False)
        return y

    @functools.lru_cache(maxsize=None)
    def reference(self, weights, skip_edges):
        """Per row: (terms (wave_sse, si_sdr, valid), the float64 gradient, the two yardstick errors and the bar over the whole row,
        the same three over frames 1 .. F - 2 alone (None where there are none, or where they are all zero))."""
        out = []
        for i in range(self.N):
            F = self.frames[i]
            res = {m: wf.wave_loss(self.mag[i], self.ph[i], self.clean[i], self.lengths[i], F, weights[0] / BATCH, weights[1] / BATCH,
                                   skip_edges, *self.framing, mode=m, y=self.rebuilt(i, m)) for m in wf.MODES}
            terms, g = res["f64"][0], res["f64"][1]
            g.setflags(write=False)

            def yardsticks(sl):
                scale = float(np.abs(g[sl]).max()) if g[sl].size else 0.0
                if not scale:
                    return None
                yard = tuple(float(np.abs(res[m][1][sl] - g[sl]).max()) / scale for m in wf.MODES[1:])
                return yard, MARGIN * max(yard)

            whole = yardsticks(slice(None)) or ((0.0, 0.0), 0.0)
            out.append((terms, g, whole[0], whole[1], yardsticks(slice(1, max(F - 1, 1)))))
        return out


@functools.lru_cache(maxsize=None)
def batch(framing):
    return Batch(*framing)
