"""Test infrastructure: the ragged batches that test_mr_stft_host.py (the guard on the bars) and test_mr_stft_gpu.py (the device held
to them) share, with their float64 references and the bars.  Computed once, left unchanged.

The bar on a gradient is the rule of wave_loss_cases.py: MARGIN = 4 times the error of float32 restatements of the same chain
(mr_stft_np: plain order, and the device's association), the larger of the two, per row and case, every error taken as the
largest element's over the largest entry of the row's float64 gradient.

A term is a scalar: the error of a float64 sum of some ten thousand rounded magnitudes is one draw of a random walk, and four
times one draw of a yardstick does not bound another draw.  So the rule is applied where it is stable -- to the magnitudes: a
restatement's |X|_eps are off by e (an array; the larger of the two chains, element by element), the device's may be off by
MARGIN e in the 2-norm -- and carried to the terms by the triangle inequality (term_bars): with E_c = MARGIN ||e_c||,
E_y = MARGIN ||e_y||, rho the same with relative errors,
    |d sqrt(A)| <= E_c + E_y,  |d sqrt(B)| <= E_c,  |d ||ln C - ln Y|| | <= rho_c + rho_y,
and sc = sqrt(A) / sqrt(B), lsd = ||ln C - ln Y||^2 / (129 J)."""

import functools

import numpy as np

import mr_stft_np as mr
import wave_loss_fr_cases as fc
import wave_loss_fr_np as wf
from wave_loss_cases import MARGIN  # noqa: F401  (4: the project's)

MR_STFT_8K = ((256, 64, "hanning"), (128, 32, "hanning"), (64, 16, "hanning"))
# the default set | W no multiple of S, S no multiple of 8, two window names | four resolutions, every window name the issue lists |
# one resolution
SETS = {"8k": MR_STFT_8K,
        "odd": ((100, 30, "bartlett"), (64, 16, "hamming")),
        "four": ((160, 80, "hamming"), (256, 64, "hanning"), (100, 30, "bartlett"), (64, 16, "hamming")),
        "one": ((64, 16, "hamming"),)}
IDS = sorted(SETS)
BATCH = 4
WEIGHT = 0.75
# 1500: 72 and 90 frames at (64, 16), past the 64-frame block | 576 = 256 + 5 * 64: hi exactly at a frame's end | 575: one sample
# short of it | 256: J = 1 at the widest | 200: J = 0 at the widest resolution only | 0 | 700 against a silent reference | 63: J = 0
# at every resolution (an invalid term)
LENGTHS = (1500, 576, 575, 256, 200, 0, 700, 63)
SILENT = 6
WIDTH = max(LENGTHS)
EST_STRIDE, REF_STRIDE = WIDTH + 37, WIDTH + 74     # rows of wider buffers: odd strides, no 16-byte alignment
# The signals' scale.  1 / |Y|^2 at a row's smallest magnitude conditions the log-magnitude part's gradient, and among ten thousand
# Rayleigh magnitudes the smallest is an outlier: at full scale one bin carries a row's whole float32 error, the yardsticks become
# single draws, and four times one draw bounds no other.  At this scale the magnitudes are some 1e-3 and half a percent of them sit
# at the floor sqrt(eps) = 1e-4 the definition gives them: the worst conditioning is met by many bins of every row, in every chain.
QUIET = 1e-4


@functools.lru_cache(maxsize=None)
def signals():
    """(est, ref) [N, WIDTH] float32: a coloured reference, the estimate 0.8 of it plus noise at a third of its rms; QUIET."""
    rng = np.random.default_rng(4242)
    n = len(LENGTHS)
    ref = rng.standard_normal((n, WIDTH + 8))
    ref = (QUIET * (ref[:, 8:] + 0.9 * ref[:, 7:-1] + 0.5 * ref[:, 4:-4])).astype(np.float32)
    est = (0.8 * ref + 0.33 * np.sqrt(np.mean(ref * ref)) * rng.standard_normal(ref.shape)).astype(np.float32)
    ref[SILENT] = 0
    for a in (est, ref):
        a.setflags(write=False)
    return est, ref


def term_bars(y, c, lo, hi, resolutions, detail):
    """(bar on the term, [(bar on sc, bar on lsd)] per resolution) from the yardsticks' magnitude errors (the module's text).
    y: the signal, or {mode: the signal as that mode has it} (a rebuild)."""
    of = (lambda x, mode: x[mode]) if isinstance(y, dict) else (lambda x, mode: x)
    bars = []
    for (W, S, name), (sc, lsd, J) in zip(resolutions, detail):
        if J == 0:
            bars.append((0.0, 0.0))
            continue
        E, rho = [], []
        for x, pick in ((c, lambda x, mode: x), (y, of)):
            m = mr.magnitudes(pick(x, "f64"), lo, hi, W, S, name)
            e = np.maximum(*(np.abs(mr.magnitudes(pick(x, mode), lo, hi, W, S, name, mode) - m) for mode in mr.MODES[1:]))
            E.append(MARGIN * float(np.sqrt(np.sum(e * e))))
            rho.append(MARGIN * float(np.sqrt(np.sum((e / m) ** 2))))
        cm = mr.magnitudes(c, lo, hi, W, S, name)
        rA, rB = sc * float(np.sqrt(np.sum(cm * cm))), float(np.sqrt(np.sum(cm * cm)))
        assert E[0] < 0.5 * rB
        b_sc = (rA + E[0] + E[1]) / (rB - E[0]) - sc
        nd = float(np.sqrt(lsd * mr.BINS * J))
        b_lsd = ((nd + rho[0] + rho[1]) ** 2 - nd ** 2) / (mr.BINS * J)
        bars.append((b_sc, b_lsd))
    return sum(a + b for a, b in bars) / len(resolutions), bars


@functools.lru_cache(maxsize=None)
def reference(key):
    """Per row of the direct batch at SETS[key]: ((term, valid, detail), the float64 gradient [WIDTH] of WEIGHT / BATCH * term, the
    two yardstick errors, the gradient's bar, (bar on the term, per-resolution bars))."""
    est, ref = signals()
    out = []
    for i, l in enumerate(LENGTHS):
        res = {m: mr.mr_stft(est[i], ref[i], 0, l, SETS[key], WEIGHT / BATCH, m) for m in mr.MODES}
        terms, g = res["f64"]
        g.setflags(write=False)
        scale = float(np.abs(g).max())
        yard = tuple(float(np.abs(res[m][1] - g).max()) / scale for m in mr.MODES[1:]) if scale else (0.0, 0.0)
        out.append((terms, g, yard, MARGIN * max(yard), term_bars(est[i], ref[i], 0, l, SETS[key], terms[2])))
    return out


# ---- the wave objective with the term: one ragged batch at 160 / 80 / hamming, T = 67 ------------------------------------------------
FRAMING = (160, 80, "hamming")
# 67: past the 64-frame block | 64 | 9 | 3: R is 160 samples under skip_edges, J = 1 at W = 160 and J = 0 at the widest | 2 | 1: an
# empty range under skip_edges | no samples | a silent clean row
FRAMES = (67, 64, 9, 3, 2, 1, 0, 5)
WAVE_SILENT = 7
WAVE_SETS = {"two": ((160, 80, "hamming"), (64, 16, "hamming")), "8k": MR_STFT_8K}
WAVE_WEIGHTS = ((0.0, 0.0, 1.0), (0.5, 1.0, 0.5))       # (wave_sse, si_sdr, mr_stft): the term alone, all three
WAVE_CASES = tuple((k, w, s) for k in sorted(WAVE_SETS) for w in WAVE_WEIGHTS for s in (True, False))


class WaveBatch(object):
    def __init__(self):
        W, S, name = FRAMING
        self.framing = FRAMING
        self._refs = {}
        self.frames = FRAMES
        self.lengths = tuple(fc.length_of(F, W, S) for F in FRAMES)
        assert tuple(wf.num_frames(v, W, S) for v in self.lengths) == FRAMES
        self.N, self.T = len(FRAMES), max(FRAMES)
        self.clean_width = max(self.lengths)
        self.clean_stride = (self.clean_width + 74) | 1
        rng = np.random.default_rng(777)
        X = rng.standard_normal((self.N, self.T, 129)) + 1j * rng.standard_normal((self.N, self.T, 129))
        self.mag = (30 * QUIET * (np.abs(X) + 0.01)).astype(np.float32)          # (|Y| of the rebuild: some 1e-3, as the direct batch's)
        self.ph = np.exp(1j * np.angle(X)).astype(np.complex64)
        self.clean = np.zeros((self.N, self.clean_width), np.float32)
        for i, (l, F) in enumerate(zip(self.lengths, FRAMES)):
            if l and i != WAVE_SILENT:
                y = self.rebuilt(i, "f64")[:l]
                self.clean[i, :l] = 0.7 * y + 0.5 * np.sqrt(np.mean(y * y)) * rng.standard_normal(l)
        for a in (self.mag, self.ph, self.clean):
            a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def rebuilt(self, row, mode):
        y = wf.rebuild(self.mag[row], self.ph[row], FRAMES[row], *FRAMING, mode=mode)
        y.setflags(write=False)
        return y

    def stand_in(self):
        """The rebuilt rows every chain starts from where there is no device: the float64 rebuild rounded to float32."""
        return [self.rebuilt(i, "f64").astype(np.float32) for i in range(self.N)]

    def reference(self, key, weights, skip_edges, ys=None):
        """Per row: ((wave_sse, si_sdr, valid, mr_stft, mr_valid), the float64 gradient [T, 129], the two yardstick errors, the bar,
        (bar on the term, per-resolution bars)).  ys: the rebuilt rows, float32, that EVERY chain starts from -- the device's own
        (rced_istft_ola_fr) in the GPU test, stand_in() without one.  The rebuild has bars of its own (test_framing_gpu.py); its
        float32 chains differ from each other by a slow drift that the term's gradient and the transposed de-emphasis scan carry to
        the lowest bins, several yardsticks apart from chain to chain, and a bar made of that would be a bar on the draw."""
        cached = ys is None
        if cached and (key, weights, skip_edges) in self._refs:
            return self._refs[(key, weights, skip_edges)]
        ys = self.stand_in() if ys is None else ys
        out = []
        a = tuple(w / BATCH for w in weights)
        for i in range(self.N):
            F, l = FRAMES[i], self.lengths[i]
            y32 = np.asarray(ys[i], np.float32)
            res = {m: mr.wave_loss_mr(self.mag[i], self.ph[i], self.clean[i], l, F, a[0], a[1], a[2], skip_edges, *FRAMING,
                                      resolutions=WAVE_SETS[key], mode=m, y=y32.astype(np.float64) if m == "f64" else y32) for m in mr.MODES}
            terms, g, detail = res["f64"]
            g.setflags(write=False)
            scale = float(np.abs(g).max())
            yard = tuple(float(np.abs(res[m][1] - g).max()) / scale for m in mr.MODES[1:]) if scale else (0.0, 0.0)
            lo, hi = wf.scored_range(l, F, skip_edges, *FRAMING[:2])
            bars = term_bars(y32[:wf.n_out(F, *FRAMING[:2])], self.clean[i], lo, hi, WAVE_SETS[key], detail)
            out.append((terms, g, yard, MARGIN * max(yard), bars))
        if cached:
            self._refs[(key, weights, skip_edges)] = out
        return out


@functools.lru_cache(maxsize=None)
def wave_batch():
    return WaveBatch()
