"""numpy float64 restatement of the ragged FIR (rced_convolve) and of the loader's reverberant batches (not a test module),
in the style of tests/loader_np.py.  The reference has no reverberation: the pin is this restatement, checked against a
literal double loop and scipy.signal.fftconvolve by tests/test_conv_host.py."""

import numpy as np

import eval_closed_form as cf
import loader_np

MAX_TAPS = 8192


def convolve_ref(x, h, d, length):
    """(np.convolve(x64, h64)[d : d + length], abs_bound): abs_bound is the same convolution over |x|, |h| -- the sum of the
    magnitudes of the terms of every output, what a rounding-error bound scales with.  No taps: zeros."""
    full, full_abs = convolve_full(x, h, length)
    assert length == 0 or full.size == 0 or 0 <= d < np.asarray(h).size
    return cut(full, d, length), cut(full_abs, d, length)


def convolve_full(x, h, length):
    """(np.convolve(x64[:length], h64), the same over |x|, |h|): every shift's answer is a cut of these.  Empty where there is
    nothing to convolve."""
    x, h = np.asarray(x, np.float64).reshape(-1), np.asarray(h, np.float64).reshape(-1)
    assert length <= x.size
    if length == 0 or h.size == 0:
        return np.zeros(0), np.zeros(0)
    x = x[:length]
    return np.convolve(x, h), np.convolve(np.abs(x), np.abs(h))


def cut(full, d, length):
    return full[d:d + length].copy() if full.size else np.zeros(length)


def convolve_loop(x, h, d, length):
    """The definition, literally: y[p] = sum_k h[k] x[p + d - k], k ascending, x = 0 outside [0, length)."""
    y = np.zeros(length)
    for p in range(length):
        for k in range(len(h)):
            q = p + d - k
            if 0 <= q < length:
                y[p] += np.float64(h[k]) * np.float64(x[q])
    return y


def bar(ref, abs_bound, taps):
    """|dev - ref| <= 2^-24 |ref| + K 2^-52 abs_bound: one fp32 rounding at the store, plus the worst case of an fp64
    accumulation of K terms in any order (K 2^-53 abs_bound to first order), doubled."""
    return 2.0 ** -24 * np.abs(ref) + taps * 2.0 ** -52 * abs_bound


# ---- the loader with rir= ------------------------------------------------------------------------------------------------

def plan_noise(ls, ln):
    """loader.plan_noise's draws, restated: (start, every gain drawn)."""
    if ls >= ln:
        return 0, [np.random.uniform(0, 2) for _ in range(int(np.ceil((ls - ln) / ln)))]
    return int(np.random.randint(0, ln - ls)), []


def plan(cid, nid, clean_lengths, noise_lengths, n_rir=None, rir_prob=1.0):
    """DataSet.plan restated.  Without rir (n_rir None) the parent's 4-tuple and draws; with it, uniform(0, 1) and
    randint(0, n_rir) first, always both, then add_noise's draws, and the response's id (None: the item stays dry) fifth.
    The gains are every draw made (the loader keeps those that can reach the speech, a prefix)."""
    if n_rir is None:
        return (cid, nid) + plan_noise(int(clean_lengths[cid]), int(noise_lengths[nid]))
    u = np.random.uniform(0, 1)
    rid = int(np.random.randint(0, n_rir))
    return (cid, nid) + plan_noise(int(clean_lengths[cid]), int(noise_lengths[nid])) + (rid if u < rir_prob else None,)


def early_taps(taps, direct, early_ms, sample_rate):
    return min(taps, direct + int(round(early_ms * sample_rate / 1000.0)) + 1)


def build_batch(clean, noise, rirs, directs, plan_rows, snr, target, early_ms=50.0, sample_rate=8000):
    """clean, noise: lists of int16 / float signals; rirs: float32 responses as the RirCorpus stores them, directs their
    direct-path indices; plan_rows: DataSet.plan's 5-tuples.  Returns (batch_mix, batch_clean [N, T, 129, 1], mixes, targets,
    target_bounds): the spectrograms, the float64 signals, and per row (ref, abs_bound, taps) of the target where it is a
    convolution (None where it is the gathered speech).  Every stage's result is rounded to float32 where the device stores it."""
    def signal(a):
        a = np.asarray(a)
        return a.astype(np.float64) / 32768.0 if a.dtype == np.int16 else a.astype(np.float64)

    def f32(a):
        return a.astype(np.float32).astype(np.float64)

    mix_mag, clean_mag, mixes, targets, bounds = [], [], [], [], []
    for cid, nid, start, gains, rid in plan_rows:
        dry = signal(clean[cid])
        ls = len(dry)
        h, d = (np.asarray(rirs[rid], np.float64), int(directs[rid])) if rid is not None else (np.ones(1), 0)
        wet, wet_abs = convolve_ref(dry, h, d, ls)
        bound = None
        if target == "dry":
            tgt = dry
        elif target == "reverberant":
            tgt, bound = f32(wet), (wet, wet_abs, len(h))
        else:
            ke = early_taps(len(h), d, early_ms, sample_rate)
            e, e_abs = convolve_ref(dry, h[:ke], d, ls)
            tgt, bound = f32(e), (e, e_abs, ke)
        nz = signal(noise[nid])
        mixed = cf.mix(f32(wet), nz[start:start + ls] if len(nz) > ls else nz, snr, 0, [] if len(nz) > ls else gains)
        mixed = f32(mixed)
        mixes.append(mixed)
        targets.append(tgt)
        bounds.append(bound)
        mix_mag.append(loader_np.magnitudes(mixed))
        clean_mag.append(loader_np.magnitudes(tgt))
    return loader_np.pad_batch(mix_mag), loader_np.pad_batch(clean_mag), mixes, targets, bounds
