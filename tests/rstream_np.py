"""The resampler lanes of DESIGN.md 3.4g in float64 numpy: the state a lane keeps on the device (units pushed, the last `hist`
source frames as float64), the same push / finish shape, every output as the tap-by-tap sum of the phase table that
tests/resample_np.py defines.  Also the delay by brute force over the table, and a driver that takes ragged signals through
the lanes of this restatement or of the library's audio.StreamingResampler alike."""

import numpy as np

import resample_np as R


def reaches(p, q, left, width, m):
    """First and last source frame that output m of the offline result reads."""
    n0 = (m * q) // p
    return n0 - left, n0 - left + width - 1


def brute_delay(p, q, left, width, unit_in, unit_out, pushes=40):
    """The smallest D for which every output a push emits reaches only frames already pushed, by trying D = 0, 1, .. against
    every push of one unit: the push that brings a lane to H units emits stream positions below H unit_out, that is outputs
    m <= H unit_out - 1 - D, and holds H unit_in frames."""
    def fits(D):
        for H in range(1, pushes + 1):
            for m in range(max(0, (H - 1) * unit_out - D), H * unit_out - D):
                if reaches(p, q, left, width, m)[1] > H * unit_in - 1:
                    return False
        return True
    D = 0
    while not fits(D):
        D += 1
    return D


class LanesNP(object):
    """audio.StreamingResampler's surface.  Per lane: H (units pushed) and hist [ceil(D q / p) + left] float64 frames."""

    def __init__(self, sr_in, sr_out, lanes, unit_in, unit_out, delay=None):
        self.sr_in, self.sr_out, self.lanes, self.unit_in, self.unit_out = sr_in, sr_out, lanes, unit_in, unit_out
        self.p, self.q, self.left, self.table = R.taps(sr_in, sr_out)
        self.width = self.table.shape[1]
        assert unit_in * self.p == unit_out * self.q
        self.delay = (self.width - 1 - self.left) * self.p // self.q if delay is None else delay
        self.hist_len = -((-self.delay * self.q) // self.p) + self.left
        self.H = [0] * lanes
        self.hist = [np.zeros(self.hist_len) for _ in range(lanes)]

    def _outputs(self, s, new, m_lo, m_hi, strict):
        """Outputs [m_lo, m_hi) of the offline result from the lane's history and the call's frames `new`; strict: a frame
        past them is an error (a push), not zero (a finish)."""
        F0 = self.H[s] * self.unit_in
        have = np.concatenate([self.hist[s], new])            # frames F0 - hist_len .. F0 + len(new)
        if m_hi <= m_lo:
            return np.zeros(0)
        n0, r = np.divmod(np.arange(m_lo, m_hi, dtype=np.int64) * self.q, self.p)
        at = n0 - self.left - (F0 - self.hist_len)            # the first frame of every output, as an index into `have`
        assert at.min() >= 0, "a push reaches behind the history"
        assert not strict or at.max() + self.width <= have.size, "a push reaches a frame not pushed yet"
        rows = np.lib.stride_tricks.sliding_window_view(np.concatenate([have, np.zeros(self.width)]), self.width)[at]
        return (rows * self.table[r]).sum(axis=1)

    def push(self, pcm, active=None):
        pcm = np.asarray(pcm)
        K = pcm.shape[1] // self.unit_in
        assert pcm.shape[:2] == (self.lanes, K * self.unit_in) and K >= 1
        out = np.zeros((self.lanes, K * self.unit_out))
        for s in range(self.lanes):
            if active is not None and not active[s]:
                continue
            new = R.to_mono(pcm[s])
            first = self.H[s] * self.unit_out - self.delay
            m_lo, m_hi = max(0, first), max(0, first + K * self.unit_out)
            out[s, m_lo - first:m_hi - first] = self._outputs(s, new, m_lo, m_hi, True)
            self.hist[s] = np.concatenate([self.hist[s], new])[new.size:]
            self.H[s] += K
        return out

    def finish(self, lanes, tails):
        out = []
        for s, tail in zip(lanes, tails):
            new = R.to_mono(np.asarray(tail))
            assert new.size < self.unit_in
            M = R.length(self.H[s] * self.unit_in + new.size, self.sr_in, self.sr_out)
            out.append(self._outputs(s, new, max(0, self.H[s] * self.unit_out - self.delay), M, False))
            self.reset(s)
        return out

    def reset(self, lane=-1):
        for s in (range(self.lanes) if lane < 0 else [lane]):
            self.H[s], self.hist[s] = 0, np.zeros(self.hist_len)


def run_lanes(stream, jobs, unit_counts):
    """jobs[lane]: the signals ([frames] or [frames, channels]) that lane takes one after the other.  Every push carries
    unit_counts[i] units (cycled), or as many as the lane with the most left still has; a lane with fewer whole units left sits
    the push out (idle), a lane with less than a unit left is finished with the others like it and goes on to its next signal.
    Returns per lane the list of (concatenated output of the signal, units pushed)."""
    n, unit = stream.lanes, stream.unit_in
    which, at = [0] * n, [0] * n
    pieces = [[] for _ in range(n)]
    done = [[] for _ in range(n)]
    tail_shape = jobs[0][0].shape[1:]
    dtype = jobs[0][0].dtype
    i = 0
    while True:
        ending = [s for s in range(n) if which[s] < len(jobs[s]) and len(jobs[s][which[s]]) - at[s] < unit]
        if ending:
            for s, rest in zip(ending, stream.finish(ending, [jobs[s][which[s]][at[s]:] for s in ending])):
                done[s].append((np.concatenate(pieces[s] + [np.asarray(rest)]), at[s] // unit))
                pieces[s], at[s], which[s] = [], 0, which[s] + 1
            continue
        left = [(len(jobs[s][which[s]]) - at[s]) // unit if which[s] < len(jobs[s]) else 0 for s in range(n)]
        if not any(left):
            return done
        k = min(unit_counts[i % len(unit_counts)], max(left))
        active = [int(v >= k) for v in left]
        pcm = np.full((n, k * unit) + tail_shape, 77, dtype)              # an idle lane's row is not read
        for s in range(n):
            if active[s]:
                pcm[s] = jobs[s][which[s]][at[s]:at[s] + k * unit]
        out = np.asarray(stream.push(pcm, active))
        for s in range(n):
            if active[s]:
                pieces[s].append(out[s])
                at[s] += k * unit
            else:
                assert not out[s].any()                                  # an idle lane's row is zeros
        i += 1


def delayed(y, delay, units, unit_out):
    """What a lane hands out for a signal whose offline result is y: the zeros its pushes returned first, then y."""
    return np.concatenate([np.zeros(min(delay, units * unit_out), y.dtype), y])
