"""The free-running resampler lanes of DESIGN.md 3.4h in float64 numpy: how many outputs a lane has emitted after F frames (the
closed form and by brute force over the phase table), the history it needs by brute force, the host's mirror of a ring, the
prefill Z of audio.BlockDenoiser by brute force over the calls, the lane itself with audio.FreeResampler's surface -- every output
as the tap-by-tap sum of the phase table that tests/resample_np.py defines --, and a driver that takes ragged signals in ragged
pushes and takes through the lanes of this restatement or of the library alike."""

import numpy as np

import resample_np as R


def emitted(p, q, left, width, F):
    """A(F) = ceil((F - right) p / q) for F > right, else 0."""
    right = width - 1 - left
    return -((-(F - right) * p) // q) if F > right else 0


def brute_emitted(p, q, left, width, F):
    """Outputs whose last tap, frame floor(m q / p) + right, is among the first F frames: counted one by one."""
    right = width - 1 - left
    m = 0
    while (m * q) // p + right <= F - 1:
        m += 1
    return m


def brute_history(p, q, left, width, frames):
    """The most frames before F that an output not yet emitted at F reads, over F = 0 .. frames: the first such output is
    A(F) (counted), and it reads from floor(m q / p) - left on."""
    right = width - 1 - left
    worst, m = 0, 0
    for F in range(frames + 1):
        while (m * q) // p + right <= F - 1:
            m += 1
        worst = max(worst, F - ((m * q) // p - left))
    return worst


def geometry(sr_in, sr_out):
    p, q, left, table = R.taps(sr_in, sr_out)
    return p, q, left, table.shape[1]


def available(sr_in, sr_out, F):
    return emitted(*geometry(sr_in, sr_out), F)


def brute_prefill(block, sr_in, sr_out, calls):
    """(Z, the set of hops per call) of a BlockDenoiser by walking `calls` calls with counters that move one output at a time: the
    down lane's outputs after j blocks, the whole hops H among them, the up lane's outputs after 128 H frames; Z is the most that
    j * block_out ever exceeds those by."""
    pd, qd, ld, wd = geometry(sr_in, 8000)
    pu, qu, lu, wu = geometry(8000, sr_out)
    rd, ru = wd - 1 - ld, wu - 1 - lu
    block_out = block * sr_out // sr_in
    assert block_out * sr_in == block * sr_out
    z, hops, md, mu, h_prev = 0, set(), 0, 0, 0
    for j in range(1, calls + 1):
        while (md * qd) // pd + rd <= j * block - 1:
            md += 1
        h = md // 128
        while (mu * qu) // pu + ru <= 128 * h - 1:
            mu += 1
        hops.add(h - h_prev)
        h_prev = h
        z = max(z, j * block_out - mu)
    return z, hops


class LanesNP(object):
    """audio.FreeResampler's surface.  Per lane: the frames given, the last width - 1 of them as float64, the ring (a list)."""

    def __init__(self, sr_in, sr_out, lanes, max_frames=4096, max_take=None, prefill=0):
        self.sr_in, self.sr_out, self.lanes, self.prefill = sr_in, sr_out, lanes, prefill
        self.p, self.q, self.left, self.table = R.taps(sr_in, sr_out)
        self.width = self.table.shape[1]
        self.max_frames = max_frames
        self.max_take = -((-max_frames * sr_out) // sr_in) if max_take is None else max_take
        self.capacity = prefill + -((-max_frames * self.p) // self.q) + self.max_take
        self.taken = [0] * lanes
        self.F, self.hist, self.ring = [0] * lanes, [None] * lanes, [None] * lanes
        self.reset()

    def reset(self, lane=-1):
        for s in (range(self.lanes) if lane < 0 else [lane]):
            self.F[s], self.hist[s], self.ring[s] = 0, np.zeros(self.width - 1), np.zeros(self.prefill)

    @property
    def in_ring(self):
        return [len(r) for r in self.ring]

    def _outputs(self, s, new, m_lo, m_hi, strict):
        """Outputs [m_lo, m_hi) from the lane's history and the call's frames `new`; strict: a frame past them is an error (a
        push), not zero (a finish)."""
        if m_hi <= m_lo:
            return np.zeros(0)
        have = np.concatenate([self.hist[s], new])             # frames F - (width - 1) .. F + len(new)
        n0, r = np.divmod(np.arange(m_lo, m_hi, dtype=np.int64) * self.q, self.p)
        at = n0 - self.left - (self.F[s] - (self.width - 1))
        assert at.min() >= 0, "a push reaches behind the history"
        assert not strict or at.max() + self.width <= have.size, "a push reaches a frame not pushed yet"
        rows = np.lib.stride_tricks.sliding_window_view(np.concatenate([have, np.zeros(self.width)]), self.width)[at]
        return (rows * self.table[r]).sum(axis=1)

    def push(self, pcm, counts=None, take=None):
        n = 0 if pcm is None else np.asarray(pcm).shape[1]
        counts = [n] * self.lanes if counts is None else list(counts)
        for s in range(self.lanes):
            if counts[s] < 0:
                continue
            new = R.to_mono(np.asarray(pcm)[s][:counts[s]]) if counts[s] else np.zeros(0)
            a0 = emitted(self.p, self.q, self.left, self.width, self.F[s])
            a1 = emitted(self.p, self.q, self.left, self.width, self.F[s] + new.size)
            self.ring[s] = np.concatenate([self.ring[s], self._outputs(s, new, a0, a1, True)])
            assert len(self.ring[s]) <= self.capacity, "the ring overruns"
            self.hist[s] = np.concatenate([self.hist[s], new])[new.size:]
            self.F[s] += new.size
        if take is None:
            take = [min(len(self.ring[s]), self.max_take) if counts[s] >= 0 else 0 for s in range(self.lanes)]
        elif isinstance(take, int):
            take = [take] * self.lanes
        out = np.zeros((self.lanes, max(take)))
        for s in range(self.lanes):
            assert 0 <= take[s] <= len(self.ring[s]) and (counts[s] >= 0 or not take[s])
            out[s, :take[s]] = self.ring[s][:take[s]]
            self.ring[s] = self.ring[s][take[s]:]
        self.taken = list(take)
        return out

    def finish(self, lanes, tails):
        out, self.owed = [], []
        for s, tail in zip(lanes, tails):
            new = R.to_mono(np.asarray(tail))
            a0 = emitted(self.p, self.q, self.left, self.width, self.F[s])
            M = R.length(self.F[s] + new.size, self.sr_in, self.sr_out)
            out.append(np.concatenate([self.ring[s], self._outputs(s, new, a0, M, False)]))
            self.owed.append(len(out[-1]))
            self.reset(s)
        return out


def run_free(stream, jobs, seed, choices=(0, 1, 7, 441, 480, 1023), idle=0.15):
    """jobs[lane]: the signals ([frames] or [frames, channels]) that lane takes one after the other.  Every push gives every lane
    a number of frames drawn from `choices` (or leaves it idle) and takes from it a number drawn between what must leave its ring
    for the next push to fit and what the mirror says is there; a lane whose draw reaches its signal's end is finished with the
    rest as its tail, with the others like it, and goes on to its next signal.  The mirror is this file's: prefill + A(frames) -
    taken, asserted against the stream's own `.in_ring` at every step and against the counts `finish` reports.
    Returns per lane the list of outputs, one per signal: everything taken, then what finish handed out."""
    rng = np.random.RandomState(seed)
    n = stream.lanes
    geo = geometry(stream.sr_in, stream.sr_out)
    which, at, frames, taken = [0] * n, [0] * n, [0] * n, [0] * n
    pieces = [[] for _ in range(n)]
    done = [[] for _ in range(n)]
    tail_shape = jobs[0][0].shape[1:]
    dtype = jobs[0][0].dtype
    room = stream.capacity - -((-stream.max_frames * geo[0]) // geo[1])      # what may stay in a ring before a push of any size
    while any(which[s] < len(jobs[s]) for s in range(n)):
        draw = [int(rng.choice(choices)) if which[s] < len(jobs[s]) and rng.uniform() >= idle else -1 for s in range(n)]
        ending = [s for s in range(n) if draw[s] >= 0 and draw[s] >= len(jobs[s][which[s]]) - at[s]]
        if ending:
            rest = stream.finish(ending, [jobs[s][which[s]][at[s]:] for s in ending])
            for i, s in enumerate(ending):
                total = len(jobs[s][which[s]])
                assert stream.owed[i] == len(rest[i]) == stream.prefill + R.length(total, stream.sr_in, stream.sr_out) - taken[s]
                done[s].append(np.concatenate(pieces[s] + [np.asarray(rest[i])]))
                pieces[s], at[s], frames[s], taken[s], which[s] = [], 0, 0, 0, which[s] + 1
            continue
        cols = max(draw + [0])
        pcm = np.full((n, cols) + tail_shape, 77, dtype)                      # what lies past a lane's count is not read
        take = [0] * n
        for s in range(n):
            if draw[s] < 0:
                continue
            pcm[s, :draw[s]] = jobs[s][which[s]][at[s]:at[s] + draw[s]]
            there = stream.prefill + emitted(*geo, frames[s] + draw[s]) - taken[s]
            take[s] = int(rng.randint(max(0, there - room), min(there, stream.max_take) + 1))
        out = stream.push(pcm if cols else None, draw, take)
        out = out.cpu().numpy() if hasattr(out, "is_cuda") else np.asarray(out)
        assert out.shape == (n, max(take))
        for s in range(n):
            if draw[s] >= 0:
                pieces[s].append(out[s, :take[s]])
                at[s] += draw[s]
                frames[s] += draw[s]
                taken[s] += take[s]
            assert not out[s, take[s]:].any()                                 # zeros behind what was taken, and for an idle lane
        assert stream.in_ring == [stream.prefill + emitted(*geo, frames[s]) - taken[s] for s in range(n)]
    return done
