"""Float64 restatement of a denoiser lane at a framing (include/rced.h "streaming at a framing"), built on
tests/framing_np.py and oracle/rced_c.py: the same push / finish shape as the library and the same state per lane.  Test
infrastructure, not product code: tests/test_stream_fr_host.py pins it to the whole-utterance chain of framing_np,
tests/test_stream_fr_gpu.py compares the device with both.

Hop = S samples, R = ceil(W / S), D = (R + 3) S.  State of a lane, as the library keeps it: the hops pushed (H), the last input
sample, the last (R - 1) S samples pre-emphasised (W - S where S divides W: frame H - R + 1 starts that far back), the 7 newest
magnitude frames with their phases, the numerator addends pending for the next W - S output samples (summed in ascending frame
order; the reference rebuild has one addend a sample), the de-emphasis carry.  All zero is the start of an utterance.
A push of K hops completes frames H - R + 1 .. H + K - R (rows 7 .. 6 + K of the window), the net gives the masks of frames
H - R - 3 .. H + K - R - 4 (rows 3 .. K + 2), and output position p of the push is hop H - R - 3 + p.  A finish is a push of
R + 4 hops made of the tail and zeros, with the utterance's frame count T: frames at or past T are zero rows going in and are
not rebuilt."""

import numpy as np

import framing_np as fnp
from oracle import rced_c

KEEP, FUTURE, MAX_OVERLAP = 7, 4, 8
BINS = fnp.BINS


def overlap(W, S):
    return -(-W // S)


def delay(W, S):
    return (overlap(W, S) + 3) * S


def finish_slots(W, S):
    return overlap(W, S) + FUTURE


def num_frames(L, W, S):
    return fnp.num_frames(L, W, S) if L > 0 else 0


def owed(H, r, W, S):
    return H * S + r - max(0, H * S - delay(W, S))


def brute_delay(W, S, hops=12):
    """D by search over the frame dependencies.  A hop can leave once every frame that covers one of its samples (the reference
    rebuild reads a subset of them, and always the newest) is complete, its last sample pushed, together with the 4 frames
    after it.  d: the smallest number such that hop h can leave with the push that brings its lane to h + d hops; that push's
    newest input hop is h + d - 1, so the output runs d - 1 hops behind the input."""
    def ready(h, pushed):
        for i in range(h * S, (h + 1) * S):
            for t in range(0, i // S + 1):
                if t * S <= i < t * S + W and (t + FUTURE) * S + W > pushed * S:
                    return False
        return True
    d = 1
    while not all(ready(h, h + d) for h in range(hops)):
        d += 1
    return (d - 1) * S


class _Lane(object):
    def __init__(self, W, S):
        self.hops = 0
        self.sample = np.float32(0)
        self.tail = np.zeros((overlap(W, S) - 1) * S)
        self.mag = np.zeros((KEEP, BINS))
        self.phase = np.ones((KEEP, BINS), np.complex128)
        self.pend = np.zeros(W - S)
        self.carry = 0.0


class StreamFrNP(object):
    def __init__(self, net_work, weights, lanes, W, S, name, rebuild="ola", nfft=512, max_hops=8):
        assert rebuild in ("ola", "reference") and overlap(W, S) <= MAX_OVERLAP
        self.net_work, self.weights, self.lanes, self.max_hops = net_work, weights, int(lanes), int(max_hops)
        self.W, self.S, self.name, self.rebuild, self.nfft = W, S, name, rebuild, int(nfft)
        self.R, self.hop, self.delay = overlap(W, S), S, delay(W, S)
        self.w = fnp.window(name, W)
        self.lane = [_Lane(W, S) for _ in range(self.lanes)]

    def reset(self, lane=-1):
        for i in (range(self.lanes) if lane < 0 else [lane]):
            self.lane[i] = _Lane(self.W, self.S)

    def _pre_emphasis(self, st, x):
        """float32, one multiply and one subtract per sample (framing_np.stft); only the lane's very first sample is e = s."""
        x = np.asarray(x, np.float32)
        if not x.size:
            return np.zeros(0)
        before = np.concatenate([[st.sample], x[:-1]]).astype(np.float32)
        e = x - np.float32(fnp.PRE) * before
        if st.hops == 0:
            e[0] = x[0]
        return e.astype(np.float64)

    def _run(self, st, fresh, k, T):
        """fresh: the k S new samples, pre-emphasised (zero-filled past the utterance's end) -> the k S output samples, and the
        lane's new tail, window, pending sum and carry.  T: the utterance's frame count, or None while it is not known."""
        W, S, R, H = self.W, self.S, self.R, st.hops
        ext = np.concatenate([st.tail, fresh, np.zeros(W)])    # frame H - R + 1 + h starts at ext[h S]
        mag = np.zeros((KEEP + k, BINS))
        phase = np.ones((KEEP + k, BINS), np.complex128)
        mag[:KEEP], phase[:KEEP] = st.mag, st.phase
        for h in range(k):
            t = H - R + 1 + h
            if t >= 0 and (T is None or t < T):
                spec = np.fft.rfft(ext[h * S:h * S + W] * self.w, fnp.NFFT)
                mag[KEEP + h], phase[KEEP + h] = np.abs(spec), np.exp(1j * np.angle(spec))
        masks = rced_c.forward(self.net_work, self.weights, mag[None, :, :, None].astype(np.float32), np.float64)[0, :, :, 0]
        hb = H - R - 3                                         # the frame in slot 0 = the hop at output position 0
        num = np.zeros(k * S + W - S)
        num[:W - S] = st.pend
        for p in range(k):                                     # ascending frame order, behind the pending sum
            t = hb + p
            if t < 0 or (T is not None and t >= T):
                continue
            if self.rebuild == "ola":
                num[p * S:p * S + W] += self.w * np.fft.irfft(masks[p + 3] * phase[p + 3], fnp.NFFT)[:W]
            else:
                x = np.fft.irfft(masks[p + 3] * phase[p + 3], self.nfft)[:W] / self.w
                num[p * S + W - S:p * S + W] += x[W - S:]
                if t == 0:
                    num[p * S:p * S + W - S] += x[:W - S]
        e = num[:k * S].copy()
        if self.rebuild == "ola":
            w2 = self.w * self.w
            for j in range(k * S):
                i = hb * S + j
                den = sum(w2[i - t * S] for t in range(max(0, -(-(i - W + 1) // S)), i // S + 1)
                          if i >= 0 and (T is None or t < T))
                e[j] = e[j] / den if den > fnp.DEN_FLOOR else 0.0
        out = np.empty(k * S)
        carry = st.carry
        for j in range(k * S):
            carry = e[j] + fnp.PRE * carry
            out[j] = carry
        tail = ext[k * S:k * S + len(st.tail)]
        return out, tail, mag[k:], phase[k:], num[k * S:], carry

    def push(self, pcm, active=None):
        """pcm [lanes, K S] -> [lanes, K S] float64."""
        pcm = np.asarray(pcm, np.float32)
        k = pcm.shape[1] // self.S
        assert pcm.shape == (self.lanes, k * self.S) and 1 <= k <= self.max_hops
        out = np.zeros(pcm.shape)
        for s, st in enumerate(self.lane):
            if active is not None and not active[s]:
                continue
            out[s], st.tail, st.mag, st.phase, st.pend, st.carry = self._run(st, self._pre_emphasis(st, pcm[s]), k, None)
            st.sample = pcm[s, -1]
            st.hops += k
        return out

    def finish(self, lanes, tails):
        """The owed samples of every lane listed (tails: fewer than S samples each); those lanes start over."""
        out = []
        W, S = self.W, self.S
        k = finish_slots(W, S)
        for s, tail in zip(lanes, tails):
            st = self.lane[s]
            tail = np.asarray(tail, np.float32).reshape(-1)
            r, H = tail.size, st.hops
            assert r < S
            fresh = np.zeros(k * S)                            # zero padding AFTER pre-emphasis
            fresh[:r] = self._pre_emphasis(st, tail)
            y = self._run(st, fresh, k, num_frames(H * S + r, W, S))[0]
            out.append(y[S * max(0, self.R + 3 - H):][:owed(H, r, W, S)].copy())
            self.lane[s] = _Lane(W, S)
        return out


def offline(net_work, weights, sig, W, S, name, rebuild="ola", nfft=512):
    """The whole-utterance float64 chain at a framing, cut to the signal's length."""
    sig = np.asarray(sig, np.float32)
    mag, phase = fnp.stft(sig, W, S, name)
    pred = rced_c.forward(net_work, weights, mag.astype(np.float32)[None, :, :, None], np.float64)[0, :, :, 0]
    if rebuild == "ola":
        return fnp.rebuild_ola(pred, phase, pred.shape[0], W, S, name)[:len(sig)]
    return fnp.rebuild_reference(pred, phase, W, S, nfft, name)[:len(sig)]


def run_lanes(stream, jobs, hop_counts):
    """tests/stream_np.run_lanes in hops of stream.hop: jobs[lane] holds the signals that lane takes one after the other; every
    push carries hop_counts[i] hops (cycled), or as many as the lane with the most left still has; a lane with fewer whole hops
    left sits the push out (idle), a lane with less than a hop left is finished with the others like it and goes on to its next
    signal.  Returns per lane the list of (concatenated output of the signal, hops pushed); works on StreamFrNP and on the
    library's StreamingDenoiser alike."""
    n, unit = stream.lanes, stream.hop
    jobs = [[np.asarray(s, np.float32) for s in lane] for lane in jobs]
    which, at = [0] * n, [0] * n
    pieces = [[] for _ in range(n)]
    done = [[] for _ in range(n)]
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
        k = min(hop_counts[i % len(hop_counts)], max(left))
        active = [int(v >= k) for v in left]
        pcm = np.zeros((n, k * unit), np.float32)
        for s in range(n):
            if active[s]:
                pcm[s] = jobs[s][which[s]][at[s]:at[s] + k * unit]
        out = np.asarray(stream.push(pcm, active))
        for s in range(n):
            if active[s]:
                pieces[s].append(out[s])
                at[s] += k * unit
            else:
                assert not out[s].any()                         # an idle lane's row is zeros
        i += 1


def drop_delay(out, hops, length, W, S):
    """The signal's output without the zeros the pushes returned first; those are exactly zero."""
    zeros = min(delay(W, S), S * hops)
    assert hops == length // S and len(out) == zeros + length, (len(out), hops, length)
    assert not out[:zeros].any()
    return out[zeros:]


def lengths(W, S):
    """The lengths every test of a framing runs at: around a hop, a window and the delay, a ragged long one, and a multiple of
    the hop above the window."""
    D = delay(W, S)
    return sorted(set([1, S - 1, S, S + 1, W - 1, W, W + 1, D, D + 1, 12 * S + W + 7, (W // S + 2) * S]) - {0})
