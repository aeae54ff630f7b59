"""Float64 restatement of the streaming denoiser's contract (include/rced.h "streaming"), built from the
oracle's own pieces (oracle/audio_np.py, oracle/rced_c.py): the same push / finish shape as the library, the same state per
lane, one frame and one hop at a time.  Test infrastructure, not product code: tests/test_stream_host.py pins it to the
whole-utterance oracle chain, tests/test_stream_gpu.py compares the device with both.

State of a lane, as the library keeps it: the hops pushed (H), the last input sample, the previous hop pre-emphasised, the
7 newest magnitude frames with their phases, the pending output hop (its last sample is the de-emphasis carry).
Frame t = hops t, t + 1, complete after hop t + 1; its mask needs frames t - 3 .. t + 4, so hop t + 5; frame t rebuilds
hop t + 1 and frame 0 also hop 0: output position p of a push to a lane at H hops is hop H - 5 + p of the result."""

import numpy as np

from oracle import audio_np, rced_c

STEP, FRAME, BINS = audio_np.STEP, audio_np.FRAME, audio_np.BINS
KEEP, DELAY_HOPS, FINISH_SLOTS = 7, 5, 6
DELAY = DELAY_HOPS * STEP


class _Lane(object):
    def __init__(self):
        self.hops = 0
        self.sample = np.float32(0)
        self.prev = np.zeros(STEP)                         # the previous hop, pre-emphasised
        self.mag = np.zeros((KEEP, BINS))
        self.phase = np.ones((KEEP, BINS), np.complex128)
        self.pend = np.zeros(STEP)


def _frame_spectrum(samples):
    """One frame as audio_np.stft treats it: hamming, rfft(256), magnitude and unit phase."""
    spec = np.fft.rfft(samples * np.hamming(FRAME), audio_np.NFFT)
    return np.abs(spec), np.exp(1j * np.angle(spec))


class StreamNP(object):
    def __init__(self, net_work, weights, lanes, max_hops=8, nfft=512):
        self.net_work, self.weights, self.max_hops, self.nfft = net_work, weights, int(max_hops), int(nfft)
        self.lanes = int(lanes)
        self.lane = [_Lane() for _ in range(self.lanes)]

    def reset(self, lane=-1):
        for i in (range(len(self.lane)) if lane < 0 else [lane]):
            self.lane[i] = _Lane()

    def _pre_emphasis(self, st, x):
        """float32, one multiply and one subtract per sample (audio_np.stft); only the lane's very first sample is e = s."""
        x = np.asarray(x, np.float32)
        if not x.size:
            return np.zeros(0)
        before = np.concatenate([[st.sample], x[:-1]]).astype(np.float32)
        e = x - np.float32(audio_np.PRE_EMPHASIS) * before
        if st.hops == 0:
            e[0] = x[0]
        return e.astype(np.float64)

    def _run(self, st, frames, live, k):
        """frames [k, 256] pre-emphasised (live[h]: the frame exists) -> the k + 1 hops in time order: the pending one, then
        those of frames H - 5 .. H + k - 6 (the head of frame 0 in the place of hop 0), and the new state's window."""
        mag = np.zeros((KEEP + k, BINS))
        phase = np.ones((KEEP + k, BINS), np.complex128)
        mag[:KEEP], phase[:KEEP] = st.mag, st.phase
        for h in range(k):
            if live[h]:
                mag[KEEP + h], phase[KEEP + h] = _frame_spectrum(frames[h])
        masks = rced_c.forward(self.net_work, self.weights, mag[None, :, :, None].astype(np.float32), np.float64)[0, :, :, 0]
        hops = [st.pend.copy()]
        carry = st.pend[-1]
        for p in range(k):
            t = st.hops - DELAY_HOPS + p                       # the frame in window row p + 3
            if t < 0:
                hops.append(np.zeros(STEP))
                continue
            x = np.fft.irfft(masks[p + 3] * phase[p + 3], self.nfft)[:FRAME] / np.hamming(FRAME)
            if t == 0:                                         # de-emphasis starts here: y[0] = x[0]
                hops[p] = self._de_emphasis(x[:STEP], 0.0)
                carry = hops[p][-1]
            hops.append(self._de_emphasis(x[STEP:], carry))
            carry = hops[-1][-1]
        return hops, mag[k:], phase[k:]

    @staticmethod
    def _de_emphasis(x, carry):
        out = np.empty(len(x))
        for i, v in enumerate(x):
            carry = v + audio_np.PRE_EMPHASIS * carry
            out[i] = carry
        return out

    def push(self, pcm, active=None):
        """pcm [lanes, K*128] -> [lanes, K*128] float64."""
        pcm = np.asarray(pcm, np.float32)
        k = pcm.shape[1] // STEP
        assert pcm.shape == (len(self.lane), k * STEP) and 1 <= k <= self.max_hops
        out = np.zeros(pcm.shape)
        for s, st in enumerate(self.lane):
            if active is not None and not active[s]:
                continue
            e = np.concatenate([st.prev, self._pre_emphasis(st, pcm[s])])
            frames = [e[h * STEP:h * STEP + FRAME] for h in range(k)]
            live = [st.hops + h >= 1 for h in range(k)]        # hop 0 alone completes no frame
            hops, mag, phase = self._run(st, frames, live, k)
            out[s] = np.concatenate(hops[:k])
            st.mag, st.phase, st.pend, st.prev = mag, phase, hops[k], e[-STEP:]
            st.sample = pcm[s, -1]
            st.hops += k
        return out

    def finish(self, lanes, tails):
        """The owed samples of every lane listed (tails: fewer than 128 samples each); those lanes start over."""
        out = []
        for s, tail in zip(lanes, tails):
            st = self.lane[s]
            tail = np.asarray(tail, np.float32).reshape(-1)
            r, H = tail.size, st.hops
            assert r < STEP
            e = np.zeros(STEP)                                  # zero padding AFTER pre-emphasis
            e[:r] = self._pre_emphasis(st, tail)
            frames = [np.concatenate([st.prev, e]), np.concatenate([e, np.zeros(STEP)])] + [np.zeros(FRAME)] * 4
            # the reference's frame set (audio_feature.py:70): frame H - 1 from the tail exists if the tail is not empty or it
            # is frame 0; the frame that starts inside the tail only as frame 0 or 1 (L < 256)
            live = [H >= 1 and (r > 0 or H == 1), H <= 1 and r > 0] + [False] * 4
            hops, _, _ = self._run(st, frames, live, FINISH_SLOTS)
            seq = np.concatenate(hops)[STEP * max(0, DELAY_HOPS - H):]
            out.append(seq[:STEP * H + r - max(0, STEP * H - DELAY)].copy())
            self.lane[s] = _Lane()
        return out


def run_signal(stream, lane, sig, hop_counts):
    """Push `sig` through one lane in pushes of hop_counts[0], hop_counts[1], ... hops (cycled; the other lanes idle), then
    finish: the concatenated output and the number of whole hops pushed."""
    sig = np.asarray(sig, np.float32)
    n_lanes = stream.lanes
    active = [int(i == lane) for i in range(n_lanes)]
    pieces, at, i = [], 0, 0
    while len(sig) - at >= STEP:
        k = min(hop_counts[i % len(hop_counts)], (len(sig) - at) // STEP)
        pcm = np.zeros((n_lanes, k * STEP), np.float32)
        pcm[lane] = sig[at:at + k * STEP]
        pieces.append(np.asarray(stream.push(pcm, active))[lane])
        at += k * STEP
        i += 1
    pieces.append(stream.finish([lane], [sig[at:]])[0])
    return np.concatenate(pieces), at // STEP


def run_lanes(stream, jobs, hop_counts):
    """jobs[lane]: the signals that lane takes one after the other.  Every push carries hop_counts[i] hops (cycled), or as
    many as the lane with the most left still has; a lane with fewer whole hops left sits the push out (idle), a lane with
    less than a hop left is finished with the others like it and goes on to its next signal.  Returns per lane the list of
    (concatenated output of the signal, hops pushed); works on StreamNP and on the library's StreamingDenoiser alike."""
    n = stream.lanes
    jobs = [[np.asarray(s, np.float32) for s in lane] for lane in jobs]
    which, at = [0] * n, [0] * n
    pieces = [[] for _ in range(n)]
    done = [[] for _ in range(n)]
    i = 0
    while True:
        ending = [s for s in range(n) if which[s] < len(jobs[s]) and len(jobs[s][which[s]]) - at[s] < STEP]
        if ending:
            for s, rest in zip(ending, stream.finish(ending, [jobs[s][which[s]][at[s]:] for s in ending])):
                done[s].append((np.concatenate(pieces[s] + [np.asarray(rest)]), at[s] // STEP))
                pieces[s], at[s], which[s] = [], 0, which[s] + 1
            continue
        left = [(len(jobs[s][which[s]]) - at[s]) // STEP if which[s] < len(jobs[s]) else 0 for s in range(n)]
        if not any(left):
            return done
        k = min(hop_counts[i % len(hop_counts)], max(left))
        active = [int(v >= k) for v in left]
        pcm = np.zeros((n, k * STEP), np.float32)
        for s in range(n):
            if active[s]:
                pcm[s] = jobs[s][which[s]][at[s]:at[s] + k * STEP]
        out = np.asarray(stream.push(pcm, active))
        for s in range(n):
            if active[s]:
                pieces[s].append(out[s])
                at[s] += k * STEP
            else:
                assert not out[s].any()                         # an idle lane's row is zeros
        i += 1
