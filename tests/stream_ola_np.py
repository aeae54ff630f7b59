"""Float64 restatement of the streaming denoiser's overlap-add form (include/rced.h "streaming", rebuild = RCED_STREAM_REBUILD_OLA;
DESIGN.md 3.4d), with the push / finish shape of stream_np.StreamNP, whose front end it keeps.  Test infrastructure, not product
code: tests/test_stream_ola_host.py pins it to the whole-utterance chain (ola_np.ola over the masks), tests/test_stream_ola_gpu.py
compares the device with it.

State of a lane, as the library keeps it: what StreamNP keeps, but the pending hop is replaced by the second-half addend of the
newest frame that has been rebuilt (NOT de-emphasised) and the de-emphasis carry stands alone.  With w = hamming(256),
D[s] = w[s]^2 + w[s + 128]^2 and x_t = irfft(mask_t * phase_t, 256), output position p of a push to a lane at H hops is hop
t = H - 5 + p: zero for t < 0, w x_0 / w^2 for t = 0, (w[s] x_t[s] + w[s + 128] x_{t-1}[s + 128]) / D[s] after that -- frame t is the
push's slot p, frame t - 1 the slot before it or, for p = 0, the lane's state.  The delay is StreamNP's: 640 samples."""

import numpy as np

from oracle import rced_c
from stream_np import DELAY, DELAY_HOPS, FINISH_SLOTS, FRAME, KEEP, BINS, STEP, StreamNP, _Lane, _frame_spectrum

W = np.hamming(FRAME)
DEN = W[:STEP] ** 2 + W[STEP:] ** 2
NEVER = 1 << 30      # "no last frame yet": a push never emits the utterance's last hop


def num_frames(length):
    """audio_feature.py:70, as rced_stft_num_frames"""
    return -(-abs(length - FRAME) // STEP) + 1


class _OlaLane(_Lane):
    def __init__(self):
        _Lane.__init__(self)
        self.pend = np.zeros(STEP)        # w[s + 128] x[s + 128] / D[s] of the newest frame rebuilt
        self.carry = 0.0                  # the last sample handed out


class StreamOlaNP(StreamNP):
    def __init__(self, net_work, weights, lanes, max_hops=8, nfft=512):
        StreamNP.__init__(self, net_work, weights, lanes, max_hops, nfft)
        self.reset()

    def reset(self, lane=-1):
        for i in (range(len(self.lane)) if lane < 0 else [lane]):
            self.lane[i] = _OlaLane()

    def _run(self, st, frames, live, k, T=NEVER):
        """frames [k, 256] pre-emphasised (live[h]: the frame exists) -> the k hops H - 5 .. H + k - 6 in time order; the
        window, the addend and the carry of the new state.  T: the utterance's frame count (finish); frames at or past it
        are not rebuilt, hop T has frame T - 1 alone."""
        mag = np.zeros((KEEP + k, BINS))
        phase = np.ones((KEEP + k, BINS), np.complex128)
        mag[:KEEP], phase[:KEEP] = st.mag, st.phase
        for h in range(k):
            if live[h]:
                mag[KEEP + h], phase[KEEP + h] = _frame_spectrum(frames[h])
        masks = rced_c.forward(self.net_work, self.weights, mag[None, :, :, None].astype(np.float32), np.float64)[0, :, :, 0]
        hops, below, carry = [], st.pend, st.carry
        for p in range(k):
            t = st.hops - DELAY_HOPS + p                       # the frame in window row p + 3
            first, second = np.zeros(STEP), np.zeros(STEP)
            if 0 <= t < T:                                     # any other slot is zeros: never read
                x = np.fft.irfft(masks[p + 3] * phase[p + 3], FRAME)
                first, second = W[:STEP] * x[:STEP] / DEN, W[STEP:] * x[STEP:] / DEN
            e = first + below
            if t == 0:
                e = e * DEN / W[:STEP] ** 2                    # frame 0 alone
            if t == T:
                e = e * DEN / W[STEP:] ** 2                    # frame T - 1 alone
            hops.append(self._de_emphasis(e, carry))
            below, carry = second, hops[-1][-1]
        return hops, mag[k:], phase[k:], below, carry

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
            hops, st.mag, st.phase, st.pend, st.carry = self._run(st, frames, live, k)
            out[s] = np.concatenate(hops)
            st.prev, st.sample = e[-STEP:], pcm[s, -1]
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
            live = [H >= 1 and (r > 0 or H == 1), H <= 1 and r > 0] + [False] * 4     # as StreamNP.finish
            hops = self._run(st, frames, live, FINISH_SLOTS, num_frames(STEP * H + r))[0]
            seq = np.concatenate(hops)[STEP * max(0, DELAY_HOPS - H):]
            out.append(seq[:STEP * H + r - max(0, STEP * H - DELAY)].copy())
            self.lane[s] = _OlaLane()
        return out
