"""Streaming in blocks of any size and at any rate, over the C ABI: FreeResampler, resampler lanes that count in
frames and keep their finished outputs in a ring on the device (rced_rfree_*), and BlockDenoiser, the chain of such lanes down to
8 kHz, the 8 kHz denoiser lanes (rced_stream_*, untouched) and such lanes up again, that takes a fixed block at the capture
device's rate and returns a fixed block on every call.  audio.py re-exports every public name here."""

from functools import lru_cache

import numpy as np

from . import _args, _lib
from ._args import SAMPLE_RATE, STEP
from .streaming import STREAM_DELAY, STREAM_MAX_HOPS, _Chain, _DenoiserLanes, _Lanes, drain_hops


@lru_cache(maxsize=None)
def _geometry(sr_in, sr_out):
    """(p, q, right) of a ratio's phase table (rced_resample_taps; needs no GPU)."""
    import ctypes
    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.load().rced_resample_taps(int(sr_in), int(sr_out), v[0], v[1], v[2], v[3], None, 0))
    p, q, left, width = (int(x.value) for x in v)
    return p, q, width - 1 - left


def free_available(sr_in, sr_out, frames):
    """A(F): the outputs a free-running lane sr_in -> sr_out has emitted after `frames` frames, ceil((F - right) p / q) for F >
    right, else 0 (rced_rfree_available; needs no GPU)."""
    p, q, right = _geometry(sr_in, sr_out)
    frames = int(frames)
    if frames < 0:
        raise ValueError("frames must be >= 0, got %d" % frames)
    return -((-(frames - right) * p) // q) if frames > right else 0


class FreeResampler(_Lanes):
    """resample_batch for audio that arrives in pieces of any size, for `lanes` independent streams at once, without a delay
    (rced_rfree_*).  A lane emits every output as soon as its last tap has arrived -- free_available(sr_in,
    sr_out, F) of them after F frames -- into a ring on the device that starts an utterance holding `prefill` zeros; a push hands
    a lane any number of frames and takes any number of samples that are there.  Everything a lane hands out up to the end of
    `finish` is `prefill` zeros and then resample_batch of everything it was given, bit for bit.  sr_in == sr_out passes the
    samples through: a re-blocker.  All state lives on the device; a push is one launch on the current stream.

    channels, dtype / out_dtype: as in StreamingResampler.  max_frames: the most frames one push may bring a lane; max_take: the
    most samples one push may take from a lane (default: what max_frames frames give, rounded up).  `.in_ring` is the host's
    mirror of what every lane's ring holds, `.capacity` the ring's size: a push that would leave more than that in a ring, or take
    more than is there, is a ValueError before anything is launched."""

    _family = "rced_rfree"

    def __init__(self, sr_in, sr_out, lanes, channels=1, dtype="float32", out_dtype="float32", max_frames=4096, max_take=None, prefill=0,
                 device=0):
        import ctypes
        sr_in, sr_out = int(sr_in), int(sr_out)
        if sr_in < 1 or sr_out < 1:
            raise ValueError("both rates must be positive, got %d -> %d" % (sr_in, sr_out))
        code, out_code = _args.pcm_format(dtype)[2], _args.pcm_format(out_dtype, "out_dtype")[2]
        if int(channels) < 1:
            raise ValueError("channels must be >= 1, got %d" % channels)
        if max_take is None:
            max_take = -((-int(max_frames) * sr_out) // sr_in)
        self.sr_in, self.sr_out, self.lanes = sr_in, sr_out, int(lanes)
        self.max_frames, self.max_take, self.prefill = int(max_frames), int(max_take), int(prefill)
        lib = _lib.load()
        cap, fin = ctypes.c_int(), ctypes.c_int()
        _lib.check(lib.rced_rfree_plan(sr_in, sr_out, out_code, self.lanes, self.max_frames, self.max_take, self.prefill, None, None,
                                       ctypes.byref(cap), ctypes.byref(fin)))
        self.capacity = int(cap.value)
        self._geo = _geometry(sr_in, sr_out)
        self._frames, self._taken = np.zeros(self.lanes, np.int64), np.zeros(self.lanes, np.int64)      # the host's mirror
        self.taken = [0] * self.lanes          # what the latest push took from every lane
        self._ints = {}
        h = ctypes.c_void_p()
        _lib.check(lib.rced_rfree_create(sr_in, sr_out, int(channels), code, out_code, self.lanes, self.max_frames, self.max_take, self.prefill,
                                         int(device), ctypes.byref(h)))
        self._open(h, lanes, device, int(channels), dtype, out_dtype, int(fin.value))

    def _avail(self, frames):
        """free_available for an int64 array of frame counts."""
        p, q, right = self._geo
        f = frames - right
        return np.where(f > 0, -((-f * p) // q), 0)

    @property
    def in_ring(self):
        """Samples in every lane's ring: prefill + A(frames given) - samples taken."""
        return (self.prefill + self._avail(self._frames) - self._taken).tolist()

    def _dev_ints(self, values):
        """`lanes` host integers (an int64 array) as int32 on the device; a pattern that comes again is not uploaded again."""
        import torch
        values = values.astype(np.int32)
        key = values.tobytes()
        t = self._ints.get(key)
        if t is None:
            if len(self._ints) >= 4096:
                self._ints.clear()
            t = self._ints[key] = torch.as_tensor(values, device="cuda:%d" % self.device)
        return t

    def _per_lane(self, values, what):
        """None, one integer for every lane, or `lanes` host integers -> None or an int64 array"""
        if values is None:
            return None
        if getattr(values, "is_cuda", False):
            raise TypeError("%s must be host values (the host mirrors every ring's count from them), got a device tensor" % what)
        if isinstance(values, (int, np.integer)):
            return np.full(self.lanes, int(values), np.int64)
        if not isinstance(values, np.ndarray):
            values = _args.host_ints(values, self.lanes, what)
        values = np.asarray(values, np.int64)
        if values.shape != (self.lanes,):
            raise ValueError("%s must hold lanes = %d values, got shape %s" % (what, self.lanes, values.shape))
        return values

    def _plan_push(self, n, counts, take):
        """The mirror's half of a push of n columns: (frames per lane, samples taken per lane) as int64 arrays, after every check."""
        got = self._per_lane(counts, "counts")
        if got is None:
            got = np.full(self.lanes, n, np.int64)
        if (got > n).any():
            raise ValueError("counts must be at most the %d frames pushed (negative: idle), got %r" % (n, got.tolist()))
        live = got >= 0
        there = self.prefill + self._avail(self._frames + np.maximum(got, 0)) - self._taken
        if (there[live] > self.capacity).any():
            s = int(np.argmax(live & (there > self.capacity)))
            raise ValueError("lane %d: the push would leave %d samples in a ring of %d: take more, or push less" % (s, there[s], self.capacity))
        take = self._per_lane(take, "take")
        if take is None:
            take = np.where(live, np.minimum(there, self.max_take), 0)
        bad = (take < 0) | (take > self.max_take)
        if bad.any():
            raise ValueError("take must be 0..max_take = %d, got %d for lane %d" % (self.max_take, take[np.argmax(bad)], np.argmax(bad)))
        bad = ~live & (take > 0)
        if bad.any():
            raise ValueError("lane %d is idle in this push and hands out nothing, got take %d" % (np.argmax(bad), take[np.argmax(bad)]))
        bad = take > there
        if bad.any():
            s = int(np.argmax(bad))
            raise ValueError("lane %d: take %d, but its ring holds %d after this push" % (s, take[s], there[s]))
        return got, take

    def _push(self, x, n, counts, take, cols=None):
        """x: None or a device tensor of [lanes, n(, channels)] frames; the rest as push.  Returns the device tensor [lanes, cols]."""
        import torch
        got, take = self._plan_push(n, counts, take)
        cols = int(take.max()) if cols is None else cols
        dev = torch.device("cuda:%d" % self.device)
        out = torch.empty((self.lanes, cols), dtype=self._out, device=dev)
        cdev = self._dev_ints(got) if (got != n).any() else None
        tdev = self._dev_ints(take) if (take[got >= 0] != cols).any() else None
        stream = torch.cuda.current_stream(dev)
        _lib.check(self._c["push"](self._h, x.data_ptr() if n else None, n, cdev.data_ptr() if cdev is not None else None,
                                   out.data_ptr() if cols else None, cols, tdev.data_ptr() if tdev is not None else None, stream.cuda_stream))
        _args.keep_alive(stream, x)
        self._frames += np.maximum(got, 0)
        self._taken += take
        self.taken = take.tolist()
        return out

    def _frames_of(self, pcm):
        n = _args.pcm_units(pcm.shape, self.lanes, self.channels)
        if n < 0 or n > self.max_frames:
            raise ValueError("pcm must be [lanes = %d, 0..%d frames] of %d channels, got %s"
                             % (self.lanes, self.max_frames, self.channels, tuple(pcm.shape)))
        return n

    def push(self, pcm, counts=None, take=None):
        """pcm [lanes, n] (interleaved: [lanes, n * channels] or [lanes, n, channels]), 0 <= n <= max_frames, or None (n = 0).
        counts: None (every lane is given all n frames), or `lanes` host integers: the first counts[s] frames of row s are lane
        s's, 0 .. n; negative: the lane is idle (state untouched, zeros out).  take: None (every lane hands out all its ring holds,
        at most max_take; `.taken` has the numbers), an integer, or `lanes` host integers, each at most what the lane's ring holds
        after this push.  Returns [lanes, max(take)] of out_dtype, row s holding take[s] samples and zeros behind them.  A CUDA
        tensor (or None) gives a CUDA tensor (no synchronisation), an ndarray an ndarray."""
        as_torch = pcm is None or hasattr(pcm, "is_cuda")
        n = 0 if pcm is None else self._frames_of(pcm)
        x = _args.to_device(pcm, self._in, self.device, "pcm") if n else None
        out = self._push(x, n, counts, take)
        return out if as_torch else out.cpu().numpy()

    def finish(self, lanes, tails):
        """Ends the utterance of every lane listed: tails[i] holds the last frames of lane lanes[i] ([frames] or [frames,
        channels]; any number: what exceeds max_frames goes through pushes first, the other lanes idle).  Returns a list of arrays
        of out_dtype: everything each lane had not handed out yet, up to resample_length of all it was given; the lanes are reset
        for a new utterance, the others left alone.  Synchronises (the counts come back)."""
        import torch
        lanes = _args.host_ints(lanes)
        tails = [(t.detach().cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)).astype(self._np_in, copy=False) for t in tails]
        tails = [t.reshape((-1, self.channels)) if self.channels > 1 else t.reshape(-1) for t in tails]
        if len(lanes) != len(tails) or len(set(lanes)) != len(lanes) or any(v < 0 or v >= self.lanes for v in lanes):
            raise ValueError("lanes must be distinct indices in [0, %d), one tail each, got lanes %r and %d tails" % (self.lanes, lanes, len(tails)))
        got = [[] for _ in lanes]
        n = self.max_frames
        while any(len(t) > n for t in tails):
            pcm, counts = np.zeros((self.lanes, n) + tails[0].shape[1:], self._np_in), [-1] * self.lanes
            for lane, t in zip(lanes, tails):
                if len(t) > n:
                    pcm[lane], counts[lane] = t[:n], n
            while True:      # the chunk, then takes alone until the rings are empty: a ring holds one push on top of max_take
                out = self.push(pcm, counts)
                out = out.cpu().numpy() if hasattr(out, "is_cuda") else out      # a take alone (pcm None) comes back on the device
                for i, lane in enumerate(lanes):
                    if counts[lane] >= 0:
                        got[i].append(out[lane, :self.taken[lane]])
                pcm, counts = None, [0 if c >= 0 else -1 for c in counts]
                if not any(self.in_ring[lane] for lane in lanes if counts[lane] >= 0):
                    break
            tails = [t[n:] if len(t) > n else t for t in tails]
        width = max([len(t) for t in tails] + [1])
        tail, counts = _args.pack_tails(self.lanes, width + 1, self.channels, self._np_in, lanes, tails)
        dev = "cuda:%d" % self.device
        tdev, cdev = torch.as_tensor(tail[:, :width].copy(), device=dev), torch.as_tensor(counts, device=dev)
        out = torch.empty((self.lanes, self.finish_max), dtype=self._out, device=dev)
        owed = torch.empty((self.lanes,), dtype=torch.int32, device=dev)
        _lib.check(self._c["finish"](self._h, tdev.data_ptr(), width, cdev.data_ptr(), out.data_ptr(), owed.data_ptr(),
                                     _args.current_stream(out.device)))
        out, owed = out.cpu().numpy(), owed.cpu().numpy()
        for i, lane in enumerate(lanes):
            got[i].append(out[lane, :owed[lane]].copy())
            self._frames[lane] = self._taken[lane] = 0
        self.owed = [int(owed[lane]) for lane in lanes]      # the counts the device reported for its finish launch
        return [np.concatenate(g) for g in got]

    def _on_reset(self, lane):
        for s in (range(self.lanes) if lane < 0 else [lane]):
            self._frames[s] = self._taken[s] = 0


def _block_plan(block, sample_rate, output_rate):
    """The bookkeeping of BlockDenoiser(block, sample_rate, output_rate) that needs no device: (samples out per call, the prefill
    Z, the hop counts a call can carry, sorted).  Every refusal of its arguments is made here."""
    from math import gcd
    block, rin = int(block), int(sample_rate)
    rout = SAMPLE_RATE if output_rate is None else int(output_rate)
    if block < 1:
        raise ValueError("block must be >= 1 frame, got %d" % block)
    if rin < 1 or rout < 1:
        raise ValueError("both rates must be positive, got %d -> %d" % (rin, rout))
    if STREAM_DELAY * rout % SAMPLE_RATE:
        raise ValueError("the denoiser's delay of %d samples at 8 kHz is not a whole number of samples at %d Hz: the output rate "
                         "must be a multiple of 12.5 Hz" % (STREAM_DELAY, rout))
    if block * rout % rin:
        raise ValueError("a block of %d frames at %d Hz is not a whole number of samples at %d Hz: the smallest block that is, is %d"
                         % (block, rin, rout, rin // gcd(rin, rout)))
    block_out = block * rout // rin
    pd, qd, right_d = _geometry(rin, SAMPLE_RATE)
    pu, qu, right_u = _geometry(SAMPLE_RATE, rout)
    # the pattern of hops per call repeats once both lanes emit and F has gone on by a multiple of 128 q_down frames
    period = STEP * qd // gcd(block, STEP * qd)
    z, hops, h_prev, j, steady = 0, set(), 0, 0, None
    while steady is None or j < steady + period:
        j += 1
        a = free_available(rin, SAMPLE_RATE, j * block)
        h = a // STEP
        hops.add(h - h_prev)
        h_prev = h
        z = max(z, j * block_out - free_available(SAMPLE_RATE, rout, STEP * h))
        if steady is None and j * block > right_d and STEP * h > right_u:
            steady = j
    if max(hops) > STREAM_MAX_HOPS:
        raise ValueError("a block of %d frames at %d Hz carries up to %d hops a call, more than %d" % (block, rin, max(hops), STREAM_MAX_HOPS))
    return block_out, z, sorted(hops)


def block_delay(block, sample_rate=8000, output_rate=None):
    """BlockDenoiser(..., block, sample_rate, output_rate).delay, in samples at the output's rate (needs no GPU): the prefill Z
    that lets no call run dry, plus the denoiser's STREAM_DELAY = 640 carried to the output's rate."""
    block_out, z, _ = _block_plan(block, sample_rate, output_rate)
    rout = SAMPLE_RATE if output_rate is None else int(output_rate)
    return z + STREAM_DELAY * rout // SAMPLE_RATE


class BlockDenoiser(_Chain):
    """PCM in, PCM out, a fixed block of any size at a time, at the capture device's rate, for `lanes` independent streams at once
    (DESIGN.md 3.4h).  process() takes [lanes, block] frames at sample_rate and returns [lanes, block * output_rate / sample_rate]
    float32 samples on every call, without synchronisation: free-running lanes (FreeResampler) down to 8 kHz -- at 8 kHz in, the
    re-blocker --, from whose rings the 8 kHz denoiser lanes (rced_stream_*) take the whole hops that are there, and free-running
    lanes up to output_rate (None: 8 kHz) whose rings start with Z zeros, the smallest number with which no call runs dry.  A
    lane's output is what StreamingDenoiser's chain gives -- resample_batch to 8 kHz, the denoiser, resample_batch up -- delayed by
    `.delay` = block_delay(block, sample_rate, output_rate) samples.  44.1 kHz is served like any other rate.

    model_or_engine, nfft, rebuild, channels, dtype: as in StreamingDenoiser.  framing: None or Framing() only -- the blocks run
    at 256 / 128 / hamming, and another audio.Framing is a ValueError that says so (StreamingDenoiser(framing=...) serves the
    8 kHz signal at a framing).  A lane starts its utterance with a process() call
    and ends it with finish(); the host keeps every lane's frame count, from which all the bookkeeping follows."""

    def __init__(self, model_or_engine, lanes, block, sample_rate=8000, output_rate=None, channels=1, dtype="float32", nfft=512,
                 rebuild="reference", framing=None):
        from .streaming import stream_framing
        self.rebuild = _args.check_rebuild(rebuild)
        stream_framing(framing, self.rebuild, block=(int(block), None))      # None or Framing() only: a framing has no block form yet
        self._take_model(model_or_engine, "BlockDenoiser")
        self.lanes, self.block, self.nfft, self.device = int(lanes), int(block), int(nfft), self.model.device
        self.sample_rate, self.channels, self.dtype = int(sample_rate), int(channels), dtype
        self.output_rate = SAMPLE_RATE if output_rate is None else int(output_rate)
        _args.pcm_format(dtype)
        self.block_out, self.prefill, self.hops_per_call = _block_plan(self.block, self.sample_rate, self.output_rate)
        self.delay = self.prefill + STREAM_DELAY * self.output_rate // SAMPLE_RATE
        self.max_hops = max(self.hops_per_call + [1])
        self._denoiser = _DenoiserLanes(self.model, self.lanes, self.max_hops, self.nfft, self.rebuild)
        self._push8 = self._denoiser.push        # the one name every 8 kHz push goes through, finish's drain included
        self._down = FreeResampler(self.sample_rate, SAMPLE_RATE, self.lanes, channels=self.channels, dtype=dtype, max_frames=self.block,
                                   max_take=STEP * self.max_hops, device=self.device)
        self._up = FreeResampler(SAMPLE_RATE, self.output_rate, self.lanes, max_frames=STEP * self.max_hops, max_take=self.block_out,
                                 prefill=self.prefill, device=self.device)
        self._frames = np.zeros(self.lanes, np.int64)

    def process(self, pcm, active=None):
        """pcm [lanes, block] (interleaved: [lanes, block * channels] or [lanes, block, channels]) of `dtype`: the next block of
        every lane -> [lanes, block_out] float32, the lanes' output streams.  active: None, or `lanes` host flags (a device
        tensor is a TypeError: the host keeps every lane's frame count); a lane flagged 0 is idle (state untouched, zeros
        out).  A CUDA tensor gives a CUDA tensor (no synchronisation), an ndarray an ndarray.

        One launch of the down lanes; per distinct number K > 0 of whole hops that the active lanes' rings now hold, one 8 kHz
        push of K hops with exactly those lanes active; one launch of the up lanes."""
        import torch
        if getattr(active, "is_cuda", False):
            raise TypeError("active must be host values or None (the host keeps every lane's frame count), got a tensor")
        flags = np.ones(self.lanes, bool) if active is None else np.asarray(_args.host_ints(active, self.lanes, "active"), bool)
        as_torch = hasattr(pcm, "is_cuda")
        if self._down._frames_of(pcm) != self.block:
            raise ValueError("pcm must hold block = %d frames a lane, got %s" % (self.block, tuple(pcm.shape)))
        x = _args.to_device(pcm, self._down._in, self.device, "pcm")
        # whole hops so far H(F) = floor(A_down(F) / 128); this call's are H(F + block) - H(F)
        hops = np.where(flags, self._down._avail(self._frames + self.block) // STEP - self._down._avail(self._frames) // STEP, 0)
        most = int(hops.max())
        z = self._down._push(x, self.block, np.where(flags, self.block, -1), STEP * hops, STEP * most)
        y = None
        groups = np.unique(hops[hops > 0]).tolist()
        for k in groups:
            member = hops == k
            part = self._push8(z if k == most else z[:, :STEP * k].contiguous(),
                               None if member.all() else self._down._dev_ints(member.astype(np.int64)))
            if len(groups) == 1:
                y = part
            else:       # the rows of the lanes that sat this push out are zeros
                if y is None:
                    y = torch.zeros((self.lanes, STEP * most), dtype=torch.float32, device=z.device)
                y[:, :STEP * k] += part
        out = self._up._push(y, STEP * most, np.where(flags, STEP * hops, -1), np.where(flags, self.block_out, 0), self.block_out)
        self._frames = self._frames + np.where(flags, self.block, 0)
        return out if as_torch else out.cpu().numpy()

    def finish(self, lanes, tails):
        """Ends the utterance of every lane listed: tails[i] holds the last 0 .. block - 1 frames of lane lanes[i].  The stages are
        drained in order: what the down lanes still hold goes hop by hop through the denoiser and its finish, all of that through
        the up lanes and their finish.  Returns a list of float32 arrays, the samples each lane still owed; the lanes are reset
        for a new utterance, the others left alone.  Synchronises."""
        lanes = _args.host_ints(lanes)
        for lane, t in zip(lanes, tails):
            frames = int(t.numel() if hasattr(t, "numel") else np.asarray(t).size) // self.channels
            if frames >= self.block:
                raise ValueError("a tail holds fewer than block = %d frames (process whole blocks first), lane %d's has %d"
                                 % (self.block, lane, frames))
        out = self._down.finish(lanes, tails)
        out = drain_hops(self.lanes, self._push8, self._denoiser.finish, lanes, out)
        out = self._up.finish(lanes, out)
        for lane in lanes:
            self._frames[lane] = 0
        return out

    def _on_reset(self, lane):
        for s in (range(self.lanes) if lane < 0 else [lane]):
            self._frames[s] = 0
