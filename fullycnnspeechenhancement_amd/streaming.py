"""Stateful lanes on the device, over the C ABI: the resampler lanes (rced_rstream_*), the 8 kHz denoiser lanes
(rced_stream_*), and StreamingDenoiser, the chain of up to three of them that takes audio at the capture
device's rate.  audio.py re-exports every public name here."""

import numpy as np

from . import _args, _lib
from ._args import SAMPLE_RATE, STEP
from .arena import resample_taps

STREAM_DELAY, STREAM_FINISH_MAX, STREAM_MAX_HOPS = 640, 768, 64     # rced.h: RCED_STREAM_DELAY, RCED_STREAM_FINISH_MAX, the max_hops bound


class _Lanes(object):
    """What every kind of lanes is: a handle of the library and `lanes` streams behind it on cuda:`device`, each taking frames of
    `channels` interleaved values of `dtype` and handing out samples of out_dtype; a finish hands out at most finish_max samples a
    lane.  A subclass names its family of entry points (push, finish, reset, destroy) and creates its handle.  push and finish
    here are those of lanes that count in units: unit_in frames in, unit_out samples out."""

    _family = None      # "rced_stream", "rced_rstream" or "rced_rfree"
    _h = None

    def _open(self, h, lanes, device, channels, dtype, out_dtype, finish_max):
        self.lanes, self.device, self.channels = int(lanes), int(device), channels
        self.dtype, self.out_dtype, self.finish_max = dtype, out_dtype, finish_max
        self._in, self._np_in, _ = _args.pcm_format(dtype)
        self._out = _args.pcm_format(out_dtype)[0]
        self._c = {name: getattr(_lib.load(), "%s_%s" % (self._family, name)) for name in ("push", "finish", "reset", "destroy")}
        self._h = h

    def _active(self, active):
        """None, or `lanes` flags -> int32 on the device"""
        import torch
        if active is None:
            return None
        act = _args.to_device(active, torch.int32, self.device, "active")
        if tuple(act.shape) != (self.lanes,):
            raise ValueError("active must hold lanes = %d flags, got shape %s" % (self.lanes, tuple(act.shape)))
        return act

    def push(self, pcm, active=None):
        """pcm [lanes, K * unit_in] (interleaved: [lanes, K * unit_in * channels] or [lanes, K * unit_in, channels]), K >= 1: the
        next K units of every lane -> [lanes, K * unit_out] of out_dtype.  active: None, or `lanes` flags; a lane flagged 0 is
        idle (state untouched, zeros out).  A CUDA tensor gives a CUDA tensor (no synchronisation), an ndarray an ndarray."""
        import torch
        as_torch = hasattr(pcm, "is_cuda")
        k = _args.pcm_units(pcm.shape, self.lanes, self.channels, self.unit_in)
        if k < 1:
            raise ValueError("pcm must be [lanes = %d, K * %d frames] of %d channels with K >= 1, got %s"
                             % (self.lanes, self.unit_in, self.channels, tuple(pcm.shape)))
        x = _args.to_device(pcm, self._in, self.device, "pcm")
        act = self._active(active) if active is not None else None
        out = torch.empty((self.lanes, k * self.unit_out), dtype=self._out, device=x.device)
        stream = torch.cuda.current_stream(x.device)
        _lib.check(self._c["push"](self._h, x.data_ptr(), act.data_ptr() if act is not None else None, k, out.data_ptr(), stream.cuda_stream))
        _args.keep_alive(stream, x, act)      # the launches read the inputs to their end
        return out if as_torch else out.cpu().numpy()

    def finish(self, lanes, tails):
        """Ends the utterance of every lane listed: tails[i] holds the last 0 .. unit_in - 1 frames of lane lanes[i] ([frames] or
        [frames, channels]).  Returns a list of arrays of out_dtype, the samples each lane still owed; the lanes are reset for
        a new utterance, the others left alone.  Synchronises (the counts come back)."""
        import torch
        lanes = _args.host_ints(lanes)
        tail, counts = _args.pack_tails(self.lanes, self.unit_in, self.channels, self._np_in, lanes, tails)
        dev = "cuda:%d" % self.device
        tdev, cdev = torch.as_tensor(tail, device=dev), torch.as_tensor(counts, device=dev)
        out = torch.empty((self.lanes, self.finish_max), dtype=self._out, device=dev)
        owed = torch.empty((self.lanes,), dtype=torch.int32, device=dev)
        _lib.check(self._c["finish"](self._h, tdev.data_ptr(), cdev.data_ptr(), out.data_ptr(), owed.data_ptr(),
                                     _args.current_stream(out.device)))
        out, owed = out.cpu().numpy(), owed.cpu().numpy()
        return [out[lane, :owed[lane]].copy() for lane in lanes]

    def reset(self, lane=-1):
        """Back to the start of an utterance, without output: one lane, or (-1) all of them."""
        _lib.check(self._c["reset"](self._h, int(lane)))
        self._on_reset(int(lane))

    def _on_reset(self, lane):
        """what the host keeps of a lane (or, -1, of all) goes back to the start with it"""

    def close(self):
        if self._h is not None:
            try:
                self._c["destroy"](self._h)
            except Exception:
                pass
            self._h = None

    def __del__(self):
        self.close()


def resampler_delay(sr_in, sr_out):
    """The delay D of a resampler lane (StreamingResampler.delay) in output samples, from the phase table alone
    (needs no GPU): the smallest D at which a push reaches only frames already pushed, floor(right * p / q)."""
    p, q, left, table = resample_taps(sr_in, sr_out)
    return (table.shape[1] - 1 - left) * p // q


class StreamingResampler(_Lanes):
    """resample_batch for audio that arrives unit by unit, for `lanes` independent streams at once (rced_rstream_*, DESIGN.md
    3.4g).  A push of K units hands every active lane K * unit_in source frames at sr_in and returns K * unit_out samples at
    sr_out; a lane's output is resample_batch of everything pushed before `finish`, delayed by `.delay` samples, bit for
    bit: zeros first, and `finish` hands out what is still owed (resample_length(L) - max(0, H * unit_out - delay) samples
    after H units and L frames).  All state lives on the device; a push is one launch on the current stream.

    unit_out / unit_in: give one (the other follows from the ratio; a unit that gives no whole number on the other side is a
    ValueError), both (they must stand in the ratio), or neither (the smallest pair: q frames in, p samples out).
    channels: interleaved channels per frame, averaged; dtype / out_dtype: "float32" or "int16", as in resample_arena;
    max_units: the most units one push may carry (1 <= K <= max_units); delay: None (the smallest, resampler_delay(sr_in,
    sr_out)) or a longer one."""

    _family = "rced_rstream"

    def __init__(self, sr_in, sr_out, lanes, unit_out=None, unit_in=None, channels=1, dtype="float32", out_dtype="float32",
                 max_units=8, device=0, delay=None):
        import ctypes
        from math import gcd
        sr_in, sr_out = int(sr_in), int(sr_out)
        if sr_in < 1 or sr_out < 1:
            raise ValueError("both rates must be positive, got %d -> %d" % (sr_in, sr_out))
        code, out_code = _args.pcm_format(dtype)[2], _args.pcm_format(out_dtype, "out_dtype")[2]
        p, q = sr_out // gcd(sr_in, sr_out), sr_in // gcd(sr_in, sr_out)
        if unit_out is None and unit_in is None:
            unit_in, unit_out = q, p
        elif unit_in is None:
            if int(unit_out) * q % p:
                raise ValueError("%d samples at %d Hz are not a whole number of frames at %d Hz (%d * %d / %d)"
                                 % (unit_out, sr_out, sr_in, unit_out, q, p))
            unit_in = int(unit_out) * q // p
        elif unit_out is None:
            if int(unit_in) * p % q:
                raise ValueError("%d frames at %d Hz are not a whole number of samples at %d Hz (%d * %d / %d)"
                                 % (unit_in, sr_in, sr_out, unit_in, p, q))
            unit_out = int(unit_in) * p // q
        unit_in, unit_out = int(unit_in), int(unit_out)
        if unit_in < 1 or unit_out < 1 or unit_in * p != unit_out * q:
            raise ValueError("units of %d frames in and %d samples out do not stand in the ratio %d Hz -> %d Hz (%d / %d)"
                             % (unit_in, unit_out, sr_in, sr_out, p, q))
        self.sr_in, self.sr_out, self.max_units = sr_in, sr_out, int(max_units)
        if int(channels) < 1:
            raise ValueError("channels must be >= 1, got %d" % channels)
        h = ctypes.c_void_p()
        _lib.check(_lib.load().rced_rstream_create_ex(sr_in, sr_out, int(channels), code, out_code, unit_in, unit_out, int(lanes),
                                                      self.max_units, -1 if delay is None else int(delay), int(device), ctypes.byref(h)))
        self.delay = int(_lib.load().rced_rstream_delay(h))
        self.unit_in, self.unit_out = unit_in, unit_out
        self._open(h, lanes, device, int(channels), dtype, out_dtype, unit_out + self.delay)

    def started(self, active=None):
        """[lanes] int32 on the device: 1 where the lane is active and has taken a unit since the start of its utterance
        (rced_rstream_started).  No synchronisation."""
        import torch
        act = self._active(active)
        out = torch.empty((self.lanes,), dtype=torch.int32, device="cuda:%d" % self.device)
        stream = torch.cuda.current_stream(out.device)
        _lib.check(_lib.load().rced_rstream_started(self._h, act.data_ptr() if act is not None else None, out.data_ptr(), stream.cuda_stream))
        _args.keep_alive(stream, act)
        return out


class _DenoiserLanes(_Lanes):
    """The 8 kHz lanes of the denoiser (rced_stream_*): hops of 128 mono float32 samples in and out, a push is
    three launches on the current stream; at a framing hops of its stride and four launches.  The library
    refuses a push once the model's handle is gone."""

    _family = "rced_stream"

    def __init__(self, model, lanes, max_hops, nfft, rebuild="reference", framing=None):
        """framing: None (the specialised kernels), or a Framing stream_framing has let through: hops of its stride, four launches
        a push (rced_stream_create_fr)."""
        import ctypes
        h = ctypes.c_void_p()
        lib, code = _lib.load(), _args.REBUILDS.index(rebuild)              # RCED_STREAM_REBUILD_REFERENCE = 0, _OLA = 1
        self.unit_in = self.unit_out = STEP if framing is None else framing.stride
        if framing is None:
            _lib.check(lib.rced_stream_create_ex(model._handle, int(lanes), int(max_hops), int(nfft), code, ctypes.byref(h)))
            self._open(h, lanes, model.device, 1, "float32", "float32", STREAM_FINISH_MAX)
            return
        _lib.check(lib.rced_stream_create_fr(model._handle, int(lanes), int(max_hops), int(nfft), code, framing.window, framing.stride,
                                             framing.code, ctypes.byref(h)))
        self._open(h, lanes, model.device, 1, "float32", "float32", int(lib.rced_stream_finish_max_fr(framing.window, framing.stride)))


def stream_framing(framing, rebuild="ola", **others):
    """The framing of a stream: None for None or Framing() (today's lanes, today's bits), else the Framing -- after the library's
    refusals (rced_stream_fr_check: the reference rebuild with a window that ends in zero, more than 8 frames of overlap) as
    ValueErrors with its message, before any device work.  others: arguments of the caller that a framing does not combine with
    yet, as name = (value, default): a ValueError that names the combination."""
    from . import audio
    fr = audio._general(framing)
    if fr is None:
        return None
    for name, (value, default) in sorted(others.items()):
        if value != default:
            raise ValueError("framing=%r together with %s=%r: the rate-aware chain and the block denoiser run at 256 / 128 / hamming "
                             "only (their down lanes would have to run whole hops of the framing late); stream the 8 kHz mono "
                             "float32 signal, or use InferenceEngine.denoise_pcm(framing=...)" % (fr, name, value))
    audio._refused(_lib.load().rced_stream_fr_check(fr.window, fr.stride, fr.code, _args.REBUILDS.index(rebuild)))
    return fr


def stream_delay_fr(framing=None):
    """StreamingDenoiser(..., framing=framing).delay in samples at 8 kHz (needs no GPU): (ceil(W / S) + 3) * S -- a frame is
    complete ceil(W / S) - 1 hops after the one it starts in, its mask needs 4 more frames, and the hop that leaves needs the
    frames back to the one that started ceil(W / S) - 1 hops before it.  640 at 256 / 128; 400 at 160 / 80."""
    fr = stream_framing(framing)
    return STREAM_DELAY if fr is None else int(_lib.load().rced_stream_delay_fr(fr.window, fr.stride))


def stream_delay(sample_rate=8000, output_rate=None, channels=1, dtype="float32"):
    """StreamingDenoiser(..., sample_rate, channels, dtype, output_rate).delay, in samples at the output's rate (needs no GPU):
    STREAM_DELAY = 640 at 8 kHz; with down lanes (any input but mono float32 at 8 kHz) one hop more, 128 -- the down lanes hand on
    whole hops, which costs resampler_delay's 63 rounded up to a hop --; with up lanes all of that carried to output_rate, and
    their own resampler_delay(8000, output_rate).  48 kHz in and out: (128 + 640) * 6 + 384 = 4,992."""
    d = STREAM_DELAY + (STEP if int(sample_rate) != SAMPLE_RATE or int(channels) != 1 or dtype != "float32" else 0)
    if output_rate is not None and int(output_rate) != SAMPLE_RATE:
        d = d * int(output_rate) // SAMPLE_RATE + resampler_delay(SAMPLE_RATE, output_rate)
    return d


def drain_hops(n_lanes, push, finish, lanes, seqs):
    """Whole hops of seqs[i] through lane lanes[i] of a stage of n_lanes lanes that takes the 8 kHz signal, given as its push and
    finish, one hop a push, the other lanes idle; then its finish with what is left.  Returns every lane's output, joined."""
    unit = STEP
    seqs = [np.asarray(s, np.float32) for s in seqs]
    got = [[] for _ in lanes]
    at = 0
    while any(len(s) - at >= unit for s in seqs):
        pcm, active = np.zeros((n_lanes, unit), np.float32), [0] * n_lanes
        for lane, s in zip(lanes, seqs):
            if len(s) - at >= unit:
                pcm[lane], active[lane] = s[at:at + unit], 1
        out = push(pcm, active)
        for i, (lane, s) in enumerate(zip(lanes, seqs)):
            if len(s) - at >= unit:
                got[i].append(np.asarray(out[lane]))
        at += unit
    rest = finish(lanes, [s[len(s) // unit * unit:] for s in seqs])
    return [np.concatenate(g + [np.asarray(r)]) for g, r in zip(got, rest)]


class _Chain(object):
    """What StreamingDenoiser and BlockDenoiser (freerun.py) are: a model's denoiser lanes between optional lanes down to 8 kHz and
    up again, reset and closed together."""

    _down = _denoiser = _up = None

    def _take_model(self, model_or_engine, name):
        self.model = getattr(model_or_engine, "model", model_or_engine)
        if getattr(self.model, "_handle", None) is None:
            raise ValueError("%s needs an inference model (Model(is_training=False)) or an engine that holds one" % name)

    def _stages(self):
        return [s for s in (self._down, self._denoiser, self._up) if s is not None]

    def reset(self, lane=-1):
        """Back to the start of an utterance, without output: one lane, or (-1) all of them."""
        for stage in self._stages():
            stage.reset(lane)
        self._on_reset(int(lane))

    def _on_reset(self, lane):
        """what the host keeps of a lane (or, -1, of all) goes back to the start with it"""

    def close(self):
        for stage in self._stages():
            stage.close()
        self._down = self._denoiser = self._up = None

    def __del__(self):
        self.close()


class StreamingDenoiser(_Chain):
    """PCM in, PCM out, a hop (128 samples, 16 ms) at a time, for `lanes` independent streams at once (rced_stream_*,
    DESIGN.md 3.4d).  A lane's output is InferenceEngine.denoise_pcm of everything pushed before `finish`, delayed by
    STREAM_DELAY = 640 samples: zeros first, and `finish` hands out what is still owed.  All state lives on the device; a
    push is three launches on the current stream.

    model_or_engine: a model of this package (is_training=False) or an engine holding one as `.model`; the stream runs the
    forward form that model has selected.  max_hops: the most hops one push may carry (1..64); nfft: 512 (the reference's
    rebuild as shipped) or 256.  rebuild: "reference", or "ola" -- the lane's output is then denoise_pcm(..., rebuild="ola"), weighted
    overlap-add, at the same delay (hop h needs frames h and h - 1, and both are there when the reference rebuild hands out hop h);
    nfft is checked and plays no part.

    sample_rate, channels, dtype ("float32" or "int16"), output_rate: the capture and playback device's format.  With the
    defaults this is the 8 kHz object above.  Otherwise a push takes [lanes, K * hop_in (* channels)] at sample_rate, hop_in =
    128 * sample_rate / 8000, through resampler lanes (StreamingResampler) down to 8 kHz, the denoiser, and --
    with output_rate, normally sample_rate -- resampler lanes up again, without synchronisation; the output is float32 mono,
    InferenceEngine.denoise_pcm(x, sample_rate=...) (resampled to output_rate) delayed by `.delay` = stream_delay(...)
    samples.  A rate at which the hop is not a whole number of frames (44.1 kHz: 128 * 441 / 80) is a ValueError naming the
    rate: denoise_pcm serves those rates offline.

    framing: None or Framing() -- all of the above --, or another audio.Framing: the hop (`.hop`) is its stride S,
    push and finish take and give units of S samples, and a lane's output is denoise_pcm(..., rebuild=rebuild, framing=framing)
    delayed by `.delay` = stream_delay_fr(framing) = (ceil(W / S) + 3) * S samples; a push is four launches.  8 kHz mono float32
    only: with sample_rate, channels, dtype or output_rate it is a ValueError, and so is what the library refuses (the reference
    rebuild with a window that ends in zero, more than 8 frames of overlap)."""

    def __init__(self, model_or_engine, lanes, max_hops=8, nfft=512, sample_rate=8000, channels=1, dtype="float32", output_rate=None,
                 rebuild="reference", framing=None):
        self.rebuild = _args.check_rebuild(rebuild)
        self._take_model(model_or_engine, "StreamingDenoiser")
        self.framing = stream_framing(framing, self.rebuild, sample_rate=(int(sample_rate), SAMPLE_RATE), channels=(int(channels), 1),
                                      dtype=(dtype, "float32"), output_rate=(output_rate, None))
        self.lanes, self.max_hops, self.nfft, self.device = int(lanes), int(max_hops), int(nfft), self.model.device
        self.sample_rate, self.channels, self.dtype = int(sample_rate), int(channels), dtype
        self.output_rate = int(output_rate) if output_rate is not None else None
        for rate in (self.sample_rate, self.output_rate):
            if rate is not None and (rate < 1 or STEP * rate % SAMPLE_RATE):
                raise ValueError("a hop of %d samples at 8 kHz is not a whole number of frames at %r Hz: streaming serves rates that are a "
                                 "multiple of 62.5 Hz, InferenceEngine.denoise_pcm(sample_rate=...) every rate" % (STEP, rate))
        self._denoiser = _DenoiserLanes(self.model, self.lanes, self.max_hops, self.nfft, self.rebuild, self.framing)
        self._push8 = self._denoiser.push        # the one name every 8 kHz push goes through, finish's drain included
        self.hop = STEP if self.framing is None else self.framing.stride
        self.hop_in = self.hop * self.sample_rate // SAMPLE_RATE
        self.delay = stream_delay(self.sample_rate, self.output_rate, self.channels, dtype) if self.framing is None else stream_delay_fr(self.framing)
        if self.sample_rate != SAMPLE_RATE or self.channels != 1 or dtype != "float32":
            self._down = StreamingResampler(self.sample_rate, SAMPLE_RATE, self.lanes, unit_out=STEP, channels=self.channels, dtype=dtype,
                                            max_units=self.max_hops, device=self.device, delay=STEP)
        if self.output_rate is not None and self.output_rate != SAMPLE_RATE:
            self._up = StreamingResampler(SAMPLE_RATE, self.output_rate, self.lanes, unit_in=STEP, max_units=self.max_hops,
                                          device=self.device)

    def _chain(self):
        """(push, finish) of every stage, in order"""
        return ([(self._down.push, self._down.finish)] if self._down is not None else []) + [(self._push8, self._denoiser.finish)] + (
            [(self._up.push, self._up.finish)] if self._up is not None else [])

    def push(self, pcm, active=None):
        """pcm [lanes, K*128] (1 <= K <= max_hops): the next K hops of every lane -> [lanes, K*128], the lanes' output streams.
        active: None, or `lanes` flags; a lane flagged 0 is idle (state untouched, zeros out).  A CUDA tensor gives a CUDA
        tensor (no synchronisation), an ndarray an ndarray.
        At the device's rate: pcm [lanes, K * hop_in (* channels)] of `dtype` -> [lanes, K*128] at 8 kHz, or with output_rate
        [lanes, K * 128 * output_rate / 8000], float32.  At a framing: [lanes, K * hop] in and out, hop = the framing's stride.

        down lanes -> the three launches of the 8 kHz push -> up lanes, nothing waits.  The down lanes run a whole hop behind
        (delay 128), so what they hand on is whole hops of the 8 kHz signal -- except the first hop of a lane's first push, which
        is the delay's zeros and not signal: the denoiser takes that hop apart from the others, for the lanes that have started
        only (StreamingResampler.started), and returns zeros for the rest."""
        as_torch = hasattr(pcm, "is_cuda")
        y = pcm if as_torch else _args.to_device(pcm, (self._down or self._denoiser)._in, self.device, "pcm")
        act = active
        if self._down is not None:
            import torch
            act = self._down._active(active)
            started = self._down.started(act)
            z = self._down.push(y, act)                              # [lanes, K * 128] at 8 kHz, one hop late
            y = self._push8(z[:, :STEP], started)
            if z.shape[1] > STEP:
                y = torch.cat([y, self._push8(z[:, STEP:], act)], dim=1)
        else:
            y = self._push8(y, act)
        if self._up is not None:
            y = self._up.push(y, act)
        return y if as_torch else y.cpu().numpy()

    def _drain(self, push, finish, lanes, seqs):
        return drain_hops(self.lanes, push, finish, lanes, seqs)

    def finish(self, lanes, tails):
        """Ends the utterance of every lane listed: tails[i] holds the last 0..127 samples of lane lanes[i].  Returns a list of
        float32 arrays, the samples each lane still owed (L - max(0, 128 H - 640) of them); the lanes are reset for a new
        utterance, the others left alone.  Synchronises (the counts come back).
        At a framing: the last 0 .. hop - 1 samples; L - max(0, hop * H - delay) samples are owed.
        At the device's rate: tails[i] holds fewer than hop_in frames; the stages are drained in order -- what the down lanes
        owe goes hop by hop through the denoiser and its finish, all of that through the up lanes and their finish."""
        lanes = _args.host_ints(lanes)
        chain = self._chain()
        out = chain[0][1](lanes, tails)
        for push, finish in chain[1:]:
            out = self._drain(push, finish, lanes, out)
        return out
