"""The training objective's waveform terms on the device, over the C ABI (rced.h rced_wave_loss): the squared
error and the SI-SDR of the overlap-add rebuild against the clean signal, and their gradient with respect to the magnitudes.
audio.py re-exports every public name here."""

import ctypes
import math

from . import _args, _lib
from ._args import BINS


class WaveObjective(object):
    """loss = spectral * sum((target - M)^2) / B + wave_sse * sum_n wave_sse_n / B - si_sdr * sum_valid si_sdr_n / B, B the batch
    size (rced.h, rced_wave_loss).  The weights are finite, >= 0 and not all zero; WaveObjective() is the spectral loss alone.
    skip_edges: score only the hops two frames cover (the default) or the whole rebuilt signal.
    mr_stft > 0 adds  + mr_stft * sum_valid mr_stft_n / B, the multi-resolution STFT term of the rebuilt signal against the clean one
    over the same scored range (rced.h, rced_mr_stft), at `resolutions`: a tuple of 1 to 4 audio.Framing, None meaning
    audio.MR_STFT_8K.  An immutable value."""

    __slots__ = ("spectral", "wave_sse", "si_sdr", "skip_edges", "mr_stft", "resolutions")

    def __init__(self, spectral=1.0, wave_sse=0.0, si_sdr=0.0, skip_edges=True, mr_stft=0.0, resolutions=None):
        w = []
        for name, v in (("spectral", spectral), ("wave_sse", wave_sse), ("si_sdr", si_sdr), ("mr_stft", mr_stft)):
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError("%s must be a number, got %r" % (name, v))
            if not (math.isfinite(f) and f >= 0.0):
                raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
            w.append(f)
        if not any(w):
            raise ValueError("the weights spectral, wave_sse and si_sdr must not all be zero")
        if not isinstance(skip_edges, (bool, int)) or skip_edges not in (0, 1):
            raise ValueError("skip_edges must be True or False, got %r" % (skip_edges,))
        if resolutions is not None or w[3] > 0.0:
            from . import audio
            if resolutions is None:
                resolutions = audio.MR_STFT_8K
            try:
                resolutions = tuple(resolutions)
            except TypeError:
                raise ValueError("resolutions must be a tuple of 1 to 4 audio.Framing or None, got %r" % (resolutions,))
            if not 1 <= len(resolutions) <= 4 or not all(isinstance(r, audio.Framing) for r in resolutions):
                raise ValueError("resolutions must be a tuple of 1 to 4 audio.Framing or None, got %r" % (resolutions,))
        for name, v in zip(self.__slots__, w[:3] + [bool(skip_edges), w[3], resolutions]):
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError("a WaveObjective is immutable")

    __delattr__ = __setattr__

    @property
    def has_wave_term(self):
        return self.wave_sse > 0.0 or self.si_sdr > 0.0 or self.mr_stft > 0.0

    def _key(self):
        return (self.spectral, self.wave_sse, self.si_sdr, self.skip_edges, self.mr_stft, self.resolutions)

    def mr_args(self):
        """rced.h: rced_mr_args of the multi-resolution term (mr_stft > 0)."""
        return mr_args(self.resolutions, self.mr_stft)

    def __eq__(self, other):
        return isinstance(other, WaveObjective) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        if self.mr_stft == 0.0 and self.resolutions is None:
            return "WaveObjective(spectral=%r, wave_sse=%r, si_sdr=%r, skip_edges=%r)" % self._key()[:4]
        return "WaveObjective(spectral=%r, wave_sse=%r, si_sdr=%r, skip_edges=%r, mr_stft=%r, resolutions=%r)" % self._key()


def mr_args(resolutions, weight):
    """_lib.MrArgs (rced.h: rced_mr_args) of a tuple of 1 to 4 audio.Framing (None: audio.MR_STFT_8K) and the term's weight; what the
    library refuses is a ValueError with its reason."""
    from . import audio
    res = audio.MR_STFT_8K if resolutions is None else tuple(resolutions)
    if not 1 <= len(res) <= 4 or not all(isinstance(r, audio.Framing) for r in res):
        raise ValueError("resolutions must be a tuple of 1 to 4 audio.Framing or None, got %r" % (resolutions,))
    a = _lib.MrArgs()
    a.w_mr, a.n_res = float(weight), len(res)
    for i, r in enumerate(res):
        a.window[i], a.stride[i], a.window_name[i] = r.window, r.stride, r.code
    if _lib.load().rced_mr_stft_check(ctypes.byref(a)) != _lib.RCED_OK:
        raise ValueError(_lib.load().rced_last_error().decode())
    return a


def wave_loss_batch(mag, phase, clean, lengths, objective, batch_size, frames=None, grad=True, framing=None):
    """The waveform terms of `objective` for a batch and their gradient, on the device (rced_wave_loss; at a framing other than
    the default, rced_wave_loss_fr).
    mag [N, T, 129(,1)] float32 (the prediction), phase [N, T, 129] complex64 (the mixture's unit phase), clean [N, >= max length]
    float32 with contiguous rows (a view of a wider buffer is fine), all torch.cuda; lengths: N sample counts in [0, clean's width];
    frames: N frame counts (list / tensor, clamped into [0, T]) or None (= audio.num_frames(length, framing)); batch_size: B >= 1.
    framing: an audio.Framing, or None for Framing() -- both of which run the entry specialised for 256 / 128 / hamming.
    Returns (terms, grad): terms torch.float64 [N, 3] = (wave_sse, si_sdr, valid) per utterance, unweighted; grad float32
    [N, T, 129] = d(wave_sse / B * sum wave_sse_n - si_sdr / B * sum_valid si_sdr_n) / d mag, or None with grad=False.  The
    spectral weight plays no part here.  With objective.mr_stft > 0 (rced_wave_loss_mr, always the general kernels) terms is
    [N, 5] = (wave_sse, si_sdr, valid, mr_stft, mr_valid) and grad includes + mr_stft / B * sum_valid mr_stft_n.
    Current stream, asynchronous."""
    import torch
    if not isinstance(objective, WaveObjective):
        raise ValueError("objective must be an audio.WaveObjective, got %r" % (objective,))
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("batch_size must be a whole number >= 1, got %r" % (batch_size,))
    from .audio import _general
    fr = _general(framing)
    if not (hasattr(mag, "is_cuda") and mag.is_cuda):
        raise ValueError("mag must be a CUDA/HIP tensor [N, T, 129]")
    if mag.dim() == 4:
        mag = mag.squeeze(-1)
    mag = mag.float().contiguous()
    ph = torch.view_as_real(phase.to(torch.complex64).contiguous()).contiguous()
    n, t = int(mag.shape[0]), int(mag.shape[1]) if mag.dim() > 1 else 0
    if tuple(mag.shape) != (n, t, BINS) or tuple(ph.shape) != (n, t, BINS, 2) or ph.device != mag.device:
        raise ValueError("mag must be [N, T, 129], phase [N, T, 129] complex, on one device")
    dev = mag.device
    clean = _args.rows(clean, "clean")
    if int(clean.shape[0]) != n or clean.device != dev:
        raise ValueError("clean must hold N = %d rows on %s" % (n, dev))
    lens = _args.host_ints(lengths, n, "lengths")
    if lens is None or any(v < 0 or v > int(clean.shape[1]) for v in lens):
        raise ValueError("lengths must hold N values in [0, %d]" % int(clean.shape[1]))
    ldev = torch.tensor(lens, dtype=torch.int32, device=dev)
    fdev = None
    if frames is not None:
        if hasattr(frames, "is_cuda") and frames.is_cuda:
            fdev = frames.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            if int(fdev.shape[0]) != n:
                raise ValueError("frames must hold N = %d values, got %d" % (n, int(fdev.shape[0])))
        else:
            fdev = torch.tensor(_args.host_ints(frames, n, "frames"), dtype=torch.int32, device=dev)
    mr = objective.mr_stft > 0.0
    terms = torch.empty((n, 5 if mr else 3), dtype=torch.float64, device=dev)
    g = torch.empty((n, t, BINS), dtype=torch.float32, device=dev) if grad else None
    if n and mr:
        from .audio import Framing
        at = fr if fr is not None else Framing()
        _lib.check(_lib.load().rced_wave_loss_mr(mag.data_ptr() if t else None, ph.data_ptr() if t else None, _args.ptr(fdev),
                                                 clean.data_ptr(), _args.row_stride(clean), ldev.data_ptr(), n, t, at.window, at.stride,
                                                 at.code, objective.wave_sse, objective.si_sdr, int(objective.skip_edges),
                                                 1.0 / float(batch_size), ctypes.byref(objective.mr_args()), terms.data_ptr(), _args.ptr(g),
                                                 dev.index, _args.current_stream(dev)))
    elif n and fr is not None:
        _lib.check(_lib.load().rced_wave_loss_fr(mag.data_ptr() if t else None, ph.data_ptr() if t else None, _args.ptr(fdev),
                                                 clean.data_ptr(), _args.row_stride(clean), ldev.data_ptr(), n, t, fr.window, fr.stride,
                                                 fr.code, objective.wave_sse, objective.si_sdr, int(objective.skip_edges),
                                                 1.0 / float(batch_size), terms.data_ptr(), _args.ptr(g), dev.index,
                                                 _args.current_stream(dev)))
    elif n:
        _lib.check(_lib.load().rced_wave_loss(mag.data_ptr() if t else None, ph.data_ptr() if t else None, _args.ptr(fdev),
                                              clean.data_ptr(), _args.row_stride(clean), ldev.data_ptr(),
                                              n, t, objective.wave_sse, objective.si_sdr, int(objective.skip_edges),
                                              1.0 / float(batch_size), terms.data_ptr(), _args.ptr(g), dev.index,
                                              _args.current_stream(dev)))
    return terms, g



def mr_stft_batch(est, ref, lengths, resolutions=None, grad=False, weight=1.0, batch_size=1):
    """The multi-resolution STFT term between two ragged row sets, on the device (rced.h, rced_mr_stft).
    est, ref [N, >= max length] float32 torch.cuda tensors with contiguous rows (views of wider buffers are fine); lengths: N sample
    counts in [0, the narrower width]; resolutions: a tuple of 1 to 4 audio.Framing, None meaning audio.MR_STFT_8K.
    Returns (terms, g): terms torch.float64 [N, 2 + 3 K] = (term, valid, then sc_r, lsd_r, J_r per resolution), unweighted; g float32
    [N, est's width] = d(weight / batch_size * sum_n term_n) / d est with zeros from the length on, or None with grad=False.
    Current stream, asynchronous."""
    import torch
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("batch_size must be a whole number >= 1, got %r" % (batch_size,))
    a = mr_args(resolutions, weight)
    est, ref = _args.rows(est, "est"), _args.rows(ref, "ref")
    n = int(est.shape[0])
    if int(ref.shape[0]) != n or ref.device != est.device:
        raise ValueError("ref must hold N = %d rows on %s" % (n, est.device))
    width = min(int(est.shape[1]), int(ref.shape[1]))
    lens = _args.host_ints(lengths, n, "lengths")
    if lens is None or any(v < 0 or v > width for v in lens):
        raise ValueError("lengths must hold N values in [0, %d]" % width)
    dev = est.device
    ldev = torch.tensor(lens, dtype=torch.int32, device=dev)
    terms = torch.empty((n, 2 + 3 * a.n_res), dtype=torch.float64, device=dev)
    g = torch.empty((n, int(est.shape[1])), dtype=torch.float32, device=dev) if grad else None
    if n:
        # the gradient's rows are est's width apart; est's own rows may be further apart (a view)
        e = est if not grad or _args.row_stride(est) == int(est.shape[1]) else est.contiguous()
        _lib.check(_lib.load().rced_mr_stft(e.data_ptr(), _args.row_stride(e), ref.data_ptr(), _args.row_stride(ref), ldev.data_ptr(), n,
                                            ctypes.byref(a), 1.0 / float(batch_size), terms.data_ptr(), _args.ptr(g), dev.index,
                                            _args.current_stream(dev)))
    return terms, g
