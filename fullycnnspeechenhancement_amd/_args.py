"""Argument plumbing that the host-side entry points share (audio.py, evaluation.py, arena.py, streaming.py, engine.py): one
copy of every check and conversion between what a caller hands over and what the C ABI takes.  Also the front end's
constants, so that every module above can have them without importing another."""

import numpy as np

from . import _lib

FRAME, STEP, BINS, SAMPLE_RATE = 256, 128, 129, 8000

PCM_DTYPES = ("float32", "int16")
_PCM_CODES = {"float32": _lib.PCM_F32, "int16": _lib.PCM_S16}     # rced.h: RCED_PCM_F32, RCED_PCM_S16


def pcm_format(name, what="dtype"):
    """A sample format's name -> (torch dtype, numpy dtype, RCED_PCM_* code)."""
    import torch
    if name not in PCM_DTYPES:
        raise ValueError("%s must be 'float32' or 'int16', got %r" % (what, name))
    return getattr(torch, name), np.dtype(name), _PCM_CODES[name]


REBUILDS = ("reference", "ola")     # AudioReBuild.rebuild_audio as shipped (rced_istft) / weighted overlap-add (rced_istft_ola)


def check_rebuild(rebuild, kernels="x6"):
    """The `rebuild` keyword of everything that turns spectra into audio, checked before any device work.  Returns it."""
    if rebuild not in REBUILDS:
        raise ValueError("rebuild must be 'reference' (AudioReBuild as the reference ships it) or 'ola' (weighted overlap-add), got %r"
                         % (rebuild,))
    if rebuild == "ola" and kernels == "f32":
        raise ValueError("rebuild='ola' has no kernels='f32' form (the fp32-MFMA comparators cover the reference rebuild only)")
    return rebuild


def pcm_name(dtype):
    """The name of a torch or numpy dtype if it is a sample format, else None."""
    name = str(dtype).rsplit(".", 1)[-1]
    return name if name in PCM_DTYPES else None


def host_ints(values, n=None, what="values"):
    """A list, ndarray or tensor (None passes through) as a list of Python ints; with n, it must hold that many."""
    if values is None:
        return None
    out = [int(v) for v in (values.tolist() if hasattr(values, "tolist") else values)]
    if n is not None and len(out) != n:
        raise ValueError("%s must hold N = %d values, got %d" % (what, n, len(out)))
    return out


def rows(x, what):
    """A float32 CUDA/HIP matrix whose rows are contiguous; the row stride may be wider than the row (a view of a padded buffer)."""
    if not (hasattr(x, "is_cuda") and x.is_cuda and x.dim() == 2):
        raise ValueError("%s must be a CUDA/HIP tensor [N, L]" % what)
    x = x.float()
    if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def row_stride(x):
    return int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1])


def ptr(t):
    """A tensor's address as the C ABI takes it; None is the null pointer."""
    return t.data_ptr() if t is not None else None


def scoring_args(clean, estimate, lengths):
    """What rced_sdr and rced_stoi both take: (clean, estimate, n, device, clean's row stride, estimate's row stride, the
    lengths on the device or None), from clean [N, Lc], estimate [N, Le] and N lengths in [0, min(Lc, Le)] or None."""
    import torch
    clean, estimate = rows(clean, "clean"), rows(estimate, "estimate")
    n = int(clean.shape[0])
    if int(estimate.shape[0]) != n or estimate.device != clean.device:
        raise ValueError("clean and estimate must hold the same number of utterances on one device")
    dev = clean.device
    cap = min(int(clean.shape[1]), int(estimate.shape[1]))
    lens = host_ints(lengths, n, "lengths")
    if lens is not None and any(v < 0 or v > cap for v in lens):
        raise ValueError("lengths must lie in [0, %d]" % cap)
    sc, se = row_stride(clean), row_stride(estimate)
    if lens is None and min(sc, se) != cap:
        lens = [cap] * n                                  # a strided view: the row's width, not its stride, bounds it
    ldev = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    return clean, estimate, n, dev, sc, se, ldev


def check_out(out, n, L, dev, dtype, exact=False):
    """`out`, the matrix a caller gave to write into: a [n, >= L] tensor of torch `dtype` on `dev` with contiguous rows (a view
    of a wider or taller buffer is fine); exact: [n, L] and contiguous as a whole.  Returns it."""
    ok = (hasattr(out, "is_cuda") and out.is_cuda and out.device == dev and out.dtype == dtype and out.dim() == 2
          and int(out.shape[0]) == n and int(out.shape[1]) >= L
          and (out.shape[1] <= 1 or out.stride(1) == 1) and (n <= 1 or out.stride(0) >= out.shape[1]))
    if ok and exact:
        ok = int(out.shape[1]) == L and out.is_contiguous()
    if not ok:
        got = ("%s %s with strides %s on %s" % (out.dtype, tuple(out.shape), tuple(out.stride()), out.device)
               if hasattr(out, "is_cuda") else repr(type(out)))
        raise ValueError("out must be a %s%s [N = %d, %s%d] matrix on %s with contiguous rows, got %s"
                         % ("contiguous " if exact else "", pcm_name(dtype) or dtype, n, "" if exact else ">= ", L, dev, got))
    return out


def to_device(x, dtype, device, what):
    """An ndarray (or anything numpy takes), or a tensor on cuda:`device`, as a contiguous tensor of torch `dtype` there; a
    tensor that lives anywhere else is refused."""
    import torch
    if hasattr(x, "is_cuda"):
        if not x.is_cuda or x.device.index != device:
            raise ValueError("%s must live on cuda:%d (or be a numpy array), got a tensor on %s" % (what, device, x.device))
        return x.to(dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x, dtype=str(dtype).rsplit(".", 1)[-1]), device="cuda:%d" % device)


def current_stream(dev):
    """The handle of torch's current stream on a device, as the C ABI takes it."""
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def keep_alive(stream, *tensors):
    """Keeps the memory of temporaries (None is skipped) that the work just queued on `stream`, a torch stream, reads until the
    stream has passed."""
    for t in tensors:
        if t is not None:
            t.record_stream(stream)


def pcm_units(shape, lanes, channels, unit=1):
    """How many units of `unit` frames a lane the PCM of `shape` holds -- [lanes, n * unit] interleaved ([lanes, n * unit * channels])
    or [lanes, n * unit, channels] --, or -1 where it is neither."""
    shape = tuple(shape)
    per = unit * (channels if len(shape) == 2 else 1)
    n = shape[1] // per if len(shape) in (2, 3) else -1
    return n if shape in ((lanes, n * unit * channels), (lanes, n * unit, channels)) else -1


def pack_tails(lanes_total, unit, channels, np_dtype, lanes, tails):
    """What a finish uploads: (tail [lanes_total, unit(, channels)] of np_dtype, counts int32 [lanes_total]) with tails[i], the
    last 0 .. unit - 1 frames of lane lanes[i] ([frames], [frames * channels] or [frames, channels]; arrays or tensors), in its
    lane's row and its frame count beside it; the lanes not listed count -1.  Touches no device."""
    lanes = host_ints(lanes)
    if len(lanes) != len(tails) or len(set(lanes)) != len(lanes) or any(v < 0 or v >= lanes_total for v in lanes):
        raise ValueError("lanes must be distinct indices in [0, %d), one tail each, got lanes %r and %d tails"
                         % (lanes_total, lanes, len(tails)))
    tail = np.zeros((lanes_total, unit) + ((channels,) if channels > 1 else ()), np_dtype)
    counts = np.full((lanes_total,), -1, np.int32)
    for lane, t in zip(lanes, tails):
        t = (t.detach().cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)).astype(np_dtype, copy=False)
        if t.size % channels:
            raise ValueError("a tail holds whole frames of %d channels, lane %d's has %d values" % (channels, lane, t.size))
        frames = t.size // channels
        if frames >= unit:
            raise ValueError("a tail holds fewer than %d frames (push whole units first), lane %d's has %d" % (unit, lane, frames))
        tail[lane, :frames] = t.reshape((frames,) + tail.shape[2:])
        counts[lane] = frames
    return tail, counts
