"""Rows cut out of a device-resident corpus, and resampling on the device, over the C ABI.  audio.py
re-exports every public name here."""

import numpy as np

from . import _args, _lib
from ._args import PCM_DTYPES  # noqa: F401


def _arena(arena, flat):
    """The checks both entry points make of their source buffer; returns its RCED_PCM_* code."""
    if not (hasattr(arena, "is_cuda") and arena.is_cuda and (arena.dim() == 1 or not flat) and arena.is_contiguous()
            and _args.pcm_name(arena.dtype)):
        raise ValueError("arena must be a contiguous %sCUDA/HIP tensor of int16 or float32" % ("1-D " if flat else ""))
    return _args.pcm_format(_args.pcm_name(arena.dtype))[2]


def gather_pcm(arena, begins, counts, L=None, out=None):
    """Rows of a zero-padded batch cut out of a device-resident corpus (rced_gather_pcm).
    arena: torch.cuda int16 or float32 [S], contiguous; begins [N]: absolute sample indices; counts [N]: samples per row.
    Row n = arena[begins[n] : begins[n] + counts[n]] as float32 (int16 / 32768, exact), zeros up to column L.
    L: the row width (None = the largest count, rounded up to a multiple of 4 so that every row starts 16-byte aligned);
    out: a float32 [N, >= L] device matrix with contiguous rows to write into (columns past L are left alone) -- a view of a
    wider or taller buffer is fine, nothing is copied.  Every range must lie inside the arena and every count in [0, L]:
    ValueError otherwise (the library would clamp).  Returns the [N, L] rows (a view of `out` when given), current stream."""
    import torch
    code = _arena(arena, True)
    dev, S = arena.device, int(arena.shape[0])
    b = _args.host_ints(begins, None, "begins")
    n = len(b)
    c = _args.host_ints(counts, n, "counts")
    if L is None:
        L = out.shape[1] if out is not None else (max(c + [0]) + 3) // 4 * 4
    L = int(L)
    for i in range(n):
        if c[i] < 0 or c[i] > L:
            raise ValueError("counts[%d] = %d outside [0, L = %d]" % (i, c[i], L))
        if b[i] < 0 or b[i] + c[i] > S:
            raise ValueError("row %d: samples [%d, %d) leave the arena [0, %d)" % (i, b[i], b[i] + c[i], S))
    out = torch.empty((n, L), dtype=torch.float32, device=dev) if out is None else _args.check_out(out, n, L, dev, torch.float32)
    if n and L:
        bdev = torch.tensor(b, dtype=torch.int64, device=dev)
        cdev = torch.tensor(c, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().rced_gather_pcm(arena.data_ptr(), code, S, bdev.data_ptr(), cdev.data_ptr(), n, L, out.data_ptr(),
                                               _args.row_stride(out), dev.index, _args.current_stream(dev)))
    return out[:, :L]


def resample_length(n, sr_orig, sr_new):
    """Output samples of n input frames: int(n * (float(sr_new) / sr_orig)) (rced_resample_length; needs no GPU)."""
    m = int(_lib.load().rced_resample_length(int(n), int(sr_orig), int(sr_new)))
    if m < 0:
        raise ValueError("resample_length(%r, %r, %r): a negative length or a rate that is not positive" % (n, sr_orig, sr_new))
    return m


def resample_taps(sr_orig, sr_new):
    """The phase table of a ratio (rced_resample_taps; needs no GPU): (p, q, left, table float64 [p, width]),
    table[r, c] the weight of input frame n0 - left + c in an output of phase r.  A refused ratio raises RcedError."""
    import ctypes
    lib = _lib.load()
    v = [ctypes.c_int() for _ in range(4)]
    _lib.check(lib.rced_resample_taps(int(sr_orig), int(sr_new), v[0], v[1], v[2], v[3], None, 0))
    p, q, left, width = (int(x.value) for x in v)
    table = np.empty((p, width), np.float64)
    _lib.check(lib.rced_resample_taps(int(sr_orig), int(sr_new), None, None, None, None,
                                      table.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), table.size))
    return p, q, left, table


def resample_arena(arena, begins, counts, channels, sr_orig, sr_new, L=None, out=None, out_begins=None, dtype="float32"):
    """Ranges of a device-resident buffer of interleaved frames, resampled from sr_orig to sr_new (rced_resample).
    arena: torch.cuda int16 or float32, contiguous, `channels` values per frame (any shape: it is read flat); begins [N],
    counts [N]: first frame and frames of every row.  int16 samples count / 32768, the channels are averaged.
    Row n has resample_length(counts[n], sr_orig, sr_new) outputs.
    Row mode (out_begins None): returns (rows [N, L], out_lengths), zero past every row's length up to L (None = the longest
    output, or out's width); out: a [N, >= L] device matrix of `dtype` with contiguous rows to write into.
    Packed mode (out_begins [N]): row n's outputs go to out[out_begins[n]:], a contiguous 1-D device tensor of `dtype` that
    must hold them -- a corpus arena, say --, nothing else is written; returns (out, out_lengths).
    dtype: "float32", or "int16" = clip(rint(y * 32768)).  Every range must lie inside its buffer: ValueError otherwise (the
    library would clamp).  Current stream."""
    import torch
    code = _arena(arena, False)
    tdtype, _, out_code = _args.pcm_format(dtype)
    channels, sr_orig, sr_new = int(channels), int(sr_orig), int(sr_new)
    if channels < 1 or sr_orig < 1 or sr_new < 1:
        raise ValueError("channels and both rates must be positive, got %d, %d -> %d" % (channels, sr_orig, sr_new))
    dev, frames = arena.device, int(arena.numel()) // channels
    b = _args.host_ints(begins, None, "begins")
    n = len(b)
    c = _args.host_ints(counts, n, "counts")
    for i in range(n):
        if c[i] < 0 or b[i] < 0 or b[i] + c[i] > frames:
            raise ValueError("row %d: frames [%d, %d) leave the arena [0, %d)" % (i, b[i], b[i] + c[i], frames))
    lens = [resample_length(v, sr_orig, sr_new) for v in c]
    if out_begins is None:
        if L is None:
            L = int(out.shape[1]) if out is not None else max(lens + [0])
        L = int(L)
        if any(v > L for v in lens):
            raise ValueError("the longest row gives %d samples, L = %d" % (max(lens), L))
        out = torch.empty((n, L), dtype=tdtype, device=dev) if out is None else _args.check_out(out, n, L, dev, tdtype)
        odev, stride, result = None, _args.row_stride(out), out[:, :L]
    else:
        ob = _args.host_ints(out_begins, n, "out_begins")
        if not (hasattr(out, "is_cuda") and out.is_cuda and out.device == dev and out.dtype == tdtype and out.dim() == 1
                and out.is_contiguous()):
            raise ValueError("packed mode needs out: a contiguous 1-D %s tensor on the arena's device" % dtype)
        for i in range(n):
            if ob[i] < 0 or ob[i] + lens[i] > int(out.shape[0]):
                raise ValueError("row %d: outputs [%d, %d) leave out [0, %d)" % (i, ob[i], ob[i] + lens[i], int(out.shape[0])))
        L = max(lens + [0])
        odev, stride, result = torch.tensor(ob, dtype=torch.int64, device=dev), 0, out
    if n and L:
        bdev = torch.tensor(b, dtype=torch.int64, device=dev)
        cdev = torch.tensor(c, dtype=torch.int32, device=dev)
        _lib.check(_lib.load().rced_resample(arena.data_ptr(), code, channels, frames, bdev.data_ptr(), cdev.data_ptr(), n, sr_orig,
                                             sr_new, out.data_ptr(), out_code, odev.data_ptr() if odev is not None else None, stride,
                                             L, dev.index, _args.current_stream(dev)))
    return result, lens


def resample_batch(pcm, sr_orig, sr_new, lengths=None, out=None, dtype="float32", device=0):
    """A batch of signals from sr_orig to sr_new on the device: what librosa.load(sr=sr_new) does to a file's samples, as
    DESIGN.md 3.4f defines it.  pcm: [N, L] (mono) or [N, L, C] (interleaved channels, averaged), int16 (counted / 32768) or
    float; a torch.cuda tensor, or an array (uploaded to `device`); a 1-D signal is one row.  lengths: frames per row or
    None (= L each).  Returns (rows [N, Lout] of `dtype` on the device, zero past each row's length; out_lengths).
    out: as in resample_arena's row mode."""
    import torch
    if not hasattr(pcm, "is_cuda"):
        a = np.asarray(pcm)
        pcm = _args.to_device(a, torch.int16 if a.dtype == np.int16 else torch.float32, device, "pcm")
    if pcm.dim() == 1:
        pcm = pcm[None]
    if not (pcm.is_cuda and pcm.dim() in (2, 3)):
        raise ValueError("pcm must be [N, L] or [N, L, C], on the device or an array")
    if pcm.dtype != torch.int16:
        pcm = pcm.float()
    pcm = pcm.contiguous()
    n, L = int(pcm.shape[0]), int(pcm.shape[1])
    channels = int(pcm.shape[2]) if pcm.dim() == 3 else 1
    lens = _args.host_ints(lengths, n, "lengths") if lengths is not None else [L] * n
    if any(v < 0 or v > L for v in lens):
        raise ValueError("lengths must lie in [0, %d]" % L)
    return resample_arena(pcm, [i * L for i in range(n)], lens, channels, sr_orig, sr_new, out=out, dtype=dtype)
