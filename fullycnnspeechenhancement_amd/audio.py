"""Host-side mirror of the reference's STFT front-end and ISTFT rebuild, over the C ABI.

Reference surface kept:
    AudioFeature(windows_name).compute_spectrogram(signal, sample_rate, window_s, stride_s, nfft, use_complex)
        data_utils/audio_feature.py:12-44  (+ power_spectrum :102-110, divide_phase :113-115)
    AudioReBuild(windows_name, nfft).rebuild_audio(sig_length_list, spec, phase, sample_rate, windows_ms, stride_ms)
        model_utils/utils.py:93-183
Only the configuration the reference's cfgs use is built (8 kHz, 32 ms / 16 ms, hamming, rfft 256); anything
else raises.  The batch functions `stft_batch` / `istft_batch` keep everything on the device
(torch.cuda tensors in and out) so that STFT -> CNN -> ISTFT runs without leaving HBM.
"""

import numpy as np

from . import _lib

FRAME, STEP, BINS, SAMPLE_RATE = 256, 128, 129, 8000


def num_frames(length):
    return int(_lib.load().rced_stft_num_frames(int(length)))


KERNELS = {"x6": 1, "f32": 0}     # rced.h: RCED_AUDIO_X6 (the product: three-part bf16 products), RCED_AUDIO_F32 (the fp32-MFMA comparators)


def _kernels(name):
    if name not in KERNELS:
        raise ValueError("kernels must be 'x6' (the product) or 'f32' (the fp32-MFMA comparator), got %r" % (name,))
    return KERNELS[name]


def _check_cfg(sample_rate, window_s, stride_s, nfft=None):
    if int(round(window_s * sample_rate)) != FRAME or int(round(stride_s * sample_rate)) != STEP:
        raise ValueError("only 256-sample windows with a 128-sample stride are built (8 kHz, 32 ms / 16 ms)")
    if nfft is not None and nfft != 256:
        raise ValueError("only rfft(256) -> 129 bins is built (data_loader.py:59 hard-codes it)")


def stft_batch(pcm, lengths=None, frames=None, with_phase=True, kernels="x6"):
    """pcm: torch.cuda float32 [N, L]; lengths: per-utterance sample counts (list / tensor) or None.
    Returns (mag [N, T, 129, 1], phase [N, T, 129] complex64 or None); T = frames or the batch maximum
    (zero-padded like DataLoader.padding_batch, data_loader.py:198-209)."""
    import torch
    if not (pcm.is_cuda and pcm.dim() == 2):
        raise ValueError("pcm must be a CUDA/HIP tensor [N, L]")
    pcm = pcm.float().contiguous()
    n, L = int(pcm.shape[0]), int(pcm.shape[1])
    dev = pcm.device
    if lengths is None:
        lens = [L] * n
        ldev = None
    else:
        lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        if len(lens) != n or any(v < 1 or v > L for v in lens):
            raise ValueError("lengths must hold N values in [1, L]")
        ldev = torch.tensor(lens, dtype=torch.int32, device=dev)
    t = int(frames) if frames is not None else (max(num_frames(v) for v in lens) if n else 0)
    mag = torch.empty((n, t, BINS, 1), dtype=torch.float32, device=dev)
    ph = torch.empty((n, t, BINS, 2), dtype=torch.float32, device=dev) if with_phase else None
    if n and t:
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().rced_stft_ex(pcm.data_ptr(), ldev.data_ptr() if ldev is not None else None, n, L, t,
                                            mag.data_ptr(), ph.data_ptr() if ph is not None else None, dev.index, st, _kernels(kernels)))
    return mag, (torch.view_as_complex(ph) if ph is not None else None)


def istft_batch(mag, phase, nfft=512, kernels="x6"):
    """mag [N, T, 129(,1)] float32, phase [N, T, 129] complex64 (torch.cuda) -> audio [N, (T+1)*128]."""
    import torch
    if mag.dim() == 4:
        mag = mag.squeeze(-1)
    mag = mag.float().contiguous()
    ph = torch.view_as_real(phase.to(torch.complex64).contiguous()).contiguous()
    n, t = int(mag.shape[0]), int(mag.shape[1])
    if tuple(mag.shape) != (n, t, BINS) or tuple(ph.shape) != (n, t, BINS, 2):
        raise ValueError("mag must be [N, T, 129], phase [N, T, 129] complex")
    out = torch.empty((n, (t + 1) * STEP), dtype=torch.float32, device=mag.device)
    if n and t:
        st = torch.cuda.current_stream(mag.device).cuda_stream
        _lib.check(_lib.load().rced_istft_ex(mag.data_ptr(), ph.data_ptr(), n, t, int(nfft), out.data_ptr(),
                                             mag.device.index, st, _kernels(kernels)))
    return out


def _host_ints(values, n, what):
    if values is None:
        return None
    out = [int(v) for v in (values.tolist() if hasattr(values, "tolist") else values)]
    if len(out) != n:
        raise ValueError("%s must hold N = %d values, got %d" % (what, n, len(out)))
    return out


def _rows(x, what):
    """A float32 CUDA/HIP matrix whose rows are contiguous; the row stride may be wider than the row (a view of a padded buffer)."""
    if not (hasattr(x, "is_cuda") and x.is_cuda and x.dim() == 2):
        raise ValueError("%s must be a CUDA/HIP tensor [N, L]" % what)
    x = x.float()
    if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x


def _row_stride(x):
    return int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1])


def sdr_batch(clean, estimate, lengths=None):
    """SDR.sdr (model_utils/utils.py:68-86) per utterance on the device: clean [N, Lc], estimate [N, Le] torch.cuda float32,
    row n holding utterance n from column 0 (the estimate may be istft_batch's [N, (T+1)*128] buffer as it is: the length
    trims, nothing is copied); lengths: per-utterance sample counts in [0, min(Lc, Le)] or None (= min(Lc, Le) each).
    Returns torch.float64 [N] (dB) on the device, current stream."""
    import torch
    clean, estimate = _rows(clean, "clean"), _rows(estimate, "estimate")
    n = int(clean.shape[0])
    if int(estimate.shape[0]) != n or estimate.device != clean.device:
        raise ValueError("clean and estimate must hold the same number of utterances on one device")
    dev = clean.device
    cap = min(int(clean.shape[1]), int(estimate.shape[1]))
    lens = _host_ints(lengths, n, "lengths")
    if lens is not None and any(v < 0 or v > cap for v in lens):
        raise ValueError("lengths must lie in [0, %d]" % cap)
    sc, se = _row_stride(clean), _row_stride(estimate)
    if lens is None and min(sc, se) != cap:
        lens = [cap] * n                                  # a strided view: the row's width, not its stride, bounds it
    ldev = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    out = torch.empty((n,), dtype=torch.float64, device=dev)
    if n:
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().rced_sdr(clean.data_ptr(), sc, estimate.data_ptr(), se,
                                        ldev.data_ptr() if ldev is not None else None, n, out.data_ptr(), None, dev.index, st))
    return out


STOI_RATES = (8000, 10000)


def stoi_batch(clean, estimate, lengths=None, sample_rate=8000, detail=False):
    """STOI (Taal et al. 2011; the reference's pystoi.stoi(clean, denoise, sr, extended=False), tester.py:92-167) per utterance
    on the device, as DESIGN.md "STOI" specifies it.  clean [N, Lc], estimate [N, Le], lengths: as in sdr_batch (the estimate
    may be istft_batch's buffer as it is).  sample_rate: 8000 (resampled to 10 kHz on the device) or 10000.
    Returns torch.float64 [N] on the device, current stream; with detail=True also torch.int32 [N, 3]: frames at 10 kHz,
    frames kept by the 40 dB silent-frame removal, 30-frame segments (0 segments: the score is 1e-5)."""
    import torch
    if int(sample_rate) not in STOI_RATES:
        raise ValueError("sample_rate must be 8000 or 10000, got %r" % (sample_rate,))
    clean, estimate = _rows(clean, "clean"), _rows(estimate, "estimate")
    n = int(clean.shape[0])
    if int(estimate.shape[0]) != n or estimate.device != clean.device:
        raise ValueError("clean and estimate must hold the same number of utterances on one device")
    dev = clean.device
    cap = min(int(clean.shape[1]), int(estimate.shape[1]))
    lens = _host_ints(lengths, n, "lengths")
    if lens is not None and any(v < 0 or v > cap for v in lens):
        raise ValueError("lengths must lie in [0, %d]" % cap)
    sc, se = _row_stride(clean), _row_stride(estimate)
    if lens is None and min(sc, se) != cap:
        lens = [cap] * n                                  # a strided view: the row's width, not its stride, bounds it
    ldev = torch.tensor(lens, dtype=torch.int32, device=dev) if lens is not None else None
    out = torch.empty((n,), dtype=torch.float64, device=dev)
    det = torch.empty((n, 3), dtype=torch.int32, device=dev) if detail else None
    if n:
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().rced_stoi(clean.data_ptr(), sc, estimate.data_ptr(), se,
                                         ldev.data_ptr() if ldev is not None else None, n, int(sample_rate), out.data_ptr(),
                                         det.data_ptr() if det is not None else None, dev.index, st))
    return (out, det) if detail else out


def gains_needed(len_speech, len_noise):
    """How many of add_noise's uniform(0, 2) draws can reach the first len_speech samples: bit_length((ls - 1) // ln)."""
    if len_speech < len_noise or len_speech < 1:
        return 0
    return int((len_speech - 1) // len_noise).bit_length()


def gather_pcm(arena, begins, counts, L=None, out=None):
    """Rows of a zero-padded batch cut out of a device-resident corpus (rced_gather_pcm).
    arena: torch.cuda int16 or float32 [S], contiguous; begins [N]: absolute sample indices; counts [N]: samples per row.
    Row n = arena[begins[n] : begins[n] + counts[n]] as float32 (int16 / 32768, exact), zeros up to column L.
    L: the row width (None = the largest count, rounded up to a multiple of 4 so that every row starts 16-byte aligned);
    out: a float32 [N, >= L] device matrix with contiguous rows to write into (columns past L are left alone) -- a view of a
    wider or taller buffer is fine, nothing is copied.  Every range must lie inside the arena and every count in [0, L]:
    ValueError otherwise (the library would clamp).  Returns the [N, L] rows (a view of `out` when given), current stream."""
    import torch
    if not (hasattr(arena, "is_cuda") and arena.is_cuda and arena.dim() == 1 and arena.is_contiguous()
            and arena.dtype in (torch.int16, torch.float32)):
        raise ValueError("arena must be a contiguous 1-D CUDA/HIP tensor of int16 or float32")
    dev, S = arena.device, int(arena.shape[0])
    b = [int(v) for v in (begins.tolist() if hasattr(begins, "tolist") else begins)]
    c = _host_ints(counts, len(b), "counts")
    n = len(b)
    if L is None:
        L = out.shape[1] if out is not None else (max(c + [0]) + 3) // 4 * 4
    L = int(L)
    for i in range(n):
        if c[i] < 0 or c[i] > L:
            raise ValueError("counts[%d] = %d outside [0, L = %d]" % (i, c[i], L))
        if b[i] < 0 or b[i] + c[i] > S:
            raise ValueError("row %d: samples [%d, %d) leave the arena [0, %d)" % (i, b[i], b[i] + c[i], S))
    if out is None:
        out = torch.empty((n, L), dtype=torch.float32, device=dev)
    elif not (hasattr(out, "is_cuda") and out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.dim() == 2
              and int(out.shape[0]) == n and int(out.shape[1]) >= L
              and (out.shape[1] <= 1 or out.stride(1) == 1) and (n <= 1 or out.stride(0) >= out.shape[1])):
        raise ValueError("out must be a float32 [N = %d, >= %d] matrix on the arena's device with contiguous rows" % (n, L))
    if n and L:
        bdev = torch.tensor(b, dtype=torch.int64, device=dev)
        cdev = torch.tensor(c, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().rced_gather_pcm(arena.data_ptr(), _lib.PCM_S16 if arena.dtype == torch.int16 else _lib.PCM_F32, S,
                                               bdev.data_ptr(), cdev.data_ptr(), n, L, out.data_ptr(), _row_stride(out), dev.index,
                                               st))
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


PCM_DTYPES = ("float32", "int16")


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
    if not (hasattr(arena, "is_cuda") and arena.is_cuda and arena.is_contiguous() and arena.dtype in (torch.int16, torch.float32)):
        raise ValueError("arena must be a contiguous CUDA/HIP tensor of int16 or float32")
    if dtype not in PCM_DTYPES:
        raise ValueError("dtype must be 'float32' or 'int16', got %r" % (dtype,))
    channels, sr_orig, sr_new = int(channels), int(sr_orig), int(sr_new)
    if channels < 1 or sr_orig < 1 or sr_new < 1:
        raise ValueError("channels and both rates must be positive, got %d, %d -> %d" % (channels, sr_orig, sr_new))
    tdtype = torch.float32 if dtype == "float32" else torch.int16
    dev, frames = arena.device, int(arena.numel()) // channels
    b = [int(v) for v in (begins.tolist() if hasattr(begins, "tolist") else begins)]
    c = _host_ints(counts, len(b), "counts")
    n = len(b)
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
        if out is None:
            out = torch.empty((n, L), dtype=tdtype, device=dev)
        elif not (hasattr(out, "is_cuda") and out.is_cuda and out.device == dev and out.dtype == tdtype and out.dim() == 2
                  and int(out.shape[0]) == n and int(out.shape[1]) >= L
                  and (out.shape[1] <= 1 or out.stride(1) == 1) and (n <= 1 or out.stride(0) >= out.shape[1])):
            raise ValueError("out must be a %s [N = %d, >= %d] matrix on the arena's device with contiguous rows" % (dtype, n, L))
        odev, stride, result = None, _row_stride(out), out[:, :L]
    else:
        ob = _host_ints(out_begins, n, "out_begins")
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
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().rced_resample(arena.data_ptr(), _lib.PCM_S16 if arena.dtype == torch.int16 else _lib.PCM_F32, channels,
                                             frames, bdev.data_ptr(), cdev.data_ptr(), n, sr_orig, sr_new, out.data_ptr(),
                                             _lib.PCM_F32 if dtype == "float32" else _lib.PCM_S16,
                                             odev.data_ptr() if odev is not None else None, stride, L, dev.index, st))
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
        a = np.ascontiguousarray(a, dtype=np.int16 if a.dtype == np.int16 else np.float32)
        pcm = torch.as_tensor(a, device="cuda:%d" % device)
    if pcm.dim() == 1:
        pcm = pcm[None]
    if not (pcm.is_cuda and pcm.dim() in (2, 3)):
        raise ValueError("pcm must be [N, L] or [N, L, C], on the device or an array")
    if pcm.dtype != torch.int16:
        pcm = pcm.float()
    pcm = pcm.contiguous()
    n, L = int(pcm.shape[0]), int(pcm.shape[1])
    channels = int(pcm.shape[2]) if pcm.dim() == 3 else 1
    lens = _host_ints(lengths, n, "lengths") if lengths is not None else [L] * n
    if any(v < 0 or v > L for v in lens):
        raise ValueError("lengths must lie in [0, %d]" % L)
    return resample_arena(pcm, [i * L for i in range(n)], lens, channels, sr_orig, sr_new, out=out, dtype=dtype)


def mix_snr_batch(speech, noise, snr, speech_lengths=None, noise_lengths=None, starts=None, gains=None, out=None):
    """AudioParser.add_noise (data_utils/data_loader.py:35-52) for a batch on the device, in closed form.
    speech [N, Ls], noise [N, Ln] torch.cuda float32 with per-utterance lengths (lists / tensors, or None = the full row);
    starts [N]: the crop offsets (used where the noise is longer than the speech; None = 0);
    gains [N, n_gains] float64 (array, or a list of per-utterance sequences, padded with 1): the uniform(0, 2) draws
    u_0.. (used where the speech is at least as long as the noise) -- loader.plan_noise makes both as the reference would.
    out: None, or a contiguous float32 [N, Ls] device tensor to write into (e.g. the lower half of a [2N, Ls] buffer).
    Returns mix [N, Ls] float32 on the device (0 past each speech length), current stream."""
    import torch
    speech, noise = _rows(speech, "speech").contiguous(), _rows(noise, "noise").contiguous()
    n, Ls, Ln = int(speech.shape[0]), int(speech.shape[1]), int(noise.shape[1])
    if int(noise.shape[0]) != n or noise.device != speech.device:
        raise ValueError("speech and noise must hold the same number of utterances on one device")
    dev = speech.device
    sl, nl = _host_ints(speech_lengths, n, "speech_lengths"), _host_ints(noise_lengths, n, "noise_lengths")
    if sl is not None and any(v < 0 or v > Ls for v in sl):
        raise ValueError("speech_lengths must lie in [0, %d]" % Ls)
    if nl is not None and any(v < 1 or v > Ln for v in nl):
        raise ValueError("noise_lengths must lie in [1, %d]" % Ln)
    if n and Ls and Ln < 1:
        raise ValueError("empty noise")
    ls_of = sl if sl is not None else [Ls] * n
    ln_of = nl if nl is not None else [Ln] * n
    st_host = _host_ints(starts, n, "starts")
    if st_host is not None:
        for i in range(n):
            if ls_of[i] < ln_of[i] and not 0 <= st_host[i] <= ln_of[i] - ls_of[i]:
                raise ValueError("starts[%d] = %d outside [0, %d]" % (i, st_host[i], ln_of[i] - ls_of[i]))
    if gains is not None and hasattr(gains, "is_cuda"):      # already on the device: [N, n_gains], every row complete
        gdev = gains.to(device=dev, dtype=torch.float64).reshape(n, -1).contiguous()
        have = [int(gdev.shape[1])] * n
    else:
        rows = [np.asarray(r, np.float64).reshape(-1) for r in gains] if gains is not None else [np.zeros(0)] * n
        if len(rows) != n:
            raise ValueError("gains must hold N = %d rows" % n)
        have = [r.size for r in rows]
        g = np.ones((n, max(have + [0])), np.float64)
        for i, r in enumerate(rows):
            g[i, :r.size] = r
        gdev = torch.from_numpy(g).to(dev) if g.shape[1] else None
    for i in range(n):       # the library cannot see the lengths; this side can
        if gains_needed(ls_of[i], ln_of[i]) > have[i]:
            raise _lib.RcedError(_lib.RCED_ERR_ARG, "utterance %d (speech %d, noise %d samples) needs %d gains, got %d"
                                 % (i, ls_of[i], ln_of[i], gains_needed(ls_of[i], ln_of[i]), have[i]))
    n_gains = int(gdev.shape[1]) if gdev is not None else 0
    if out is None:
        mix = torch.empty((n, Ls), dtype=torch.float32, device=dev)
    elif (hasattr(out, "is_cuda") and out.is_cuda and out.device == dev and out.dtype == torch.float32
          and tuple(out.shape) == (n, Ls) and out.is_contiguous()):
        mix = out
    else:
        raise ValueError("out must be a contiguous float32 [%d, %d] tensor on the speech's device" % (n, Ls))
    if n and Ls:
        sdev = torch.tensor(sl, dtype=torch.int32, device=dev) if sl is not None else None
        ndev = torch.tensor(nl, dtype=torch.int32, device=dev) if nl is not None else None
        tdev = torch.tensor(st_host, dtype=torch.int32, device=dev) if st_host is not None else None
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().rced_mix_snr(speech.data_ptr(), ptr(sdev), n, Ls, noise.data_ptr(), ptr(ndev), Ln, ptr(tdev),
                                            ptr(gdev), n_gains, float(snr), mix.data_ptr(), dev.index, st))
    return mix


def denoise_and_score(forward, mix, clean, lengths, nfft=512, kernels="x6", stoi=False):
    """The device core of the evaluation loop (tester.py:100-146 / trainer.py:260-307 without PESQ / wav files):
    STFT of the mixtures -> forward (device [N, T, 129, 1] -> same) -> ISTFT rebuild -> SDR (and, with stoi=True, STOI) of
    every rebuilt row against its clean row over its own length.  mix, clean: torch.cuda float32 [N, L] zero-padded;
    lengths: N sample counts.
    Returns (audio [N, (T+1)*128] on the device -- the caller trims row n to lengths[n] --, sdr torch.float64 [N]), with
    stoi=True (audio, sdr, stoi torch.float64 [N])."""
    mag, phase = stft_batch(mix, lengths, kernels=kernels)
    pred = forward(mag)
    out = istft_batch(pred, phase, nfft, kernels=kernels)
    if stoi:
        return out, sdr_batch(clean, out, lengths), stoi_batch(clean, out, lengths, SAMPLE_RATE)
    return out, sdr_batch(clean, out, lengths)


STREAM_DELAY, STREAM_FINISH_MAX, STREAM_MAX_HOPS = 640, 768, 64     # rced.h: RCED_STREAM_DELAY, RCED_STREAM_FINISH_MAX, the max_hops bound


class StreamingDenoiser(object):
    """PCM in, PCM out, a hop (128 samples, 16 ms) at a time, for `lanes` independent streams at once (rced_stream_*,
    DESIGN.md 3.4d).  A lane's output is InferenceEngine.denoise_pcm of everything pushed before `finish`, delayed by
    STREAM_DELAY = 640 samples: zeros first, and `finish` hands out what is still owed.  All state lives on the device; a
    push is three launches on the current stream.

    model_or_engine: a model of this package (is_training=False) or an engine holding one as `.model`; the stream runs the
    forward form that model has selected.  max_hops: the most hops one push may carry (1..64); nfft: 512 (the reference's
    rebuild as shipped) or 256.

    sample_rate, channels, dtype ("float32" or "int16"), output_rate: the capture and playback device's format.  With the
    defaults this is the 8 kHz object above.  Otherwise a push takes [lanes, K * hop_in (* channels)] at sample_rate, hop_in =
    128 * sample_rate / 8000, through resampler lanes (StreamingResampler) down to 8 kHz, the denoiser, and --
    with output_rate, normally sample_rate -- resampler lanes up again, without synchronisation; the output is float32 mono,
    InferenceEngine.denoise_pcm(x, sample_rate=...) (resampled to output_rate) delayed by `.delay` = stream_delay(...)
    samples.  A rate at which the hop is not a whole number of frames (44.1 kHz: 128 * 441 / 80) is a ValueError naming the
    rate: denoise_pcm serves those rates offline."""

    def __init__(self, model_or_engine, lanes, max_hops=8, nfft=512, sample_rate=8000, channels=1, dtype="float32", output_rate=None):
        import ctypes
        self._h = self._down = self._up = None
        self.model = getattr(model_or_engine, "model", model_or_engine)
        if getattr(self.model, "_handle", None) is None:
            raise ValueError("StreamingDenoiser needs an inference model (Model(is_training=False)) or an engine that holds one")
        self.lanes, self.max_hops, self.nfft, self.device = int(lanes), int(max_hops), int(nfft), self.model.device
        h = ctypes.c_void_p()
        self.sample_rate, self.channels, self.dtype = int(sample_rate), int(channels), dtype
        self.output_rate = int(output_rate) if output_rate is not None else None
        for rate in (self.sample_rate, self.output_rate):
            if rate is not None and (rate < 1 or STEP * rate % SAMPLE_RATE):
                raise ValueError("a hop of %d samples at 8 kHz is not a whole number of frames at %r Hz: streaming serves rates that are a "
                                 "multiple of 62.5 Hz, InferenceEngine.denoise_pcm(sample_rate=...) every rate" % (STEP, rate))
        _lib.check(_lib.load().rced_stream_create(self.model._handle, self.lanes, self.max_hops, self.nfft, ctypes.byref(h)))
        self._h = h
        self.hop_in = STEP * self.sample_rate // SAMPLE_RATE
        self.delay = stream_delay(self.sample_rate, self.output_rate, self.channels, dtype)
        if self.sample_rate != SAMPLE_RATE or self.channels != 1 or dtype != "float32":
            self._down = StreamingResampler(self.sample_rate, SAMPLE_RATE, self.lanes, unit_out=STEP, channels=self.channels, dtype=dtype,
                                            max_units=self.max_hops, device=self.device, delay=STEP)
        if self.output_rate is not None and self.output_rate != SAMPLE_RATE:
            self._up = StreamingResampler(SAMPLE_RATE, self.output_rate, self.lanes, unit_in=STEP, max_units=self.max_hops,
                                          device=self.device)

    def _tensor(self, x, dtype, shape, what):
        import torch
        dev = "cuda:%d" % self.device
        if hasattr(x, "is_cuda"):
            if not x.is_cuda or x.device.index != self.device:
                raise ValueError("%s must live on cuda:%d (or be a numpy array)" % (what, self.device))
            t = x.to(dtype).contiguous()
        else:
            t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32 if dtype == torch.float32 else np.int32), device=dev)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, got %s" % (what, tuple(shape), tuple(t.shape)))
        return t

    def push(self, pcm, active=None):
        """pcm [lanes, K*128] (1 <= K <= max_hops): the next K hops of every lane -> [lanes, K*128], the lanes' output streams.
        active: None, or `lanes` flags; a lane flagged 0 is idle (state untouched, zeros out).  A CUDA tensor gives a CUDA
        tensor (no synchronisation), an ndarray an ndarray.
        At the device's rate: pcm [lanes, K * hop_in (* channels)] of `dtype` -> [lanes, K*128] at 8 kHz, or with output_rate
        [lanes, K * 128 * output_rate / 8000], float32."""
        import torch
        if self._down is not None or self._up is not None:
            return self._push_rate(pcm, active)
        return self._push8(pcm, active)

    def _push8(self, pcm, active=None):
        import torch
        as_torch = hasattr(pcm, "is_cuda")
        cols = int(pcm.shape[1]) if len(pcm.shape) == 2 else -1
        if len(pcm.shape) != 2 or int(pcm.shape[0]) != self.lanes or cols < STEP or cols % STEP:
            raise ValueError("pcm must be [lanes = %d, K * 128] with K >= 1, got %s" % (self.lanes, tuple(pcm.shape)))
        x = self._tensor(pcm, torch.float32, (self.lanes, cols), "pcm")
        act = self._tensor(active, torch.int32, (self.lanes,), "active") if active is not None else None
        out = torch.empty_like(x)
        st = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.load().rced_stream_push(self._h, x.data_ptr(), act.data_ptr() if act is not None else None, cols // STEP,
                                                out.data_ptr(), st))
        for t in (x, act):          # the last launch reads the inputs again: keep a temporary's memory until the stream has passed
            if t is not None:
                t.record_stream(torch.cuda.current_stream(x.device))
        return out if as_torch else out.cpu().numpy()

    def _push_rate(self, pcm, active):
        """down lanes -> the three launches of the 8 kHz push -> up lanes, nothing waits.  The down lanes run a whole hop behind
        (delay 128), so what they hand on is whole hops of the 8 kHz signal -- except the first hop of a lane's first push, which
        is the delay's zeros and not signal: the denoiser takes that hop apart from the others, for the lanes that have started
        only (StreamingResampler.started), and returns zeros for the rest."""
        import torch
        as_torch = hasattr(pcm, "is_cuda")
        dev = "cuda:%d" % self.device
        x = pcm
        if not as_torch:
            a = np.asarray(pcm)
            x = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int16 if self.dtype == "int16" else np.float32), device=dev)
        if self._down is not None:
            act = self._down._active(active)
            started = self._down.started(act)
            z = self._down.push(x, act)                              # [lanes, K * 128] at 8 kHz, one hop late
            y = self._push8(z[:, :STEP], started)
            if z.shape[1] > STEP:
                y = torch.cat([y, self._push8(z[:, STEP:], act)], dim=1)
        else:
            act = active
            y = self._push8(x, act)
        if self._up is not None:
            y = self._up.push(y, act)
        return y if as_torch else y.cpu().numpy()

    def _drain(self, stage, unit, lanes, seqs):
        """Whole units of seqs[i] through lane lanes[i] of `stage`, one unit a push, the other lanes idle; then its finish with
        what is left.  Returns every lane's output, joined."""
        seqs = [np.asarray(s, np.float32) for s in seqs]
        got = [[] for _ in lanes]
        at = 0
        while any(len(s) - at >= unit for s in seqs):
            pcm, active = np.zeros((self.lanes, unit), np.float32), [0] * self.lanes
            for lane, s in zip(lanes, seqs):
                if len(s) - at >= unit:
                    pcm[lane], active[lane] = s[at:at + unit], 1
            out = stage.push(pcm, active) if stage is not self else self._push8(pcm, active)
            for i, (lane, s) in enumerate(zip(lanes, seqs)):
                if len(s) - at >= unit:
                    got[i].append(np.asarray(out[lane]))
            at += unit
        tails = [s[len(s) // unit * unit:] for s in seqs]
        rest = stage.finish(lanes, tails) if stage is not self else self._finish8(lanes, tails)
        return [np.concatenate(g + [np.asarray(r)]) for g, r in zip(got, rest)]

    def finish(self, lanes, tails):
        """Ends the utterance of every lane listed: tails[i] holds the last 0..127 samples of lane lanes[i].  Returns a list of
        float32 arrays, the samples each lane still owed (L - max(0, 128 H - 640) of them); the lanes are reset for a new
        utterance, the others left alone.  Synchronises (the counts come back).
        At the device's rate: tails[i] holds fewer than hop_in frames; the stages are drained in order -- what the down lanes
        owe goes hop by hop through the denoiser and its finish, all of that through the up lanes and their finish."""
        if self._down is None and self._up is None:
            return self._finish8(lanes, tails)
        lanes = [int(v) for v in lanes]
        seqs = self._down.finish(lanes, tails) if self._down is not None else None
        out = self._drain(self, STEP, lanes, seqs) if seqs is not None else self._finish8(lanes, tails)
        return self._drain(self._up, STEP, lanes, out) if self._up is not None else out

    def _finish8(self, lanes, tails):
        import torch
        lanes = [int(v) for v in lanes]
        if len(lanes) != len(tails) or len(set(lanes)) != len(lanes) or any(v < 0 or v >= self.lanes for v in lanes):
            raise ValueError("lanes must be distinct indices in [0, %d), one tail each" % self.lanes)
        tail = np.zeros((self.lanes, STEP), np.float32)
        counts = np.full((self.lanes,), -1, np.int32)
        for lane, t in zip(lanes, tails):
            t = (t.detach().cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t, np.float32)).reshape(-1)
            if t.size >= STEP:
                raise ValueError("a tail holds fewer than %d samples (push whole hops first), got %d" % (STEP, t.size))
            tail[lane, :t.size] = t
            counts[lane] = t.size
        dev = "cuda:%d" % self.device
        tdev, cdev = torch.as_tensor(tail, device=dev), torch.as_tensor(counts, device=dev)
        out = torch.empty((self.lanes, STREAM_FINISH_MAX), dtype=torch.float32, device=dev)
        owed = torch.empty((self.lanes,), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(_lib.load().rced_stream_finish(self._h, tdev.data_ptr(), cdev.data_ptr(), out.data_ptr(), owed.data_ptr(), st))
        out, owed = out.cpu().numpy(), owed.cpu().numpy()
        return [out[lane, :owed[lane]].copy() for lane in lanes]

    def reset(self, lane=-1):
        """Back to the start of an utterance, without output: one lane, or (-1) all of them."""
        _lib.check(_lib.load().rced_stream_reset(self._h, int(lane)))
        for stage in (self._down, self._up):
            if stage is not None:
                stage.reset(lane)

    def close(self):
        for stage in (getattr(self, "_down", None), getattr(self, "_up", None)):
            if stage is not None:
                stage.close()
        self._down = self._up = None
        if self._h is not None:
            try:
                _lib.load().rced_stream_destroy(self._h)
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


def stream_delay(sample_rate=8000, output_rate=None, channels=1, dtype="float32"):
    """StreamingDenoiser(..., sample_rate, channels, dtype, output_rate).delay, in samples at the output's rate (needs no GPU):
    STREAM_DELAY = 640 at 8 kHz; with down lanes (any input but mono float32 at 8 kHz) one hop more, 128 -- the down lanes hand on
    whole hops, which costs resampler_delay's 63 rounded up to a hop --; with up lanes all of that carried to output_rate, and
    their own resampler_delay(8000, output_rate).  48 kHz in and out: (128 + 640) * 6 + 384 = 4,992."""
    d = STREAM_DELAY + (STEP if int(sample_rate) != SAMPLE_RATE or int(channels) != 1 or dtype != "float32" else 0)
    if output_rate is not None and int(output_rate) != SAMPLE_RATE:
        d = d * int(output_rate) // SAMPLE_RATE + resampler_delay(SAMPLE_RATE, output_rate)
    return d


class StreamingResampler(object):
    """resample_batch for audio that arrives unit by unit, for `lanes` independent streams at once (rced_rstream_*, DESIGN.md
    3.4g).  A push of K units hands every active lane K * unit_in source frames at sr_in and returns K * unit_out samples at
    sr_out; a lane's output is resample_batch of everything pushed before `finish`, delayed by `.delay` samples, bit for
    bit: zeros first, and `finish` hands out what is still owed.  All state lives on the device; a push is one launch on
    the current stream.

    unit_out / unit_in: give one (the other follows from the ratio; a unit that gives no whole number on the other side is a
    ValueError), both (they must stand in the ratio), or neither (the smallest pair: q frames in, p samples out).
    channels: interleaved channels per frame, averaged; dtype / out_dtype: "float32" or "int16", as in resample_arena;
    max_units: the most units one push may carry; delay: None (the smallest, resampler_delay(sr_in, sr_out)) or a longer one."""

    def __init__(self, sr_in, sr_out, lanes, unit_out=None, unit_in=None, channels=1, dtype="float32", out_dtype="float32",
                 max_units=8, device=0, delay=None):
        import ctypes
        from math import gcd
        self._h = None
        sr_in, sr_out = int(sr_in), int(sr_out)
        if sr_in < 1 or sr_out < 1:
            raise ValueError("both rates must be positive, got %d -> %d" % (sr_in, sr_out))
        if dtype not in PCM_DTYPES or out_dtype not in PCM_DTYPES:
            raise ValueError("dtype and out_dtype must be 'float32' or 'int16', got %r, %r" % (dtype, out_dtype))
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
        self.sr_in, self.sr_out, self.lanes, self.channels, self.device = sr_in, sr_out, int(lanes), int(channels), int(device)
        self.unit_in, self.unit_out, self.max_units, self.dtype, self.out_dtype = unit_in, unit_out, int(max_units), dtype, out_dtype
        if self.channels < 1:
            raise ValueError("channels must be >= 1, got %d" % self.channels)
        h = ctypes.c_void_p()
        code = lambda d: _lib.PCM_F32 if d == "float32" else _lib.PCM_S16      # noqa: E731
        _lib.check(_lib.load().rced_rstream_create_ex(sr_in, sr_out, self.channels, code(dtype), code(out_dtype), unit_in, unit_out,
                                                      self.lanes, self.max_units, -1 if delay is None else int(delay), self.device,
                                                      ctypes.byref(h)))
        self._h = h
        self.delay = int(_lib.load().rced_rstream_delay(h))
        self.finish_max = unit_out + self.delay

    def _torch_dtype(self, name):
        import torch
        return torch.float32 if name == "float32" else torch.int16

    def _frames(self, x, frames, what):
        """[lanes, frames] (mono), [lanes, frames * channels] or [lanes, frames, channels] -> contiguous, on the device, of `dtype`"""
        import torch
        shapes = [(self.lanes, frames, self.channels), (self.lanes, frames * self.channels)]
        if tuple(x.shape) not in shapes:
            raise ValueError("%s must have shape %s or %s, got %s" % (what, shapes[0], shapes[1], tuple(x.shape)))
        if hasattr(x, "is_cuda"):
            if not x.is_cuda or x.device.index != self.device:
                raise ValueError("%s must live on cuda:%d (or be a numpy array)" % (what, self.device))
            return x.to(self._torch_dtype(self.dtype)).contiguous()
        a = np.ascontiguousarray(x, dtype=np.float32 if self.dtype == "float32" else np.int16)
        return torch.as_tensor(a, device="cuda:%d" % self.device)

    def _active(self, active):
        import torch
        if active is None:
            return None
        dev = "cuda:%d" % self.device
        act = (active.to(torch.int32).contiguous() if hasattr(active, "is_cuda")
               else torch.as_tensor(np.ascontiguousarray(active, dtype=np.int32), device=dev))
        if tuple(act.shape) != (self.lanes,) or not act.is_cuda or act.device.index != self.device:
            raise ValueError("active must hold lanes = %d flags on the stream's device" % self.lanes)
        return act

    def started(self, active=None):
        """[lanes] int32 on the device: 1 where the lane is active and has taken a unit since the start of its utterance
        (rced_rstream_started).  No synchronisation."""
        import torch
        act = self._active(active)
        out = torch.empty((self.lanes,), dtype=torch.int32, device="cuda:%d" % self.device)
        st = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(_lib.load().rced_rstream_started(self._h, act.data_ptr() if act is not None else None, out.data_ptr(), st))
        if act is not None:
            act.record_stream(torch.cuda.current_stream(out.device))
        return out

    def push(self, pcm, active=None):
        """pcm [lanes, K * unit_in] (interleaved: [lanes, K * unit_in * channels] or [lanes, K * unit_in, channels]), 1 <= K <=
        max_units: the next K units of every lane -> [lanes, K * unit_out] of out_dtype.  active: None, or `lanes` flags; a lane
        flagged 0 is idle (state untouched, zeros out).  A CUDA tensor gives a CUDA tensor (no synchronisation), an ndarray an
        ndarray."""
        import torch
        as_torch = hasattr(pcm, "is_cuda")
        per = self.unit_in * (self.channels if len(pcm.shape) == 2 else 1)
        cols = int(pcm.shape[1]) if len(pcm.shape) in (2, 3) else 0
        if cols < per or cols % per:
            raise ValueError("pcm must be [lanes = %d, K * %d frames] with K >= 1, got %s" % (self.lanes, self.unit_in, tuple(pcm.shape)))
        k = cols // per
        x = self._frames(pcm, k * self.unit_in, "pcm")
        act = self._active(active)
        out = torch.empty((self.lanes, k * self.unit_out), dtype=self._torch_dtype(self.out_dtype), device=x.device)
        st = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.load().rced_rstream_push(self._h, x.data_ptr(), act.data_ptr() if act is not None else None, k, out.data_ptr(), st))
        for t in (x, act):          # a temporary's memory stays until the stream has passed
            if t is not None:
                t.record_stream(torch.cuda.current_stream(x.device))
        return out if as_torch else out.cpu().numpy()

    def finish(self, lanes, tails):
        """Ends the utterance of every lane listed: tails[i] holds the last 0 .. unit_in - 1 frames of lane lanes[i] ([frames] or
        [frames, channels]).  Returns a list of arrays of out_dtype, the samples each lane still owed
        (resample_length(L) - max(0, H * unit_out - delay) of them); the lanes are reset for a new utterance, the others left
        alone.  Synchronises (the counts come back)."""
        import torch
        lanes = [int(v) for v in lanes]
        if len(lanes) != len(tails) or len(set(lanes)) != len(lanes) or any(v < 0 or v >= self.lanes for v in lanes):
            raise ValueError("lanes must be distinct indices in [0, %d), one tail each" % self.lanes)
        np_dtype = np.float32 if self.dtype == "float32" else np.int16
        tail = np.zeros((self.lanes, self.unit_in, self.channels), np_dtype)
        counts = np.full((self.lanes,), -1, np.int32)
        for lane, t in zip(lanes, tails):
            t = (t.detach().cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)).astype(np_dtype, copy=False)
            if t.size % self.channels:
                raise ValueError("a tail holds whole frames of %d channels, got %d values" % (self.channels, t.size))
            t = t.reshape(-1, self.channels)
            if t.shape[0] >= self.unit_in:
                raise ValueError("a tail holds fewer than %d frames (push whole units first), got %d" % (self.unit_in, t.shape[0]))
            tail[lane, :t.shape[0]] = t
            counts[lane] = t.shape[0]
        dev = "cuda:%d" % self.device
        tdev, cdev = torch.as_tensor(tail, device=dev), torch.as_tensor(counts, device=dev)
        out = torch.empty((self.lanes, self.finish_max), dtype=self._torch_dtype(self.out_dtype), device=dev)
        owed = torch.empty((self.lanes,), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(_lib.load().rced_rstream_finish(self._h, tdev.data_ptr(), cdev.data_ptr(), out.data_ptr(), owed.data_ptr(), st))
        out, owed = out.cpu().numpy(), owed.cpu().numpy()
        return [out[lane, :owed[lane]].copy() for lane in lanes]

    def reset(self, lane=-1):
        """Back to the start of an utterance, without output: one lane, or (-1) all of them."""
        _lib.check(_lib.load().rced_rstream_reset(self._h, int(lane)))

    def close(self):
        if self._h is not None:
            try:
                _lib.load().rced_rstream_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def __del__(self):
        self.close()


class AudioFeature(object):
    """data_utils/audio_feature.py:12-115 on the GPU (numpy in, numpy out, like the reference)."""

    def __init__(self, windows_name=None, device=0, kernels="x6"):
        if windows_name not in (None, "hamming"):
            raise ValueError("only the hamming window is built (it is what every reference run uses: SURVEY F7)")
        self.device, self.kernels = device, kernels
        _kernels(kernels)

    def compute_spectrogram(self, signal, sample_rate, window_s=0.02, stride_s=0.01, nfft=512, use_complex=False):
        import torch
        if stride_s > window_s:
            raise ValueError("Stride size must not be greater than window size.")   # audio_feature.py:29-30
        _check_cfg(sample_rate, window_s, stride_s, nfft)
        sig = torch.as_tensor(np.asarray(signal, dtype=np.float32), device="cuda:%d" % self.device)[None]
        mag, ph = stft_batch(sig, with_phase=use_complex, kernels=self.kernels)
        if use_complex:   # [129, T] complex, like np.transpose(fft_frames)
            return (mag[0, :, :, 0] * ph[0]).cpu().numpy().T
        return mag[0, :, :, 0].cpu().numpy().T

    @staticmethod
    def power_spectrum(frames):
        return np.absolute(frames)

    @staticmethod
    def divide_phase(fft_frames):
        return np.exp(1.j * np.angle(fft_frames))


class AudioReBuild(object):
    """model_utils/utils.py:93-183 on the GPU.  nfft defaults to 512 exactly as the reference's does."""

    def __init__(self, windows_name=None, nfft=512, device=0, kernels="x6"):
        if windows_name not in (None, "hamming"):
            raise ValueError("only the hamming window is built")
        if nfft not in (256, 512):
            raise ValueError("nfft must be 512 (reference default) or 256")
        self.nfft, self.device, self.kernels = nfft, device, kernels
        _kernels(kernels)

    def rebuild_audio(self, sig_length_list, spec, phase, sample_rate, windows_ms, stride_ms):
        import torch
        _check_cfg(sample_rate, windows_ms / 1000.0, stride_ms / 1000.0)
        dev = "cuda:%d" % self.device
        mag = torch.as_tensor(np.asarray(spec, dtype=np.float32), device=dev)
        ph = torch.as_tensor(np.asarray(phase).astype(np.complex64), device=dev)
        audio = istft_batch(mag, ph, self.nfft, kernels=self.kernels).cpu().numpy()
        return [audio[i][:sig_length_list[i]] for i in range(len(audio))]
