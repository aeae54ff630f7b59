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
    rebuild as shipped) or 256."""

    def __init__(self, model_or_engine, lanes, max_hops=8, nfft=512):
        import ctypes
        self._h = None
        self.model = getattr(model_or_engine, "model", model_or_engine)
        if getattr(self.model, "_handle", None) is None:
            raise ValueError("StreamingDenoiser needs an inference model (Model(is_training=False)) or an engine that holds one")
        self.lanes, self.max_hops, self.nfft, self.device = int(lanes), int(max_hops), int(nfft), self.model.device
        h = ctypes.c_void_p()
        _lib.check(_lib.load().rced_stream_create(self.model._handle, self.lanes, self.max_hops, self.nfft, ctypes.byref(h)))
        self._h = h

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
        tensor (no synchronisation), an ndarray an ndarray."""
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

    def finish(self, lanes, tails):
        """Ends the utterance of every lane listed: tails[i] holds the last 0..127 samples of lane lanes[i].  Returns a list of
        float32 arrays, the samples each lane still owed (L - max(0, 128 H - 640) of them); the lanes are reset for a new
        utterance, the others left alone.  Synchronises (the counts come back)."""
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

    def close(self):
        if self._h is not None:
            try:
                _lib.load().rced_stream_destroy(self._h)
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
