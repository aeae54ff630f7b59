"""The evaluation loop's entry points on the device, over the C ABI: SDR, STOI, ESTOI, SI-SDR,
segmental SNR, LLR, WSS, fwSNRseg, CD and the SDR of BSS Eval per utterance, add_noise's SNR mixing in closed form, the ragged FIR behind the loader's room impulse responses (convolve_batch), and the core of the loop, STFT -> forward -> ISTFT -> scores.  audio.py re-exports
every public name here."""

import numpy as np

from . import _args, _lib
from ._args import SAMPLE_RATE, ptr


class _Pairs(object):
    """What every pair-scoring *_batch goes through: scoring_args, the result `out` (float64 [N]), further [N, ...] tensors
    from new(), and call(): the entry with the shared head (both matrices and their row strides, the lengths, N), the entry's own
    arguments and the (device, stream) tail -- skipped for an empty batch.  cap: the samples a row holds in both matrices."""

    def __init__(self, clean, estimate, lengths):
        self.head = _args.scoring_args(clean, estimate, lengths)
        self.n, self.dev, self.cap = self.head[2], self.head[3], min(self.head[4:6])
        self.out = self.new()

    def new(self, *tail, dtype="float64", zeros=False):
        import torch
        return (torch.zeros if zeros else torch.empty)((self.n,) + tail, dtype=getattr(torch, dtype), device=self.dev)

    def call(self, entry, *middle):
        clean, estimate, n, dev, sc, se, ldev = self.head
        if n:
            _lib.check(getattr(_lib.load(), entry)(clean.data_ptr(), sc, estimate.data_ptr(), se, ptr(ldev), n, *middle, dev.index,
                                                   _args.current_stream(dev)))
        return self.out


def sdr_batch(clean, estimate, lengths=None):
    """SDR.sdr (model_utils/utils.py:68-86) per utterance on the device: clean [N, Lc], estimate [N, Le] torch.cuda float32,
    row n holding utterance n from column 0 (the estimate may be istft_batch's [N, (T+1)*128] buffer as it is: the length
    trims, nothing is copied); lengths: per-utterance sample counts in [0, min(Lc, Le)] or None (= min(Lc, Le) each).
    Returns torch.float64 [N] (dB) on the device, current stream."""
    p = _Pairs(clean, estimate, lengths)
    return p.call("rced_sdr", p.out.data_ptr(), None)


STOI_RATES = (8000, 10000)


def stoi_batch(clean, estimate, lengths=None, sample_rate=8000, detail=False, extended=False):
    """STOI (Taal et al. 2011; the reference's pystoi.stoi(clean, denoise, sr, extended=False), tester.py:92-167) per utterance
    on the device, as DESIGN.md "STOI" specifies it.  clean [N, Lc], estimate [N, Le], lengths: as in sdr_batch (the estimate
    may be istft_batch's buffer as it is).  sample_rate: 8000 (resampled to 10 kHz on the device) or 10000.
    extended: False = STOI; True = ESTOI (Jensen, Taal 2016, DESIGN.md "ESTOI") in its place; "both" = (stoi, estoi) from one
    call that resamples, removes silent frames and takes the band spectra once.
    Returns torch.float64 [N] on the device, current stream (two of them for "both"); with detail=True also, last,
    torch.int32 [N, 3]: frames at 10 kHz, frames kept by the 40 dB silent-frame removal, 30-frame segments (0 segments: the
    score is 1e-5)."""
    if int(sample_rate) not in STOI_RATES:
        raise ValueError("sample_rate must be 8000 or 10000, got %r" % (sample_rate,))
    if not (extended is False or extended is True or extended == "both"):
        raise ValueError("extended must be False, True or 'both', got %r" % (extended,))
    p = _Pairs(clean, estimate, lengths)
    det = p.new(3, dtype="int32") if detail else None
    if extended is False:
        out = p.call("rced_stoi", int(sample_rate), p.out.data_ptr(), ptr(det))
        return (out, det) if detail else out
    classic = p.new() if extended == "both" else None
    which = _lib.STOI_EXTENDED | (_lib.STOI_CLASSIC if classic is not None else 0)
    ext = p.call("rced_stoi_ex", int(sample_rate), which, ptr(classic), p.out.data_ptr(), ptr(det))
    scores = (classic, ext) if classic is not None else (ext,)
    if detail:
        return scores + (det,)
    return scores if classic is not None else ext


def si_sdr_batch(clean, estimate, lengths=None):
    """SI-SDR per utterance on the device (DESIGN.md "SI-SDR": alpha = sum(y x) / sum(x x), 10 log10(sum((alpha x)^2) /
    sum((y - alpha x)^2)), two passes, no mean removal).  Arguments as in sdr_batch.  Returns torch.float64 [N] (dB) on the
    device, current stream; +inf where the estimate is a power-of-two multiple of the clean row, nan for an all-zero row or
    a length of 0."""
    p = _Pairs(clean, estimate, lengths)
    return p.call("rced_si_sdr", p.out.data_ptr(), None)


SEG_SNR_WINDOW = (4, 1440)


def seg_snr_window(sample_rate):
    """Samples per frame of the segmental SNR at a rate, (3 sr + 50) // 100 (30 ms); ValueError where the library refuses it."""
    sr = int(sample_rate)
    w = (3 * sr + 50) // 100 if sr > 0 else 0
    if sr != sample_rate or not SEG_SNR_WINDOW[0] <= w <= SEG_SNR_WINDOW[1]:
        raise ValueError("sample_rate %r gives frames of %d samples: outside [%d, %d]" % ((sample_rate, w) + SEG_SNR_WINDOW))
    return w


def seg_snr_batch(clean, estimate, lengths=None, sample_rate=8000, detail=False):
    """Segmental SNR per utterance on the device (DESIGN.md "Segmental SNR": 30 ms Hann-windowed frames at a quarter-frame
    hop, each frame's SNR clamped to [-10, 35] dB, the mean over the frames).  Arguments as in sdr_batch; sample_rate: any
    rate whose frame has 4 .. 1440 samples.  Returns torch.float64 [N] (dB) on the device, current stream -- nan for an
    utterance shorter than one frame; with detail=True also torch.int32 [N], the frames of each utterance."""
    seg_snr_window(sample_rate)
    p = _Pairs(clean, estimate, lengths)
    frames = p.new(dtype="int32") if detail else None
    out = p.call("rced_seg_snr", int(sample_rate), p.out.data_ptr(), ptr(frames))
    return (out, frames) if detail else out


SPECTRAL_RATES = (8000, 16000)


def _spectral_rate(sample_rate):
    if sample_rate not in SPECTRAL_RATES:
        raise ValueError("sample_rate must be 8000 or 16000, got %r" % (sample_rate,))
    return int(sample_rate)


def _spectral_batch(entry, clean, estimate, lengths, sample_rate, detail, *limit):
    """What the frame-based scores at 8 / 16 kHz share; *limit: the entry's own arguments between the rate and the outputs."""
    fs = _spectral_rate(sample_rate)
    p = _Pairs(clean, estimate, lengths)
    w = (3 * fs + 50) // 100
    most = (p.cap - w) // (w // 4) + 1 if p.cap >= w else 0      # the frames of a row read to its end
    nf = p.new(dtype="int32") if detail else None
    frames = p.new(most, zeros=True) if detail else None
    out = p.call(entry, fs, *limit, p.out.data_ptr(), ptr(frames), most, ptr(nf))
    return (out, nf, frames) if detail else out


def llr_batch(clean, estimate, lengths=None, sample_rate=8000, limit=2.0, detail=False):
    """Log-likelihood ratio of the two signals' LPC models per utterance on the device (DESIGN.md "LLR": the segmental SNR's
    frames of x + eps and y + eps, order 10 below 10 kHz else 16, Levinson-Durbin, ln of the ratio of the two models'
    residual energies on the clean frame, the mean of the lowest 95 % of the frames).  Arguments as in sdr_batch;
    sample_rate: 8000 or 16000; limit: each frame's value enters the mean as min(value, limit) -- None or inf for none, the
    form metrics.composite takes.  Returns torch.float64 [N] on the device, current stream -- nan for an utterance shorter
    than one frame; with detail=True also torch.int32 [N], the frames of each utterance, and torch.float64 [N, F], every
    frame's value before the limit in frame order (0 past an utterance's frames).  Built as DESIGN.md writes it: parity
    with pysepm is unpinned."""
    limit = float("inf") if limit is None else float(limit)
    if limit != limit:
        raise ValueError("limit must be a number or None, got nan")
    return _spectral_batch("rced_llr", clean, estimate, lengths, sample_rate, detail, limit)


def wss_batch(clean, estimate, lengths=None, sample_rate=8000, detail=False):
    """Weighted spectral slope distance per utterance on the device (DESIGN.md "WSS": the segmental SNR's frames, an fp64
    DFT, 25 critical-band energies in dB, their 24 slopes weighted by the nearest peak and the global maximum, the mean of
    the lowest 95 % of the frames).  Arguments and returns as in llr_batch, without the limit."""
    return _spectral_batch("rced_wss", clean, estimate, lengths, sample_rate, detail)


def fw_seg_snr_batch(clean, estimate, lengths=None, sample_rate=8000, detail=False):
    """Frequency-weighted segmental SNR per utterance on the device (DESIGN.md "fwSNRseg": the segmental SNR's frames, an fp64
    DFT, each signal's magnitudes over their sum, the 25 critical-band filters of WSS on those, weights E_x ** 0.2, each
    band's SNR limited to [-10, 35] dB, the plain mean over the frames).  Arguments as in sdr_batch; sample_rate: 8000 or
    16000.  Returns torch.float64 [N] (dB) on the device, current stream -- nan for an utterance shorter than one frame or
    with a digitally silent frame; with detail=True also torch.int32 [N], the frames of each utterance, and torch.float64
    [N, F], every frame's value in frame order (0 past an utterance's frames).  Built as DESIGN.md writes it: parity with
    pysepm is unpinned."""
    return _spectral_batch("rced_fwseg", clean, estimate, lengths, sample_rate, detail)


CEP_MAX_ORDER = 16


def _cep_order(order, sample_rate):
    if order is None:
        return 10 if _spectral_rate(sample_rate) < 10000 else 16       # LLR's order at the rate
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= order <= CEP_MAX_ORDER:
        raise ValueError("order must be None or an integer in [1, %d], got %r" % (CEP_MAX_ORDER, order))
    return int(order)


def cep_dist_batch(clean, estimate, lengths=None, sample_rate=8000, order=None, detail=False):
    """Cepstral distance of the two signals' LPC models per utterance on the device (DESIGN.md "CD": LLR's frames, lags and
    Levinson-Durbin, the models' first `order` cepstral coefficients, (10 / ln 10) sqrt(2 sum (cx - cy)^2) limited to
    [0, 10] per frame, the mean of the lowest 95 % of the frames).  Arguments as in llr_batch; order: None for LLR's order
    at the rate (10 below 10 kHz, else 16) or an integer in [1, 16], anything else is a ValueError before any device work.
    Returns as llr_batch does; the per-frame values are the limited ones.  Parity with pysepm is unpinned."""
    return _spectral_batch("rced_cepd", clean, estimate, lengths, sample_rate, detail, _cep_order(order, sample_rate))


BSS_MAX_FILTER = 512


def _filter_length(filter_length):
    if isinstance(filter_length, bool) or not isinstance(filter_length, (int, np.integer)) or not 1 <= filter_length <= BSS_MAX_FILTER:
        raise ValueError("filter_length must be an integer in [1, %d], got %r" % (BSS_MAX_FILTER, filter_length))
    return int(filter_length)


def bss_sdr_batch(clean, estimate, lengths=None, filter_length=512, detail=False):
    """The SDR of BSS Eval (Vincent, Gribonval, Fevotte 2006) for a single source, per utterance on the device (DESIGN.md
    "BSS Eval SDR"): the estimate is projected onto the span of the clean row delayed by 0 .. filter_length - 1 samples --
    r = autocorrelation of x, d = cross-correlation of x and y at lags 0 .. F - 1, toeplitz(r) c = d, s = x * c,
    e = [y, 0 ..] - s over L + F - 1 samples, 10 log10(sum s^2 / sum e^2) -- so a fixed linear filtering or a delay of the
    estimate is forgiven.  All of it in fp64.  Arguments as in si_sdr_batch; filter_length: an integer in [1, 512], anything
    else is a ValueError before any device work; 1 gives si_sdr_batch's score.
    Returns torch.float64 [N] (dB) on the device, current stream -- nan for a length of 0, an all-zero clean row or an all-zero
    estimate; with detail=True also torch.float64 [N, filter_length], the filters c, and torch.float64 [N, 2], sum s^2 and
    sum e^2.  Nothing is regularised and there is no least-squares fallback: a singular toeplitz(r) (a clean row with an
    empty band) gives whatever the recursion gives.  This is bss_eval_sources for one source; parity with mir_eval or museval
    is unpinned, the pin is the float64 restatement in tests/bsseval_np.py."""
    taps = _filter_length(filter_length)
    p = _Pairs(clean, estimate, lengths)
    filt = p.new(taps) if detail else None
    energies = p.new(2) if detail else None
    out = p.call("rced_bss_sdr", taps, p.out.data_ptr(), ptr(filt), ptr(energies))
    return (out, filt, energies) if detail else out


# every score `extra` can name -> (its batch function, the keywords the evaluation loop calls it with)
_EXTRA = {"estoi": (stoi_batch, {"sample_rate": SAMPLE_RATE, "extended": True}),
          "si_sdr": (si_sdr_batch, {}),
          "seg_snr": (seg_snr_batch, {"sample_rate": SAMPLE_RATE}),
          "llr": (llr_batch, {"sample_rate": SAMPLE_RATE, "limit": 2.0}),
          "wss": (wss_batch, {"sample_rate": SAMPLE_RATE}),
          "bss_sdr": (bss_sdr_batch, {"filter_length": 512})}
EXTRA_METRICS = ("estoi", "si_sdr", "seg_snr")
SPECTRAL_METRICS = ("llr", "wss")       # the composite measures' two spectral terms; `extra` takes names from all three tuples
PROJECTION_METRICS = ("bss_sdr",)       # BSS Eval's SDR at its filter length of 512
ALL_EXTRA = tuple(_EXTRA)
assert ALL_EXTRA == EXTRA_METRICS + SPECTRAL_METRICS + PROJECTION_METRICS
# The two further objective measures of Hu and Loizou (2008), a table and a tuple of their own: the six names above and the
# tuples that hold them keep their values for the callers that pinned them.  `extra` takes names from both tables.
_EXTRA_SEPM = {"fw_seg_snr": (fw_seg_snr_batch, {"sample_rate": SAMPLE_RATE}),
               "cd": (cep_dist_batch, {"sample_rate": SAMPLE_RATE, "order": None})}
SEPM_METRICS = tuple(_EXTRA_SEPM)       # fwSNRseg, and CD at LLR's order
EVERY_EXTRA = ALL_EXTRA + SEPM_METRICS


def check_extra(extra):
    """The evaluation loop's `extra` argument as a tuple of names from EXTRA_METRICS + SPECTRAL_METRICS + PROJECTION_METRICS +
    SEPM_METRICS, in the caller's order; ValueError for anything else.  Touches no device."""
    names = (extra,) if isinstance(extra, str) else tuple(extra)
    for name in names:
        if name not in EVERY_EXTRA:
            raise ValueError("extra names must come from %r, got %r" % (EVERY_EXTRA, name))
    if len(set(names)) != len(names):
        raise ValueError("extra names must be distinct, got %r" % (names,))
    return names


def gains_needed(len_speech, len_noise):
    """How many of add_noise's uniform(0, 2) draws can reach the first len_speech samples: bit_length((ls - 1) // ln)."""
    if len_speech < len_noise or len_speech < 1:
        return 0
    return int((len_speech - 1) // len_noise).bit_length()


def mix_snr_batch(speech, noise, snr, speech_lengths=None, noise_lengths=None, starts=None, gains=None, out=None):
    """AudioParser.add_noise (data_utils/data_loader.py:35-52) for a batch on the device, in closed form.
    speech [N, Ls], noise [N, Ln] torch.cuda float32 with per-utterance lengths (lists / tensors, or None = the full row);
    starts [N]: the crop offsets (used where the noise is longer than the speech; None = 0);
    gains [N, n_gains] float64 (array, or a list of per-utterance sequences, padded with 1): the uniform(0, 2) draws
    u_0.. (used where the speech is at least as long as the noise) -- loader.plan_noise makes both as the reference would.
    out: None, or a contiguous float32 [N, Ls] device tensor to write into (e.g. the lower half of a [2N, Ls] buffer).
    Returns mix [N, Ls] float32 on the device (0 past each speech length), current stream."""
    import torch
    speech, noise = _args.rows(speech, "speech").contiguous(), _args.rows(noise, "noise").contiguous()
    n, Ls, Ln = int(speech.shape[0]), int(speech.shape[1]), int(noise.shape[1])
    if int(noise.shape[0]) != n or noise.device != speech.device:
        raise ValueError("speech and noise must hold the same number of utterances on one device")
    dev = speech.device
    sl, nl = _args.host_ints(speech_lengths, n, "speech_lengths"), _args.host_ints(noise_lengths, n, "noise_lengths")
    if sl is not None and any(v < 0 or v > Ls for v in sl):
        raise ValueError("speech_lengths must lie in [0, %d]" % Ls)
    if nl is not None and any(v < 1 or v > Ln for v in nl):
        raise ValueError("noise_lengths must lie in [1, %d]" % Ln)
    if n and Ls and Ln < 1:
        raise ValueError("empty noise")
    ls_of = sl if sl is not None else [Ls] * n
    ln_of = nl if nl is not None else [Ln] * n
    st_host = _args.host_ints(starts, n, "starts")
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
    mix = torch.empty((n, Ls), dtype=torch.float32, device=dev) if out is None else _args.check_out(out, n, Ls, dev, torch.float32, exact=True)
    if n and Ls:
        sdev = torch.tensor(sl, dtype=torch.int32, device=dev) if sl is not None else None
        ndev = torch.tensor(nl, dtype=torch.int32, device=dev) if nl is not None else None
        tdev = torch.tensor(st_host, dtype=torch.int32, device=dev) if st_host is not None else None
        _lib.check(_lib.load().rced_mix_snr(speech.data_ptr(), ptr(sdev), n, Ls, noise.data_ptr(), ptr(ndev), Ln, ptr(tdev),
                                            ptr(gdev), n_gains, float(snr), mix.data_ptr(), dev.index, _args.current_stream(dev)))
    return mix


CONV_MAX_TAPS = 8192      # rced.h: RCED_CONV_MAX_TAPS


def _overlap(a, b):
    """Whether the memory two tensors' elements span intersects."""
    def span(t):
        reach = sum((int(s) - 1) * int(st) for s, st in zip(t.shape, t.stride())) + 1 if t.numel() else 0
        return t.data_ptr(), t.data_ptr() + reach * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def convolve_batch(signal, filters, lengths=None, filter_lengths=None, shifts=None, out=None):
    """A ragged batched FIR on the device (rced_convolve): row n of the result is np.convolve(x_n, h_n)[d_n : d_n + len_n] --
    the signal's length is kept, tap d_n (a room impulse response's direct path) has zero delay, the tail is dropped --,
    zeros from len_n to L.  Products and sums in fp64 on the f64 matrix pipe, one rounding at the float32 store; a row's bits
    do not depend on the batch around it.
    signal [N, L], filters [N, Kmax] torch.cuda float32 (a 1-D signal is one row, and comes back 1-D; rows may be views of wider
    buffers); lengths [N] in [0, L] (None = L each), filter_lengths [N] in [0, Kmax] (None = Kmax each; at most CONV_MAX_TAPS =
    8192), shifts [N] with 0 <= d_n < max(K_n, 1) (None = 0): lists, arrays or tensors, read on the host.
    out: None, or a contiguous float32 [N, L] device tensor to write into (as mix_snr_batch takes it); it must not overlap
    signal or filters.  ValueError before any device work for more than 8192 taps, a shift outside its filter, a length
    outside its row, mismatched N or device.  Returns [N, L] float32 on the device, current stream."""
    import torch
    one = hasattr(signal, "dim") and signal.dim() == 1
    if one:
        signal = signal[None]
        filters = filters[None] if hasattr(filters, "dim") and filters.dim() == 1 else filters
    signal, filters = _args.rows(signal, "signal"), _args.rows(filters, "filters")
    n, L, kmax = int(signal.shape[0]), int(signal.shape[1]), int(filters.shape[1])
    if int(filters.shape[0]) != n or filters.device != signal.device:
        raise ValueError("signal and filters must hold the same number of rows on one device, got %d on %s and %d on %s"
                         % (n, signal.device, int(filters.shape[0]), filters.device))
    if kmax < 1:
        raise ValueError("filters must hold at least one column (filter_lengths may still say 0 taps)")
    dev = signal.device
    xl, hl = _args.host_ints(lengths, n, "lengths"), _args.host_ints(filter_lengths, n, "filter_lengths")
    sh = _args.host_ints(shifts, n, "shifts")
    if xl is not None and any(v < 0 or v > L for v in xl):
        raise ValueError("lengths must lie in [0, %d]" % L)
    if hl is not None and any(v < 0 or v > kmax for v in hl):
        raise ValueError("filter_lengths must lie in [0, %d]" % kmax)
    taps = hl if hl is not None else [kmax] * n
    if any(v > CONV_MAX_TAPS for v in taps):
        raise ValueError("a filter has %d taps: at most CONV_MAX_TAPS = %d are convolved" % (max(taps), CONV_MAX_TAPS))
    if sh is not None:
        for i, (d, k) in enumerate(zip(sh, taps)):
            if not 0 <= d < max(k, 1):
                raise ValueError("shifts[%d] = %d outside its filter of %d taps" % (i, d, k))
    if hl is None and _args.row_stride(filters) != kmax:
        hl = taps                                         # a strided view: the row's width, not its stride, bounds it
    y = torch.empty((n, L), dtype=torch.float32, device=dev) if out is None else _args.check_out(out, n, L, dev, torch.float32, exact=True)
    if out is not None and (_overlap(y, signal) or _overlap(y, filters)):
        raise ValueError("out must not overlap signal or filters: the convolution does not run in place")
    if n and L:
        xdev = torch.tensor(xl, dtype=torch.int32, device=dev) if xl is not None else None
        hdev = torch.tensor(hl, dtype=torch.int32, device=dev) if hl is not None else None
        sdev = torch.tensor(sh, dtype=torch.int32, device=dev) if sh is not None else None
        _lib.check(_lib.load().rced_convolve(signal.data_ptr(), _args.row_stride(signal), ptr(xdev), filters.data_ptr(),
                                             _args.row_stride(filters), ptr(hdev), ptr(sdev), n, L, y.data_ptr(), L, dev.index,
                                             _args.current_stream(dev)))
    return y[0] if one else y


def denoise_and_score(forward, mix, clean, lengths, nfft=512, kernels="x6", stoi=False, extra=(), rebuild="reference", framing=None):
    """The device core of the evaluation loop (tester.py:100-146 / trainer.py:260-307 without PESQ / wav files):
    STFT of the mixtures -> forward (device [N, T, 129, 1] -> same) -> ISTFT rebuild -> SDR (and, with stoi=True, STOI) of
    every rebuilt row against its clean row over its own length.  mix, clean: torch.cuda float32 [N, L] zero-padded;
    lengths: N sample counts.  extra: names from EXTRA_METRICS + SPECTRAL_METRICS + PROJECTION_METRICS + SEPM_METRICS, further
    scores of the same pairs ("llr" is the form limited at 2, "bss_sdr" BSS Eval's SDR with 512 taps, "cd" at LLR's order).
    Returns (audio [N, (T+1)*128] on the device -- the caller trims row n to lengths[n] --, sdr torch.float64 [N]), with
    stoi=True (audio, sdr, stoi torch.float64 [N]); with extra, one more element last: a dict name -> torch.float64 [N]
    (STOI and ESTOI, asked for together, come from one rced_stoi_ex call).
    rebuild: "reference" or "ola" (audio.istft_batch; "ola" rebuilds utterance n from its own num_frames(lengths[n]) frames).
    framing: an audio.Framing for the STFT and the rebuild (the audio is then [N, (W - S) + T * S]), or None for the default."""
    from . import audio
    extra = check_extra(extra)
    _args.check_rebuild(rebuild, kernels)
    if rebuild == "reference":
        audio.check_reference_rebuild(framing)       # before any device work
    mag, phase = audio.stft_batch(mix, lengths, kernels=kernels, framing=framing)
    pred = forward(mag)
    frames = [audio.num_frames(v, framing) for v in _args.host_ints(lengths)] if rebuild == "ola" else None
    out = audio.istft_batch(pred, phase, nfft, kernels=kernels, rebuild=rebuild, frames=frames, framing=framing)
    scored = (out, sdr_batch(clean, out, lengths))
    more = {}
    if stoi and "estoi" in extra:
        st, more["estoi"] = stoi_batch(clean, out, lengths, SAMPLE_RATE, extended="both")
        scored += (st,)
    elif stoi:
        scored += (stoi_batch(clean, out, lengths, SAMPLE_RATE),)
    for name, (batch, kw) in list(_EXTRA.items()) + list(_EXTRA_SEPM.items()):
        if name in extra and name not in more:
            more[name] = batch(clean, out, lengths, **kw)
    return scored + ({name: more[name] for name in extra},) if extra else scored
