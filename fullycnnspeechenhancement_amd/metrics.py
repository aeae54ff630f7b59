"""Host-side mirror of the reference's scoring helpers (model_utils/utils.py:13-29, 64-90) over the C ABI.

AverageMeter is plain Python.  SDR keeps the reference's call surface -- `SDR()(y, y_pred)`, numpy 1-D in, Python float
out -- and computes on the device (rced_sdr); a batch is scored without leaving the device by `audio.sdr_batch`.
STOI does the same over rced_stoi / `audio.stoi_batch`; the reference takes it from pystoi, which this project cannot
reach: parity is pinned to the restatement of the published algorithm in tests/stoi_np.py (DESIGN.md "STOI").
ESTOI (pystoi's extended=True), SISDR (the optimal-scaling form the reference carries, commented out, inside SDR.sdr,
utils.py:80-85) and SegSNR have the same call surface over rced_stoi_ex / rced_si_sdr / rced_seg_snr; each is pinned to the
float64 restatement of its definition in tests/ (DESIGN.md "ESTOI", "SI-SDR", "Segmental SNR"), not to pystoi or pysepm.
LLR and WSS (rced_llr / rced_wss, pinned to tests/sepm_np.py in the same way) are the two spectral terms of the composite
measures of Hu and Loizou (2008); `composite` turns them, the segmental SNR and a PESQ column into CSIG / CBAK / COVL.
FwSegSNR and CepDist (rced_fwseg / rced_cepd, pinned to tests/sepm2_np.py) are the frequency-weighted segmental SNR and the
cepstral distance of the same paper.
BSSSDR (rced_bss_sdr, pinned to tests/bsseval_np.py) is the SDR of BSS Eval for one source: the estimate is projected onto
the clean signal's delayed copies first, so a fixed filtering or delay is forgiven.
PESQ is not built (the reference takes it from pypesq); everything else the composite measures need is.
"""

import numpy as np


class AverageMeter(object):
    """Computes and stores the average and current value (utils.py:13-29)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val          # as the reference: the sum grows by val, the count by n
        self.count += n
        self.avg = self.sum / self.count


def _pair(x, y):
    """Two 1-D signals of one length, as STOI takes them, stacked [2, L] float32."""
    x, y = np.asarray(x), np.asarray(y)
    if len(x.shape) != 1 or len(y.shape) != 1:
        raise ValueError("x and y must be 1-D signals, got shapes %s and %s" % (x.shape, y.shape))
    if len(x) != len(y):
        raise ValueError("x and y must have the same length, got %d and %d" % (len(x), len(y)))
    return np.stack([x.astype(np.float32), y.astype(np.float32)])


def _score_pair(batch_fn, pair, device, **kw):
    import torch
    both = torch.as_tensor(pair, device="cuda:%d" % device)
    return float(batch_fn(both[0:1], both[1:2], **kw)[0])


class SDR(object):
    """utils.py:64-90: 10 * log10(sum(y^2) / (sum((y_pred - y)^2) + float32 eps))."""

    def __init__(self, device=0):
        self.device = device

    def sdr(self, y, y_pred):
        from . import audio
        y, y_pred = np.asarray(y), np.asarray(y_pred)
        if len(y.shape) != 1:                                   # the reference's two asserts (utils.py:74-75)
            raise ValueError("y must be a 1-D signal, got shape %s" % (y.shape,))
        if len(y) != len(y_pred):
            raise ValueError("y and y_pred must have the same length, got %d and %d" % (len(y), len(y_pred)))
        return _score_pair(audio.sdr_batch, np.stack([y.astype(np.float32), y_pred.astype(np.float32).reshape(-1)]), self.device)

    def __call__(self, x, y):
        return self.sdr(x, y)


class _PairMetric(object):
    """What the mirrors below share: `Metric(...)(x, y)`, two numpy 1-D signals of one length in, a Python float out, from one
    audio.*_batch call over the single pair on cuda:`device`; `empty`: the score of two empty signals, given without a device.
    A subclass checks its arguments, keeps them as attributes and names its method after the score."""

    def __init__(self, device, method, empty, batch, **keywords):
        self.device, self._method, self._empty, self._batch, self._keywords = device, method, empty, batch, keywords

    def _score(self, x, y):
        from . import audio
        pair = _pair(x, y)
        if not pair.shape[1]:
            return self._empty
        return _score_pair(getattr(audio, self._batch), pair, self.device, **self._keywords)

    def __call__(self, x, y):
        return getattr(self, self._method)(x, y)


class STOI(_PairMetric):
    """The reference's `stoi(clean, denoise, sr, extended=False)` (tester.py:92-167) with SDR's call surface:
    `STOI(sr)(clean, processed)`, numpy 1-D in, Python float out, computed on the device (rced_stoi)."""

    def __init__(self, sr=8000, device=0):
        from . import audio
        if sr not in audio.STOI_RATES:
            raise ValueError("sr must be 8000 or 10000, got %r" % (sr,))
        self.sr = int(sr)
        _PairMetric.__init__(self, device, "stoi", 1e-5, "stoi_batch", sample_rate=self.sr)

    def stoi(self, x, y):
        return self._score(x, y)


class ESTOI(_PairMetric):
    """Extended STOI (Jensen, Taal 2016; pystoi's `stoi(clean, denoise, sr, extended=True)`) with STOI's call surface:
    `ESTOI(sr)(clean, processed)`, numpy 1-D in, Python float out, computed on the device (rced_stoi_ex)."""

    def __init__(self, sr=8000, device=0):
        from . import audio
        if sr not in audio.STOI_RATES:
            raise ValueError("sr must be 8000 or 10000, got %r" % (sr,))
        self.sr = int(sr)
        _PairMetric.__init__(self, device, "estoi", 1e-5, "stoi_batch", sample_rate=self.sr, extended=True)

    def estoi(self, x, y):
        return self._score(x, y)


class SISDR(_PairMetric):
    """Scale-invariant SDR, `SISDR()(y, y_pred)` as `SDR()(y, y_pred)`: numpy 1-D in, Python float (dB) out, computed on the
    device (rced_si_sdr).  Two empty signals give nan, as the definition does."""

    def __init__(self, device=0):
        _PairMetric.__init__(self, device, "si_sdr", float("nan"), "si_sdr_batch")

    def si_sdr(self, y, y_pred):
        return self._score(y, y_pred)


class BSSSDR(_PairMetric):
    """The SDR of BSS Eval for one source, `BSSSDR(filter_length)(y, y_pred)` as `SISDR()(y, y_pred)`: numpy 1-D in, Python
    float (dB) out, computed on the device (rced_bss_sdr): the estimate is scored after its projection onto the clean signal
    delayed by 0 .. filter_length - 1 samples (512 as bss_eval_sources has it; parity with mir_eval is unpinned, the pin is
    tests/bsseval_np.py).  Two empty signals give nan, as the definition does."""

    def __init__(self, filter_length=512, device=0):
        from . import evaluation
        self.filter_length = evaluation._filter_length(filter_length)      # ValueError outside 1 .. 512
        _PairMetric.__init__(self, device, "bss_sdr", float("nan"), "bss_sdr_batch", filter_length=self.filter_length)

    def bss_sdr(self, y, y_pred):
        return self._score(y, y_pred)


class SegSNR(_PairMetric):
    """Segmental SNR, `SegSNR(sr)(clean, processed)`: numpy 1-D in, Python float (dB) out, computed on the device
    (rced_seg_snr).  Signals shorter than one frame give nan."""

    def __init__(self, sr=8000, device=0):
        from . import audio
        self.window = audio.seg_snr_window(sr)           # ValueError for a rate the library refuses
        self.sr = int(sr)
        _PairMetric.__init__(self, device, "seg_snr", float("nan"), "seg_snr_batch", sample_rate=self.sr)

    def seg_snr(self, x, y):
        return self._score(x, y)


class LLR(_PairMetric):
    """Log-likelihood ratio of the LPC models, `LLR(sr, limit)(clean, processed)`: numpy 1-D in, Python float out, computed
    on the device (rced_llr).  limit: the cap on a frame's value (2 as published; None for none, the form `composite`
    takes).  Signals shorter than one frame give nan."""

    def __init__(self, sr=8000, limit=2.0, device=0):
        from . import audio
        if sr not in audio.SPECTRAL_RATES:
            raise ValueError("sr must be 8000 or 16000, got %r" % (sr,))
        if limit is not None and float(limit) != float(limit):
            raise ValueError("limit must be a number or None, got nan")
        self.sr, self.limit = int(sr), limit
        _PairMetric.__init__(self, device, "llr", float("nan"), "llr_batch", sample_rate=self.sr, limit=limit)

    def llr(self, x, y):
        return self._score(x, y)


class WSS(_PairMetric):
    """Weighted spectral slope distance, `WSS(sr)(clean, processed)`: numpy 1-D in, Python float out, computed on the device
    (rced_wss).  Signals shorter than one frame give nan."""

    def __init__(self, sr=8000, device=0):
        from . import audio
        if sr not in audio.SPECTRAL_RATES:
            raise ValueError("sr must be 8000 or 16000, got %r" % (sr,))
        self.sr = int(sr)
        _PairMetric.__init__(self, device, "wss", float("nan"), "wss_batch", sample_rate=self.sr)

    def wss(self, x, y):
        return self._score(x, y)


class FwSegSNR(_PairMetric):
    """Frequency-weighted segmental SNR, `FwSegSNR(sr)(clean, processed)`: numpy 1-D in, Python float (dB) out, computed on the
    device (rced_fwseg).  Signals shorter than one frame give nan."""

    def __init__(self, sr=8000, device=0):
        from . import audio
        if sr not in audio.SPECTRAL_RATES:
            raise ValueError("sr must be 8000 or 16000, got %r" % (sr,))
        self.sr = int(sr)
        _PairMetric.__init__(self, device, "fw_seg_snr", float("nan"), "fw_seg_snr_batch", sample_rate=self.sr)

    def fw_seg_snr(self, x, y):
        return self._score(x, y)


class CepDist(_PairMetric):
    """Cepstral distance of the LPC models, `CepDist(sr, order)(clean, processed)`: numpy 1-D in, Python float out, computed on
    the device (rced_cepd).  order: None for LLR's order at the rate, or an integer in [1, 16].  Signals shorter than one
    frame give nan."""

    def __init__(self, sr=8000, order=None, device=0):
        from . import audio, evaluation
        if sr not in audio.SPECTRAL_RATES:
            raise ValueError("sr must be 8000 or 16000, got %r" % (sr,))
        self.sr, self.order = int(sr), evaluation._cep_order(order, sr)      # ValueError outside 1 .. 16
        _PairMetric.__init__(self, device, "cd", float("nan"), "cep_dist_batch", sample_rate=self.sr, order=self.order)

    def cd(self, x, y):
        return self._score(x, y)


def composite(pesq, llr, wss, seg_snr):
    """The composite measures of Hu and Loizou (2008), elementwise over numpy-broadcastable columns, on the host:
        CSIG = 3.093 - 1.029 LLR + 0.603 PESQ - 0.009 WSS
        CBAK = 1.634 + 0.478 PESQ - 0.007 WSS + 0.063 segSNR
        COVL = 1.594 + 0.805 PESQ - 0.512 LLR - 0.007 WSS
    each clipped to [1, 5].  llr is the unlimited form (audio.llr_batch(limit=None) / LLR(limit=None)), wss and seg_snr as
    audio.wss_batch and audio.seg_snr_batch give them.  pesq is the caller's: this project does not compute it.
    Returns (csig, cbak, covl), numpy float64."""
    pesq, llr, wss, seg_snr = (np.asarray(v, np.float64) for v in (pesq, llr, wss, seg_snr))
    csig = 3.093 - 1.029 * llr + 0.603 * pesq - 0.009 * wss
    cbak = 1.634 + 0.478 * pesq - 0.007 * wss + 0.063 * seg_snr
    covl = 1.594 + 0.805 * pesq - 0.512 * llr - 0.007 * wss
    return tuple(np.clip(v, 1.0, 5.0) for v in (csig, cbak, covl))
