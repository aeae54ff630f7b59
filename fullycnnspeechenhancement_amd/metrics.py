"""Host-side mirror of the reference's scoring helpers (model_utils/utils.py:13-29, 64-90) over the C ABI.

AverageMeter is plain Python.  SDR keeps the reference's call surface -- `SDR()(y, y_pred)`, numpy 1-D in, Python float
out -- and computes on the device (rced_sdr); a batch is scored without leaving the device by `audio.sdr_batch`.
STOI does the same over rced_stoi / `audio.stoi_batch`; the reference takes it from pystoi, which this project cannot
reach: parity is pinned to the restatement of the published algorithm in tests/stoi_np.py (DESIGN.md "STOI").
PESQ is not built (the reference takes it from pypesq).
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


class SDR(object):
    """utils.py:64-90: 10 * log10(sum(y^2) / (sum((y_pred - y)^2) + float32 eps))."""

    def __init__(self, device=0):
        self.device = device

    def sdr(self, y, y_pred):
        import torch
        from . import audio
        y, y_pred = np.asarray(y), np.asarray(y_pred)
        if len(y.shape) != 1:                                   # the reference's two asserts (utils.py:74-75)
            raise ValueError("y must be a 1-D signal, got shape %s" % (y.shape,))
        if len(y) != len(y_pred):
            raise ValueError("y and y_pred must have the same length, got %d and %d" % (len(y), len(y_pred)))
        dev = "cuda:%d" % self.device
        both = torch.as_tensor(np.stack([y.astype(np.float32), y_pred.astype(np.float32).reshape(-1)]), device=dev)
        return float(audio.sdr_batch(both[0:1], both[1:2])[0])

    def __call__(self, x, y):
        return self.sdr(x, y)


class STOI(object):
    """The reference's `stoi(clean, denoise, sr, extended=False)` (tester.py:92-167) with SDR's call surface:
    `STOI(sr)(clean, processed)`, numpy 1-D in, Python float out, computed on the device (rced_stoi)."""

    def __init__(self, sr=8000, device=0):
        from . import audio
        if sr not in audio.STOI_RATES:
            raise ValueError("sr must be 8000 or 10000, got %r" % (sr,))
        self.sr, self.device = int(sr), device

    def stoi(self, x, y):
        import torch
        from . import audio
        x, y = np.asarray(x), np.asarray(y)
        if len(x.shape) != 1 or len(y.shape) != 1:
            raise ValueError("x and y must be 1-D signals, got shapes %s and %s" % (x.shape, y.shape))
        if len(x) != len(y):
            raise ValueError("x and y must have the same length, got %d and %d" % (len(x), len(y)))
        if len(x) == 0:
            return 1e-5
        dev = "cuda:%d" % self.device
        both = torch.as_tensor(np.stack([x.astype(np.float32), y.astype(np.float32)]), device=dev)
        return float(audio.stoi_batch(both[0:1], both[1:2], sample_rate=self.sr)[0])

    def __call__(self, x, y):
        return self.stoi(x, y)
