"""Host-side mirror of the reference's scoring helpers (model_utils/utils.py:13-29, 64-90) over the C ABI.

AverageMeter is plain Python.  SDR keeps the reference's call surface -- `SDR()(y, y_pred)`, numpy 1-D in, Python float
out -- and computes on the device (rced_sdr); a batch is scored without leaving the device by `audio.sdr_batch`.
PESQ and STOI are not built (the reference takes them from pypesq / pystoi).
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
