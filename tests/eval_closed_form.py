"""numpy float64 restatements the evaluation-loop tests compare against (not a test module).

`tiled_noise` / `mix` write AudioParser.add_noise (data_utils/data_loader.py:35-52) without its doubling buffer: the
buffer after n doublings holds noise[p % ln] * prod(u_k for every bit k set in p // ln) at position p.  Checked against
the reference's own output (tests/golden/eval_ref.npz) by tests/test_eval_host.py, so the GPU tests may use it where
the reference cannot run (speech hundreds of times longer than the noise)."""

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS32 = float(np.finfo(np.float32).eps)
NFFTS, GAINS = (512, 256), (1.0, 0.5)


def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "eval_ref.npz"))
    return {k: z[k] for k in z.files}


def rebuilt(gold, i, nfft, gain):
    """The reference's rebuilt signal (float32); only gain 1 is stored, gain 0.5 is bit for bit half of it."""
    return np.float32(gain) * gold["rebuilt_%d_%d_10" % (i, nfft)]


def tiled_noise(noise, ls, start, gains):
    noise = np.asarray(noise, np.float64)
    ln = len(noise)
    if ls < ln:
        return noise[start:start + ls]
    p = np.arange(ls)
    q, r = p // ln, p % ln
    g = np.ones(ls)
    for k, u in enumerate(gains):
        g = np.where((q >> k) & 1, g * u, g)
    assert not (q >> len(gains)).any(), "a tile index has a bit without a gain"
    return noise[r] * g


def mix(speech, noise, snr, start, gains):
    speech = np.asarray(speech, np.float64)
    back = tiled_noise(noise, len(speech), start, gains)
    p_sig, p_back = np.sum(speech ** 2), np.sum(back ** 2)
    return speech + np.sqrt(p_sig / (10 ** (snr / 10)) / p_back) * back


def sdr(y, y_pred):
    """SDR.sdr's formula (model_utils/utils.py:76-78) on arrays widened to float64."""
    y, y_pred = np.asarray(y, np.float64), np.asarray(y_pred, np.float64)
    with np.errstate(divide="ignore"):
        return 10 * np.log10(np.sum(y ** 2) / (np.sum((y_pred - y) ** 2) + EPS32))
