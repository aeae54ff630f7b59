"""CR-CED V3, bin 128: the product form computes a frame's last bin in a tail shared by the four frames of a workgroup tile (layers 2
and 3 of every block) and hands its partials to the frame's right-hand wave.  These cases put the weight of the output on bins
120..128 -- loud inputs there, and frequency kernels whose right-hand taps (the ones through which bin 128 reaches bins 124..127)
are raised -- where a wrong hand-off would show, and run utterance lengths that leave a workgroup tile with one to three frames.
Held at 5e-6 of the scale against the fp32-MFMA comparator, these tests would also pass a hand-off that only changed the order of
the additions; that the product's masks are bit-identical to the form before the tail is shown by comparing `bench.py
--dump-outputs` of both builds (np.array_equal), not here."""
import numpy as np
import pytest

from conftest import RTOL, check_parity, rel_err
from oracle import rced_c, rced_np

pytestmark = pytest.mark.gpu

V3_FORMS_AGREE = 5e-6   # the product vs the fp32-MFMA comparator: fp32 summation noise (as in test_forward_gpu.py)


def _edge_weights(seed, gain=3.0):
    """Synthetic V3 weights with the taps right of centre of every 1 x K frequency kernel raised by `gain`."""
    w = rced_np.make_weights("FullyCNNV3", seed=seed)
    for k, v in w.items():
        if v.ndim == 4 and v.shape[0] == 1 and v.shape[1] in (5, 9):
            v = v.copy()
            v[:, v.shape[1] // 2 + 1:] *= np.float32(gain)
            w[k] = v
    return w


def _models(w):
    from fullycnnspeechenhancement_amd import model as M
    prod = M.FullyCNNSEModelV3(False, weights=w, device=0)
    assert prod.get_option("v3_l2x6") == 3
    comp = M.FullyCNNSEModelV3(False, weights=w, device=0)
    comp.set_option("v3_l2x6", 0)
    return prod, comp


def _edge_input(n, t, seed, scale):
    """Magnitudes with bins 120..128 raised by `scale` (the rest as usual)."""
    x = rced_np.make_input(n, t, seed=seed)
    x[:, :, 120:129] *= np.float32(scale)
    return x


def _check(prod, comp, w, x, what):
    ref = rced_c.forward("FullyCNNV3", w, x, np.float64)
    yp, yc = np.asarray(prod(x)), np.asarray(comp(x))
    check_parity(yp, ref, what="%s product" % what)
    check_parity(yc, ref, what="%s comparator" % what)
    n, t = x.shape[:2]
    ep, ec = yp.reshape(n, t, -1)[:, :, 120:129], yc.reshape(n, t, -1)[:, :, 120:129]
    err = float(np.abs(ep.astype(np.float64) - ec).max() / max(np.abs(yc).max(), 1e-30))
    assert err <= V3_FORMS_AGREE, (what, err)
    assert rel_err(yp, ref) <= RTOL
    return err


@pytest.mark.parametrize("t", range(1, 10))
def test_bin128_single_utterance_every_short_length(t, built):
    """Batch 1, T = 1..9: one workgroup tile with 1..4 real frames, then a second one."""
    w = _edge_weights(128 + t)
    prod, comp = _models(w)
    _check(prod, comp, w, _edge_input(1, t, seed=900 + t, scale=30.0), "B=1 T=%d" % t)


@pytest.mark.parametrize("t", [37, 38, 39])
def test_bin128_ragged_batches(t, built, capsys):
    """T mod 4 = 1, 2, 3 over a few utterances (the last tile of each holds fewer than four frames), edge bins raised by 1 .. 1000."""
    w = _edge_weights(4000 + t)
    prod, comp = _models(w)
    worst = 0.0
    for k, scale in enumerate((1.0, 30.0, 1000.0)):
        worst = max(worst, _check(prod, comp, w, _edge_input(3, t, seed=77 * t + k, scale=scale), "B=3 T=%d x%g" % (t, scale)))
    with capsys.disabled():
        print("\n[bin 128, T=%d] bins 120..128, the product vs the fp32-MFMA form: %.2e of the scale" % (t, worst))


def test_bin128_only_the_edge_is_loud(built):
    """Every bin but 120..128 silent: the output there comes from the tail and its neighbours alone."""
    w = _edge_weights(31)
    prod, comp = _models(w)
    x = rced_np.make_input(2, 11, seed=5)
    x[:, :, :120] = 0.0
    x[:, :, 120:129] *= np.float32(100.0)
    _check(prod, comp, w, x, "edge only")
