"""CR-CED V3, layer 1's tap 8: the product form computes the ninth frequency tap of every 1 x 9 (first layer: 8 x 9) layer-1 kernel in
two MFMAs whose k-quads hold four / two of the tap's six three-part products (kernels_fused_v3_l23.h, layer1_x6l) instead of in a
third K = 32 chunk beside three zero taps.  These cases put the weight of the layer on that tap, or take it away, in all five
blocks (the first layer included), at small and large input scales and on utterance lengths that leave a workgroup tile with one to
three frames.  Every case is held to the suite's two bars: 1e-4 of the scale against the oracle in float64 (conftest.check_parity)
and 5e-6 of the scale against the fp32-MFMA comparator (option v3_l2x6 = 0), which does not know the fold."""
import numpy as np
import pytest

from conftest import RTOL, check_parity, rel_err
from oracle import rced_c, rced_np

pytestmark = pytest.mark.gpu

V3_FORMS_AGREE = 5e-6   # the product vs the fp32-MFMA comparator: fp32 summation noise (as in test_forward_gpu.py)
LENGTHS = (1, 3, 5, 41)


def _l1_weights(seed, mode):
    """Synthetic V3 weights whose layer-1 kernels ([rows, 9 taps, cin, 18], all five blocks) are changed along the tap axis:
    "only8" = zero except tap 8, "no8" = tap 8 zero, "big8" = tap 8 a thousand times the other taps (they are scaled by 1e-3)."""
    w = rced_np.make_weights("FullyCNNV3", seed=seed)
    n = 0
    for k in list(w):
        v = w[k]
        if k.endswith("_encode_1/kernel"):
            assert v.ndim == 4 and v.shape[1] == 9 and v.shape[3] == 18, (k, v.shape)
            v = v.copy()
            if mode == "only8":
                v[:, :8] = 0.0
            elif mode == "no8":
                v[:, 8] = 0.0
            elif mode == "big8":
                v[:, :8] *= np.float32(1e-3)
            else:
                raise ValueError(mode)
            w[k] = v
            n += 1
    assert n == 5
    return w


def _models(w):
    from fullycnnspeechenhancement_amd import model as M
    prod = M.FullyCNNSEModelV3(False, weights=w, device=0)
    assert prod.get_option("v3_l2x6") == 3
    comp = M.FullyCNNSEModelV3(False, weights=w, device=0)
    comp.set_option("v3_l2x6", 0)
    return prod, comp


def _check(prod, comp, w, x, what):
    """-> (error of the product against the oracle, against the comparator), both of the scale; printed before they are asserted"""
    ref = rced_c.forward("FullyCNNV3", w, x, np.float64)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0, what
    yp, yc = np.asarray(prod(x)), np.asarray(comp(x))
    eo, ef = rel_err(yp, ref), rel_err(yp, yc)
    print("[l1 fold] %-34s vs fp64 %.2e  vs fp32-MFMA %.2e" % (what, eo, ef))
    check_parity(yp, ref, what="%s product" % what)
    check_parity(yc, ref, what="%s comparator" % what)
    assert eo <= RTOL, (what, eo)
    assert ef <= V3_FORMS_AGREE, (what, ef)
    return eo, ef


@pytest.mark.parametrize("mode", ["only8", "no8"])
def test_l1_tap8_alone_and_absent(mode, built, capsys):
    """Layer 1 is tap 8 only (everything it computes goes through the folded MFMAs) / has no tap 8 (the folded MFMAs add zeros),
    T = 1, 3, 5, 41 at batch 1..3."""
    w = _l1_weights(70 + len(mode), mode)
    prod, comp = _models(w)
    with capsys.disabled():
        print()
        for i, t in enumerate(LENGTHS):
            _check(prod, comp, w, rced_np.make_input(1 + i % 3, t, seed=300 + t), "%s B=%d T=%d" % (mode, 1 + i % 3, t))


@pytest.mark.parametrize("scale", [1e-3, 30.0])
def test_l1_tap8_a_thousand_times_the_other_taps(scale, built, capsys):
    """Tap 8's products are a thousand times the other taps': the small terms of chunks 0 and 1 meet the folded MFMAs' large ones in one
    accumulator.  Input scales 1e-3 and 30, T = 1, 3, 5, 41."""
    w = _l1_weights(91, "big8")
    prod, comp = _models(w)
    with capsys.disabled():
        print()
        for i, t in enumerate(LENGTHS):
            x = rced_np.make_input(1 + (i + 1) % 3, t, seed=500 + t) * np.float32(scale)
            _check(prod, comp, w, x, "big8 x%g B=%d T=%d" % (scale, x.shape[0], t))


@pytest.mark.parametrize("mode", ["only8", "big8"])
def test_l1_fold_nan_stays_inside_its_receptive_field(mode, built):
    """A NaN magnitude in one input bin, (utterance 1, frame 24, bin 60), with layer 1 resting on tap 8.  Frame t of the output needs
    frames t - 3 .. t + 4 of the input, so frames 20..27 are the NaN's receptive field; every frame outside it is bit-identical to the
    run on the clean input.  (What the kernel guarantees is stated per workgroup tile of four frames -- zero-weight k-slots turn
    NaN x 0 into NaN inside a tile, test_forward_gpu.test_non_finite_input_stays_inside_its_tiles -- and frame 24 is chosen so that
    its field is exactly tiles 20..23 and 24..27: the assertion is the strict one.  The folded MFMA's k-quads with zero weights read
    the row of the SAME pixel as the others, so they add no reach.)"""
    w = _l1_weights(17, mode)
    prod, _ = _models(w)
    x = rced_np.make_input(3, 41, seed=6)
    clean = np.asarray(prod(x))
    xb = x.copy()
    xb[1, 24, 60, 0] = np.nan
    y = np.asarray(prod(xb))
    field = np.zeros((3, 41), bool)
    field[1, 20:28] = True
    assert np.isfinite(clean).all()
    differ = [(int(u), int(t)) for u, t in zip(*np.nonzero(~field)) if not np.array_equal(y[u, t], clean[u, t])]
    assert not differ, "frames (utterance, frame) outside the field that changed: %s" % differ
    assert not np.array_equal(y[field], clean[field])
    assert np.array_equal(np.asarray(prod(x)), clean)
