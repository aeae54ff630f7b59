"""The cases of test_train_tiles_gpu.py are not vacuous: from the fp64 restatement alone (no device).
(1) Every (net, shape, margin) finds its screened input within screened_input's 400 draws.  (2) For the 3 x 3 and 5 x 5
inputs the device tests use, a kernel that mishandled the half-empty last tile would be seen: the loss term of the whole last
frame, or of its bin 128 only, is removed (that target set to the prediction), and every gradient tensor's distance from the
true gradient is measured the way the device test measures its error.  These are conditions on the inputs, not on the
device: an input that failed one would be replaced by the next screened seed, and that said here.  No input had to be;
the targets are chosen so that the border pixel's loss term is of ordinary size (train_tiles_cases.screened says why).
Measured: at most 59 draws (CR-CED, 1 x 9); last frame dropped, worst tensor 2.3e-2 and median at least 1.3e-1; its bin
128 dropped, worst tensor 4.9e-4 and median at least 1.0e-2."""

import numpy as np
import pytest

import train_tiles_cases as cases
from conftest import NETS
from test_train_gpu import TIGHT


@pytest.mark.parametrize("n,t", cases.SHAPES)
@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_every_case_finds_a_screened_input(net_work, tag, variant, n, t, capsys):
    x, y, seed, draws = cases.screened(net_work, n, t)       # raises where 400 draws were not enough
    with capsys.disabled():
        print("\n[tile cases] %s %dx%d margin %.0e: seed %d, %d draw(s)" % (net_work, n, t, cases.margin_of(n, t), seed, draws))
    assert x.shape == y.shape == (n, t, 129, 1) and 1 <= draws <= 400


@pytest.mark.parametrize("n,t", [(3, 3), (5, 5)])
@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_a_mishandled_last_tile_would_be_seen_at_tight(net_work, tag, variant, n, t, capsys):
    x, y, _, g_true = cases.reference(net_work, n, t)
    pred = cases.prediction(net_work, x)
    y_frame = np.asarray(y, np.float64).copy()
    y_frame[-1, -1] = pred[-1, -1]                # the last frame's loss term vanishes
    y_bin = np.asarray(y, np.float64).copy()
    y_bin[-1, -1, 128] = pred[-1, -1, 128]        # ... or only that of its bin 128 (the border tap of the half-empty tile)
    d_frame = cases.distances(cases.loss_and_grads(net_work, x, y_frame)[1], g_true)
    d_bin = cases.distances(cases.loss_and_grads(net_work, x, y_bin)[1], g_true)
    with capsys.disabled():
        print("\n[tile cases] %s %dx%d: last frame dropped min %.2e median %.2e; its bin 128 dropped min %.2e median %.2e (%d tensors)"
              % (net_work, n, t, min(d_frame.values()), np.median(list(d_frame.values())), min(d_bin.values()),
                 np.median(list(d_bin.values())), len(d_bin)))
    assert min(d_frame.values()) > 100 * TIGHT, min(d_frame, key=d_frame.get)
    assert np.median(list(d_bin.values())) > 10 * TIGHT
    assert min(d_bin.values()) >= TIGHT, min(d_bin, key=d_bin.get)
