"""Every gradient of every layer at TIGHT against the fp64 restatement, on the edges of the persistent tile loops of the
training kernels (kernels_train_mfma.h): half-empty last tiles, workgroups that walk several two-frame tiles, statistics
sums carried in registers and flushed mid-walk, T below, at and above the first layer's 8-row time kernel.
RCED_TRAIN_MAX_GRID caps the workgroup count so that batches of at most 25 frames -- small enough for screened inputs and
the tight bar -- walk tiles; every capped case asserts from FullyCNNTrainer.grid_stats() that the cap was honoured and the
walk is as long as train_tiles_cases.SHAPES promises, or it would only repeat the uncapped case.  The same cases anchor
every switched form of the step (RCED_TRAIN_* = 0) to fp64; elsewhere the forms are tight only against each other.
Inputs, references and why they are not vacuous: train_tiles_cases.py, test_train_tiles_host.py.

Measured on an MI355X, 81 cases: the loss within 2.2e-7; worst gradient error, of its tensor's largest entry, R-CED V1 2.0e-6
(1 x 17, cap 2), R-CED V2 4.8e-6 (1 x 9, cap 2), CR-CED 1.09e-5 (1 x 1: 129 pixels per BatchNorm channel); a bias in front of
BatchNorm at most 7.5e-7 of its kernel's gradient.  The file runs in under 5 s; every case prints its own figures before it asserts."""

import numpy as np
import pytest

import train_tiles_cases as cases
from conftest import NETS
from test_train_gpu import TIGHT

pytestmark = pytest.mark.gpu

ALL_SWITCHES = ["RCED_TRAIN_MFMA", "RCED_TRAIN_FUSE_ACT", "RCED_TRAIN_FUSE_DZ", "RCED_TRAIN_FUSE_SUMS", "RCED_TRAIN_FUSE_BWD", "RCED_TRAIN_X6",
                "RCED_TRAIN_DET"]
R_CED_SWITCHES = ["RCED_TRAIN_MFMA", "RCED_TRAIN_FUSE_ACT", "RCED_TRAIN_FUSE_DZ", "RCED_TRAIN_FUSE_SUMS", "RCED_TRAIN_FUSE_BWD"]


def step_on_device(net_work, n, t, cap, monkeypatch, switch=None):
    """One fresh trainer, one step: (loss, gradients, variables, grid_stats)."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    x, y, _, _ = cases.reference(net_work, n, t)
    if cap:
        monkeypatch.setenv("RCED_TRAIN_MAX_GRID", str(cap))
    else:
        monkeypatch.delenv("RCED_TRAIN_MAX_GRID", raising=False)
    if switch:
        monkeypatch.setenv(switch, "0")
    tr = FullyCNNTrainer(net_work, batch_size=cases.BATCH_SIZE, lr=1e-4, weights=cases.weights(net_work))
    try:
        loss, _, _ = tr.train_step(x, y)
        return loss, tr.gradients(), tr.variables(), tr.grid_stats()
    finally:
        tr.close()


def check_case(net_work, n, t, cap, monkeypatch, capsys, switch=None):
    _, _, loss_ref, g_ref = cases.reference(net_work, n, t)
    loss, g, _, (grid, walk) = step_on_device(net_work, n, t, cap, monkeypatch, switch)
    worst, dead = ("", 0.0), 0.0
    for name, gr in g_ref.items():
        if cases.dead_bias(name, g_ref):
            dead = max(dead, np.abs(g[name]).max() / max(np.abs(g[name[:-5] + "/kernel"]).max(), 1e-30))
            continue
        err = float(np.abs(g[name].astype(np.float64) - gr).max() / np.abs(gr).max())
        if err >= worst[1]:
            worst = (name, err)
    dloss = abs(loss - loss_ref) / abs(loss_ref)
    with capsys.disabled():
        print("\n[train tiles] %s %dx%d cap %s %s: grid %d, %d tile(s) per workgroup, loss %.2e, worst gradient %s %.2e of its max, "
              "dead bias %.1e of its kernel's" % (net_work, n, t, cap or "-", (switch + "=0") if switch else "default", grid, walk, dloss,
                                                 worst[0], worst[1], dead))
    if cap and switch != "RCED_TRAIN_MFMA":     # (RCED_TRAIN_MFMA=0 launches no tile-walking kernel: nothing to cap)
        assert (grid, walk) == cases.walk_of(n, t, cap), "the cap was not honoured: this case would repeat the uncapped one"
    assert dloss <= 1e-5
    assert worst[1] < TIGHT, worst
    assert dead <= 1e-4, "a bias in front of BatchNorm has gradient 0"


MATRIX = [(n, t, cap) for (n, t) in cases.SHAPES for cap in (0, 1, 2)] + [(5, 5, 3)]


@pytest.mark.parametrize("n,t,cap", MATRIX, ids=["%dx%d-cap%d" % c for c in MATRIX])
@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_every_gradient_tight_on_the_tile_edges(net_work, tag, variant, n, t, cap, built, monkeypatch, capsys):
    check_case(net_work, n, t, cap, monkeypatch, capsys)


@pytest.mark.parametrize("switch", ALL_SWITCHES)
@pytest.mark.parametrize("n,t,cap", [(3, 3, 1), (5, 5, 2)])
def test_every_switched_form_tight_on_cr_ced(n, t, cap, switch, built, monkeypatch, capsys):
    check_case("FullyCNNV3", n, t, cap, monkeypatch, capsys, switch)


@pytest.mark.parametrize("switch", R_CED_SWITCHES)
@pytest.mark.parametrize("net_work", ["FullyCNN", "FullyCNNV2"])
def test_every_switched_form_tight_on_the_r_ced_nets(net_work, switch, built, monkeypatch, capsys):
    check_case(net_work, 3, 3, 1, monkeypatch, capsys, switch)


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_a_capped_step_is_reproducible_bit_for_bit(net_work, tag, variant, built, monkeypatch):
    """3 x 3 under cap 1: one workgroup's slices in tmm::wg_reduce, fewer than on any other shape the suite runs."""
    a = step_on_device(net_work, 3, 3, 1, monkeypatch)
    b = step_on_device(net_work, 3, 3, 1, monkeypatch)
    assert a[3] == b[3] == cases.walk_of(3, 3, 1)
    assert a[0] == b[0]
    for part in (1, 2):
        for name in a[part]:
            assert np.array_equal(a[part][name].view(np.uint32), b[part][name].view(np.uint32)), name
