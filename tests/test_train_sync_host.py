"""CPU tests of the float64 restatement of the synchronised sharded step (tests/train_sync_np.py): over
the row ranges of one batch it IS the unsharded step, per-shard BatchNorm (tests/train_shard_np.py) is not, and ragged
shards share the statistics of all their pixels."""

import functools

import numpy as np
import pytest

from conftest import NETS
from oracle import rced_np, train_ref
from test_train_gpu import LOOSE, rel

import train_shard_np
import train_sync_np

# Restatement against restatement, both float64, the same arithmetic in another order of summation: a sum of n terms moves
# by at most n 2^-53 of the sum of its terms' sizes; the longest sums here run over the 3 x 9 x 129 = 3483 < 2^12 pixels of
# a channel, and an error made at one of the 16 layers passes through at most 16 layers forward and 16 backward: at most
# 2 * 16 * 2^12 * 2^-53 = 2^-36 of a tensor's scale in the worst case (no cancellation assumed anywhere; what is measured
# is around 2^-48).
F64_BAR = 2.0 ** 16 * 2.0 ** -52

PARTITIONS = {"2+1": [(0, 2), (2, 3)], "1+1+1": [(0, 1), (1, 2), (2, 3)], "1+2": [(0, 1), (1, 3)]}


def batch(variant):
    return rced_np.make_input(3, 9, seed=70 + variant), rced_np.make_input(3, 9, seed=80 + variant)


@functools.lru_cache(maxsize=None)
def whole(net_work, variant):
    """Once per net, shared and left unchanged: the unsharded float64 gradient and step over the whole 3 x 9 batch."""
    w = rced_np.make_weights(net_work, seed=7)
    x, y = batch(variant)
    a = train_ref.TrainRef(net_work, w, batch_size=8)
    loss, g, _ = a.loss_and_grads(x, y)
    b = train_ref.TrainRef(net_work, w, batch_size=8)
    b.train_step(x, y, 1e-3)
    return loss, {k: v.numpy() for k, v in g.items()}, b.weights()


def cut(x, y, bounds):
    return [(x[a:b], y[a:b]) for a, b in bounds]


@pytest.mark.parametrize("part", sorted(PARTITIONS))
@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_synchronised_restatement_is_the_unsharded_step(net_work, tag, variant, part):
    loss_un, g_un, v_un = whole(net_work, variant)
    x, y = batch(variant)
    ref = train_ref.TrainRef(net_work, rced_np.make_weights(net_work, seed=7), batch_size=8)
    loss, g, step = train_sync_np.synced_step(ref, cut(x, y, PARTITIONS[part]), 1e-3)
    v = ref.weights()
    assert step == 1 and abs(loss - loss_un) <= F64_BAR * abs(loss_un)
    # A bias in front of a BatchNorm layer has gradient 0: what is left is rounding, on both sides, with no scale of its
    # own (and Adam turns it into a step of its sign).  It is held to the bar at the scale of its layer's kernel gradient.
    dead = [k for k in g_un if k.endswith("/bias") and (k[:-5] + "/batch_norm/gamma") in g_un]
    for k in dead:
        assert max(np.abs(g[k].numpy()).max(), np.abs(g_un[k]).max()) <= F64_BAR * np.abs(g_un[k[:-5] + "/kernel"]).max(), k
    worst = max(rel(g[k].numpy(), g_un[k]) for k in g_un if k not in dead)
    worst_v = max(rel(v[k], v_un[k]) for k in v_un if k not in dead)   # every variable after Adam, and the moving statistics
    print("[%s %s] gradient %.2e, variables %.2e of the tensor's scale" % (net_work, part, worst, worst_v))
    assert g.keys() == g_un.keys() and len(dead) < len(g_un) and worst <= F64_BAR, worst
    assert any("moving_" in k for k in v_un) and worst_v <= F64_BAR, worst_v


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_per_shard_batchnorm_misses_the_whole_batch_gradient_and_the_synchronised_step_does_not(net_work, tag, variant):
    """The feature's reason, on the reference alone: 2 + 1 rows with per-shard BatchNorm miss the whole batch's gradient by
    more than LOOSE (the bar a device gradient is held to) on at least one tensor, with shared statistics on none."""
    _, g_un, _ = whole(net_work, variant)
    x, y = batch(variant)
    w = rced_np.make_weights(net_work, seed=7)
    shards = cut(x, y, PARTITIONS["2+1"])
    _, g_sh, _ = train_shard_np.sharded_step(train_ref.TrainRef(net_work, w, batch_size=8), shards, 1e-3)
    _, g_sy, _ = train_sync_np.synced_step(train_ref.TrainRef(net_work, w, batch_size=8), shards, 1e-3)
    # (the bias in front of a BatchNorm layer has gradient 0 up to rounding: no scale to hold a distance against)
    names = [n for n in g_un if not (n.endswith("/bias") and (n[:-5] + "/batch_norm/gamma") in g_un)]
    miss_sh = [n for n in names if rel(g_sh[n].numpy(), g_un[n]) > LOOSE]
    miss_sy = [n for n in names if rel(g_sy[n].numpy(), g_un[n]) > LOOSE]
    print("[%s] per-shard BatchNorm misses LOOSE on %d of %d tensors (worst %.2f), synchronised on %d"
          % (net_work, len(miss_sh), len(names), max(rel(g_sh[n].numpy(), g_un[n]) for n in names), len(miss_sy)))
    assert miss_sh and not miss_sy


def test_ragged_shards_share_the_statistics_of_all_their_pixels():
    """2 x 9 frames and 1 x 1 frame: the first BatchNorm layer's pre-activations depend on no normalisation, so its shared
    statistics must be the pixel-weighted combination of what each shard has alone (19 frames' pixels in all); and the
    one-frame shard is not normalised by its own variance: changing the OTHER shard alone changes its output."""
    net_work = "FullyCNNV3"
    w = rced_np.make_weights(net_work, seed=7)
    xa, xb = rced_np.make_input(2, 9, seed=61), rced_np.make_input(1, 1, seed=63)
    ref = train_ref.TrainRef(net_work, w, batch_size=8)
    import torch
    with torch.no_grad():
        preds, stats = train_sync_np.forward_sync(ref, [xa, xb])
        (_, sa), (_, sb) = ref.forward_train(xa), ref.forward_train(xb)
        preds2, _ = train_sync_np.forward_sync(ref, [rced_np.make_input(2, 9, seed=62), xb])
        alone, _ = ref.forward_train(xb)
    assert [tuple(p.shape) for p in preds] == [(2, 9, 129, 1), (1, 1, 129, 1)]
    assert all(n == 19 * 129 for _, _, _, n in stats)
    (scope, mean, var, n), (scope_a, ma, va, na), (scope_b, mb, vb, nb) = stats[0], sa[0], sb[0]
    assert scope == scope_a == scope_b and na == 18 * 129 and nb == 129
    want_mean = (na * ma + nb * mb) / n
    want_var = (na * (va + ma * ma) + nb * (vb + mb * mb)) / n - want_mean * want_mean
    assert rel(mean.numpy(), want_mean.numpy()) < 1e-12 and rel(var.numpy(), want_var.numpy()) < 1e-10
    assert rel(var.numpy(), vb.numpy()) > 1e-2                      # not the one-frame shard's own variance
    assert rel(preds2[1].numpy(), preds[1].numpy()) > 1e-3          # the other shard's content reaches it through the statistics
    assert rel(alone.numpy(), preds[1].numpy()) > 1e-3              # and it is not what the shard gives alone


def test_sync_symbols_are_bound():
    """The new entry points are in the ctypes table under the names the header declares (test_abi.py holds the two equal
    and checks the library's exports)."""
    from fullycnnspeechenhancement_amd import _lib
    for name in ("points", "begin", "next", "end", "abort", "reduce"):
        assert "rced_train_sync_" + name in _lib.SYMBOLS
    assert "rced_train_copy_variables" in _lib.SYMBOLS
