"""The inputs and fp64 references of the tile-walk tests (test_train_tiles_gpu.py runs them on the device,
test_train_tiles_host.py shows from the restatement alone that they are not vacuous).  Test infrastructure: oracle only.

Every shape is the smallest that reaches one edge of the persistent tile loops of kernels_train_mfma.h (two-frame tiles,
sums carried over kSumFlush = 4 tiles); see SHAPES.  Every input is screened as test_train_gpu.screened_input screens: no
value entering a ReLU within the margin of zero in the fp64 restatement, so no ReLU mask can flip on the device and every
gradient can be held to TIGHT.  The margin is screened_input's 1e-5 up to 9 frames and, from 16 frames up, the 3e-6 of
test_train_sync_gpu.RAGGED_MARGIN for its reason: the device's fp32 pre-activations differ from fp64 by about 1e-6 at unit
scale, and 1e-5 would leave too few draws at that many pixels."""

import functools

import numpy as np
import torch

from oracle import rced_np, train_ref
from test_train_gpu import screened_input

K_TF, K_SUM_FLUSH = 2, 4          # tmm::kTF, tmm::kSumFlush
WEIGHT_SEED, BATCH_SIZE = 11, 4   # (the configured batch size the loss divides by, not the dynamic N)

# (N, T): frames, tiles -- what it reaches
SHAPES = [
    (1, 1),    # 1 frame, 1 tile: one half-empty tile and nothing else; every time tap of the first layer but one in padding
    (3, 3),    # 9 frames, 5 tiles: odd, tiles straddle utterances; cap 1: a flush at the fourth tile, then a half-empty fifth
    (1, 9),    # 9 frames, 5 tiles: T above the first layer's 8-row time kernel in one utterance
    (2, 8),    # 16 frames, 8 tiles: T equal to the kernel height, every tile full; cap 1: two complete flush periods
    (1, 17),   # 17 frames, 9 tiles: cap 2: a five-tile walk and a four-tile walk
    (5, 5),    # 25 frames, 13 tiles: cap 2: walks of seven and six tiles; cap 3: three walks of uneven length
]
VARIANT = {"FullyCNN": 1, "FullyCNNV2": 2, "FullyCNNV3": 3}


def margin_of(n, t):
    return 1e-5 if n * t <= 9 else 3e-6


def ntiles(n, t):
    return (n * t + K_TF - 1) // K_TF


def walk_of(n, t, cap):
    """(grid, tiles per workgroup) of a tile-walking launcher under a cap of `cap` workgroups."""
    grid = min(ntiles(n, t), cap)
    return grid, (ntiles(n, t) + grid - 1) // grid


def seed_base(net_work, n, t):
    return 20000 + 20000 * VARIANT[net_work] + 2000 * SHAPES.index((n, t))


def weights(net_work):
    return rced_np.make_weights(net_work, seed=WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def screened(net_work, n, t):
    """Once per (net, shape): (x, y, seed of x, draws the screen needed).
    The target is a condition on the inputs too.  What a wrong border tap of the last tile does to the gradients is
    proportional to the loss term of the pixel it touches, and with a target drawn independently of the prediction that one
    residual is small by chance in one draw of a few (measured: 3 % of the batch's RMS residual at R-CED V1's first 3 x 3
    draw, and every tensor's sensitivity 17 times below the typical one).  So the target is the first draw whose residual
    at the last frame's bin 128 is at least half the RMS residual of the batch: a loss term of ordinary size."""
    ref = train_ref.TrainRef(net_work, weights(net_work), batch_size=BATCH_SIZE)
    base = seed_base(net_work, n, t)
    x, seed = screened_input(ref, n, t, base, margin=margin_of(n, t))
    pred = prediction(net_work, x)
    for s in range(400):
        y = rced_np.make_input(n, t, seed=base + 1000 + s)
        r = y - pred
        if abs(r[-1, -1, 128, 0]) >= 0.5 * np.sqrt((r ** 2).mean()):
            return x, y, seed, seed - base + 1
    raise AssertionError("no target with an ordinary residual at the border pixel in 400 draws")


def loss_and_grads(net_work, x, y):
    ref = train_ref.TrainRef(net_work, weights(net_work), batch_size=BATCH_SIZE)
    loss, grads, _ = ref.loss_and_grads(x, y)
    return loss, {k: v.numpy() for k, v in grads.items()}


@functools.lru_cache(maxsize=None)
def reference(net_work, n, t):
    """Once per (net, shape), shared and left unchanged: (x, y, fp64 loss, fp64 gradients by name)."""
    x, y, _, _ = screened(net_work, n, t)
    return (x, y) + loss_and_grads(net_work, x, y)


def dead_bias(name, names):
    """A bias in front of a BatchNorm: the batch mean removes it, its true gradient is exactly 0."""
    return name.endswith("/bias") and (name[:-5] + "/batch_norm/gamma") in names


def prediction(net_work, x):
    ref = train_ref.TrainRef(net_work, weights(net_work), batch_size=BATCH_SIZE)
    with torch.no_grad():
        return ref.forward_train(x)[0].numpy()


def distances(g, g_true):
    """Per compared tensor, the measure TIGHT is a bar on: max |g - g_true| over the tensor's largest true entry."""
    return {k: float(np.abs(g[k] - v).max() / np.abs(v).max()) for k, v in g_true.items() if not dead_bias(k, g_true)}
