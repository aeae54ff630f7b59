"""The synchronised sharded step on the GPU (rced_train_sync_*, FullyCNNTrainer.grad_step_sync /
train_step_sharded(sync_bn=True), dist.DataParallelTrainer(sync_bn=True)).  The chain: one shard with its
own pixel count = grad_step (bit for bit); shards with the statistics of their union = the unsharded step over the whole
batch (to the bars every device step is held to against float64); a world of W ranks = W shards on one device (bit for
bit).  The float64 restatement is tests/train_sync_np.py."""

import functools
import math
import os
import time

import numpy as np
import pytest

from conftest import NETS, ROOT
from oracle import layers as L, rced_np, train_ref
from test_train_gpu import COS, LOOSE, TIGHT, cosine, net_layers_last, rel
from test_train_shard_gpu import KW, MOVING_BAR, _batch, _flat, _restated, same_bits, same_state, state_of

import train_sync_np

pytestmark = pytest.mark.gpu

PARTITIONS = {"2+1": [(0, 2), (2, 3)], "1+2": [(0, 1), (1, 3)], "1+1+1": [(0, 1), (1, 2), (2, 3)]}
# two results that are each within an angle acos(COS) of a third are within twice that angle of each other
COS2 = math.cos(2.0 * math.acos(COS))


def cut(x, y, bounds):
    return [(x[a:b], y[a:b]) for a, b in bounds]


def dead_bias(name, names):
    """A bias in front of a BatchNorm layer: its gradient is 0 up to rounding and has no scale of its own."""
    return name.endswith("/bias") and (name[:-5] + "/batch_norm/gamma") in names


def bn_layers(net_work):
    return sum(1 for l in L.layers_for(net_work) if l.use_norm)


def run_untouched(tr, x, y):
    """grad_step_sync with the yielded tensor left as it is: (loss, number of exchange points)."""
    gen = tr.grad_step_sync(x, y, x.shape[0] * x.shape[1] * 129)
    n = 0
    while True:
        try:
            next(gen)
            n += 1
        except StopIteration as e:
            return e.value, n


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_one_shard_with_its_own_count_is_grad_step_bit_for_bit(net_work, tag, variant, built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights(net_work, seed=7)
    x, y = _batch(variant)
    a = FullyCNNTrainer(net_work, weights=w, **KW)
    b = FullyCNNTrainer(net_work, weights=w, **KW)
    n_points = 2 * bn_layers(net_work)                  # every BatchNorm layer forward and backward: 18 / 30 / 30
    assert b.sync_points() == (n_points, 64)            # (S1, S2) of up to 32 channels
    for step in (1, 2):
        loss_a, _, step_a = a.train_step(x, y)
        loss_b, points = run_untouched(b, x, y)
        assert points == n_points and b.global_step == step - 1
        step_b = b.apply_step()
        assert loss_a == loss_b and step_a == step_b == step
        same_state(state_of(a), state_of(b))            # the variables include the moving statistics
    a.close()
    b.close()


@functools.lru_cache(maxsize=None)
def _device(net_work, variant, part):
    """Once per net and partition, shared and left unchanged: the synchronised step on the device, run TWICE on fresh
    trainers (loss, gradients, variables of each run); part None: the unsharded train_step, "per-shard": the default
    sharded step over 2 + 1 rows."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights(net_work, seed=7)
    x, y = _batch(variant)
    runs = []
    for _ in range(1 if part in (None, "per-shard") else 2):
        tr = FullyCNNTrainer(net_work, weights=w, **KW)
        if part is None:
            loss, _, step = tr.train_step(x, y)
        elif part == "per-shard":
            loss, _, step = tr.train_step_sharded(cut(x, y, PARTITIONS["2+1"]))
        else:
            loss, _, step = tr.train_step_sharded(cut(x, y, PARTITIONS[part]), sync_bn=True)
        assert step == 1
        runs.append((loss, tr.gradients(), tr.variables()))
        tr.close()
    return runs


def check_against(g, g_ref, v, v_ref, net_work, k=1.0):
    """The gradient bars of test_train_gpu.py and MOVING_BAR for every BatchNorm layer, times k; returns the worst moving
    statistics distance and the worst gradient distance."""
    worst_g = 0.0
    for name, gr in g_ref.items():
        if "moving_" in name:                               # (the device's gradient blob has them, as zeros)
            continue
        if dead_bias(name, g_ref):
            assert np.abs(g[name]).max() <= 1e-3 * max(np.abs(g[name[:-5] + "/kernel"]).max(), 1.0)   # ~0
            continue
        e = rel(g[name], gr)
        worst_g = max(worst_g, e)
        assert e < k * (TIGHT if name.startswith(net_layers_last(net_work)) else LOOSE), (name, e)
        assert cosine(g[name], gr) > (COS if k == 1.0 else COS2), name
    moving = [n for n in v_ref if "moving_" in n]
    assert len(moving) == 2 * bn_layers(net_work)
    e_mov = max(rel(v[n], v_ref[n]) for n in moving)
    assert e_mov < k * MOVING_BAR, e_mov
    return e_mov, worst_g


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_synchronised_step_against_the_float64_unsharded_step(net_work, tag, variant, built, capsys):
    """2 + 1 rows of the 3 x 9 batch with sync_bn=True against TrainRef.train_step over the WHOLE batch: the loss to 1e-5,
    the gradients under TIGHT / LOOSE / COS, the moving statistics of every BatchNorm layer under MOVING_BAR.  The default
    per-shard step on the same shards misses MOVING_BAR against the same reference (its later layers see activations that
    were normalised per shard): that is the difference the mode removes."""
    _, (loss_ref, g_ref, v_ref) = _restated(net_work, variant)
    loss, g, v = _device(net_work, variant, "2+1")[0]
    _, _, v_ps = _device(net_work, variant, "per-shard")[0]
    moving = [n for n in v_ref if "moving_" in n]
    e_ps = max(rel(v_ps[n], v_ref[n]) for n in moving)
    e_sync = max(rel(v[n], v_ref[n]) for n in moving)
    with capsys.disabled():
        print("\n[synchronised step, %s] loss rel err %.2e; moving statistics vs the float64 unsharded step: synchronised %.2e, "
              "per-shard BatchNorm %.2e (bar %.0e)" % (net_work, abs(loss - loss_ref) / abs(loss_ref), e_sync, e_ps, MOVING_BAR))
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref)
    check_against(g, g_ref, v, v_ref, net_work)
    assert e_ps > MOVING_BAR, e_ps


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_synchronised_step_against_the_device_unsharded_step(net_work, tag, variant, built, capsys):
    """The same step against the device's own train_step over the whole batch: each side is held to one bar against the same
    float64 step, so the two are within two bars of each other.  Not bit-equal: the fp64 records of a layer are added in
    another grouping (per shard, then over shards), and every later layer reads activations normalised with statistics that
    may differ in their last bits.  Measured on the MI355X, R-CED V1 / V2 / CR-CED V3, max |difference| / max |unsharded|
    over the worst tensor: gradients 2.8e-7 / 2.4e-7 / 3.3e-7 (the bar is 2 LOOSE = 6e-2; per-shard BatchNorm is 0.65 /
    0.93 / 1.42 away), moving statistics 0 / 0 / 0 (the same fp32 bits on this batch; the bar is 8e-7), loss 0 / 0 / 1.4e-16."""
    loss_un, g_un, v_un = _device(net_work, variant, None)[0]
    loss, g, v = _device(net_work, variant, "2+1")[0]
    e_mov, e_g = check_against(g, g_un, v, v_un, net_work, k=2.0)
    with capsys.disabled():
        print("\n[synchronised vs unsharded on the device, %s] loss %.2e, worst gradient tensor %.2e, moving statistics %.2e"
              % (net_work, abs(loss - loss_un) / abs(loss_un), e_g, e_mov))
    assert abs(loss - loss_un) <= 2e-5 * abs(loss_un)


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_partitions_agree_and_each_is_bit_reproducible(net_work, tag, variant, built):
    res = {part: _device(net_work, variant, part) for part in PARTITIONS}
    for part, (a, b) in res.items():
        assert a[0] == b[0], part
        same_bits(a[1], b[1], "gradient " + part)
        same_bits(a[2], b[2], "variable " + part)
    parts = sorted(res)
    for i, p in enumerate(parts):
        for q in parts[i + 1:]:
            (lp, gp, vp), (lq, gq, vq) = res[p][0], res[q][0]
            assert abs(lp - lq) <= 2e-5 * abs(lq)
            check_against(gp, gq, vp, vq, net_work, k=2.0)


# The ragged case is not a cut of the screened 3 x 9 batch, so its inputs are screened here, as test_train_gpu.screened_input
# screens: no value entering a ReLU within RAGGED_MARGIN of zero in the float64 restatement, or a ReLU mask can flip on the
# device and move a gradient by whole terms.  The device's fp32 pre-activations differ from float64 by about 1e-6 at
# unit scale; the margin is three times that.  (The 1e-5 of screened_input would leave about one draw in 250 at the
# 19 x 129 pixels x ~300 channels here; 3e-6 leaves about one in five, and LOOSE is there for the flip that still slips by.
# Unscreened, seed 63 puts 7 CR-CED pre-activations within 3e-6 of zero and one gamma gradient 6e-2 off.)
RAGGED_MARGIN = 3e-6


@functools.lru_cache(maxsize=None)
def _ragged(net_work):
    """Once per net, shared and left unchanged: (shards, float64 loss, gradients, variables after the step) of 2 x 9 frames
    and 1 x 1 frame, the one-frame shard's input redrawn until the union passes the screen."""
    w = rced_np.make_weights(net_work, seed=7)
    big = (rced_np.make_input(2, 9, seed=61), rced_np.make_input(2, 9, seed=62))
    probe = train_ref.TrainRef(net_work, w, batch_size=8)
    for seed in range(63, 463):
        small = (rced_np.make_input(1, 1, seed=seed), rced_np.make_input(1, 1, seed=1000 + seed))
        if train_sync_np.min_abs_preactivation(probe, [big[0], small[0]]) > RAGGED_MARGIN:
            break
    else:
        raise AssertionError("no screened input in 400 draws")
    shards = [big, small]
    ref = train_ref.TrainRef(net_work, w, batch_size=8)
    loss, g, _ = train_sync_np.synced_step(ref, shards, 1e-3)
    return shards, loss, {k: v.numpy() for k, v in g.items()}, ref.weights()


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_ragged_shards_against_the_float64_restatement(net_work, tag, variant, built):
    """2 x 9 frames and 1 x 1 frame, statistics over all 19 frames' pixels, against train_sync_np.synced_step."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    shards, loss_ref, g_ref, v_ref = _ragged(net_work)
    tr = FullyCNNTrainer(net_work, weights=rced_np.make_weights(net_work, seed=7), **KW)
    loss, _, step = tr.train_step_sharded(shards, sync_bn=True)
    g, v = tr.gradients(), tr.variables()
    tr.close()
    assert step == 1 and abs(loss - loss_ref) <= 1e-5 * abs(loss_ref)
    check_against(g, g_ref, v, v_ref, net_work)


def test_a_pending_pass_refuses_every_other_call_and_an_abort_frees_the_handle(built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, _lib
    w = rced_np.make_weights("FullyCNNV3", seed=7)
    x, y = _batch(3)
    tr = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
    twin = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
    gen = tr.grad_step_sync(x, y, 3 * 9 * 129)
    next(gen)
    next(gen)                                           # somewhere inside the forward
    for call in (lambda: tr.train_step(x, y), lambda: tr.grad_step(x, y), tr.apply_step, tr.variables, tr.gradients,
                 tr.optimizer_state, lambda: tr.valid_step(x), lambda: next(tr.grad_step_sync(x, y, 3 * 9 * 129))):
        with pytest.raises(_lib.RcedError) as ei:
            call()
        assert ei.value.code == _lib.RCED_ERR_STATE and "pending" in str(ei.value)
    gen.close()                                         # the early close aborts the pass
    assert tr.global_step == 0
    same_bits(tr.variables(), twin.variables(), "variable")      # the pass changed nothing
    assert tr.train_step(x, y) == twin.train_step(x, y)
    same_state(state_of(tr), state_of(twin))
    tr.close()
    twin.close()
    acc = FullyCNNTrainer("FullyCNNV3", weights=w, accumulate=2, **KW)
    with pytest.raises(ValueError) as ei:
        acc.train_step_sharded(cut(x, y, PARTITIONS["2+1"]), sync_bn=True)
    assert "sync_bn" in str(ei.value) and "accumulate" in str(ei.value) and acc.global_step == 0
    acc.close()


# ---- a world of two ranks on one GPU ------------------------------------------------------------------------------------
W2_SEEDS = dict(w=7, x=67, y=68, bad=69)


def _world2_sync_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)      # RCCL refuses two ranks on one device
    try:
        from fullycnnspeechenhancement_amd import FullyCNNTrainer
        from fullycnnspeechenhancement_amd.dist import DataParallelTrainer
        torch.cuda.set_device(0)
        w = rced_np.make_weights("FullyCNNV3", seed=W2_SEEDS["w"])
        x, y = rced_np.make_input(3, 9, seed=W2_SEEDS["x"]), rced_np.make_input(3, 9, seed=W2_SEEDS["y"])
        dp = DataParallelTrainer(FullyCNNTrainer("FullyCNNV3", weights=w, device=0, **KW), device="cuda:0", sync_bn=True)
        out = {"loss": np.array([dp.fit_step(x, y)[0] for _ in range(3)], np.float64)}
        v, g, m, s, step = state_of(dp.trainer)
        out.update(_flat("v:", v), **_flat("g:", g), **_flat("m:", m), **_flat("s:", s))
        out["step"], out["lr"] = np.array(step), np.array(dp.lr, np.float64)
        # rank 1 is handed a target of the wrong shape: both ranks raise, neither applies, every gather of the step is met
        bad_y = rced_np.make_input(3, 10, seed=W2_SEEDS["bad"]) if rank == 1 else y
        try:
            dp.fit_step(x, bad_y)
            raised = "none"
        except Exception as e:
            raised = type(e).__name__
        out["raised"], out["step_after_failure"] = np.array(raised), np.array(dp.global_step)
        loss4, _, step4 = dp.fit_step(x, y)        # rank 0 aborted its pass when it saw the peer fail: the handle is free again
        out["loss4"], out["step4"] = np.array(loss4, np.float64), np.array(step4)
        out.update(_flat("v4:", dp.trainer.variables()))
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        dist.barrier()
        dp.trainer.close()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def world2_sync(built, tmp_path_factory):
    """ONE spawn of two processes that share device 0 (gloo for the exchange): three synchronised data-parallel steps on a
    global batch of 3 rows (shards 2 + 1), a step that fails on rank 1, and a good step behind it."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path_factory.mktemp("world2_sync"))
    ctx = mp.spawn(_world2_sync_worker, args=(2, port, out), nprocs=2, join=False)
    deadline = time.time() + 120            # two interpreters that load torch and open the device, then five tiny steps
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish in 120 s")
    return [dict(np.load(os.path.join(out, "rank%d.npz" % r))) for r in range(2)]


def test_world_of_two_is_two_synchronised_shards_on_one_device(world2_sync, built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd.dist import shard_bounds
    r0, r1 = world2_sync
    assert r0.keys() == r1.keys()
    for k in r0:
        if k != "raised":
            assert np.array_equal(r0[k], r1[k]), k                   # both ranks end with identical bits
    w = rced_np.make_weights("FullyCNNV3", seed=W2_SEEDS["w"])
    x, y = rced_np.make_input(3, 9, seed=W2_SEEDS["x"]), rced_np.make_input(3, 9, seed=W2_SEEDS["y"])
    bounds = shard_bounds(3, 2)
    assert bounds == [(0, 2), (2, 3)]
    tr = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
    losses = []
    for _ in range(3):
        out = tr.train_step_sharded(cut(x, y, bounds), sync_bn=True)
        tr.lr = tr.noam_scheme(out[2], tr.warmup_steps)
        losses.append(out[0])
    assert np.array_equal(r0["loss"], np.array(losses, np.float64))
    v, g, m, s, step = state_of(tr)
    assert int(r0["step"]) == step == 3 and float(r0["lr"]) == tr.lr
    for prefix, d in (("v:", v), ("g:", g), ("m:", m), ("s:", s)):
        same_bits(_flat(prefix, d), {k: a for k, a in r0.items() if k.startswith(prefix)}, prefix)
    # the good step behind the failed one continues the same run
    out = tr.train_step_sharded(cut(x, y, bounds), sync_bn=True)
    assert float(r0["loss4"]) == out[0] and int(r0["step4"]) == out[2] == 4
    same_bits(_flat("v4:", tr.variables()), {k: a for k, a in r0.items() if k.startswith("v4:")}, "after the failure")
    tr.close()


def test_a_failure_on_one_rank_of_the_synchronised_world_fails_both_and_none_applies(world2_sync):
    r0, r1 = world2_sync
    assert str(r1["raised"]) == "ValueError"            # its own exception where the pass raised ...
    assert str(r0["raised"]) == "PeerTrainError"        # ... and the peer's name for it everywhere else
    for r in (r0, r1):
        assert int(r["step_after_failure"]) == 3
        assert int(r["step4"]) == 4 and np.isfinite(float(r["loss4"]))
