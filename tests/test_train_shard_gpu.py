"""The training step in shards on the GPU (rced_train_grad / rced_train_apply, FullyCNNTrainer.grad_step / apply_step /
train_step_sharded / accumulate=k, dist.DataParallelTrainer).  The chain of equalities:
train_step = one shard (bit for bit), k shards = the ordered fp32 sum of the shards' gradients (bit for bit), a world of W
ranks = W shards on one device (bit for bit); the float64 restatement is tests/train_shard_np.py."""

import functools
import os
import time

import numpy as np
import pytest

from conftest import NETS, ROOT
from oracle import rced_np, train_ref
from test_train_gpu import COS, LOOSE, TIGHT, cosine, net_layers_last, rel

import train_shard_np

pytestmark = pytest.mark.gpu

KW = dict(batch_size=8, lr=1e-3, warmup_steps=10.0)     # the configured batch size is not the number of rows, on purpose


def same_bits(a, b, what=""):
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), "%s %s" % (what, name)


def state_of(tr):
    m, v, step = tr.optimizer_state()
    return tr.variables(), tr.gradients(), m, v, step


def same_state(a, b):
    for da, db, what in zip(a[:4], b[:4], ("variable", "gradient", "adam m", "adam v")):
        same_bits(da, db, what)
    assert a[4] == b[4]


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_one_shard_is_the_step_bit_for_bit(net_work, tag, variant, built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights(net_work, seed=7)
    x, y = rced_np.make_input(3, 9, seed=70 + variant), rced_np.make_input(3, 9, seed=80 + variant)
    a = FullyCNNTrainer(net_work, weights=w, **KW)
    b = FullyCNNTrainer(net_work, weights=w, **KW)
    for step in (1, 2):
        loss_a, _, step_a = a.train_step(x, y)
        loss_b = b.grad_step(x, y)
        assert b.global_step == step - 1
        step_b = b.apply_step()
        assert loss_a == loss_b and step_a == step_b == step
        same_state(state_of(a), state_of(b))       # the variables include the moving statistics
    a.close()
    b.close()


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_grad_step_changes_nothing(net_work, tag, variant, built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights(net_work, seed=7)
    x, y = rced_np.make_input(3, 9, seed=70 + variant), rced_np.make_input(3, 9, seed=80 + variant)
    tr = FullyCNNTrainer(net_work, weights=w, **KW)
    tr.train_step(x, y)                            # Adam slots and moving statistics that are not their start values
    v0, _, m0, s0, step0 = state_of(tr)
    pred0 = tr.valid_step(x)
    tr.grad_step(x, y)
    tr.grad_step(y, x, accumulate=True)
    v1, _, m1, s1, step1 = state_of(tr)
    same_bits(v0, v1, "variable")
    same_bits(m0, m1, "adam m")
    same_bits(s0, s1, "adam v")
    assert step0 == step1 == 1
    assert np.array_equal(tr.valid_step(x), pred0)
    tr.close()


def test_moving_statistics_are_written_by_the_optimizer_epilogue_alone(built):
    """No forward writes a variable, in any form of the step: after grad_step, and after a grad_step_sync run to its end
    with one shard, variables() -- the moving statistics among them -- are the start values bit for bit; the apply_step that
    follows leaves the variables of a train_step on the same batch, bit for bit."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd import spec
    w = rced_np.make_weights("FullyCNNV3", seed=7)
    x, y = rced_np.make_input(2, 3, seed=73), rced_np.make_input(2, 3, seed=83)
    a = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
    b = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
    start = a.variables()
    assert any("moving_" in name for name in start)
    a.grad_step(x, y)
    same_bits(a.variables(), start, "after grad_step: variable")
    for _ in a.grad_step_sync(x, y, 2 * 3 * spec.FEATURE_DIM):      # the yielded sums stay as they are: this shard is all there is
        pass
    same_bits(a.variables(), start, "after grad_step_sync: variable")
    assert a.apply_step() == 1
    b.train_step(x, y)
    moved = b.variables()
    assert any(not np.array_equal(moved[name], start[name]) for name in start if "moving_" in name)
    same_bits(a.variables(), moved, "after apply_step: variable")
    a.close()
    b.close()


def test_accumulation_is_the_ordered_sum_of_the_shards(built):
    """Shards of unequal shape, (2 rows, T = 9) and (1 row, T = 12): the applied gradient is g_0 + g_1 formed in numpy
    float32 from each shard's own grad_step on a fresh trainer, the loss is loss_0 + loss_1 in float64, both exactly."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights("FullyCNNV3", seed=7)
    shards = [(rced_np.make_input(2, 9, seed=61), rced_np.make_input(2, 9, seed=62)),
              (rced_np.make_input(1, 12, seed=63), rced_np.make_input(1, 12, seed=64))]
    alone = []
    for x, y in shards:
        tr = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
        loss = tr.grad_step(x, y)
        tr.apply_step()
        alone.append((loss, tr.gradients()))
        tr.close()
    tr = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
    loss, _, step = tr.train_step_sharded(shards)
    g = tr.gradients()
    assert step == 1 and loss == alone[0][0] + alone[1][0]
    for name in g:
        want = alone[0][1][name].astype(np.float32) + alone[1][1][name].astype(np.float32)
        assert want.dtype == np.float32 and np.array_equal(g[name], want), name
    assert any(np.abs(v).max() > 0 for v in g.values())
    tr.close()


# ---- against the float64 restatement -----------------------------------------------------------------------------------
def _batch(variant):
    return rced_np.make_input(3, 9, seed=70 + variant), rced_np.make_input(3, 9, seed=80 + variant)


@functools.lru_cache(maxsize=None)
def _restated(net_work, variant):
    """Once per net, shared and left unchanged: the float64 sharded step over rows [0, 2) and [2, 3) of the batch, and the
    float64 unsharded step over the whole batch."""
    w = rced_np.make_weights(net_work, seed=7)
    x, y = _batch(variant)
    sh = train_ref.TrainRef(net_work, w, batch_size=8)
    loss_sh, g_sh, _ = train_shard_np.sharded_step(sh, [(x[:2], y[:2]), (x[2:], y[2:])], 1e-3)
    un = train_ref.TrainRef(net_work, w, batch_size=8)
    loss_un, g_un, _ = un.loss_and_grads(x, y)
    un2 = train_ref.TrainRef(net_work, w, batch_size=8)
    un2.train_step(x, y, 1e-3)
    return (loss_sh, {k: v.numpy() for k, v in g_sh.items()}, sh.weights()), (loss_un, {k: v.numpy() for k, v in g_un.items()}, un2.weights())


# Moving statistics, device (fp32 convolutions, fp64 sums, one rounding to fp32) against float64, as
# max |difference| / max |reference| over a tensor.  The bar is reasoned, not fitted: the stored value is rounded to fp32
# once (2^-24 = 6e-8 of its own size) and carries 0.01 of the batch statistic's error, which is the fp32 convolutions'
# (a few 1e-6 relative to the activations' scale): about 1e-7 together; the bar is a small multiple of that, 4e-7.
# Measured (see the docstring of the test): the unsharded step up to 1.10e-7, the sharded step up to 1.18e-7.
MOVING_BAR = 4e-7


def ulp_apart(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))).max())


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_sharded_step_against_the_float64_restatement(net_work, tag, variant, built, capsys):
    """One sharded step (rows [0, 2) and [2, 3) of a 3 x 9 batch, batch_size 8) against train_shard_np.sharded_step: the loss
    to 1e-5, the gradients under the bars of test_train_gpu.py (TIGHT for the last layer, LOOSE and COS elsewhere), the
    moving statistics to MOVING_BAR -- and the unsharded step on the same batch against TrainRef.train_step to the same
    bar, which is where the bar's size is checked.  Measured on the MI355X, worst tensor of R-CED V1 / V2 / CR-CED V3,
    max |difference| / max |reference|: unsharded 8.6e-8 / 1.10e-7 / 7.7e-8, sharded 9.1e-8 / 1.18e-7 / 7.8e-8.

    Sharded against unsharded on the device, same batch: the FIRST BatchNorm layer's pre-activations do not depend on any
    normalisation, so its sums differ only by the rounding of the fp64 additions and its moving statistics are held to
    1 ulp of float32 (measured: 0 ulp).  Every later layer reads activations that were normalised per shard, so its
    moving statistics differ by what per-shard BatchNorm changes, not by rounding (measured 1.2e-4 / 2.3e-4 / 7.4e-5 of the
    tensor's largest entry; the float64 restatement shows the same difference to 6.8e-8 / 7.0e-8 / 8.6e-8): there the
    device's difference is held to the restatement's difference, within twice MOVING_BAR.  The distance between the
    sharded (= world-2) and the unsharded gradient is printed, not judged: it is the price of per-shard BatchNorm
    (DESIGN.md 3.5b)."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights(net_work, seed=7)
    x, y = _batch(variant)
    (loss_ref, g_ref, v_ref), (loss_un_ref, g_un_ref, v_un_ref) = _restated(net_work, variant)
    sh = FullyCNNTrainer(net_work, weights=w, **KW)
    loss, _, step = sh.train_step_sharded([(x[:2], y[:2]), (x[2:], y[2:])])
    g, v = sh.gradients(), sh.variables()
    sh.close()
    un = FullyCNNTrainer(net_work, weights=w, **KW)
    un.train_step(x, y)
    g_un, v_un = un.gradients(), un.variables()
    un.close()
    moving = [n for n in v if "moving_" in n]
    first = min(moving, key=list(v).index).rsplit("/", 1)[0]           # the first BatchNorm layer, in graph order
    e_sh = max(rel(v[n], v_ref[n]) for n in moving)
    e_un = max(rel(v_un[n], v_un_ref[n]) for n in moving)
    ulp_first = max(ulp_apart(v[n], v_un[n]) for n in moving if n.startswith(first))
    d_dev = max(rel(v[n], v_un[n]) for n in moving)
    d_gap = max(float(np.abs((v[n].astype(np.float64) - v_un[n]) - (v_ref[n] - v_un_ref[n])).max() / np.abs(v_un_ref[n]).max())
                for n in moving)
    trainable = [n for n in g_ref if not (n.endswith("/bias") and (n[:-5] + "/batch_norm/gamma") in g_ref)]
    d_grad = max((rel(g[n], g_un[n]), n) for n in trainable)
    d_grad_ref = max((rel(g_ref[n], g_un_ref[n]), n) for n in trainable)
    d_med = float(np.median([rel(g[n], g_un[n]) for n in trainable]))
    d_cos = cosine(np.concatenate([g[n].ravel() for n in trainable]), np.concatenate([g_un[n].ravel() for n in trainable]))
    with capsys.disabled():
        print("\n[sharded step, %s] loss rel err %.2e; moving statistics vs float64: sharded %.2e, unsharded %.2e; sharded vs "
              "unsharded on the device: first BatchNorm layer %.1f ulp, any layer %.2e (restatement agrees to %.2e); gradient sharded vs "
              "unsharded: device worst tensor %.2e (%s), float64 %.2e (%s), median tensor %.2e, cosine of the whole gradient %.4f"
              % (net_work, abs(loss - loss_ref) / abs(loss_ref), e_sh, e_un, ulp_first, d_dev, d_gap, d_grad[0], d_grad[1],
                 d_grad_ref[0], d_grad_ref[1], d_med, d_cos))
    assert step == 1 and abs(loss - loss_ref) <= 1e-5 * abs(loss_ref)
    for name, gr in g_ref.items():
        if name.endswith("/bias") and (name[:-5] + "/batch_norm/gamma") in g_ref:
            assert np.abs(g[name]).max() <= 1e-3 * max(np.abs(g[name[:-5] + "/kernel"]).max(), 1.0)   # ~0
            continue
        assert rel(g[name], gr) < (TIGHT if name.startswith(net_layers_last(net_work)) else LOOSE), name
        assert cosine(g[name], gr) > COS, name
    assert e_un < MOVING_BAR and e_sh < MOVING_BAR, (e_un, e_sh)
    assert ulp_first <= 1.0, ulp_first
    assert d_gap < 2 * MOVING_BAR, d_gap


def test_accumulate_through_fit_step(built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd.dist import shard_bounds
    w = rced_np.make_weights("FullyCNNV3", seed=7)
    x, y = rced_np.make_input(4, 9, seed=65), rced_np.make_input(4, 9, seed=66)
    a = FullyCNNTrainer("FullyCNNV3", weights=w, accumulate=2, **KW)
    b = FullyCNNTrainer("FullyCNNV3", weights=w, **KW)
    assert shard_bounds(4, 2) == [(0, 2), (2, 4)]
    for step in (1, 2, 3):
        out_a = a.fit_step(x, y)
        out_b = b.train_step_sharded([(x[lo:hi], y[lo:hi]) for lo, hi in shard_bounds(4, 2)])
        b.lr = b.noam_scheme(out_b[2], b.warmup_steps)
        assert out_a == out_b and out_a[2] == step and a.lr == b.lr
    same_state(state_of(a), state_of(b))
    a.close()
    b.close()
    c = FullyCNNTrainer("FullyCNNV3", weights=w, accumulate=5, **KW)
    with pytest.raises(ValueError):
        c.fit_step(x, y)
    assert c.global_step == 0
    c.close()


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_sharded_steps_are_bit_reproducible(net_work, tag, variant, built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights(net_work, seed=91)
    x, y = rced_np.make_input(4, 12, seed=92), rced_np.make_input(4, 12, seed=93)
    runs = []
    for _ in range(2):
        tr = FullyCNNTrainer(net_work, weights=w, accumulate=3, **KW)
        losses = [tr.fit_step(x, y)[0] for _ in range(3)]
        runs.append((losses, state_of(tr)))
        tr.close()
    assert runs[0][0] == runs[1][0]
    same_state(runs[0][1], runs[1][1])


# ---- a world of two ranks on one GPU ------------------------------------------------------------------------------------
W2_SEEDS = dict(w=7, x=67, y=68, bad=69)


def _flat(prefix, d):
    return {prefix + k.replace("/", "|"): v for k, v in d.items()}


def _world2_worker(rank, world, port, out_dir):
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
        dp = DataParallelTrainer(FullyCNNTrainer("FullyCNNV3", weights=w, device=0, **KW), device="cuda:0")
        out = {"loss": np.array([dp.fit_step(x, y)[0] for _ in range(3)], np.float64)}
        v, g, m, s, step = state_of(dp.trainer)
        out.update(_flat("v:", v), **_flat("g:", g), **_flat("m:", m), **_flat("s:", s))
        out["step"], out["lr"] = np.array(step), np.array(dp.lr, np.float64)
        # rank 1 is handed a target of the wrong shape: both ranks raise, neither applies
        bad_y = rced_np.make_input(3, 10, seed=W2_SEEDS["bad"]) if rank == 1 else y
        try:
            dp.fit_step(x, bad_y)
            raised = "none"
        except Exception as e:
            raised = type(e).__name__
        out["raised"], out["step_after_failure"] = np.array(raised), np.array(dp.global_step)
        too_few = "none"
        try:
            dp.fit_step(x[:1], y[:1])                # a world of 2 on a batch of 1 row: refused on every rank, nothing gathered
        except ValueError:
            too_few = "ValueError"
        out["too_few"] = np.array(too_few)
        loss4, _, step4 = dp.fit_step(x, y)        # the group and the object are still usable
        out["loss4"], out["step4"] = np.array(loss4, np.float64), np.array(step4)
        out.update(_flat("v4:", dp.trainer.variables()))
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        dist.barrier()
        dp.trainer.close()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def world2(built, tmp_path_factory):
    """ONE spawn of two processes that share device 0 (gloo for the exchange): three data-parallel steps on a global batch of
    3 rows (shards 2 + 1), a step that fails on rank 1, and a good step behind it.  What each rank saw, by rank."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path_factory.mktemp("world2"))
    ctx = mp.spawn(_world2_worker, args=(2, port, out), nprocs=2, join=False)
    deadline = time.time() + 120            # two interpreters that load torch and open the device, then seven tiny steps
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish in 120 s")
    return [dict(np.load(os.path.join(out, "rank%d.npz" % r))) for r in range(2)]


def test_world_of_two_is_two_shards_on_one_device(world2, built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd.dist import shard_bounds
    r0, r1 = world2
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
        out = tr.train_step_sharded([(x[lo:hi], y[lo:hi]) for lo, hi in bounds])
        tr.lr = tr.noam_scheme(out[2], tr.warmup_steps)
        losses.append(out[0])
    assert np.array_equal(r0["loss"], np.array(losses, np.float64))
    v, g, m, s, step = state_of(tr)
    assert int(r0["step"]) == step == 3 and float(r0["lr"]) == tr.lr
    for prefix, d in (("v:", v), ("g:", g), ("m:", m), ("s:", s)):
        same_bits(_flat(prefix, d), {k: a for k, a in r0.items() if k.startswith(prefix)}, prefix)
    # the good step behind the failed one continues the same run
    out = tr.train_step_sharded([(x[lo:hi], y[lo:hi]) for lo, hi in bounds])
    assert float(r0["loss4"]) == out[0] and int(r0["step4"]) == out[2] == 4
    same_bits(_flat("v4:", tr.variables()), {k: a for k, a in r0.items() if k.startswith("v4:")}, "after the failure")
    tr.close()


def test_a_failure_on_one_rank_fails_every_rank_and_none_applies(world2):
    r0, r1 = world2
    assert str(r1["raised"]) == "ValueError"            # its own exception where the gradient pass raised ...
    assert str(r0["raised"]) == "PeerTrainError"        # ... and the peer's name for it everywhere else
    for r in (r0, r1):
        assert int(r["step_after_failure"]) == 3 and str(r["too_few"]) == "ValueError"
        assert int(r["step4"]) == 4 and np.isfinite(float(r["loss4"]))
