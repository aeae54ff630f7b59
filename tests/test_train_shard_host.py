"""The sharded training step without a GPU: the ABI's three entry points and their refusals, the row ranges
`accumulate=k` cuts, the float64 restatement (tests/train_shard_np.py) pinned to oracle.train_ref.TrainRef, and
dist.DataParallelTrainer's protocol at world 2 over gloo with a stand-in trainer."""

import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import rced_np, train_ref

import train_shard_np


def test_the_three_symbols_are_exported_with_the_declared_argument_types(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "rced.h")) as fh:
        header = fh.read()
    vp, i, dp, szp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_size_t)
    want = {
        "rced_train_exchange_size": [vp, szp, szp],
        "rced_train_grad": [vp, vp, vp, i, i, vp, vp, i, dp, vp],
        "rced_train_apply": [vp, vp, vp, ctypes.c_float, vp],
    }
    for name, args in want.items():
        assert name + "(" in header and hasattr(lib, name), name
        assert _lib.SYMBOLS[name] == (ctypes.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int, name


def test_library_refusals_come_before_a_device_is_looked_for(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()

    def refused(rc):
        return rc == _lib.RCED_ERR_ARG and len(lib.rced_last_error()) > 0

    # a stand-in for a handle and for device buffers: the refusals below are decided before any of them is looked into
    mem = (ctypes.c_double * 64)()
    p = ctypes.addressof(mem)
    nf, nd, loss = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_double()
    assert refused(lib.rced_train_exchange_size(None, ctypes.byref(nf), ctypes.byref(nd)))
    assert refused(lib.rced_train_exchange_size(p, None, ctypes.byref(nd)))
    assert refused(lib.rced_train_exchange_size(p, ctypes.byref(nf), None))
    assert refused(lib.rced_train_grad(None, p, p, 2, 9, p, p, 0, ctypes.byref(loss), None))
    for n, t in ((0, 9), (-1, 9), (2, 0), (2, -3)):
        assert refused(lib.rced_train_grad(p, p, p, n, t, p, p, 0, ctypes.byref(loss), None)), (n, t)
        assert str(n).encode() in lib.rced_last_error() and str(t).encode() in lib.rced_last_error()
    assert refused(lib.rced_train_grad(p, None, p, 2, 9, p, p, 0, ctypes.byref(loss), None))
    assert refused(lib.rced_train_grad(p, p, None, 2, 9, p, p, 0, ctypes.byref(loss), None))
    assert refused(lib.rced_train_grad(p, p, p, 2, 9, None, p, 1, ctypes.byref(loss), None))
    assert refused(lib.rced_train_grad(p, p, p, 2, 9, p, None, 1, ctypes.byref(loss), None))
    assert refused(lib.rced_train_apply(None, p, p, 1e-3, None))
    assert refused(lib.rced_train_apply(p, None, p, 1e-3, None))
    assert refused(lib.rced_train_apply(p, p, None, 1e-3, None))


@pytest.mark.parametrize("n,k,want", [(4, 2, [(0, 2), (2, 4)]), (3, 2, [(0, 2), (2, 3)]), (5, 4, [(0, 2), (2, 3), (3, 4), (4, 5)])])
def test_accumulation_cuts_contiguous_balanced_row_ranges(n, k, want):
    from fullycnnspeechenhancement_amd.dist import shard_bounds
    from fullycnnspeechenhancement_amd.trainer import accumulation_slices
    assert accumulation_slices(n, k) == want == shard_bounds(n, k)
    rows = np.arange(n)
    assert np.array_equal(np.concatenate([rows[a:b] for a, b in want]), rows) and all(b > a for a, b in want)


def test_more_shards_than_rows_and_bad_accumulate_are_value_errors():
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd.trainer import accumulation_slices
    with pytest.raises(ValueError):
        accumulation_slices(4, 5)
    for bad in (0, -1, -4, 1.5):
        with pytest.raises(ValueError):        # refused before a model (and with it a device) is asked for
            FullyCNNTrainer("FullyCNNV3", batch_size=4, accumulate=bad)


def _state(ref):
    return {k: v.detach().numpy().copy() for k, v in ref.vars.items()}


@pytest.mark.parametrize("net_work", ["FullyCNN", "FullyCNNV3"])
def test_one_shard_of_the_restatement_is_the_oracles_train_step(net_work):
    w = rced_np.make_weights(net_work, seed=7)
    x, y = rced_np.make_input(3, 9, seed=71), rced_np.make_input(3, 9, seed=81)
    a = train_ref.TrainRef(net_work, w, batch_size=8)
    b = train_ref.TrainRef(net_work, w, batch_size=8)
    for step in range(2):
        loss_a, step_a = a.train_step(x, y, 1e-3)
        loss_b, _, step_b = train_shard_np.sharded_step(b, [(x, y)], 1e-3)
        assert step_a == step_b == step + 1 and abs(loss_a - loss_b) <= 1e-12 * abs(loss_a)
        va, vb = _state(a), _state(b)
        for name in va:
            assert np.allclose(vb[name], va[name], rtol=1e-12, atol=1e-12), name
        for name in a.m:
            assert np.allclose(b.m[name].numpy(), a.m[name].numpy(), rtol=1e-12, atol=1e-12), name
            assert np.allclose(b.v[name].numpy(), a.v[name].numpy(), rtol=1e-12, atol=1e-12), name


def test_two_identical_shards_at_twice_the_batch_size_give_the_one_shard_gradient():
    """Exact by construction: with identical content every shard's statistics are the union's, each shard's gradient is
    half the one-shard gradient (the loss divides by twice the batch size), and the moving statistics see the same mean
    and biased variance over twice the pixels."""
    w = rced_np.make_weights("FullyCNNV3", seed=9)
    x, y = rced_np.make_input(2, 9, seed=72), rced_np.make_input(2, 9, seed=82)
    one = train_ref.TrainRef("FullyCNNV3", w, batch_size=4)
    two = train_ref.TrainRef("FullyCNNV3", w, batch_size=8)
    loss1, g1, _ = train_shard_np.sharded_step(one, [(x, y)], 1e-3)
    loss2, g2, _ = train_shard_np.sharded_step(two, [(x, y), (x, y)], 1e-3)
    assert abs(loss1 - loss2) <= 1e-12 * abs(loss1)
    for name in g1:
        a, b = g1[name].numpy(), g2[name].numpy()
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(a).max(), 1e-30), name
    v1, v2 = _state(one), _state(two)
    for name in v1:
        if name.endswith("moving_mean"):
            assert np.allclose(v2[name], v1[name], rtol=1e-12, atol=1e-12), name


# ---- DataParallelTrainer's protocol over gloo, with a stand-in trainer on the CPU --------------------------------------
class _StandInTrainer(object):
    """What DataParallelTrainer uses of a FullyCNNTrainer, on CPU tensors: the "gradient" of a shard is the sum of its
    rows, the "statistics" its row count, and apply adds both into a running state."""

    device, lr, warmup_steps = 0, 1.0, 10.0

    def __init__(self):
        import torch
        self.g, self.s = torch.zeros(4, dtype=torch.float32), torch.zeros(3, dtype=torch.float64)
        self.state, self.global_step = torch.zeros(4, dtype=torch.float64), 0

    def exchange_tensors(self):
        return self.g, self.s

    def grad_step(self, x, y, accumulate=False):
        import torch
        if x.shape != y.shape:
            raise ValueError("input and target must have one shape")
        self.g.copy_(torch.as_tensor(x).float().sum(0))
        self.s.fill_(float(x.shape[0]))
        return float(y.sum())

    def apply_step(self):
        self.state += self.g.double() * self.s[0]
        self.global_step += 1
        return self.global_step

    def noam_scheme(self, step, warmup):
        return 1.0 / (step + 1)


def _dp_cpu_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from fullycnnspeechenhancement_amd.dist import DataParallelTrainer, PeerTrainError
        dp = DataParallelTrainer(_StandInTrainer(), device="cpu")
        x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
        loss, _, step = dp.fit_step(x, x)
        assert step == 1 and loss == float(x.sum()) and dp.lr == 0.5
        assert torch.equal(dp.trainer.g, x.sum(0)) and float(dp.trainer.s[0]) == 3.0      # rows 2 + 1, summed in rank order
        try:
            dp.fit_step(x, x[:, :3] if rank == 1 else x)
            raised = None
        except Exception as e:
            raised = e
        assert isinstance(raised, ValueError if rank == 1 else PeerTrainError), raised
        assert dp.global_step == 1                                                       # none applied
        with pytest.raises(ValueError):
            dp.fit_step(x[:1], x[:1])                                                    # a world of 2 on one row
        assert dp.fit_step(x, x)[2] == 2                                                 # still usable
        open(os.path.join(out_dir, "ok%d" % rank), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_data_parallel_protocol_over_gloo_with_a_stand_in_trainer(tmp_path):
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd import dist as pkg_dist
    assert pkg.DataParallelTrainer is pkg_dist.DataParallelTrainer and "DataParallelTrainer" in pkg.__all__
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_cpu_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(str(tmp_path / ("ok%d" % r))) for r in range(2))
