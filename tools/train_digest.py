#!/usr/bin/env python3
"""sha256 digests of what the training step computes, in every form it has (train_api.hip and the kernels it launches), on
seeded inputs, one JSON line: run it once per library (RCED_LIB=exp/<name>.so, or the product) in fresh processes ON ONE
DEVICE -- grids follow the CU count -- and compare the lines: a refactor of the training host code leaves every digest as it
was.  Public Python API only.  Sections named as arguments run alone (default: all).  Seconds.
Every section digests the losses, every entry of gradients() and of variables() (the moving statistics are among them) and,
where a step was applied, optimizer_state().
  step      the three nets, batch [5, 7, 129, 1] (35 frames: odd, a half-empty tile; 162 partial-sum records for an 18-channel
            layer: bn_finish's four-chain loop and its tail), three fit_steps
  step_big  CR-CED, batch [37, 131, 129, 1] (more tiles than persistent workgroups, the 2048-record cap), three fit_steps
  tiny      the weights and the input of tests/test_train_gpu.py::test_gamma_zero_and_tiny_gamma_get_their_true_gradients
            (gamma 0 and +-2e-4 / 3e-4 in four layers), batch [2, 3, 129, 1]: one train_step; one train_step_sharded over its
            two rows as two shards; the same with sync_bn=True
  forward   valid_step before and after a step, and variables() after the first: the start values
  shards    CR-CED and R-CED V2 (odd channel counts: phantom channels), rows cut 1 + 3 + 1: two steps of train_step_sharded; the
            same with sync_bn=True
  generic   CR-CED and R-CED V2, batch [5, 7, 129, 1], in a child process started with RCED_TRAIN_MFMA=0 (the switch is read
            at create): two fit_steps through the chan_reduce forms.  NOT REPRODUCIBLE: train::conv_wgrad adds its 3 workgroups'
            partial sums with fp32 atomics, so two runs of ONE library already differ here; compare generic_small instead
  generic_small  the same with batch [2, 7, 129, 1]: 14 frames are one conv_wgrad workgroup, every atomic has one contributor"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from fullycnnspeechenhancement_amd import FullyCNNTrainer  # noqa: E402
from oracle import rced_np  # noqa: E402

NETS = ("FullyCNN", "FullyCNNV2", "FullyCNNV3")
OUT = {}


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def named(d):
    return [d[k] for k in sorted(d)]


def digest(tag, tr, losses=None, applied=True):
    if losses is not None:
        OUT[tag + "/loss"] = sha([np.asarray(losses, np.float64)])
    OUT[tag + "/grads"] = sha(named(tr.gradients()))
    OUT[tag + "/vars"] = sha(named(tr.variables()))
    if applied:
        m, v, step = tr.optimizer_state()
        OUT[tag + "/adam"] = sha(named(m) + named(v) + [np.asarray(step, np.int64)])


def batch(n, t, seed):
    return rced_np.make_input(n, t, seed=seed), rced_np.make_input(n, t, seed=seed + 1)


def fit_steps(tag, net, n, t, steps, seed):
    tr = FullyCNNTrainer(net, batch_size=n, lr=1e-3, weights=rced_np.make_weights(net, seed=seed))
    x, y = batch(n, t, seed + 100)
    digest(tag, tr, [tr.fit_step(x, y)[0] for _ in range(steps)])
    tr.close()


def step():
    for i, net in enumerate(NETS):
        fit_steps("step/" + net, net, 5, 7, 3, 20 + i)


def step_big():
    fit_steps("step_big", "FullyCNNV3", 37, 131, 3, 30)


def tiny():
    w = {k: v.copy() for k, v in rced_np.make_weights("FullyCNNV3", seed=11).items()}
    for scope, c, gam, bet in (("CE2_encode_1", 5, 0.0, 0.3), ("CD1_encode_2", 17, 0.0, 0.2), ("CE3_encode_2", 3, 2e-4, 0.25),
                               ("CD2_encode_1", 11, -3e-4, 0.4)):
        w[scope + "/batch_norm/gamma"][c] = gam
        w[scope + "/batch_norm/beta"][c] = bet
    x = rced_np.make_input(2, 3, seed=9104)      # the draw that test's screening takes (seeds from 9100 on)
    y = rced_np.make_input(2, 3, seed=78)
    rows = [(x[0:1], y[0:1]), (x[1:2], y[1:2])]
    for tag, run in (("step", lambda tr: tr.train_step(x, y)), ("sharded", lambda tr: tr.train_step_sharded(rows)),
                     ("sync", lambda tr: tr.train_step_sharded(rows, sync_bn=True))):
        tr = FullyCNNTrainer("FullyCNNV3", batch_size=4, lr=1e-4, weights=w)
        digest("tiny/" + tag, tr, [run(tr)[0]])
        tr.close()


def forward():
    w = rced_np.make_weights("FullyCNNV3", seed=40)
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, lr=1e-3, weights=w)
    x, y = batch(3, 5, 41)
    OUT["forward/before"] = sha([tr.valid_step(x)])
    v = tr.variables()
    OUT["forward/vars"] = sha(named(v))
    OUT["forward/vars_are_the_start_values"] = all(np.array_equal(v[k], w[k]) for k in w)
    tr.train_step(x, y)
    OUT["forward/after"] = sha([tr.valid_step(x)])
    digest("forward/stepped", tr)
    tr.close()


def shards():
    for net in ("FullyCNNV3", "FullyCNNV2"):
        x, y = batch(5, 4, 51)
        cut = [(x[a:b], y[a:b]) for a, b in ((0, 1), (1, 4), (4, 5))]
        for sync in (False, True):
            tr = FullyCNNTrainer(net, batch_size=5, lr=1e-3, weights=rced_np.make_weights(net, seed=50))
            digest("shards/%s/%s" % (net, "sync" if sync else "own"), tr, [tr.train_step_sharded(cut, sync_bn=sync)[0] for _ in range(2)])
            tr.close()


def generic_child(tag, n):
    for i, net in enumerate(("FullyCNNV3", "FullyCNNV2")):
        fit_steps("%s/%s" % (tag, net), net, n, 7, 2, 60 + i)


def generic(tag="generic", n=5):
    env = dict(os.environ, RCED_TRAIN_MFMA="0")
    OUT.update(json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "generic_child", tag, str(n)], env=env,
                                         check=True, stdout=subprocess.PIPE, timeout=300).stdout))


def generic_small():
    generic("generic_small", 2)


if __name__ == "__main__":
    sections = (step, step_big, tiny, forward, shards, generic, generic_small)
    asked = sys.argv[1:]
    if asked[:1] == ["generic_child"]:
        generic_child(asked[1], int(asked[2]))
    else:
        unknown = set(asked) - set(s.__name__ for s in sections)
        if unknown:
            sys.exit("no such section: %s (there are: %s)" % (", ".join(sorted(unknown)), ", ".join(s.__name__ for s in sections)))
        for section in sections:
            if not asked or section.__name__ in asked:
                section()
    print(json.dumps(OUT, sort_keys=True))
