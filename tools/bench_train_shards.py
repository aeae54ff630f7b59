#!/usr/bin/env python
"""What the split of the training step costs: `train_step` beside `grad_step` + `apply_step` over S = 1, 2 and 4
accumulation shards, at BASELINE config 5's size (CR-CED V3, 256 x 512 frames), all in one run.

    python tools/bench_train_shards.py [--batch 256] [--frames 512] [--steps 5] [--rounds 5] [--warmup 2] [--sync]

One trainer runs every form (each is one optimizer step over the same batch).  The forms alternate: a round times `steps`
calls of each form in turn, and the figure of a form is the median over the rounds of its per-step time, printed with the
fastest and the slowest round.  Every call ends in a device synchronise (the step returns the loss), so a host clock around
the calls measures the device work plus the launches.  `train_step` is the unsharded path and the yardstick; S = 1 adds to
it the two exchange kernels of the gradient pass and the memset, scatter and moving-statistics kernels of the apply.
S = 2 and 4 run the same pixels in 2 and 4 passes: shorter grids per pass, the weights packed once per pass.
--sync adds the synchronised step (`train_step_sharded(cut, sync_bn=True)`) over the same S in the same
run, as `sync_S`: S trainers on this device in lockstep, thirty stops a step, each with S small copies and S ordered-sum
launches on the stream and no host synchronise.  It is what the stops cost on ONE device; a world of ranks under gloo adds
a stream synchronise and a host all_gather per stop, which this tool does not measure.  The replicas hold activations of
their own: --sync needs about twice the memory.
Prints one JSON line.  Needs a GPU: there is no other way to take these numbers."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shards", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--sync", action="store_true", help="also time the synchronised step over the same shard counts")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_shards needs a GPU")
    import __graft_entry__ as ge
    ge.build_hip()
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, weights
    from fullycnnspeechenhancement_amd.dist import shard_bounds
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn((a.batch, a.frames, 129, 1), generator=g, device="cuda").abs_()
    y = 0.5 * torch.randn((a.batch, a.frames, 129, 1), generator=g, device="cuda").abs_()
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=a.batch, lr=1e-3, weights=weights.synthetic_weights(3, seed=42))
    forms = {"train_step": lambda: tr.train_step(x, y)}
    for s in a.shards:
        cut = [(x[lo:hi], y[lo:hi]) for lo, hi in shard_bounds(a.batch, s)]
        forms["shards_%d" % s] = (lambda cut=cut: tr.train_step_sharded(cut))
        if a.sync:
            forms["sync_%d" % s] = (lambda cut=cut: tr.train_step_sharded(cut, sync_bn=True))
    for fn in forms.values():              # every shape the timed window uses, before it
        for _ in range(a.warmup):
            fn()
    per_round = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            per_round[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    out = {"workload": "CR-CED V3 training step, %d x %d frames" % (a.batch, a.frames), "steps_per_round": a.steps, "rounds": a.rounds,
           "ms": {name: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                  for name, v in per_round.items()}}
    base = out["ms"]["train_step"]["median"]
    out["over_train_step"] = {name: round(v["median"] / base, 4) for name, v in out["ms"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
