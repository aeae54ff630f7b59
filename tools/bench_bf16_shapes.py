#!/usr/bin/env python3
"""The bf16 kernels over call sizes (device-resident, ms per call after a warm-up): tools/bench_bf16_shapes.py -> one JSON line.
R-CED V2 / V1 in "bf16" mode; CR-CED with option "v3_bf16" on ("FullyCNNV3 bf16 NxT") and, on the same handle, inputs and shapes, in its
default form ("FullyCNNV3 default NxT": the fp32-quality kernel the headline runs).
Used to compare builds (RCED_LIB=exp/<name>.so): the four-wave product against the eight-wave form on small and large calls."""
import os, sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fullycnnspeechenhancement_amd import build_model, weights, spec
SHAPES = ((1, 64), (1, 256), (8, 512), (64, 512), (256, 512))
out = {}


def ms_per_call(m, x, y, warm=150, reps=300):     # a 0.5 ms kernel needs about 100 launches before its time settles
    for _ in range(warm): m(x, out=y)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): m(x, out=y)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / reps * 1e3, 4)


for net in ("FullyCNNV2", "FullyCNN"):
    m = build_model(net, False, weights=weights.synthetic_weights(spec.variant_of(net)), dtype="bfloat16")
    for (n, t) in SHAPES:
        x = torch.randn((n, t, 129, 1), device="cuda").abs_()
        out["%s %dx%d" % (net, n, t)] = ms_per_call(m, x, torch.empty_like(x))
    m.close()
m = build_model("FullyCNNV3", False, weights=weights.synthetic_weights(spec.variant_of("FullyCNNV3")))
for (n, t) in SHAPES:
    x = torch.randn((n, t, 129, 1), device="cuda").abs_()
    y = torch.empty_like(x)
    for mode, on in (("bf16", 1), ("default", 0)):
        m.set_option("v3_bf16", on)
        out["FullyCNNV3 %s %dx%d" % (mode, n, t)] = ms_per_call(m, x, y)
m.close()
print(json.dumps(out))
