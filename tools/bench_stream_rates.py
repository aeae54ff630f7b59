#!/usr/bin/env python3
"""Times what streaming at the device's rate adds to a push: for 256 lanes and K = 1, 8 and 32 hops per push, the
8 kHz denoiser push (audio.StreamingDenoiser, CR-CED) and, for 16 kHz and 48 kHz in and out from int16, the same object at that
rate (`push_ms`) and its resampler lanes alone (audio.StreamingResampler down to 8 kHz from int16, and up again to float32), beside
the offline audio.resample_batch of the same number of samples.  Device-resident, torch.cuda events; every case is warmed up,
timed in windows that alternate between the cases, and reported as the median window.  One JSON line per K and rate."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fullycnnspeechenhancement_amd import audio, build_model
from fullycnnspeechenhancement_amd import weights as _weights

LANES, WINDOWS = 256, 7
model = build_model("FullyCNNV3", False, weights=_weights.synthetic_weights(3, seed=42))


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def medians(cases, reps):
    """cases: {name: fn}.  Ten warm-up calls each, then WINDOWS rounds over all cases in turn; the median ms per call of each."""
    for fn in cases.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name in cases}
    for _ in range(WINDOWS):
        for name, fn in cases.items():
            got[name].append(window(fn, reps))
    return {name: statistics.median(v) for name, v in got.items()}


for k in (1, 8, 32):
    reps = 1000 // k + 30
    stream = audio.StreamingDenoiser(model, LANES, max_hops=k)
    pcm8 = torch.randn((LANES, k * 128), device="cuda") * 0.1
    cases, held = {"push_8k": lambda: stream.push(pcm8)}, [stream]
    for rate in (16000, 48000):
        f = rate // 8000
        down = audio.StreamingResampler(rate, 8000, LANES, unit_out=128, dtype="int16", max_units=k)
        up = audio.StreamingResampler(8000, rate, LANES, unit_in=128, max_units=k)
        src = (torch.randn((LANES, k * 128 * f), device="cuda") * 3000).to(torch.int16)
        cases["down_%d" % rate] = lambda down=down, src=src: down.push(src)
        cases["up_%d" % rate] = lambda up=up: up.push(pcm8)
        cases["offline_down_%d" % rate] = lambda src=src, rate=rate: audio.resample_batch(src, rate, 8000)
        cases["offline_up_%d" % rate] = lambda rate=rate: audio.resample_batch(pcm8, 8000, rate)
        at_rate = audio.StreamingDenoiser(model, LANES, max_hops=k, sample_rate=rate, dtype="int16", output_rate=rate)
        cases["push_%d" % rate] = lambda at_rate=at_rate, src=src: at_rate.push(src)
        held += [down, up, at_rate]
    ms = medians(cases, reps)
    for s in held:
        s.close()
    for rate in (16000, 48000):
        added = ms["down_%d" % rate] + ms["up_%d" % rate]
        print(json.dumps({"lanes": LANES, "hops_per_push": k, "rate": rate, "push_8k_ms": ms["push_8k"], "down_ms": ms["down_%d" % rate],
                          "up_ms": ms["up_%d" % rate], "lanes_ms": added, "push_ms": ms["push_%d" % rate],
                          "added_ms": ms["push_%d" % rate] - ms["push_8k"], "added_over_push_8k": ms["push_%d" % rate] / ms["push_8k"] - 1.0,
                          "offline_down_ms": ms["offline_down_%d" % rate], "offline_up_ms": ms["offline_up_%d" % rate],
                          "realtime_lanes_per_device": 16.0 * k / ms["push_%d" % rate] * LANES}))   # a hop is 16 ms of audio
