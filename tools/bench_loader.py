#!/usr/bin/env python3
"""Times one batch build of the device loader (loader.DataLoader.build) at BASELINE config-5 scale: 256
utterances of 65,664 samples (512 frames), cut out of int16 arenas on the device -- gather x2, mix, one STFT over the 2N rows --
the same build with every utterance under a room impulse response of 4096 taps (DataSet(rir=...): one rced_convolve launch more),
beside the only way the code offered before: AudioParser.add_noise + parse_audio x2 per utterance (numpy in, numpy out: an
upload and a download each), on the same signals, and both against the 39.6-39.8 ms training step.

Device time comes from torch.cuda events around `reps` builds after a warm-up (it includes the host's gaps between the
launches: the plan's small uploads are part of a build); the wall time ends in a synchronise.  The stages are timed alone, each
over its own repetitions.  The per-utterance path returns numpy arrays, so its host clock ends in a copy back.  Half of the
noises are longer than the speech (cropped by the gather), half are shorter (tiled with gains by the mix).  One JSON line."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from fullycnnspeechenhancement_amd import audio, loader

N, LS, REPS, STEP_MS = 256, 65664, 20, (39.6, 39.8)
rng = np.random.default_rng(5)
clean = [np.round(0.2 * rng.standard_normal(LS) * 32768).clip(-32768, 32767).astype(np.int16) for _ in range(N)]
noise = [np.round(0.1 * rng.standard_normal(LS * 2 if i % 2 else LS // 3) * 32768).clip(-32768, 32767).astype(np.int16)
         for i in range(N)]
cc, nc = loader.Corpus.from_arrays(clean), loader.Corpus.from_arrays(noise)
ds = loader.DataSet(cc, noise=nc, snr=0)
dl = loader.DataLoader(ds, N)
np.random.seed(1)
plan = [ds.plan(i) for i in range(N)]


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3 / reps


build_ms, build_wall_ms = timed(lambda: dl.build(plan), REPS)

# the reverberant build of the same plan: synthetic responses cut to 4096 taps, every row under one (rir_prob = 1)
RIR_TAPS, RIR_REPS = 4096, 5
rc = loader.RirCorpus.from_arrays([h[:RIR_TAPS] for h in loader.synthetic_rirs(8, rt60=(0.6, 0.6), seed=5)])
assert all(int(k) == RIR_TAPS for k in rc.lengths)
dl_rir = loader.DataLoader(loader.DataSet(cc, noise=nc, snr=0, rir=rc), N)
plan_rir = [p + (i % len(rc),) for i, p in enumerate(plan)]
rir_build_ms, rir_build_wall_ms = timed(lambda: dl_rir.build(plan_rir), RIR_REPS)

# the stages alone, on the buffers a build uses
ids = list(range(N))
both = torch.empty((2 * N, LS), dtype=torch.float32, device="cuda")
starts = [p[2] if nc.lengths[p[1]] > LS else 0 for p in plan]
counts = [LS if nc.lengths[p[1]] > LS else int(nc.lengths[p[1]]) for p in plan]
gains = [p[3] for p in plan]
nrows = nc.gather(ids, starts, counts)
filt, taps, shifts = rc.filters([p[4] for p in plan_rir])
dry = cc.gather(ids, L=LS)
stages = {
    "convolve_ms": timed(lambda: audio.convolve_batch(dry, filt, [LS] * N, taps, shifts, out=both[:N]), RIR_REPS)[0],
    "gather_speech_ms": timed(lambda: cc.gather(ids, L=LS, out=both[:N]), REPS)[0],
    "gather_noise_ms": timed(lambda: nc.gather(ids, starts, counts), REPS)[0],
    "mix_ms": timed(lambda: audio.mix_snr_batch(both[:N], nrows, 0, speech_lengths=[LS] * N, noise_lengths=counts, gains=gains,
                                                out=both[N:]), REPS)[0],
    "stft_2n_ms": timed(lambda: audio.stft_batch(both, [LS] * (2 * N), with_phase=False), REPS)[0],
}

# the per-utterance path: the same signals as float32 arrays on the host, the same draws
parser = loader.AudioParser(sample_rate=8000, window_ms=32, stride_ms=16, snr=0)
host_clean = [c.astype(np.float32) / 32768 for c in clean]
host_noise = [n.astype(np.float32) / 32768 for n in noise]


def per_utterance(count):
    for i in range(count):
        mix = parser.add_noise(host_clean[i], host_noise[i])
        parser.parse_audio(host_clean[i])
        parser.parse_audio(mix)


np.random.seed(1)
per_utterance(8)                                   # warm-up
torch.cuda.synchronize()
np.random.seed(1)
t0 = time.perf_counter()
per_utterance(N)
torch.cuda.synchronize()
per_utt_ms = (time.perf_counter() - t0) * 1e3

row = {"utterances": N, "samples_each": LS, "batch_build_ms": build_ms, "batch_build_wall_ms": build_wall_ms,
       "rir_taps": RIR_TAPS, "rir_batch_build_ms": rir_build_ms, "rir_batch_build_wall_ms": rir_build_wall_ms,
       "per_utterance_path_ms": per_utt_ms, "train_step_ms": list(STEP_MS),
       "batch_build_over_step": build_ms / STEP_MS[0], "rir_batch_build_over_step": rir_build_ms / STEP_MS[0], "per_utterance_path_over_step": per_utt_ms / STEP_MS[0]}
row.update(stages)
print(json.dumps(row))
