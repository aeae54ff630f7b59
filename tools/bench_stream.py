#!/usr/bin/env python3
"""Times the streaming denoiser (audio.StreamingDenoiser, CR-CED) for 256 lanes at K = 1, 8 and 32 hops per push, device-resident,
with torch.cuda events: ms per push and frames/s, beside the offline PCM-to-PCM chain (stft_batch -> model -> istft_batch) at the
same total frame count (256 utterances of K frames) and at BASELINE config-3 scale (256 x 512 frames).  One JSON line per row.
A push recomputes 7 frames per lane for the CNN: `recompute` is (K + 7) / K.
--rebuild both (the default) times a reference-rebuild stream and an overlap-add stream (rebuild="ola") in the same run, in alternating
rounds, and reports each one's median round and their ratio; --rebuild reference / ola times one of them.
The last line times audio.BlockDenoiser (--blocks: that line alone): ms per process() for 256 lanes at 48 kHz in blocks of 480
and of 768 frames and at 44.1 kHz in blocks of 441, beside StreamingDenoiser(48000, 48000)'s push of one hop (768 frames), all four in
alternating rounds of the same run; one JSON line.
After it (--framing: that line alone) the lanes at a framing, overlap-add, 256 lanes at K = 1, 8 and 32 hops per push:
the general stream (rced_stream_create_fr) at 256 / 128 / hamming beside the specialised one, and at 160 / 80 / hamming and 256 / 64 /
hanning, all four in alternating rounds of the same run; ms per push, and per framing the audio a push carries; one JSON line."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fullycnnspeechenhancement_amd import audio, build_model
from fullycnnspeechenhancement_amd import weights as _weights

parser = argparse.ArgumentParser(description=__doc__)
parser.add_argument("--rebuild", choices=("both", "reference", "ola"), default="both",
                    help="the streams' rebuild; both (default): one stream of each, timed in alternating rounds of the same run")
parser.add_argument("--rounds", type=int, default=5, help="timed rounds per stream; the median is reported")
parser.add_argument("--framing", action="store_true", help="time the lanes at a framing beside the specialised stream, that line alone")
parser.add_argument("--blocks", action="store_true", help="time BlockDenoiser.process at 48 and 44.1 kHz beside the one-hop push at 48 kHz")
args = parser.parse_args()
REBUILDS = ("reference", "ola") if args.rebuild == "both" else (args.rebuild,)

LANES = 256
model = build_model("FullyCNNV3", False, weights=_weights.synthetic_weights(3, seed=42))


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def offline(n, t):
    pcm = torch.randn((n, (t - 1) * 128 + 256), device="cuda") * 0.1

    def chain():
        mag, ph = audio.stft_batch(pcm)
        return audio.istft_batch(model(mag), ph)
    return chain


def block_rows():
    cases = {"block_480_at_48000": (48000, 480), "block_768_at_48000": (48000, 768), "block_441_at_44100": (44100, 441)}
    objs = {name: audio.BlockDenoiser(model, LANES, block, sample_rate=rate, output_rate=rate) for name, (rate, block) in cases.items()}
    pcm = {name: torch.randn((LANES, block), device="cuda") * 0.1 for name, (rate, block) in cases.items()}
    calls = {name: (lambda name=name: objs[name].process(pcm[name])) for name in cases}
    hop = audio.StreamingDenoiser(model, LANES, max_hops=1, sample_rate=48000, output_rate=48000)
    hop_pcm = torch.randn((LANES, 768), device="cuda") * 0.1
    calls["hop_push_768_at_48000"] = lambda: hop.push(hop_pcm)
    rounds = {name: [] for name in calls}
    for _ in range(args.rounds):               # a period of the 44.1 kHz pattern is 128 calls: 1,280 calls cover ten
        for name, fn in calls.items():
            rounds[name].append(timed(fn, 1280))
    row = {"lanes": LANES, "rounds": args.rounds}
    for name, v in rounds.items():
        row[name] = {"ms": statistics.median(v), "ms_rounds": [round(x, 5) for x in v]}
        if name in objs:
            row[name].update(delay=objs[name].delay, hops_per_call=objs[name].hops_per_call)
    print(json.dumps(row), flush=True)
    for o in list(objs.values()) + [hop]:
        o.close()


def framing_rows():
    from fullycnnspeechenhancement_amd.streaming import _DenoiserLanes
    cases = {"general_256_128_hamming": audio.Framing(256, 128, "hamming"), "general_160_80_hamming": audio.Framing(160, 80, "hamming"),
             "general_256_64_hanning": audio.Framing(256, 64, "hanning")}
    row = {"lanes": LANES, "rounds": args.rounds, "rebuild": "ola"}
    for k in (1, 8, 32):
        # _DenoiserLanes with a Framing always makes the general stream, at the default framing too (StreamingDenoiser would not)
        objs = {"specialised_256_128_hamming": audio.StreamingDenoiser(model, LANES, max_hops=k, rebuild="ola")}
        objs.update({name: _DenoiserLanes(model, LANES, k, 512, "ola", fr) for name, fr in cases.items()})
        hop = {name: cases[name].stride if name in cases else 128 for name in objs}
        pcm = {name: torch.randn((LANES, k * hop[name]), device="cuda") * 0.1 for name in objs}
        reps = 2000 // k + 50
        rounds = {name: [] for name in objs}
        for _ in range(args.rounds):
            for name in objs:
                rounds[name].append(timed(lambda name=name: objs[name].push(pcm[name]), reps))
        for o in objs.values():
            o.close()
        ms = {name: statistics.median(v) for name, v in rounds.items()}
        row["hops_%d" % k] = {name: {"push_ms": ms[name], "push_ms_rounds": [round(v, 5) for v in rounds[name]], "audio_ms_per_push": k * hop[name] / 8.0,
                                     "over_specialised": ms[name] / ms["specialised_256_128_hamming"]} for name in objs}
    print(json.dumps(row), flush=True)


if args.blocks:
    block_rows()
    sys.exit(0)
if args.framing:
    framing_rows()
    sys.exit(0)

for k in (1, 8, 32):
    streams = {r: audio.StreamingDenoiser(model, LANES, max_hops=k, rebuild=r) for r in REBUILDS}
    pcm = torch.randn((LANES, k * 128), device="cuda") * 0.1
    reps = 2000 // k + 50                      # a second or so of pushes: every lane is far into its utterance
    rounds = {r: [] for r in REBUILDS}
    for _ in range(args.rounds):               # reference, ola, reference, ola, ..: what else the machine does falls on both alike
        for r in REBUILDS:
            rounds[r].append(timed(lambda: streams[r].push(pcm), reps))
    off_ms = timed(offline(LANES, k), reps)
    for s in streams.values():
        s.close()
    frames = LANES * k
    push = {r: statistics.median(v) for r, v in rounds.items()}
    row = {"lanes": LANES, "hops_per_push": k, "recompute": (k + 7) / k, "offline_same_frames_ms": off_ms,
           "offline_same_frames_per_s": frames / (off_ms * 1e-3)}
    for r, ms in push.items():
        row[r] = {"push_ms": ms, "push_ms_rounds": [round(v, 5) for v in rounds[r]], "stream_frames_per_s": frames / (ms * 1e-3),
                  "realtime_lanes_per_device": 16.0 * k / ms * LANES}     # a hop is 16 ms of audio
    if len(push) == 2:
        row["ola_over_reference"] = push["ola"] / push["reference"]
    print(json.dumps(row), flush=True)
ms = timed(offline(256, 512), 20)
print(json.dumps({"offline_utterances": 256, "offline_frames_each": 512, "offline_ms": ms, "offline_frames_per_s": 256 * 512 / (ms * 1e-3)}))
block_rows()
framing_rows()
