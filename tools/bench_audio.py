#!/usr/bin/env python3
"""Times the STFT front-end, the CNN and the ISTFT rebuild at BASELINE config-3 scale
(256 utterances x 512 frames = 65,664 samples each), device-resident, with torch.cuda events.  A second line times the
overlap-add rebuild (rebuild="ola") next to the reference rebuild, same spectra, same run.  A third line times the kernels that
take the framing as a parameter (rced_stft_fr, rced_istft_fr, rced_istft_ola_fr) at 256 / 128 / hamming, 160 / 80 / hamming and
256 / 64 / hanning next to the specialised ones, same signals, same run."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fullycnnspeechenhancement_amd import audio, build_model
from fullycnnspeechenhancement_amd import weights as _weights

N, T = 256, 512
L = (T - 1) * 128 + 256
pcm = torch.randn((N, L), device="cuda") * 0.1
model = build_model("FullyCNNV3", False, weights=_weights.synthetic_weights(3, seed=42))


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


t_stft, (mag, ph) = timed(lambda: audio.stft_batch(pcm))
assert mag.shape[1] == T
t_cnn, pred = timed(lambda: model(mag))
t_istft, _ = timed(lambda: audio.istft_batch(pred, ph))
frames = N * T
flop_dft = 2 * 256 * 258
print(json.dumps({"frames": frames, "stft_ms": t_stft, "cnn_ms": t_cnn, "istft_ms": t_istft,
                  "stft_tflops": frames * flop_dft / t_stft / 1e9, "istft_tflops": frames * flop_dft / t_istft / 1e9,
                  "stft_gbps_algorithmic": (N * L * 4 + frames * 129 * 12) / t_stft / 1e6,
                  "istft_gbps_algorithmic": (frames * 129 * 12 + N * (T + 1) * 128 * 4) / t_istft / 1e6,
                  "pipeline_frames_per_s": frames / ((t_stft + t_cnn + t_istft) * 1e-3)}))
# the two rebuilds on the same spectra, alternating, 100 calls a window (a 10-call window is 2 ms: the clock as much as the kernel)
ola, ref = [], []
for _ in range(5):
    ola.append(timed(lambda: audio.istft_batch(pred, ph, rebuild="ola"), reps=100)[0])
    ref.append(timed(lambda: audio.istft_batch(pred, ph), reps=100)[0])
t_ola, t_ref = sorted(ola)[2], sorted(ref)[2]
print(json.dumps({"frames": frames, "istft_reference_ms": t_ref, "istft_ola_ms": t_ola, "ola_over_reference": t_ola / t_ref,
                  "istft_reference_ms_windows": ref, "istft_ola_ms_windows": ola,
                  "ola_tflops": frames * 2 * 256 * 256 / t_ola / 1e9,
                  "ola_gbps_algorithmic": (frames * 129 * 12 + N * (T + 1) * 128 * 4) / t_ola / 1e6}))

# Third line: the general kernels (any framing, kernels_framing.h) next to the specialised ones, same signals, same run.  At
# 256 / 128 / hamming audio.stft_batch / istft_batch dispatch to the specialised entries, so the _fr entries are called directly.
from fullycnnspeechenhancement_amd import _args, _lib  # noqa: E402

lib, stream = _lib.load(), _args.current_stream(pcm.device)
CODES = {"hamming": 0, "hanning": 1, "blackman": 2, "bartlett": 3}


def fr_entries(W, S, name):
    """(stft, reference rebuild or None, overlap-add) closures over the _fr entries and the framing's own spectra."""
    t = lib.rced_stft_num_frames_fr(L, W, S)
    m = torch.empty((N, t, 129), dtype=torch.float32, device="cuda")
    p = torch.empty((N, t, 129, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((N, (W - S) + t * S), dtype=torch.float32, device="cuda")

    def stft():
        _lib.check(lib.rced_stft_fr(pcm.data_ptr(), None, N, L, t, W, S, CODES[name], m.data_ptr(), p.data_ptr(), 0, stream))

    def ref():
        _lib.check(lib.rced_istft_fr(m.data_ptr(), p.data_ptr(), N, t, 512, W, S, out.data_ptr(), 0, stream))

    def ola():
        _lib.check(lib.rced_istft_ola_fr(m.data_ptr(), p.data_ptr(), None, N, t, W, S, CODES[name], out.data_ptr(), 0, stream))

    return t, stft, (ref if name == "hamming" else None), ola


def median_ms(fn):
    return sorted(timed(fn, reps=100)[0] for _ in range(5))[2]


line = {"samples": L, "utterances": N,
        "specialised_256_128_hamming": {"frames": T, "stft_ms": median_ms(lambda: audio.stft_batch(pcm)),
                                        "istft_reference_ms": median_ms(lambda: audio.istft_batch(mag, ph)),
                                        "istft_ola_ms": median_ms(lambda: audio.istft_batch(mag, ph, rebuild="ola"))}}
for W, S, name in ((256, 128, "hamming"), (160, 80, "hamming"), (256, 64, "hanning")):
    t, stft, ref, ola = fr_entries(W, S, name)
    row = {"frames": t, "stft_ms": median_ms(stft)}          # the STFT first: the rebuilds read its spectra
    if ref is not None:
        row["istft_reference_ms"] = median_ms(ref)
    row["istft_ola_ms"] = median_ms(ola)
    line["general_%d_%d_%s" % (W, S, name)] = row
print(json.dumps(line))
