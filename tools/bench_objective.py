#!/usr/bin/env python3
"""Times the wave objective at BASELINE config-3 scale (256 utterances x 512 frames = 65,664 samples each), in one run:
line 1: audio.wave_loss_batch's entry (rced_wave_loss, with and without the gradient) beside audio.stft_batch and
        audio.istft_batch(rebuild="ola") on the same signals, alternating, the median of five windows of 50 calls;
line 2: the CR-CED training step with the spectral loss beside the step with each objective, one trainer, alternating, the
        median of three windows of 10 steps (the learning rate is 0: every window steps the same variables).
--entries: line 1 only (what a kernel trace of the added launches is taken from).
--framing W S name: line 1 also times, in the same alternating run and on the same signals, rced_wave_loss_fr at that framing (with
        and without the gradient) beside audio.stft_batch(framing=) and audio.istft_batch(rebuild="ola", framing=) -- the general
        kernels (kernels_framing.h, kernels_wave_loss_fr.h) next to the specialised ones; the keys end in _fr.
Line 1 always times rced_wave_loss_mr with audio.MR_STFT_8K (kernels_mr_stft.h) beside rced_wave_loss_fr at the same framing --
        256 / 128 / hamming through the general kernels -- with and without the gradient: the keys wave_loss_fr256_* and wave_loss_mr_*;
        line 2 the step with the multi-resolution STFT term beside the steps without it."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from fullycnnspeechenhancement_amd import FullyCNNTrainer, _args, _lib, audio
from fullycnnspeechenhancement_amd import weights as _weights

N, T = 256, 512
L = (T - 1) * 128 + 256
torch.manual_seed(0)
clean = torch.randn((N, L), device="cuda") * 0.1
pcm = clean + torch.randn((N, L), device="cuda") * 0.03
lengths = [L] * N


def window(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating(fns, windows, reps, warm=3):
    """name -> the median over `windows` windows of `reps` calls, the candidates taking turns."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            times[k].append(window(fn, reps))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}, times


mag, ph = audio.stft_batch(pcm)
assert mag.shape[1] == T
lib, stream = _lib.load(), _args.current_stream(pcm.device)
phr = torch.view_as_real(ph).contiguous()
m3 = mag.squeeze(-1).contiguous()
ldev = torch.tensor(lengths, dtype=torch.int32, device="cuda")
terms = torch.empty((N, 3), dtype=torch.float64, device="cuda")
grad = torch.empty((N, T, 129), dtype=torch.float32, device="cuda")


def wave(with_grad):
    _lib.check(lib.rced_wave_loss(m3.data_ptr(), phr.data_ptr(), None, clean.data_ptr(), L, ldev.data_ptr(), N, T, 0.5, 1.0, 1, 1.0 / N,
                                  terms.data_ptr(), grad.data_ptr() if with_grad else None, 0, stream))


mr_args = audio.WaveObjective(1, 0, 0, True, 0.5).mr_args()
terms5 = torch.empty((N, 5), dtype=torch.float64, device="cuda")


def wave_fr256(with_grad):
    _lib.check(lib.rced_wave_loss_fr(m3.data_ptr(), phr.data_ptr(), None, clean.data_ptr(), L, ldev.data_ptr(), N, T, 256, 128, 0, 0.5, 1.0, 1,
                                     1.0 / N, terms.data_ptr(), grad.data_ptr() if with_grad else None, 0, stream))


def wave_mr(with_grad):
    import ctypes
    _lib.check(lib.rced_wave_loss_mr(m3.data_ptr(), phr.data_ptr(), None, clean.data_ptr(), L, ldev.data_ptr(), N, T, 256, 128, 0, 0.5, 1.0, 1,
                                     1.0 / N, ctypes.byref(mr_args), terms5.data_ptr(), grad.data_ptr() if with_grad else None, 0, stream))


fns = {"stft_ms": lambda: audio.stft_batch(pcm), "istft_ola_ms": lambda: audio.istft_batch(mag, ph, rebuild="ola"),
       "wave_loss_terms_ms": lambda: wave(False), "wave_loss_ms": lambda: wave(True),
       "wave_loss_fr256_terms_ms": lambda: wave_fr256(False), "wave_loss_fr256_ms": lambda: wave_fr256(True),
       "wave_loss_mr_terms_ms": lambda: wave_mr(False), "wave_loss_mr_ms": lambda: wave_mr(True)}
shape = {"utterances": N, "frames": T, "samples": L}
if "--framing" in sys.argv[1:]:
    at = sys.argv.index("--framing")
    fr = audio.Framing(int(sys.argv[at + 1]), int(sys.argv[at + 2]), sys.argv[at + 3])
    mag_fr, ph_fr = audio.stft_batch(pcm, framing=fr)
    T_fr = int(mag_fr.shape[1])
    phr_fr, m3_fr = torch.view_as_real(ph_fr).contiguous(), mag_fr.squeeze(-1).contiguous()
    grad_fr = torch.empty((N, T_fr, 129), dtype=torch.float32, device="cuda")

    def wave_fr(with_grad):
        _lib.check(lib.rced_wave_loss_fr(m3_fr.data_ptr(), phr_fr.data_ptr(), None, clean.data_ptr(), L, ldev.data_ptr(), N, T_fr, fr.window,
                                         fr.stride, fr.code, 0.5, 1.0, 1, 1.0 / N, terms.data_ptr(),
                                         grad_fr.data_ptr() if with_grad else None, 0, stream))

    fns.update({"stft_fr_ms": lambda: audio.stft_batch(pcm, framing=fr),
                "istft_ola_fr_ms": lambda: audio.istft_batch(mag_fr, ph_fr, rebuild="ola", framing=fr),
                "wave_loss_terms_fr_ms": lambda: wave_fr(False), "wave_loss_fr_ms": lambda: wave_fr(True)})
    shape.update({"framing": [fr.window, fr.stride, fr.windows_name], "frames_fr": T_fr})
med, _ = alternating(fns, 5, 50)
med["reverse_and_adjoint_ms"] = med["wave_loss_ms"] - med["wave_loss_terms_ms"]
med["sums_ms"] = med["wave_loss_terms_ms"] - med["istft_ola_ms"]
med["mr_term_ms"] = med["wave_loss_mr_terms_ms"] - med["wave_loss_fr256_terms_ms"]
med["mr_term_and_gradient_ms"] = med["wave_loss_mr_ms"] - med["wave_loss_fr256_ms"]
if "wave_loss_fr_ms" in med:
    med["reverse_and_adjoint_fr_ms"] = med["wave_loss_fr_ms"] - med["wave_loss_terms_fr_ms"]
    med["sums_fr_ms"] = med["wave_loss_terms_fr_ms"] - med["istft_ola_fr_ms"]
print(json.dumps(dict(shape, **med)))
if "--entries" in sys.argv[1:]:
    sys.exit(0)

tr = FullyCNNTrainer("FullyCNNV3", batch_size=N, lr=0.0, weights=_weights.synthetic_weights(3, seed=42))
target, _ = audio.stft_batch(clean)
wave_args = (ph, clean, lengths)
OBJECTIVES = {"spectral": None, "spectral+wave_sse": audio.WaveObjective(1, 1, 0), "spectral+si_sdr": audio.WaveObjective(1, 0, 1),
              "spectral+wave_sse+si_sdr": audio.WaveObjective(1, 0.5, 1), "si_sdr": audio.WaveObjective(0, 0, 1),
              "spectral+wave_sse+si_sdr@fr256": audio.WaveObjective(1, 0.5, 1),
              "spectral+wave_sse+si_sdr+mr_stft": audio.WaveObjective(1, 0.5, 1, True, 0.5), "spectral+mr_stft": audio.WaveObjective(1, 0, 0, True, 0.5)}


def step(objective):
    tr.objective = objective
    tr.train_step(mag, target, wave=wave_args if objective is not None else None)


def step_fr256(objective):
    """The same objective through rced_train_step_wave_fr: the general kernels the _mr entries run, without the term."""
    import ctypes
    tr.objective = objective
    args, keep = tr._wave_args(wave_args, mag)
    loss, parts = ctypes.c_double(), (ctypes.c_double * 3)()
    _lib.check(lib.rced_train_step_wave_fr(tr._h, mag.data_ptr(), target.data_ptr(), N, T, ctypes.c_float(0.0), ctypes.byref(args), 256, 128, 0,
                                           ctypes.byref(loss), parts, stream))


med, all_windows = alternating({k: (lambda o=o, k=k: step_fr256(o) if k.endswith("@fr256") else step(o)) for k, o in OBJECTIVES.items()}, 3, 10,
                               warm=2)
print(json.dumps({"net": "FullyCNNV3", "utterances": N, "frames": T, "step_ms": med,
                  "added_ms": {k: v - med["spectral"] for k, v in med.items() if k != "spectral"}, "step_ms_windows": all_windows}))
tr.close()
