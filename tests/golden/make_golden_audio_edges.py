"""Generates tests/golden/audio_edges.npz from the REFERENCE'S OWN numpy code, as make_golden_audio.py does for
audio_stft.npz, at the edges that file leaves out:
    STFT     AudioFeature.compute_spectrogram / divide_phase at odd and very short lengths (1, 2, 127, 255, 257, 385) and at
             8321, the first length with 65 frames (one more than a 64-frame block of the kernels);
    rebuild  AudioReBuild.rebuild_audio of ARBITRARY complex spectra -- |randn| magnitudes, a uniform phase at every bin, bins 0
             and 128 included, which the STFT of a real signal never produces -- at T = 1, 2, 65 for nfft = 512 and 256.
Inputs are stored in the types the device takes them in (float32 PCM, float32 magnitude, complex64 phase), outputs as float64.
Nothing of the reference's source is copied: the script imports it from /root/reference at generation time only.

The two environment shims of make_golden_audio.py (np.mat -> np.asmatrix; empty stand-ins for librosa / pypesq / pystoi, which
model_utils/utils.py imports and AudioReBuild never touches), neither touching the algorithm.

Run from the repo root:  python tests/golden/make_golden_audio_edges.py
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

STFT_LENGTHS = [1, 2, 127, 255, 257, 385, 8321]
REBUILD_FRAMES = [1, 2, 65]
REBUILD_NFFT = [512, 256]


def main():
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    for name, attrs in (("librosa", ()), ("pypesq", ("pesq",)), ("pystoi", ("stoi",))):
        if name not in sys.modules:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[name] = m
    sys.path.insert(0, REF)
    from data_utils.audio_feature import AudioFeature
    from model_utils.utils import AudioReBuild

    sr, window_ms, stride_ms = 8000, 32, 16
    rng = np.random.default_rng(2025)
    out = {"lengths": np.asarray(STFT_LENGTHS, np.int32), "rebuild_frames": np.asarray(REBUILD_FRAMES, np.int32),
           "rebuild_nfft": np.asarray(REBUILD_NFFT, np.int32)}
    fe = AudioFeature()
    for i, L in enumerate(STFT_LENGTHS):
        sig = (0.2 * rng.standard_normal(L)).astype(np.float32)
        spec = fe.compute_spectrogram(sig, sr, window_s=window_ms / 1000, stride_s=stride_ms / 1000, nfft=256, use_complex=True)
        out["pcm_%d" % i] = sig
        out["mag_%d" % i] = fe.power_spectrum(spec).T.astype(np.float64)        # [T, 129]
        out["phase_%d" % i] = fe.divide_phase(spec).T.astype(np.complex128)
    for T in REBUILD_FRAMES:
        mag = np.abs(rng.standard_normal((T, 129))).astype(np.float32)
        phase = np.exp(1j * rng.uniform(-np.pi, np.pi, (T, 129))).astype(np.complex64)
        out["rb_mag_%d" % T], out["rb_phase_%d" % T] = mag, phase
        for nfft in REBUILD_NFFT:
            # handed over widened: the reference multiplies magnitude and phase in the precision it is given, and what is pinned
            # here is the float64 result on these (rounded) values, not a complex64 product
            audio = AudioReBuild(nfft=nfft).rebuild_audio([(T + 1) * 128], mag[None].astype(np.float64),
                                                          phase[None].astype(np.complex128), sr, window_ms, stride_ms)[0]
            out["rb_audio_%d_%d" % (T, nfft)] = np.asarray(audio, np.float64)
    path = os.path.join(HERE, "audio_edges.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
