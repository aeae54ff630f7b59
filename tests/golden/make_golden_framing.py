"""Generates tests/golden/framing_ref.npz from the REFERENCE'S OWN numpy code, at framings other than the 256 / 128 / hamming
that audio_stft.npz and audio_edges.npz pin:
    STFT     AudioFeature(windows_name).compute_spectrogram(use_complex=True) for every framing of tests/framing_np.FRAMINGS at the
             lengths 1, W - 1, W, W + 1, W + 5 S + 3;
    rebuild  AudioReBuild(nfft=nfft).rebuild_audio for the three hamming framings (256 / 128 among them) of ARBITRARY spectra --
             |randn| magnitudes, a uniform phase at every bin, bins 0 and 128 included -- at T = 1, 2, 7 and nfft = 256, 512.
Inputs are stored in the types the device takes them in (float32 PCM, float32 magnitude, complex64 phase), outputs as float64 /
complex128.  Nothing of the reference's source is copied: the script imports it from /root/reference at generation time only, with
the two environment shims of make_golden_audio_edges.py (np.mat -> np.asmatrix; empty stand-ins for librosa / pypesq / pystoi).

The framings are handed over as the reference takes them: seconds for the STFT (int(round(s * rate)) samples), milliseconds for the
rebuild (int(ms * rate / 1000) samples), at 8 kHz; the script checks that both roundings give the samples meant.

Run from the repo root:  python tests/golden/make_golden_framing.py
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import framing_np as fnp  # noqa: E402

SR = 8000
REBUILD_FRAMES = [1, 2, 7]
REBUILD_NFFT = [256, 512]


def stft_lengths(W, S):
    return [1, W - 1, W, W + 1, W + 5 * S + 3]


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

    rng = np.random.default_rng(2026)
    out = {"rebuild_frames": np.asarray(REBUILD_FRAMES, np.int32), "rebuild_nfft": np.asarray(REBUILD_NFFT, np.int32)}
    for W, S, name in fnp.FRAMINGS:
        window_s, stride_s = W / SR, S / SR
        assert int(round(window_s * SR)) == W and int(round(stride_s * SR)) == S
        fe = AudioFeature(name)
        key = fnp.tag(W, S, name)
        out["lengths_" + key] = np.asarray(stft_lengths(W, S), np.int32)
        for i, L in enumerate(stft_lengths(W, S)):
            sig = (0.2 * rng.standard_normal(L)).astype(np.float32)
            spec = fe.compute_spectrogram(sig, SR, window_s=window_s, stride_s=stride_s, nfft=256, use_complex=True)
            out["pcm_%s_%d" % (key, i)] = sig
            out["spec_%s_%d" % (key, i)] = np.asarray(spec, np.complex128).T          # [T, 129]
    for W, S, name in fnp.HAMMING_FRAMINGS:
        windows_ms, stride_ms = W * 1000.0 / SR, S * 1000.0 / SR
        assert int((windows_ms * SR) / 1000) == W and int((stride_ms * SR) / 1000) == S
        key = fnp.tag(W, S, name)
        for T in REBUILD_FRAMES:
            mag = np.abs(rng.standard_normal((T, 129))).astype(np.float32)
            phase = np.exp(1j * rng.uniform(-np.pi, np.pi, (T, 129))).astype(np.complex64)
            out["rb_mag_%s_%d" % (key, T)], out["rb_phase_%s_%d" % (key, T)] = mag, phase
            for nfft in REBUILD_NFFT:
                # handed over widened: what is pinned is the float64 result on these (rounded) values, not a complex64 product
                audio = AudioReBuild(name, nfft=nfft).rebuild_audio([fnp.width(T, W, S)], mag[None].astype(np.float64),
                                                                    phase[None].astype(np.complex128), SR, windows_ms, stride_ms)[0]
                out["rb_audio_%s_%d_%d" % (key, T, nfft)] = np.asarray(audio, np.float64)
    path = os.path.join(HERE, "framing_ref.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 631529


if __name__ == "__main__":
    main()
