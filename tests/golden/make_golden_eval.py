"""Generates tests/golden/eval_ref.npz from the REFERENCE'S OWN numpy code:
    data_utils/data_loader.py    AudioParser.add_noise                             (SNR mixing)
    data_utils/audio_feature.py  AudioFeature.compute_spectrogram / divide_phase   (STFT front-end)
    model_utils/utils.py         AudioReBuild.rebuild_audio, SDR                   (ISTFT rebuild, score)
All numpy-only, so their outputs are real reference outputs and PIN the evaluation loop's rows.  Nothing of the
reference's source is copied: the script imports it from the reference checkout named on the command line, feeds seeded
signals and stores data only.

The inputs are float32 arrays WIDENED TO FLOAT64 before they enter the reference, so every stored result is the
float64 answer for exactly representable inputs and carries none of numpy's float32 summation noise.

Environment shims as in make_golden_audio.py (np.mat alias; empty stand-ins for librosa / pypesq / pystoi, plus joblib
where it is absent: data_loader.py imports it for its DataLoader, which is not used here).

Per case i = (ls, ln, snr): speech_i, noise_i (float32), seed_i, mix_i (float64, add_noise after np.random.seed(seed_i)),
next_i (the next np.random.random() after it: where the reference leaves the stream), start_i / gains_i / draws_i (the
crop offset, the uniform(0, 2) draws that can reach the speech, the number of draws made: recorded by replaying the seed in
the order add_noise consumes it, and checked here against next_i), and for nfft in {512, 256} x mask gain in {1.0, 0.5}
(the stand-in model pred = gain * mag): sdr_i_<nfft>_<gain*10> = SDR()(clean, rebuilt) from the un-cast float64 signals,
and rebuilt_i_<nfft>_10 (float32: the cast the GPU tests apply anyway) -- the gain 0.5 signal is bit for bit half of it
(asserted below), so it is not stored twice.  ls / ln stays <= 8: beyond that the
reference's doubling noise buffer outgrows memory.

Run from the repo root:  python tests/golden/make_golden_eval.py <path to the reference checkout>
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(4000, 1500, 0), (2000, 2000, 5), (1234, 5000, -5), (8192, 1100, 10), (300, 200, 20), (256, 700, 0)]


def main():
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    for name, attrs in (("librosa", ()), ("pypesq", ("pesq",)), ("pystoi", ("stoi",)), ("joblib", ("Parallel", "delayed"))):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[name] = m
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from data_utils.data_loader import AudioParser
    from model_utils.utils import SDR, AudioReBuild

    sr, window_ms, stride_ms = 8000, 32, 16
    rng = np.random.default_rng(2025)
    out = {"cases": np.asarray(CASES, np.int32)}
    for i, (ls, ln, snr) in enumerate(CASES):
        t = np.arange(ls) / sr
        speech = (0.3 * np.sin(2 * np.pi * (200 + 60 * i) * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))
                  + 0.02 * rng.standard_normal(ls)).astype(np.float32)
        noise = (0.1 * rng.standard_normal(ln)).astype(np.float32)
        seed = 100 + i
        parser = AudioParser(sample_rate=sr, window_ms=window_ms, stride_ms=stride_ms, snr=snr, use_complex=True)
        np.random.seed(seed)
        mix = parser.add_noise(speech.astype(np.float64), noise.astype(np.float64))
        nxt = np.random.random()
        # the draws add_noise made, by replaying the seed in its order (data_loader.py:36-45)
        np.random.seed(seed)
        if ls >= ln:
            draws = [np.random.uniform(0, 2) for _ in range(int(np.ceil((ls - ln) / ln)))]
            start, used = 0, int((ls - 1) // ln).bit_length()
        else:
            draws, used = [], 0
            start = int(np.random.randint(0, ln - ls))
        assert np.random.random() == nxt, "the replay left np.random somewhere else than add_noise did"
        out["speech_%d" % i], out["noise_%d" % i] = speech, noise
        out["seed_%d" % i], out["next_%d" % i] = np.asarray(seed, np.int64), np.asarray(nxt, np.float64)
        out["start_%d" % i], out["draws_%d" % i] = np.asarray(start, np.int32), np.asarray(len(draws), np.int32)
        out["gains_%d" % i] = np.asarray(draws[:used], np.float64)
        out["mix_%d" % i] = np.asarray(mix, np.float64)
        spec = parser.parse_audio(mix)                                   # [129, T] complex
        mag, phase = parser.extractor.power_spectrum(spec), parser.extractor.divide_phase(spec)
        for nfft in (512, 256):
            rb = AudioReBuild(nfft=nfft)
            for gain in (1.0, 0.5):
                audio = rb.rebuild_audio([ls], (gain * mag).T[None], phase.T[None], sr, window_ms, stride_ms)[0]
                audio = np.asarray(audio, np.float64)
                tag = "%d_%d_%d" % (i, nfft, int(gain * 10))
                if gain == 1.0:
                    out["rebuilt_" + tag] = audio.astype(np.float32)
                else:       # the rebuild is linear and a factor 0.5 is exact in binary: stored once, halved by the tests
                    assert np.array_equal(audio.astype(np.float32), np.float32(gain) * out["rebuilt_%d_%d_10" % (i, nfft)])
                out["sdr_" + tag] = np.asarray(SDR()(speech.astype(np.float64), audio), np.float64)
                print(tag, "ls %d ln %d snr %d -> SDR %.4f dB" % (ls, ln, snr, out["sdr_" + tag]))
    path = os.path.join(HERE, "eval_ref.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
