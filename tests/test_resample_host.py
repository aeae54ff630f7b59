"""CPU tests of the sample-rate conversion: the float64 restatement (tests/resample_np.py) against scipy, the
library's phase table and output length against the restatement, tones through the restatement, and the loader's wav / manifest
reading with resample=True.  Nothing here needs a GPU."""

import ctypes
import json
import os
import wave

import numpy as np
import pytest

import resample_np as R

RATIOS = [(16000, 8000), (48000, 8000), (44100, 8000), (32000, 8000), (8000, 16000), (8000, 10000)]


@pytest.mark.parametrize("sr_orig,sr_new", RATIOS)
def test_restatement_equals_scipy(sr_orig, sr_new):
    rng = np.random.RandomState(sr_orig // 100 + sr_new)
    for n in (1, 5, 7, 2999, 4099):
        x = rng.uniform(-1, 1, n)
        y, ref = R.resample(x, sr_orig, sr_new), R.scipy_form(x, sr_orig, sr_new)
        assert y.shape == ref.shape == (R.length(n, sr_orig, sr_new),)
        if y.size:
            err = np.abs(y - ref).max() / np.abs(ref).max()
            print("%d -> %d, n = %d: %.2e of max |y|" % (sr_orig, sr_new, n, err))
            assert err <= 1e-12


@pytest.mark.parametrize("sr_orig,sr_new", RATIOS)
def test_phase_table(sr_orig, sr_new, built):
    from fullycnnspeechenhancement_amd import audio
    p, q, left, table = audio.resample_taps(sr_orig, sr_new)
    rp, rq, rleft, rtable = R.taps(sr_orig, sr_new)
    assert (p, q, left, table.shape) == (rp, rq, rleft, rtable.shape)
    err = np.abs(table - rtable).max()
    sums = table.sum(axis=1)
    print("%d -> %d: p %d q %d left %d width %d, table err %.2e, phase sums 1 %+.1e .. 1 %+.1e"
          % (sr_orig, sr_new, p, q, left, table.shape[1], err, sums.min() - 1, sums.max() - 1))
    assert err <= 1e-13
    assert np.abs(sums - 1).max() <= 1e-7


def test_same_rate_is_the_copy(built):
    from fullycnnspeechenhancement_amd import audio
    p, q, left, table = audio.resample_taps(8000, 8000)
    assert (p, q, left) == (1, 1, 0) and table.tolist() == [[1.0]]


@pytest.mark.parametrize("sr_orig,sr_new", RATIOS)
def test_output_length(sr_orig, sr_new, built):
    from fullycnnspeechenhancement_amd import _lib, audio
    lib = _lib.load()
    for n in range(5001):
        assert lib.rced_resample_length(n, sr_orig, sr_new) == int(n * (float(sr_new) / sr_orig))
    assert audio.resample_length(4099, sr_orig, sr_new) == R.length(4099, sr_orig, sr_new)
    assert lib.rced_resample_length(-1, sr_orig, sr_new) == -1
    assert lib.rced_resample_length(10, 0, sr_new) == -1 and lib.rced_resample_length(10, sr_orig, -8000) == -1
    with pytest.raises(ValueError):
        audio.resample_length(10, 0, 8000)


@pytest.mark.parametrize("sr_orig", [16000, 48000, 44100])
def test_tones_through_the_restatement(sr_orig):
    n = sr_orig // 2
    t = np.arange(n) / float(sr_orig)
    M = R.length(n, sr_orig, 8000)
    mid = slice(M // 4, M - M // 4)
    for f in (200, 1000, 3000, 4400, 5000, 7000):
        y = R.resample(np.sin(2 * np.pi * f * t), sr_orig, 8000)
        want = np.sin(2 * np.pi * f * np.arange(M) / 8000.0) if f < 4000 else np.zeros(M)
        err = np.abs(y - want)[mid].max()
        print("%d Hz from %d Hz: %.2e" % (f, sr_orig, err))
        assert err <= 1e-6


def test_refused_ratio_names_itself(built):
    from fullycnnspeechenhancement_amd import _lib, audio
    with pytest.raises(_lib.RcedError) as ei:
        audio.resample_taps(8001, 8000)
    assert ei.value.code == _lib.RCED_ERR_ARG and "8001" in str(ei.value) and "1 MiB" in str(ei.value)
    lib = _lib.load()
    v = ctypes.c_int()
    assert lib.rced_resample_taps(0, 8000, v, v, v, v, None, 0) == _lib.RCED_ERR_ARG
    small = np.zeros(4)
    assert lib.rced_resample_taps(16000, 8000, v, v, v, v, small.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                  small.size) == _lib.RCED_ERR_ARG


def write_wav(path, sig, rate):
    sig = np.asarray(sig, np.int16)
    w = wave.open(str(path), "wb")
    w.setnchannels(1 if sig.ndim == 1 else sig.shape[1])
    w.setsampwidth(2)
    w.setframerate(rate)
    w.writeframes(sig.astype("<i2").tobytes())
    w.close()
    return str(path)


def test_loader_reads_any_rate(tmp_path, built):
    from fullycnnspeechenhancement_amd import loader
    rng = np.random.RandomState(5)
    mono = rng.randint(-30000, 30000, 16000).astype(np.int16)
    stereo = rng.randint(-30000, 30000, (24001, 2)).astype(np.int16)
    short = rng.randint(-30000, 30000, 4000).astype(np.int16)
    a = write_wav(tmp_path / "a.wav", mono, 16000)
    b = write_wav(tmp_path / "b.wav", stereo, 48000)
    c = write_wav(tmp_path / "c.wav", short, 16000)
    assert loader.wav_info(a) == (16000, 1, 16000) and loader.wav_info(b) == (48000, 2, 24001)
    frames, rate = loader.read_wav_frames(a)
    assert rate == 16000 and frames.dtype == np.int16 and np.array_equal(frames, mono[:, None])
    frames, rate = loader.read_wav_frames(b)
    assert rate == 48000 and np.array_equal(frames, stereo)
    assert loader.wav_length(a, 8000, resample=True) == 8000
    assert loader.wav_length(b, 8000, resample=True) == R.length(24001, 48000, 8000) == 4000

    manifest = tmp_path / "m.json"
    with open(str(manifest), "w") as fh:
        for path, n, rate in ((a, 16000, 16000), (b, 24001, 48000), (c, 4000, 16000)):
            fh.write(json.dumps({"audio_filepath": path, "duration": n / float(rate)}) + "\n")
    index = loader.CorpusIndex.from_manifest(str(manifest), 8000, resample=True)        # c lasts 0.25 s < 0.4 s: filtered
    assert index.paths == [a, b] and index.lengths.tolist() == [8000, 4000] and index.offsets.tolist() == [0, 8000]
    index = loader.CorpusIndex.from_manifest(str(manifest), 8000, min_duration=0.0, resample=True)
    assert index.lengths.tolist() == [8000, 4000, 2000]
    for path in (a, b):          # without the option: as before, and the message names the option
        with pytest.raises(ValueError, match="resample=True"):
            loader.wav_length(path, 8000)
        with pytest.raises(ValueError):
            loader.read_wav(path, 8000)
    with pytest.raises(ValueError):
        loader.CorpusIndex.from_manifest(str(manifest), 8000)

    w = wave.open(str(tmp_path / "d.wav"), "wb")       # 8-bit: not read, with or without the option
    w.setnchannels(1)
    w.setsampwidth(1)
    w.setframerate(16000)
    w.writeframes(bytes(100))
    w.close()
    with pytest.raises(ValueError, match="PCM16"):
        loader.wav_info(str(tmp_path / "d.wav"))
    assert os.path.exists(a)
