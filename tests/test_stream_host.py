"""CPU tests of the streaming denoiser's contract: the float64 restatement (tests/stream_np.py), run hop by hop, IS the
whole-utterance oracle chain delayed by 640 samples -- for every length at which the reference's frame count changes its
rule and for every way of cutting the pushes --, and rced_stream_* is declared, exported, bound and refuses bad arguments
without a device."""

import ctypes
import os
import re

import numpy as np
import pytest

import stream_np
from conftest import ROOT
from oracle import audio_np, rced_c, rced_np

NET = "FullyCNNV3"
LENGTHS = [100, 128, 129, 200, 255, 256, 300, 384, 1280, 1357, 3000]
HOPS = {"all-1": [1], "all-3": [3], "all-8": [8], "mixed": [1, 8, 2, 5, 3, 7]}
ENTRIES = {"rced_stream_delay": 0, "rced_stream_create": 5, "rced_stream_destroy": 1, "rced_stream_push": 6, "rced_stream_finish": 6,
           "rced_stream_reset": 2}


def signal(length, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    return ((0.3 + 0.2 * np.sin(2 * np.pi * t / 700.0)) * rng.standard_normal(length)).astype(np.float32)


@pytest.fixture(scope="module")
def weights():
    return rced_np.make_weights(NET, seed=42)


@pytest.fixture(scope="module")
def offline(weights):
    """audio_np.rebuild(rced_c.forward(audio_np.stft(s))) per length, computed once."""
    ref = {}
    for n in LENGTHS:
        sig = signal(n, n)
        mag, phase = audio_np.stft(sig)
        masks = rced_c.forward(NET, weights, mag[None, :, :, None].astype(np.float32), np.float64)[0, :, :, 0]
        ref[n] = (sig, audio_np.rebuild(masks, phase, n, 512))
    return ref


@pytest.mark.parametrize("hops", sorted(HOPS))
@pytest.mark.parametrize("length", LENGTHS)
def test_restatement_is_the_offline_chain_delayed_by_640(weights, offline, length, hops):
    sig, ref = offline[length]
    stream = stream_np.StreamNP(NET, weights, lanes=2, max_hops=8)
    out, pushed = stream_np.run_signal(stream, 1, sig, HOPS[hops])
    zeros = min(stream_np.DELAY, stream_np.STEP * pushed)      # pushes return zeros until 640 samples have left
    assert pushed == length // 128 and len(out) == zeros + length
    assert not out[:zeros].any()
    err = np.abs(out[zeros:] - ref).max() / np.abs(ref).max()
    assert err <= 1e-12, (length, hops, err)
    # finish hands out exactly what is owed and leaves the lane as new
    assert stream.lane[1].hops == 0 and not stream.lane[1].pend.any()


def test_restatement_lanes_are_independent_and_idle_lanes_keep_their_state(weights, offline):
    sig, ref = offline[1357]
    other = signal(1357, 7)
    stream = stream_np.StreamNP(NET, weights, lanes=3, max_hops=8)
    got = [[], [], []]
    for at in range(0, 1280, 256):
        pcm = np.stack([sig[at:at + 256], other[at:at + 256], sig[at:at + 256]])
        out = stream.push(pcm)
        assert np.array_equal(out[0], out[2])
        for s in range(3):
            got[s].append(out[s])
        idle = stream.push(np.ones((3, 128), np.float32), active=[0, 0, 0])      # nobody listens: nothing moves
        assert not idle.any()
    rest = stream.finish([0, 2], [sig[1280:], sig[1280:]])
    for s, r in zip((0, 2), rest):
        out = np.concatenate(got[s] + [r])[640:]
        assert np.abs(out - ref).max() <= 1e-12 * np.abs(ref).max()
    assert stream.lane[1].hops == 10                              # the lane that did not finish goes on


def test_lanes_that_finish_at_different_pushes_and_are_reused(weights):
    """The driver the GPU tests share (stream_np.run_lanes), on the restatement: four lanes, signals of different lengths one
    after the other, every one equal to its own whole-utterance chain."""
    jobs = [[1357], [300, 100], [100, 200, 384], [129]]
    sigs = [[signal(n, 10 * lane + i) for i, n in enumerate(lens)] for lane, lens in enumerate(jobs)]
    done = stream_np.run_lanes(stream_np.StreamNP(NET, weights, lanes=4, max_hops=8), sigs, HOPS["mixed"])
    for lane, lens in enumerate(jobs):
        assert len(done[lane]) == len(lens)
        for sig, (out, pushed) in zip(sigs[lane], done[lane]):
            mag, phase = audio_np.stft(sig)
            masks = rced_c.forward(NET, weights, mag[None, :, :, None].astype(np.float32), np.float64)[0, :, :, 0]
            ref = audio_np.rebuild(masks, phase, len(sig), 512)
            zeros = min(stream_np.DELAY, stream_np.STEP * pushed)
            assert len(out) == zeros + len(sig) and not out[:zeros].any()
            assert np.abs(out[zeros:] - ref).max() <= 1e-12 * np.abs(ref).max()


def test_pushing_zeros_is_not_finishing(weights, offline):
    sig, ref = offline[300]
    stream = stream_np.StreamNP(NET, weights, lanes=1, max_hops=8)
    padded = np.concatenate([sig, np.zeros(1024 - 300, np.float32)])
    out = np.concatenate([stream.push(padded[None, at:at + 512])[0] for at in (0, 512)])[640:940]
    assert len(out) == 300 and np.abs(out - ref).max() > 1e-6 * np.abs(ref).max()


def test_entries_are_declared_exported_and_bound(built):
    from fullycnnspeechenhancement_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rced.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name, nargs in ENTRIES.items():
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
    assert re.search(r"#define\s+RCED_STREAM_DELAY\s+640\b", src)
    assert _lib.load().rced_stream_delay() == 640 == stream_np.DELAY


def test_bad_arguments_are_refused_before_any_device_is_touched(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    ARG = _lib.RCED_ERR_ARG
    p = ctypes.c_void_p(4096)     # never dereferenced: every case fails on an argument checked before the model is looked at
    h = ctypes.c_void_p()
    for lanes, max_hops, nfft in ((0, 8, 512), (-3, 8, 512), (4, 0, 512), (4, 65, 512), (4, 8, 128), (4, 8, 1024), (4, 8, 0)):
        assert lib.rced_stream_create(p, lanes, max_hops, nfft, ctypes.byref(h)) == ARG, (lanes, max_hops, nfft)
        assert h.value is None
    assert b"nfft" in lib.rced_last_error()
    assert lib.rced_stream_create(None, 4, 8, 512, ctypes.byref(h)) == ARG      # no model
    assert lib.rced_stream_create(p, 4, 8, 512, None) == ARG
    assert lib.rced_stream_push(None, p, None, 1, p, None) == ARG
    assert lib.rced_stream_finish(None, p, p, p, p, None) == ARG
    assert lib.rced_stream_reset(None, -1) == ARG
    lib.rced_stream_destroy(None)                                               # a no-op, like free(NULL)


def test_python_surface():
    import inspect
    import fullycnnspeechenhancement_amd as pkg
    assert pkg.StreamingDenoiser is pkg.audio.StreamingDenoiser and "StreamingDenoiser" in pkg.__all__
    sig = inspect.signature(pkg.StreamingDenoiser.__init__).parameters
    assert sig["max_hops"].default == 8 and sig["nfft"].default == 512
    assert inspect.signature(pkg.InferenceEngine.denoise_stream).parameters["hops"].default == 8
    assert inspect.isgeneratorfunction(pkg.InferenceEngine.denoise_stream)
    assert pkg.audio.STREAM_DELAY == 640
    for name in ("push", "finish", "reset"):
        assert callable(getattr(pkg.StreamingDenoiser, name))
    with pytest.raises(ValueError):
        pkg.StreamingDenoiser(object(), 4)                                      # neither a model nor an engine
