"""CPU tests of the overlap-add stream's contract: the float64 restatement (tests/stream_ola_np.py), run hop by hop, IS
ola_np.ola over the whole utterance's masks delayed by 640 samples -- the delay of the reference-rebuild stream, not a hop
more -- for every length at which the frame count changes its rule or the last hop changes its frame set, and for every way
of cutting the pushes; the `rebuild` keyword is checked before any device work."""

import ctypes
import inspect

import numpy as np
import pytest

import ola_np
import stream_np
import stream_ola_np
from oracle import audio_np, rced_c, rced_np

NET = "FullyCNNV3"
LENGTHS = [1, 100, 127, 128, 129, 200, 255, 256, 257, 300, 383, 384, 385, 512, 640, 641, 767, 768, 769, 1280, 1357, 3000]
HOPS = {"all-1": [1], "all-3": [3], "all-8": [8], "mixed": [1, 8, 2, 5, 3, 7]}


def signal(length, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    return ((0.3 + 0.2 * np.sin(2 * np.pi * t / 700.0)) * rng.standard_normal(length)).astype(np.float32)


@pytest.fixture(scope="module")
def weights():
    return rced_np.make_weights(NET, seed=42)


@pytest.fixture(scope="module")
def offline(weights):
    """ola_np.ola(rced_c.forward(audio_np.stft(s)), frames=T, length=L) per length, computed once."""
    ref = {}
    for n in LENGTHS:
        sig = signal(n, n)
        mag, phase = audio_np.stft(sig)
        assert mag.shape[0] == stream_ola_np.num_frames(n)
        masks = rced_c.forward(NET, weights, mag[None, :, :, None].astype(np.float32), np.float64)[0, :, :, 0]
        ref[n] = (sig, ola_np.ola(masks, phase, frames=mag.shape[0], length=n))
    return ref


@pytest.mark.parametrize("hops", sorted(HOPS))
@pytest.mark.parametrize("length", LENGTHS)
def test_restatement_is_the_offline_overlap_add_delayed_by_640(weights, offline, length, hops):
    sig, ref = offline[length]
    stream = stream_ola_np.StreamOlaNP(NET, weights, lanes=2, max_hops=8)
    out, pushed = stream_np.run_signal(stream, 1, sig, HOPS[hops])
    zeros = min(stream_np.DELAY, stream_np.STEP * pushed)      # pushes return zeros until 640 samples have left
    assert pushed == length // 128 and len(out) == zeros + length
    assert not out[:zeros].any()
    err = np.abs(out[zeros:] - ref).max() / np.abs(ref).max()
    assert err <= 1e-12, (length, hops, err)
    # finish leaves the lane as new
    st = stream.lane[1]
    assert st.hops == 0 and not st.pend.any() and st.carry == 0.0


def test_restatement_lanes_finish_at_different_pushes_and_are_reused(weights):
    jobs = [[1357], [300, 100], [100, 200, 384], [129, 256]]
    sigs = [[signal(n, 10 * lane + i) for i, n in enumerate(lens)] for lane, lens in enumerate(jobs)]
    done = stream_np.run_lanes(stream_ola_np.StreamOlaNP(NET, weights, lanes=4, max_hops=8), sigs, HOPS["mixed"])
    for lane, lens in enumerate(jobs):
        assert len(done[lane]) == len(lens)
        for sig, (out, pushed) in zip(sigs[lane], done[lane]):
            mag, phase = audio_np.stft(sig)
            masks = rced_c.forward(NET, weights, mag[None, :, :, None].astype(np.float32), np.float64)[0, :, :, 0]
            ref = ola_np.ola(masks, phase, frames=mag.shape[0], length=len(sig))
            zeros = min(stream_np.DELAY, stream_np.STEP * pushed)
            assert len(out) == zeros + len(sig) and not out[:zeros].any()
            assert np.abs(out[zeros:] - ref).max() <= 1e-12 * np.abs(ref).max()


def test_rebuild_keyword_is_checked_before_any_device_work(built):
    """None of these reaches a device: the machine may have none."""
    from fullycnnspeechenhancement_amd import InferenceEngine, StreamingDenoiser
    assert inspect.signature(StreamingDenoiser.__init__).parameters["rebuild"].default == "reference"
    assert inspect.signature(InferenceEngine.denoise_stream).parameters["rebuild"].default == "reference"
    for bad in ("x", "OLA", None, 1):
        with pytest.raises(ValueError, match="rebuild"):
            StreamingDenoiser(object(), 4, rebuild=bad)
        with pytest.raises(ValueError, match="rebuild"):
            next(InferenceEngine.denoise_stream(object.__new__(InferenceEngine), [np.zeros(300)], rebuild=bad))


def test_the_delay_does_not_depend_on_the_rebuild():
    from fullycnnspeechenhancement_amd import audio
    assert "rebuild" not in inspect.signature(audio.stream_delay).parameters
    assert audio.stream_delay() == audio.STREAM_DELAY == stream_np.DELAY == 640
    assert audio.stream_delay(48000, 48000) == 4992 and audio.stream_delay(16000) == 768


def test_create_ex_is_bound_and_refuses_bad_arguments_without_a_device(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    assert len(_lib.SYMBOLS["rced_stream_create_ex"][1]) == 6
    p = ctypes.c_void_p(4096)     # never dereferenced: every case fails on an argument checked before the model is looked at
    h = ctypes.c_void_p()
    for rebuild in (2, -1, 256):
        assert lib.rced_stream_create_ex(p, 4, 8, 512, rebuild, ctypes.byref(h)) == _lib.RCED_ERR_ARG, rebuild
        assert h.value is None and b"rebuild" in lib.rced_last_error()
    for rebuild in (0, 1):
        assert lib.rced_stream_create_ex(p, 4, 8, 128, rebuild, ctypes.byref(h)) == _lib.RCED_ERR_ARG      # nfft, as without _ex
        assert lib.rced_stream_create_ex(None, 4, 8, 512, rebuild, ctypes.byref(h)) == _lib.RCED_ERR_ARG   # no model
