"""CPU tests of the denoiser lanes at a framing: the float64 restatement of a lane (tests/stream_fr_np.py)
against the whole-utterance chain of tests/framing_np.py at every framing, length and push size; against the restatements of
the default lanes (tests/stream_np.py, tests/stream_ola_np.py) at 256 / 128 / hamming; the delay against a search over the frame
dependencies; every refusal that needs no device, with its message; and tests/stream_fr_plan_check.cpp, the arithmetic of
csrc/stream_fr_plan.h as a program of its own under AddressSanitizer and UBSan.  Nothing here needs a GPU."""

import ctypes
import os

import numpy as np
import pytest

import framing_np as fnp
import stream_fr_np as sfr
import stream_np
import stream_ola_np
import host_cxx
from conftest import ROOT
from oracle import rced_np

NET = "FullyCNNV3"
FRAMINGS = fnp.FRAMINGS + [(256, 128, "hamming")]
IDS = ["%d-%d-%s" % f for f in FRAMINGS]
HOPS = {"all-1": [1], "all-3": [3], "all-8": [8], "mixed": [1, 8, 2, 5, 3, 7]}
EXACT = 1e-12         # of the largest sample: two float64 computations of the same sums
_cache = {}


def weights():
    if "w" not in _cache:
        _cache["w"] = rced_np.make_weights(NET, seed=42)
    return _cache["w"]


def signal(length, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    return ((0.3 + 0.2 * np.sin(2 * np.pi * t / 700.0)) * rng.standard_normal(length)).astype(np.float32)


def check_restatement(W, S, name, rebuild, nfft=512):
    """Every length through lanes that are reused, at every push size: the lane's output is the offline chain delayed by D."""
    sigs = [signal(L, 7 * L + W) for L in sfr.lengths(W, S)]
    jobs = [sigs[0::3], sigs[1::3], sigs[2::3]]
    want = {len(s): sfr.offline(NET, weights(), s, W, S, name, rebuild, nfft) for s in sigs}
    worst = 0.0
    for hops in sorted(HOPS):
        lanes = sfr.StreamFrNP(NET, weights(), 3, W, S, name, rebuild, nfft)
        done = sfr.run_lanes(lanes, jobs, HOPS[hops])
        for lane in range(3):
            assert len(done[lane]) == len(jobs[lane])
            for sig, (out, pushed) in zip(jobs[lane], done[lane]):
                out = sfr.drop_delay(out, pushed, len(sig), W, S)
                ref = want[len(sig)]
                assert ref.shape == out.shape == (len(sig),)
                err = np.abs(out - ref).max() / max(np.abs(ref).max(), 1e-300)
                worst = max(worst, err)
                assert err <= EXACT, (W, S, name, rebuild, hops, len(sig), err)
    print("%d / %d / %s %s: worst %.2e of the largest sample over %d lengths" % (W, S, name, rebuild, worst, len(sigs)))


@pytest.mark.parametrize("framing", FRAMINGS, ids=IDS)
def test_restatement_equals_the_offline_overlap_add_chain(framing):
    check_restatement(*framing, rebuild="ola")


@pytest.mark.parametrize("nfft", [512, 256])
@pytest.mark.parametrize("framing", fnp.HAMMING_FRAMINGS, ids=["%d-%d-%s" % f for f in fnp.HAMMING_FRAMINGS])
def test_restatement_equals_the_offline_reference_chain(framing, nfft):
    check_restatement(*framing, rebuild="reference", nfft=nfft)


@pytest.mark.parametrize("rebuild", ["reference", "ola"])
def test_at_the_default_framing_it_is_the_default_lanes_restatement(rebuild):
    """Delay 640, the same owed counts, the same samples as stream_np / stream_ola_np push by push."""
    assert sfr.delay(256, 128) == stream_np.DELAY == 640 and sfr.finish_slots(256, 128) == stream_np.FINISH_SLOTS
    sigs = [signal(n, n) for n in (1357, 300, 100, 767, 768)]
    old = (stream_np.StreamNP if rebuild == "reference" else stream_ola_np.StreamOlaNP)(NET, weights(), 1, max_hops=8)
    new = sfr.StreamFrNP(NET, weights(), 1, 256, 128, "hamming", rebuild, 512)
    for sig in sigs:
        a, hops_a = stream_np.run_signal(old, 0, sig, HOPS["mixed"])
        (b, hops_b), = sfr.run_lanes(new, [[sig]], HOPS["mixed"])[0]
        assert hops_a == hops_b and a.shape == b.shape
        assert len(b) - min(640, 128 * hops_b) == len(sig) == sfr.owed(hops_b, len(sig) % 128, 256, 128) + max(0, 128 * hops_b - 640)
        assert np.abs(a - b).max() <= EXACT * np.abs(a).max()


def test_delay_is_the_brute_force_delay(built):
    from fullycnnspeechenhancement_amd import _lib, audio
    lib = _lib.load()
    cases = [(W, S) for W, S, _ in FRAMINGS] + [(2, 1), (2, 2), (3, 2), (256, 32), (256, 33), (100, 99), (100, 13), (17, 5)]
    for W, S in cases:
        want = sfr.brute_delay(W, S)
        assert want == sfr.delay(W, S) == (-(-W // S) + 3) * S
        assert lib.rced_stream_delay_fr(W, S) == want == audio.stream_delay_fr(audio.Framing(W, S)), (W, S)
        assert lib.rced_stream_finish_max_fr(W, S) >= want + S - 1
    assert audio.stream_delay_fr() == audio.stream_delay_fr(audio.Framing()) == audio.STREAM_DELAY == 640
    assert audio.stream_delay_fr(audio.Framing(160, 80)) == 400
    assert lib.rced_stream_delay_fr(256, 16) == -1 and lib.rced_stream_delay_fr(257, 128) == -1 and lib.rced_stream_delay_fr(100, 101) == -1
    assert lib.rced_stream_finish_max_fr(256, 16) == -1


def test_complete_frames_and_frames_to_come():
    """After H hops max(0, H - R + 1) frames are complete; a finish finds at most 2 frames still to come for L >= W and at most
    R + 1 for L < W, and (T - 1) S + W >= L."""
    rng = np.random.default_rng(5)
    for _ in range(20000):
        W = int(rng.integers(2, 257))
        S = int(rng.integers(1, W + 1))
        L = int(rng.integers(1, 6 * W))
        R, H = sfr.overlap(W, S), L // S
        complete = sum(1 for t in range(H + 1) if t * S + W <= H * S)
        assert complete == max(0, H - R + 1)
        T = sfr.num_frames(L, W, S)
        assert 0 <= T - complete <= (2 if L >= W else R + 1) and (T - 1) * S + W >= L
        assert sfr.owed(H, L - H * S, W, S) <= sfr.delay(W, S) + S - 1


def refusal(lib, *args):
    rc = lib.rced_stream_fr_check(*args)
    return rc, lib.rced_last_error().decode()


def test_library_refusals_touch_no_device(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    ARG, OLA, REF = _lib.RCED_ERR_ARG, 1, 0
    assert lib.rced_stream_fr_check(160, 80, 0, REF) == lib.rced_stream_fr_check(256, 64, 1, OLA) == lib.rced_stream_fr_check(256, 32, 0, OLA) == 0
    for args, words in [((257, 128, 0, OLA), "window must lie in [2, 256]"), ((1, 1, 0, OLA), "window must lie in [2, 256]"),
                        ((100, 101, 0, OLA), "stride must lie in [1, window = 100]"), ((100, 0, 0, OLA), "stride must lie in"),
                        ((160, 80, 4, OLA), "window name"), ((160, 80, 0, 2), "rebuild must be"),
                        ((256, 16, 0, OLA), "overlap of 16 frames"), ((256, 31, 1, OLA), "overlap of 9 frames"),
                        ((160, 80, 1, REF), "hanning window are zero"), ((160, 80, 2, REF), "blackman window are zero"),
                        ((160, 80, 3, REF), "bartlett window are zero")]:
        rc, msg = refusal(lib, *args)
        assert rc == ARG and words in msg, (args, msg)
    # the same words as the offline checks
    for name in (1, 2, 3):
        assert lib.rced_istft_fr_check(160, 80, name) == ARG
        offline = lib.rced_last_error().decode()
        assert refusal(lib, 160, 80, name, REF)[1] == offline
    assert lib.rced_framing_check(300, 80, 0) == ARG
    offline = lib.rced_last_error().decode()
    assert refusal(lib, 300, 80, 0, OLA)[1] == offline
    # create refuses before it looks at the model or the device
    h = ctypes.c_void_p()
    for args in [(4, 8, 512, 2, 160, 80, 0), (4, 8, 512, OLA, 256, 16, 0), (4, 8, 512, REF, 160, 80, 1), (4, 8, 512, OLA, 300, 80, 0)]:
        assert lib.rced_stream_create_fr(None, *args, ctypes.byref(h)) == ARG and not h
    assert lib.rced_stream_create_fr(None, 4, 8, 512, OLA, 160, 80, 0, None) == ARG


def test_python_refusals_come_before_any_device_work(built):
    from fullycnnspeechenhancement_amd import BlockDenoiser, InferenceEngine, StreamingDenoiser, audio
    model = type("Model", (), {"_handle": 1, "device": 0})()
    fr = audio.Framing(160, 80)
    with pytest.raises(ValueError, match=r"window must lie in \[2, 256\]"):
        audio.Framing(300, 80)
    with pytest.raises(ValueError, match="stride must lie in"):
        audio.Framing(100, 101)
    with pytest.raises(ValueError, match="overlap of 16 frames"):
        StreamingDenoiser(model, 2, rebuild="ola", framing=audio.Framing(256, 16))
    with pytest.raises(ValueError, match="overlap of 16 frames"):
        audio.stream_delay_fr(audio.Framing(256, 16))
    for name in ("hanning", "blackman", "bartlett"):
        with pytest.raises(ValueError, match="%s window are zero" % name):
            StreamingDenoiser(model, 2, rebuild="reference", framing=audio.Framing(160, 80, name))
    for kwargs, word in [({"sample_rate": 16000}, "sample_rate=16000"), ({"channels": 2}, "channels=2"), ({"dtype": "int16"}, "dtype='int16'"),
                         ({"output_rate": 16000}, "output_rate=16000")]:
        with pytest.raises(ValueError, match="framing=.*together with %s" % word):
            StreamingDenoiser(model, 2, rebuild="ola", framing=fr, **kwargs)
    with pytest.raises(ValueError, match="framing=.*together with block=441"):
        BlockDenoiser(model, 2, 441, sample_rate=44100, output_rate=44100, framing=fr)
    with pytest.raises(ValueError, match="framing must be an audio.Framing"):
        StreamingDenoiser(model, 2, framing=(160, 80))
    eng = object.__new__(InferenceEngine)
    eng.model = model
    with pytest.raises(ValueError, match="together with block=100"):
        next(eng.denoise_stream([np.zeros(300)], block=100, framing=fr))
    with pytest.raises(ValueError, match="together with sample_rate=16000"):
        next(eng.denoise_stream([np.zeros(300)], sample_rate=16000, framing=fr))
    with pytest.raises(ValueError, match="overlap of 16 frames"):
        next(eng.denoise_stream([np.zeros(300)], rebuild="ola", framing=audio.Framing(256, 16)))


def test_symbols_are_declared_exported_and_bound(built):
    import inspect
    from fullycnnspeechenhancement_amd import InferenceEngine, StreamingDenoiser, _lib
    header = open(os.path.join(ROOT, "include", "rced.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name, nargs in (("rced_stream_fr_check", 4), ("rced_stream_delay_fr", 2), ("rced_stream_finish_max_fr", 2), ("rced_stream_create_fr", 9)):
        assert name + "(" in header and hasattr(lib, name), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
    assert inspect.signature(InferenceEngine.denoise_stream).parameters["framing"].default is None
    assert inspect.signature(StreamingDenoiser.__init__).parameters["framing"].default is None


def test_plan_arithmetic_as_a_stand_alone_program(tmp_path, built):
    exe = host_cxx.build(tmp_path, "stream_fr_plan_check")
    # its own sweep, then what the library reports for this file's framings: (W, S, delay, finish_max) each
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    args = []
    for W, S, _ in FRAMINGS:
        args += [W, S, lib.rced_stream_delay_fr(W, S), lib.rced_stream_finish_max_fr(W, S)]
    assert "%d framings of the library, 0 failures" % len(FRAMINGS) in host_cxx.run(exe, args)
