"""CPU tests of the resampler lanes: the float64 restatement with a lane's state (tests/rstream_np.py) equals
the offline restatement (tests/resample_np.py, itself pinned to scipy) delayed by D; D, by brute force over the phase table, is
what the library plans and is minimal; the refusals that need no device; the total delay of StreamingDenoiser at a rate; and
tests/rstream_plan_check.cpp, the plan arithmetic of csrc/rstream_plan.h as a program of its own under AddressSanitizer and
UBSan.  Nothing here needs a GPU."""

import ctypes

import numpy as np
import pytest

import host_cxx
import resample_np as R
import rstream_np as S

# (sr_in, sr_out, unit_in, unit_out): unit 128 on the 8 kHz side; 44.1 kHz with the smallest units, all 80 phases
CONVERSIONS = [(16000, 8000, 256, 128), (48000, 8000, 768, 128), (12000, 8000, 192, 128), (8000, 16000, 128, 256),
               (8000, 48000, 128, 768), (8000, 12000, 128, 192), (44100, 8000, 441, 80)]
PUSHES = {"all-1": [1], "all-3": [3], "mixed": [2, 1, 4, 3]}


def lengths(unit_in):
    return [1, unit_in - 1, unit_in, unit_in + 1, 5 * unit_in + 7, 3000]


@pytest.mark.parametrize("sr_in,sr_out,unit_in,unit_out", CONVERSIONS)
def test_restatement_equals_the_offline_result_delayed(sr_in, sr_out, unit_in, unit_out):
    rng = np.random.RandomState(sr_in // 100 + sr_out // 100)
    for name, counts in sorted(PUSHES.items()):
        # three lanes take the six lengths two each, one after the other: they finish at different pushes and are reused
        sigs = [rng.uniform(-1, 1, n) for n in lengths(unit_in)]
        jobs = [[sigs[5], sigs[0]], [sigs[4], sigs[1]], [sigs[2], sigs[3]]]
        lanes = S.LanesNP(sr_in, sr_out, 3, unit_in, unit_out)
        done = S.run_lanes(lanes, jobs, counts)
        worst = 0.0
        for lane in range(3):
            assert len(done[lane]) == 2
            for x, (out, units) in zip(jobs[lane], done[lane]):
                assert units == len(x) // unit_in
                want = S.delayed(R.resample(x, sr_in, sr_out), lanes.delay, units, unit_out)
                assert out.shape == want.shape, (len(x), out.shape, want.shape)
                if want.size:
                    worst = max(worst, np.abs(out - want).max() / np.abs(x).max())
                zeros = min(lanes.delay, units * unit_out)
                assert not out[:zeros].any()
        print("%d -> %d, pushes %s: D %d, history %d frames, worst %.2e of max |x|" % (sr_in, sr_out, name, lanes.delay, lanes.hist_len, worst))
        assert worst <= 1e-12


@pytest.mark.parametrize("sr_in,sr_out,unit_in,unit_out", CONVERSIONS)
def test_delay_is_the_brute_force_minimum(sr_in, sr_out, unit_in, unit_out, built):
    from fullycnnspeechenhancement_amd import audio
    p, q, left, table = audio.resample_taps(sr_in, sr_out)
    width = table.shape[1]
    D = S.brute_delay(p, q, left, width, unit_in, unit_out)
    print("%d -> %d: p %d q %d left %d width %d, D %d" % (sr_in, sr_out, p, q, left, width, D))
    assert audio.resampler_delay(sr_in, sr_out) == D == (width - 1 - left) * p // q
    assert -((-(D + 1) * q) // p) >= width - left                       # ceil((D + 1) q / p) >= right + 1 ...
    assert D == 0 or -((-D * q) // p) < width - left                     # ... and D - 1 misses it
    # the restatement run at D - 1 reads a frame that has not been pushed
    if D > 0:
        lanes = S.LanesNP(sr_in, sr_out, 1, unit_in, unit_out, delay=D - 1)
        with pytest.raises(AssertionError, match="not pushed yet"):
            for _ in range(4 + 2 * D // unit_out):
                lanes.push(np.ones((1, unit_in)))


def test_the_delays_of_the_usual_rates(built):
    from fullycnnspeechenhancement_amd import audio
    got = {(a, b): audio.resampler_delay(a, b) for a, b, _, _ in CONVERSIONS}
    print(got)
    assert got[16000, 8000] == 63 and got[48000, 8000] == 63 and got[8000, 16000] == 128 and got[8000, 48000] == 384
    assert audio.resampler_delay(8000, 8000) == 0


def test_streaming_denoiser_total_delay_formula(built):
    """(128 + 640) samples at 8 kHz behind down lanes -- their 63 rounded up to the hop the denoiser takes --, carried to the output
    rate, plus the up lanes' own delay; 640 and nothing else with the defaults."""
    from fullycnnspeechenhancement_amd import audio
    assert audio.stream_delay() == audio.stream_delay(8000) == audio.STREAM_DELAY == 640
    assert audio.stream_delay(16000) == audio.stream_delay(8000, channels=2) == audio.stream_delay(8000, dtype="int16") == 768
    for rate in (16000, 48000, 12000):
        up = audio.resampler_delay(8000, rate)
        assert audio.stream_delay(rate, rate) == 768 * rate // 8000 + up
        assert audio.stream_delay(8000, rate) == 640 * rate // 8000 + up
        assert audio.resampler_delay(rate, 8000) <= 128              # the hop covers what the down lanes need
    assert audio.stream_delay(48000, 48000) == 768 * 6 + 384 == 4992 and audio.stream_delay(16000, 16000) == 768 * 2 + 128


def create(lib, *args):
    h = ctypes.c_void_p()
    rc = lib.rced_rstream_create(*args, ctypes.byref(h))
    return rc, lib.rced_last_error().decode(), h


def test_library_refusals_come_before_a_device_is_looked_for(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    F, I = _lib.PCM_F32, _lib.PCM_S16
    rc, msg, h = create(lib, 16000, 8000, 1, F, F, 256, 127, 4, 8, 0)                # units not in the ratio
    assert rc == _lib.RCED_ERR_ARG and not h and "256" in msg and "127" in msg and "1 / 2" in msg
    rc, msg, h = create(lib, 44100, 8000, 1, F, F, 705, 128, 4, 8, 0)                # 128 * 441 / 80 = 705.6
    assert rc == _lib.RCED_ERR_ARG and "80 / 441" in msg
    rc, msg, h = create(lib, 8001, 8000, 1, F, F, 8001, 8000, 4, 1, 0)               # what rced_resample_taps refuses
    assert rc == _lib.RCED_ERR_ARG and "8001" in msg and "1 MiB" in msg
    for bad in [(0, 8000, 1, F, F, 1, 1, 4, 8, 0), (16000, 8000, 0, F, F, 256, 128, 4, 8, 0), (16000, 8000, 1, 7, F, 256, 128, 4, 8, 0),
                (16000, 8000, 1, I, 7, 256, 128, 4, 8, 0), (16000, 8000, 1, F, F, 256, 128, 0, 8, 0), (16000, 8000, 1, F, F, 256, 128, 4, 0, 0),
                (16000, 8000, 1, F, F, 256, 128, 70000, 8, 0), (16000, 8000, 1, F, F, 2 ** 22, 2 ** 21, 4, 8, 0)]:
        rc, msg, h = create(lib, *bad)
        assert rc == _lib.RCED_ERR_ARG and msg and not h, bad
    h = ctypes.c_void_p()
    rc = lib.rced_rstream_create_ex(48000, 8000, 1, F, F, 768, 128, 4, 8, 62, 0, ctypes.byref(h))      # D is 63
    assert rc == _lib.RCED_ERR_ARG and not h and "less than" in lib.rced_last_error().decode()
    assert lib.rced_rstream_delay(None) == -1
    assert lib.rced_rstream_started(None, None, None, None) == _lib.RCED_ERR_ARG
    assert lib.rced_rstream_push(None, None, None, 1, None, None) == _lib.RCED_ERR_ARG
    assert lib.rced_rstream_finish(None, None, None, None, None, None) == _lib.RCED_ERR_ARG
    assert lib.rced_rstream_reset(None, 0) == _lib.RCED_ERR_ARG
    lib.rced_rstream_destroy(None)


def test_python_refusals(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser, StreamingResampler
    with pytest.raises(ValueError, match="do not stand in the ratio"):
        StreamingResampler(16000, 8000, 2, unit_out=128, unit_in=255)
    with pytest.raises(ValueError, match="44100"):
        StreamingResampler(44100, 8000, 2, unit_out=128)                              # 705.6 frames
    with pytest.raises(ValueError, match="whole number"):
        StreamingResampler(8000, 44100, 2, unit_in=128)
    with pytest.raises(ValueError, match="int16"):
        StreamingResampler(16000, 8000, 2, unit_out=128, dtype="int8")
    # the denoiser refuses a rate whose hop is not a whole number of frames before it touches the device
    model = type("Model", (), {"_handle": 1, "device": 0})()
    for kw in ({"sample_rate": 44100}, {"sample_rate": 16000, "output_rate": 44100}):
        with pytest.raises(ValueError, match="44100"):
            StreamingDenoiser(model, 2, **kw)


def test_plan_arithmetic_as_a_stand_alone_program(tmp_path, built):
    exe = host_cxx.build(tmp_path, "rstream_plan_check")
    # its own sweep, then the geometry the library reports for the conversions of this file
    from fullycnnspeechenhancement_amd import audio
    args = []
    for sr_in, sr_out, unit_in, unit_out in CONVERSIONS:
        p, q, left, table = audio.resample_taps(sr_in, sr_out)
        args += [sr_in, sr_out, p, q, left, table.shape[1], unit_in, unit_out]
    assert "%d plans, 0 failures" % (17 + len(CONVERSIONS)) in host_cxx.run(exe, args, tail=6000)
