"""CPU tests of the free-running resampler lanes and of audio.BlockDenoiser's bookkeeping: the outputs a lane
has emitted after F frames against brute force over the phase table, the history it needs, the float64 restatement of a lane
(tests/rfree_np.py) against the offline restatement (tests/resample_np.py) in ragged pushes and takes, block_delay against the
prefill found by walking the calls, the refusals that need no device, and tests/rfree_plan_check.cpp, the plan arithmetic of
csrc/rfree_plan.h as a program of its own under AddressSanitizer and UBSan.  Nothing here needs a GPU."""

import ctypes
import os

import numpy as np
import pytest

import resample_np as R
import rfree_np as S
import host_cxx
from conftest import ROOT

RATIOS = [(44100, 8000), (8000, 44100), (48000, 8000), (8000, 48000), (16000, 8000), (8000, 16000), (22050, 8000), (8000, 8000)]
# (block, sample_rate, output_rate): DESIGN.md 3.4h's table, and 44.1 kHz in with 8 kHz out
BLOCKS = [(128, 8000, 8000), (100, 8000, 8000), (256, 16000, 16000), (768, 48000, 48000), (480, 48000, 48000), (441, 44100, 44100),
          (512, 44100, 44100), (1024, 44100, 44100), (441, 44100, 8000)]


def test_the_new_classes_import(built):
    from fullycnnspeechenhancement_amd import BlockDenoiser, FreeResampler, audio
    assert audio.BlockDenoiser is BlockDenoiser and audio.FreeResampler is FreeResampler
    assert callable(audio.block_delay) and callable(audio.free_available)


@pytest.mark.parametrize("sr_in,sr_out", RATIOS)
def test_emitted_is_the_brute_force_count_and_the_history_is_width_less_one(sr_in, sr_out, built):
    from fullycnnspeechenhancement_amd import _lib, audio
    p, q, left, width = S.geometry(sr_in, sr_out)
    lp, lq, lleft, ltable = audio.resample_taps(sr_in, sr_out)
    assert (lp, lq, lleft, ltable.shape[1]) == (p, q, left, width)
    right = width - 1 - left
    lib = _lib.load()
    m = 0
    for F in range(right + 901):
        while (m * q) // p + right <= F - 1:          # S.brute_emitted, carried from F - 1
            m += 1
        assert S.emitted(p, q, left, width, F) == m == audio.free_available(sr_in, sr_out, F) == lib.rced_rfree_available(sr_in, sr_out, F), F
    for F in (0, 1, right, right + 1, right + 900):
        assert S.brute_emitted(p, q, left, width, F) == S.emitted(p, q, left, width, F)
    assert S.brute_history(p, q, left, width, right + 900) == width - 1
    hist = ctypes.c_int()
    assert lib.rced_rfree_plan(sr_in, sr_out, _lib.PCM_F32, 2, 100, 100, 0, ctypes.byref(hist), None, None, None) == 0
    assert hist.value == width - 1
    print("%d -> %d: p %d q %d left %d width %d, A(right + 900) = %d" % (sr_in, sr_out, p, q, left, width, m))


def test_the_widths_of_the_usual_rates():
    assert [S.geometry(*r)[3] for r in ((44100, 8000), (48000, 8000), (8000, 44100), (8000, 8000))] == [706, 767, 128, 1]


@pytest.mark.parametrize("sr_in,sr_out", RATIOS)
def test_restatement_equals_the_offline_result(sr_in, sr_out):
    """Three lanes, two signals each, pushes of 0, 1, 7, 441, 480 and 1023 frames and idle calls, random takes."""
    rng = np.random.RandomState(sr_in // 100 + sr_out // 50)
    lens = [[2900, 1], [2000 + 7, 1023], [480, 3100]]
    jobs = [[rng.uniform(-1, 1, n) for n in row] for row in lens]
    worst = 0.0
    for seed, prefill in ((1, 0), (2, 37)):
        lanes = S.LanesNP(sr_in, sr_out, 3, max_frames=1023, prefill=prefill)
        done = S.run_free(lanes, jobs, seed)
        for lane in range(3):
            assert len(done[lane]) == 2
            for x, out in zip(jobs[lane], done[lane]):
                want = R.resample(x, sr_in, sr_out)
                assert out.shape == (prefill + R.length(len(x), sr_in, sr_out),) and not out[:prefill].any()
                if want.size:
                    worst = max(worst, np.abs(out[prefill:] - want).max() / np.abs(x).max())
    print("%d -> %d: worst %.2e of max |x|" % (sr_in, sr_out, worst))
    assert worst <= 1e-14


@pytest.mark.parametrize("block,sample_rate,output_rate", BLOCKS)
def test_block_delay_is_the_brute_force_prefill_and_the_denoisers_delay(block, sample_rate, output_rate, built):
    from fullycnnspeechenhancement_amd import audio
    from fullycnnspeechenhancement_amd.freerun import _block_plan
    # more than the pattern's period (at most 128 q_down calls: 441 here) behind the lanes' first outputs
    z, hops = S.brute_prefill(block, sample_rate, output_rate, 1200)
    print("block %d at %d -> %d Hz: Z %d, hops per call %s, delay %d" % (block, sample_rate, output_rate, z, sorted(hops),
                                                                      z + 640 * output_rate // 8000))
    assert audio.block_delay(block, sample_rate, output_rate) == z + 640 * output_rate // 8000
    assert _block_plan(block, sample_rate, output_rate) == (block * output_rate // sample_rate, z, sorted(hops))


def test_block_delay_reproduces_the_hop_grid(built):
    from fullycnnspeechenhancement_amd import audio
    assert audio.block_delay(128) == audio.block_delay(128, 8000, 8000) == audio.STREAM_DELAY == 640
    for rate in (16000, 48000):
        assert audio.block_delay(128 * rate // 8000, rate, rate) == audio.stream_delay(rate, rate)


def create(lib, *args):
    h = ctypes.c_void_p()
    rc = lib.rced_rfree_create(*args, ctypes.byref(h))
    return rc, lib.rced_last_error().decode(), h


def test_library_refusals_come_before_a_device_is_looked_for(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    F, I = _lib.PCM_F32, _lib.PCM_S16
    # (sr_in, sr_out, channels, src_dtype, out_dtype, lanes, max_frames, max_take, prefill, device)
    rc, msg, h = create(lib, 8001, 8000, 1, F, F, 4, 100, 100, 0, 0)                  # what rced_resample_taps refuses
    assert rc == _lib.RCED_ERR_ARG and not h and "8001" in msg and "1 MiB" in msg
    for bad in [(0, 8000, 1, F, F, 4, 100, 100, 0, 0), (44100, 8000, 0, F, F, 4, 100, 100, 0, 0), (44100, 8000, 1, 7, F, 4, 100, 100, 0, 0),
                (44100, 8000, 1, I, 7, 4, 100, 100, 0, 0), (44100, 8000, 1, F, F, 0, 100, 100, 0, 0), (44100, 8000, 1, F, F, 70000, 100, 100, 0, 0),
                (44100, 8000, 1, F, F, 4, 0, 100, 0, 0), (44100, 8000, 1, F, F, 4, 100, 0, 0, 0), (44100, 8000, 1, F, F, 4, 100, 100, -1, 0),
                (44100, 8000, 1, F, F, 4, 2 ** 25, 100, 0, 0)]:
        rc, msg, h = create(lib, *bad)
        assert rc == _lib.RCED_ERR_ARG and msg and not h, bad
    assert lib.rced_rfree_create(44100, 8000, 1, F, F, 4, 100, 100, 0, 0, None) == _lib.RCED_ERR_ARG
    assert lib.rced_rfree_plan(44100, 8000, 7, 4, 100, 100, 0, None, None, None, None) == _lib.RCED_ERR_ARG
    assert lib.rced_rfree_available(44100, 8000, -1) == -1 and lib.rced_rfree_available(0, 8000, 5) == -1
    assert lib.rced_rfree_available(8001, 8000, 5) == -1
    assert lib.rced_rfree_push(None, None, 0, None, None, 0, None, None) == _lib.RCED_ERR_ARG
    assert lib.rced_rfree_finish(None, None, 0, None, None, None, None) == _lib.RCED_ERR_ARG
    assert lib.rced_rfree_reset(None, 0) == _lib.RCED_ERR_ARG
    lib.rced_rfree_destroy(None)


def test_python_refusals(built):
    from fullycnnspeechenhancement_amd import BlockDenoiser, FreeResampler, InferenceEngine, audio
    with pytest.raises(ValueError, match="int16"):
        FreeResampler(44100, 8000, 2, dtype="int8")
    with pytest.raises(ValueError, match="out_dtype"):
        FreeResampler(44100, 8000, 2, out_dtype="float64")
    with pytest.raises(ValueError, match="positive"):
        FreeResampler(0, 8000, 2)
    with pytest.raises(audio._lib.RcedError, match="max_take"):
        FreeResampler(44100, 8000, 2, max_take=0)
    # the denoiser refuses before it touches the device
    model = type("Model", (), {"_handle": 1, "device": 0})()
    with pytest.raises(ValueError, match="smallest block that is, is 441"):
        BlockDenoiser(model, 2, 480, sample_rate=44100, output_rate=8000)             # 480 * 80 / 441
    with pytest.raises(ValueError, match="smallest block that is, is 3"):
        BlockDenoiser(model, 2, 100, sample_rate=48000, output_rate=16000)
    with pytest.raises(ValueError, match="block must be >= 1"):
        BlockDenoiser(model, 2, 0, sample_rate=44100, output_rate=44100)
    with pytest.raises(ValueError, match="more than 64"):
        BlockDenoiser(model, 2, 66 * 128 * 6, sample_rate=48000, output_rate=48000)
    with pytest.raises(ValueError, match="12.5 Hz"):
        BlockDenoiser(model, 2, 8000, sample_rate=8000, output_rate=8001)
    with pytest.raises(ValueError, match="inference model"):
        BlockDenoiser(type("Model", (), {"_handle": None, "device": 0})(), 2, 441, sample_rate=44100, output_rate=44100)
    with pytest.raises(ValueError, match="rebuild"):
        BlockDenoiser(model, 2, 441, sample_rate=44100, output_rate=44100, rebuild="overlap")
    with pytest.raises(ValueError, match="smallest block"):
        audio.block_delay(100, 44100, 8000)
    # a device-tensor `active` cannot be mirrored: refused by type, before the call looks at anything else
    lane = object.__new__(BlockDenoiser)
    lane._down = lane._denoiser = lane._up = None
    with pytest.raises(TypeError, match="host values"):
        lane.process(np.zeros((2, 441), np.float32), active=_Device())
    # denoise_stream with a block goes through the same refusals, and without one refuses 44.1 kHz as before
    eng = object.__new__(InferenceEngine)
    eng.model = model
    with pytest.raises(ValueError, match="smallest block"):
        next(eng.denoise_stream([np.zeros(300)], sample_rate=44100, output_rate=8000, block=100))
    with pytest.raises(ValueError, match="44100"):
        next(eng.denoise_stream([np.zeros(300)], sample_rate=44100, output_rate=44100))


class _Device(object):
    """What process() takes for a device tensor without a device to make one on."""
    is_cuda = True


def test_symbols_are_declared_exported_and_bound(built):
    import inspect
    from fullycnnspeechenhancement_amd import InferenceEngine, _lib
    header = open(os.path.join(ROOT, "include", "rced.h")).read()
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name, nargs in (("rced_rfree_available", 3), ("rced_rfree_plan", 11), ("rced_rfree_create", 11), ("rced_rfree_destroy", 1),
                        ("rced_rfree_push", 8), ("rced_rfree_finish", 7), ("rced_rfree_reset", 2)):
        assert name + "(" in header and hasattr(lib, name), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
    assert _lib.load().rced_rfree_available.restype is ctypes.c_longlong
    assert inspect.signature(InferenceEngine.denoise_stream).parameters["block"].default is None


def test_plan_arithmetic_as_a_stand_alone_program(tmp_path, built):
    exe = host_cxx.build(tmp_path, "rfree_plan_check")
    # its own sweep, then the geometry and the sizes the library reports for the lanes a BlockDenoiser makes of this file's blocks
    from fullycnnspeechenhancement_amd import _lib, audio
    from fullycnnspeechenhancement_amd.freerun import _block_plan
    lib = _lib.load()
    args, groups = [], 0
    for block, rin, rout in BLOCKS:
        block_out, z, hops = _block_plan(block, rin, rout)
        for sr_in, sr_out, max_frames, max_take, prefill in ((rin, 8000, block, 128 * max(hops), 0), (8000, rout, 128 * max(hops), block_out, z)):
            p, q, left, table = audio.resample_taps(sr_in, sr_out)
            v = [ctypes.c_int() for _ in range(4)]
            assert lib.rced_rfree_plan(sr_in, sr_out, _lib.PCM_F32, 4, max_frames, max_take, prefill, *[ctypes.byref(x) for x in v]) == 0
            args += [sr_in, sr_out, p, q, left, table.shape[1], max_frames, max_take, prefill] + [x.value for x in v]
            groups += 1
    assert "%d plans, 0 failures" % (14 + groups) in host_cxx.run(exe, args)
