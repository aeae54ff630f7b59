"""The argument helpers that the host-side entry points share (fullycnnspeechenhancement_amd/_args.py), as far as they need no
device: tail packing, host integers, the sample-format table; and that audio.py still hands out every public name that now
lives in evaluation.py, arena.py and streaming.py."""

import numpy as np
import pytest


def test_pack_tails_refusals():
    from fullycnnspeechenhancement_amd._args import pack_tails
    z = np.zeros(3, np.float32)
    for lanes, tails in (([1, 1], [z, z]),                       # duplicate lanes
                         ([0, 4], [z, z]), ([-1], [z]),          # a lane out of range
                         ([0, 1], [z]), ([0], [z, z])):          # lanes and tails of different lengths
        with pytest.raises(ValueError, match="distinct indices"):
            pack_tails(4, 8, 1, np.float32, lanes, tails)
    with pytest.raises(ValueError, match="fewer than 8 frames"):
        pack_tails(4, 8, 1, np.float32, [2], [np.zeros(8, np.float32)])             # a whole unit is a push, not a tail
    with pytest.raises(ValueError, match="fewer than 8 frames"):
        pack_tails(4, 8, 2, np.int16, [2], [np.zeros((8, 2), np.int16)])
    with pytest.raises(ValueError, match="whole frames of 2 channels"):
        pack_tails(4, 8, 2, np.int16, [2], [np.zeros(5, np.int16)])


def test_pack_tails_layout():
    from fullycnnspeechenhancement_amd._args import pack_tails
    tail, counts = pack_tails(4, 8, 1, np.float32, [2], [np.zeros(0, np.float32)])  # an empty tail still ends its lane
    assert tail.shape == (4, 8) and tail.dtype == np.float32 and not tail.any()
    assert counts.dtype == np.int32 and counts.tolist() == [-1, -1, 0, -1]
    a, b = np.arange(1, 8, dtype=np.float64), [5.0]                                # unit - 1 frames; any sequence numpy takes
    tail, counts = pack_tails(4, 8, 1, np.float32, np.array([3, 0]), [a, b])
    assert counts.tolist() == [1, -1, -1, 7]
    assert tail[3].tolist() == [1, 2, 3, 4, 5, 6, 7, 0] and tail[0].tolist() == [5] + [0] * 7 and not tail[1:3].any()
    s = np.arange(1, 11, dtype=np.int16).reshape(5, 2)                             # 2-channel int16: [frames, 2] or interleaved
    for given in (s, s.reshape(-1)):
        tail, counts = pack_tails(3, 6, 2, np.int16, [1], [given])
        assert tail.shape == (3, 6, 2) and tail.dtype == np.int16 and tail.flags.c_contiguous
        assert counts.tolist() == [-1, 5, -1] and np.array_equal(tail[1, :5], s) and not tail[1, 5].any() and not tail[[0, 2]].any()


def test_host_ints():
    import torch
    from fullycnnspeechenhancement_amd._args import host_ints
    want = [3, 0, 70000, -2]
    for given in (want, tuple(want), np.array(want, np.int64), np.array(want, np.float64), torch.tensor(want, dtype=torch.int32)):
        got = host_ints(given, 4, "counts")
        assert got == want and all(type(v) is int for v in got)
        assert host_ints(given) == want                                            # no count asked for
        with pytest.raises(ValueError, match="counts must hold N = 5 values, got 4"):
            host_ints(given, 5, "counts")
    assert host_ints(None, 4, "counts") is None


def test_pcm_formats():
    import torch
    from fullycnnspeechenhancement_amd import _args, _lib, audio
    assert audio.PCM_DTYPES is _args.PCM_DTYPES and sorted(_args.PCM_DTYPES) == ["float32", "int16"]
    want = {"float32": (torch.float32, np.float32, _lib.PCM_F32), "int16": (torch.int16, np.int16, _lib.PCM_S16)}
    for name in _args.PCM_DTYPES:
        t, a, code = _args.pcm_format(name)
        assert (t, code) == (want[name][0], want[name][2]) and np.dtype(a) == np.dtype(want[name][1])
        assert _args.pcm_name(t) == name and _args.pcm_name(np.dtype(a)) == name and _args.pcm_name(np.zeros(1, a).dtype) == name
    with pytest.raises(ValueError, match="int16.*'int8'"):
        _args.pcm_format("int8")
    with pytest.raises(ValueError, match="out_dtype"):
        _args.pcm_format("float64", "out_dtype")
    assert _args.pcm_name(torch.int8) is None and _args.pcm_name(np.dtype(np.float64)) is None and _args.pcm_name(torch.int32) is None


REEXPORTS = {
    "_args": ["FRAME", "STEP", "BINS", "SAMPLE_RATE", "PCM_DTYPES"],
    "evaluation": ["sdr_batch", "stoi_batch", "STOI_RATES", "gains_needed", "mix_snr_batch", "denoise_and_score"],
    "arena": ["gather_pcm", "resample_length", "resample_taps", "resample_arena", "resample_batch", "PCM_DTYPES"],
    "streaming": ["StreamingDenoiser", "StreamingResampler", "resampler_delay", "stream_delay", "STREAM_DELAY", "STREAM_FINISH_MAX",
                  "STREAM_MAX_HOPS"],
}


def test_audio_hands_out_every_name_it_had():
    import importlib
    import fullycnnspeechenhancement_amd as pkg
    for module, names in REEXPORTS.items():
        mod = importlib.import_module("fullycnnspeechenhancement_amd." + module)
        for name in names:
            assert getattr(pkg.audio, name) is getattr(mod, name), (module, name)
    assert (pkg.audio.FRAME, pkg.audio.STEP, pkg.audio.BINS, pkg.audio.SAMPLE_RATE) == (256, 128, 129, 8000)
    assert (pkg.audio.STREAM_DELAY, pkg.audio.STREAM_FINISH_MAX, pkg.audio.STREAM_MAX_HOPS) == (640, 768, 64)
    for name in ("num_frames", "stft_batch", "istft_batch", "AudioFeature", "AudioReBuild"):              # what stays in audio.py
        assert getattr(pkg.audio, name).__module__ == pkg.audio.__name__
    assert pkg.audio.KERNELS == {"x6": 1, "f32": 0}
    assert pkg.StreamingDenoiser is pkg.audio.StreamingDenoiser and pkg.StreamingResampler is pkg.audio.StreamingResampler
