"""GPU tests of the overlap-add stream (rced_stream_create_ex with RCED_STREAM_REBUILD_OLA, StreamingDenoiser(rebuild="ola"),
InferenceEngine.denoise_stream(rebuild="ola")): lanes against the device's own whole-utterance overlap-add chain and the fp64
chain, at the streaming bound of tests/test_stream_gpu.py and at ITS delay; a lane against the same signal alone in every slot
layout of the 64-slot block, and the contract's invariants, bit for bit."""

import ctypes

import numpy as np
import pytest

import ola_np
import stream_np
from oracle import audio_np, rced_c
from test_stream_gpu import BOUND, HOPS, JOBS, _cache, drop_delay, engine, signal, weights

pytestmark = pytest.mark.gpu

# test_stream_gpu's four lanes and a fifth whose lengths have no tail (r = 0) or sit on the edges of the frame count T: 128, 256
# (T = 2, 1: the last hop owed is hop T - 1, then hop T), 384, 640, 768 and a single sample
JOBS_OLA = JOBS + [[128, 256, 384, 640, 768, 1]]


def oracle_chain(net, sig):
    """ola_np over the fp64 masks of the whole utterance, once per (network, signal)."""
    key = ("oracle-ola", net, sig.tobytes())
    if key not in _cache:
        mag, phase = audio_np.stft(sig)
        pred = rced_c.forward(net, weights(net), mag.astype(np.float32)[None, :, :, None], np.float64)[0, :, :, 0]
        _cache[key] = ola_np.ola(pred, phase, frames=mag.shape[0], length=len(sig))
    return _cache[key]


def check_jobs(net, hops, what):
    """The seeded weights carry biases, so the net's output on a zero row is not zero: a frame at or past T that leaked into
    hop T (finish stages 6 slots whatever T is), or a slot that took its lower half from the neighbouring lane, fails here."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    eng = engine(net)
    sigs = [[signal(n, 100 * lane + i) for i, n in enumerate(lens)] for lane, lens in enumerate(JOBS_OLA)]
    stream = StreamingDenoiser(eng, len(JOBS_OLA), max_hops=8, rebuild="ola")
    assert stream.delay == stream_np.DELAY == 640
    done = stream_np.run_lanes(stream, sigs, hops)
    stream.close()
    worst = []
    for lane, lens in enumerate(JOBS_OLA):
        assert len(done[lane]) == len(lens)
        for sig, (out, pushed) in zip(sigs[lane], done[lane]):
            out = drop_delay(out, pushed, len(sig))
            off, ref = eng.denoise_pcm(sig, rebuild="ola"), oracle_chain(net, sig)
            e_off = np.abs(out - off).max() / np.abs(off).max()
            e_ref = np.abs(out - ref).max() / np.abs(ref).max()
            msg = "[ola stream %s] lane %d L %d: vs denoise_pcm(rebuild='ola') %.2e, vs fp64 chain %.2e" % (what, lane, len(sig), e_off, e_ref)
            print(msg)
            worst.append((e_off <= BOUND and e_ref <= BOUND, msg))
    assert all(ok for ok, _ in worst), [m for ok, m in worst if not ok]


@pytest.mark.parametrize("hops", sorted(HOPS))
def test_v3_lanes_match_the_offline_overlap_add_and_the_fp64_chain(built, hops):
    check_jobs("FullyCNNV3", HOPS[hops], "V3 %s" % hops)


@pytest.mark.parametrize("net", ["FullyCNN", "FullyCNNV2"])
def test_r_ced_lanes_match_the_offline_overlap_add_and_the_fp64_chain(built, net):
    check_jobs(net, HOPS["mixed"], net)


def through(stream, sigs, k):
    """sigs [lanes, L] through every lane in pushes of k hops, then finish: [lanes] outputs"""
    whole = sigs.shape[1] // (128 * k) * 128 * k
    assert sigs.shape[1] - whole < 128
    outs = [stream.push(sigs[:, at:at + 128 * k]) for at in range(0, whole, 128 * k)]
    rest = stream.finish(list(range(len(sigs))), [s[whole:] for s in sigs])
    return [np.concatenate([o[s] for o in outs] + [rest[s]]) for s in range(len(sigs))]


# K hops per push -> 64 // K lanes per workgroup.  K = 1: every slot is a lane's slot 0, all 64 lower halves come from state, the
# 65th lane opens a second workgroup.  K = 3: 21 lanes, slot 63 unused, 43 lanes = two workgroups and one lane.  K = 17: 3 lanes
# whose slots cross the N-tile seams at 16, 32, 48 in different places.  K = 64: one lane, all three seams inside it.
LAYOUTS = {"K1": (1, 65, 9), "K3": (3, 43, 3), "K17": (17, 7, 2), "K64": (64, 2, 2)}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_a_lane_among_others_equals_the_lane_alone_bit_for_bit(built, layout):
    """Neighbouring lanes carry different signals: a slot that read the slot below it across a lane's boundary, in any of the
    ways the block offers (one lane down, one N-tile down, the previous workgroup's), would differ from the lane alone."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    k, lanes, pushes = LAYOUTS[layout]
    eng = engine("FullyCNNV3")
    sigs = np.stack([signal(128 * k * pushes + 37, 1000 + s) for s in range(lanes)])
    many = StreamingDenoiser(eng, lanes, max_hops=k, rebuild="ola")
    got = through(many, sigs, k)
    many.close()
    alone = StreamingDenoiser(eng, 1, max_hops=k, rebuild="ola")
    for s in range(lanes):
        want = through(alone, sigs[s:s + 1], k)[0]                 # finish leaves the lane as new
        assert len(want) == 640 + sigs.shape[1] and want[640:].any()
        assert np.array_equal(got[s], want), (layout, s, np.abs(got[s] - want).max())
    alone.close()
    assert not np.array_equal(got[0][640:], got[1][640:])


def test_duplicate_lanes_are_bit_equal_and_the_first_640_samples_are_zero(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    a, b = signal(1357, 1), signal(1357, 2)
    stream = StreamingDenoiser(engine("FullyCNNV3"), 4, max_hops=8, rebuild="ola")
    outs = []
    for at, k in ((0, 1), (128, 3), (512, 2), (768, 4)):           # 10 hops
        pcm = np.stack([a[at:at + 128 * k], b[at:at + 128 * k], a[at:at + 128 * k], a[at:at + 128 * k]])
        outs.append(stream.push(pcm))
    rest = stream.finish([0, 1, 2, 3], [a[1280:], b[1280:], a[1280:], a[1280:]])
    stream.close()
    out = [np.concatenate([o[s] for o in outs] + [rest[s]]) for s in range(4)]
    assert all(len(o) == 640 + 1357 for o in out)
    for o in out:
        assert not o[:640].any() and o[640:].any()
    assert np.array_equal(out[0], out[2]) and np.array_equal(out[0], out[3])     # not the lane index, not the neighbours
    assert not np.array_equal(out[0], out[1])


def test_idle_pushes_leave_a_lane_untouched(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    a, b = signal(1357, 3), signal(3000, 4)
    eng = engine("FullyCNNV3")

    def run(idle_between):
        stream = StreamingDenoiser(eng, 3, max_hops=8, rebuild="ola")
        got, fed = [], 0
        for i, at in enumerate(range(0, 1280, 256)):
            pcm = np.zeros((3, 256), np.float32)
            pcm[1] = a[at:at + 256]
            got.append(stream.push(pcm, [0, 1, 0])[1])
            if idle_between:                                       # the others talk, lane 1 is idle: with other hop counts too
                k = 1 + i % 3
                pcm = np.full((3, 128 * k), 7.0, np.float32)
                pcm[0] = b[fed:fed + 128 * k]
                out = stream.push(pcm, [1, 0, 1])
                assert not out[1].any()
                fed += 128 * k
        got.append(stream.finish([1], [a[1280:]])[0])
        stream.close()
        return np.concatenate(got)

    assert np.array_equal(run(False), run(True))


def test_reset_without_finish_equals_a_fresh_object(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    a, b = signal(1200, 5), signal(1279, 6)
    eng = engine("FullyCNNV3")

    def run(stream):
        out = [stream.push(np.stack([a[at:at + 384], b[at:at + 384]])) for at in range(0, 1152, 384)]
        rest = stream.finish([0, 1], [a[1152:], b[1152:]])
        return [np.concatenate([o[s] for o in out] + [rest[s]]) for s in range(2)]

    fresh = StreamingDenoiser(eng, 2, max_hops=3, rebuild="ola")
    want = run(fresh)
    fresh.close()
    assert len(want[0]) == 640 + 1200 and len(want[1]) == 640 + 1279
    used = StreamingDenoiser(eng, 2, max_hops=3, rebuild="ola")
    used.push(np.stack([b[:384], a[:384]]))
    used.push(np.stack([b[384:768], a[384:768]]))                  # 6 hops: the addend and the carry are not zero any more
    used.reset()                                                   # every lane, mid-utterance, nothing handed out
    got = run(used)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    used.push(np.stack([b[:384], a[:384]]))
    used.push(np.stack([b[384:768], a[384:768]]))
    used.reset(1)                                                  # one lane: the other goes on where it was
    assert not used.push(np.stack([b[768:1152], b[:384]]))[1].any()          # lane 1 is at its first three hops again
    rest = used.finish([0], [b[1152:]])[0]
    used.close()
    assert np.array_equal(rest, want[1][1152:])                    # lane 0 has had b's pushes since the reset before


def test_pushes_back_to_back_need_no_synchronisation_and_two_runs_give_the_same_bits(built):
    import torch
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    sig = np.stack([signal(2048, 8), signal(2048, 9), signal(2048, 10)])
    dev = torch.from_numpy(sig).cuda()
    eng = engine("FullyCNNV3")

    def run(sync):
        stream = StreamingDenoiser(eng, 3, max_hops=8, rebuild="ola")
        outs = []
        for at, k in ((0, 8), (1024, 1), (1152, 7)):
            outs.append(stream.push(dev[:, at:at + 128 * k]))       # device tensors in, device tensors out: nothing waits
            if sync:
                torch.cuda.synchronize()
        out = torch.cat(outs, dim=1).cpu().numpy()
        stream.close()
        return out

    queued, stepped, again = run(False), run(True), run(False)
    assert queued[:, 640:].any() and np.array_equal(queued, stepped) and np.array_equal(queued, again)


def test_denoise_stream_of_odd_pieces_equals_denoise_pcm(built):
    eng = engine("FullyCNNV3")
    sig = signal(3000, 11)
    cuts = [0, 50, 1050, 1127, 1128, 1500, 2900, 3000]              # pieces of 50, 1000, 77, 1, 372, 1400, 100 samples
    out = np.concatenate(list(eng.denoise_stream((sig[a:b] for a, b in zip(cuts, cuts[1:])), rebuild="ola")))
    assert out.dtype == np.float32 and len(out) == 640 + 3000 and not out[:640].any()
    off = eng.denoise_pcm(sig, rebuild="ola")
    err = np.abs(out[640:] - off).max() / np.abs(off).max()
    print("[denoise_stream ola] vs denoise_pcm(rebuild='ola') %.2e" % err)
    assert err <= BOUND
    assert np.abs(off - eng.denoise_pcm(sig, 256)).max() > 1e-3 * np.abs(off).max()      # and it is not the reference rebuild


def test_denoise_stream_at_48_khz_in_and_out(built):
    """The rate-aware chain needs nothing of its own: the same delays.  Reference: denoise_pcm(sample_rate=48000, rebuild="ola")
    carried back to 48 kHz by resample_batch, delayed by stream_delay(48000, 48000)."""
    from fullycnnspeechenhancement_amd import audio
    eng, rate = engine("FullyCNNV3"), 48000
    n = 1500 * rate // 8000 + 37
    rng = np.random.default_rng(12)
    sig = ((0.3 + 0.2 * np.sin(2 * np.pi * np.arange(n) / 4200.0)) * rng.standard_normal(n)).astype(np.float32)
    cuts = [0, 50, 1050, 1127, 1128, 2 * n // 3, n - 100, n]         # ragged pieces, one of a single sample
    out = np.concatenate(list(eng.denoise_stream((sig[a:b] for a, b in zip(cuts, cuts[1:])), sample_rate=rate, output_rate=rate,
                                                 rebuild="ola")))
    delay = audio.stream_delay(rate, rate)
    assert delay == 4992
    off = eng.denoise_pcm(sig, sample_rate=rate, rebuild="ola")
    rows, lens = audio.resample_batch(off[None], 8000, rate)
    ref = rows[0, :lens[0]].cpu().numpy()
    assert out.dtype == np.float32 and len(out) == delay + len(ref)
    err = np.abs(out[delay:] - ref).max() / np.abs(ref).max()
    print("[denoise_stream ola 48 kHz] delay %d, vs the offline chain %.2e" % (delay, err))
    assert err <= BOUND


def test_the_default_is_the_reference_rebuild_bit_for_bit(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    eng = engine("FullyCNNV3")
    sigs = np.stack([signal(1200, 21), signal(1200, 22)])           # 9 hops in pushes of 3, a tail of 48
    outs = []
    for kw in ({}, {"rebuild": "reference"}, {"rebuild": "ola"}):
        stream = StreamingDenoiser(eng, 2, max_hops=3, **kw)
        outs.append(through(stream, sigs, 3))
        stream.close()
    assert all(np.array_equal(a, b) and a[640:].any() for a, b in zip(outs[0], outs[1]))
    assert not np.array_equal(outs[0][0], outs[2][0])


def test_create_ex_refuses_an_unknown_rebuild(built):
    from fullycnnspeechenhancement_amd import _lib
    lib, model = _lib.load(), engine("FullyCNNV3").model
    h = ctypes.c_void_p()
    assert lib.rced_stream_create_ex(model._handle, 2, 8, 512, 2, ctypes.byref(h)) == _lib.RCED_ERR_ARG and h.value is None
    assert b"rebuild" in lib.rced_last_error()
    for rebuild in (0, 1):
        assert lib.rced_stream_create_ex(model._handle, 2, 8, 512, rebuild, ctypes.byref(h)) == _lib.RCED_OK and h.value
        lib.rced_stream_destroy(h)
