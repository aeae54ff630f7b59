"""GPU tests of the streaming denoiser (rced_stream_*, audio.StreamingDenoiser, InferenceEngine.denoise_stream): lanes that
start and finish at different pushes and are reused, against the fp64 oracle chain and against the device's own
whole-utterance chain at the bound tests/test_audio_gpu.py::test_pipeline_denoise_pcm_matches_oracle_chain uses for that
chain; the contract's invariants (leading zeros, duplicate lanes, idle lanes, reset, no synchronisation) bit for bit."""

import numpy as np
import pytest

import stream_np
from oracle import audio_np, rced_c, rced_np

pytestmark = pytest.mark.gpu

BOUND = 1e-4          # max|out - ref| <= BOUND * max|ref|: the offline device chain's bound against the oracle chain
HOPS = {"all-1": [1], "all-3": [3], "all-8": [8], "mixed": [1, 8, 2, 5, 3, 7]}
# lengths {100, 200, 300, 1357, 3000} over four lanes: the lanes finish at different pushes and take their next signal
JOBS = [[3000], [1357, 300], [100, 200, 1357], [300, 100, 200]]
_cache = {}


def signal(length, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(length)
    return ((0.3 + 0.2 * np.sin(2 * np.pi * t / 700.0)) * rng.standard_normal(length)).astype(np.float32)


def weights(net):
    if ("w", net) not in _cache:
        _cache["w", net] = rced_np.make_weights(net, seed=42)
    return _cache["w", net]


def engine(net, **options):
    """One engine per network and option set for the whole module."""
    from fullycnnspeechenhancement_amd import InferenceEngine
    key = ("engine", net, tuple(sorted(options.items())))
    if key not in _cache:
        eng = InferenceEngine(net_work=net, weights=weights(net))
        for k, v in options.items():
            eng.model.set_option(k, v)
        _cache[key] = eng
    return _cache[key]


def oracle_chain(net, sig, nfft):
    """The fp64 chain of the offline test, once per (network, signal, nfft)."""
    key = ("oracle", net, sig.tobytes(), nfft)
    if key not in _cache:
        mag, phase = audio_np.stft(sig)
        pred = rced_c.forward(net, weights(net), mag.astype(np.float32)[None, :, :, None], np.float64)[0, :, :, 0]
        _cache[key] = audio_np.rebuild(pred, phase, len(sig), nfft)
    return _cache[key]


def drop_delay(out, hops, length):
    """The signal's output without the zeros the pushes returned first; those are exactly zero."""
    zeros = min(stream_np.DELAY, stream_np.STEP * hops)
    assert hops == length // stream_np.STEP and len(out) == zeros + length, (len(out), hops, length)
    assert not out[:zeros].any()
    return out[zeros:]


def check_jobs(net, eng, nfft, jobs, hops, what, oracle=True):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    sigs = [[signal(n, 100 * lane + i) for i, n in enumerate(lens)] for lane, lens in enumerate(jobs)]
    stream = StreamingDenoiser(eng, len(jobs), max_hops=8, nfft=nfft)
    done = stream_np.run_lanes(stream, sigs, hops)
    stream.close()
    for lane, lens in enumerate(jobs):
        assert len(done[lane]) == len(lens)
        for sig, (out, pushed) in zip(sigs[lane], done[lane]):
            out = drop_delay(out, pushed, len(sig))
            off = eng.denoise_pcm(sig, nfft)
            e_off = np.abs(out - off).max() / np.abs(off).max()
            msg = "[stream %s] lane %d L %d: vs denoise_pcm %.2e" % (what, lane, len(sig), e_off)
            if oracle:
                ref = oracle_chain(net, sig, nfft)
                e_ref = np.abs(out - ref).max() / np.abs(ref).max()
                msg += ", vs fp64 oracle chain %.2e" % e_ref
            print(msg)
            assert e_off <= BOUND, msg
            if oracle:
                assert e_ref <= BOUND, msg


@pytest.mark.parametrize("hops", sorted(HOPS))
@pytest.mark.parametrize("nfft", [512, 256])
def test_v3_lanes_match_oracle_chain_and_denoise_pcm(built, nfft, hops):
    check_jobs("FullyCNNV3", engine("FullyCNNV3"), nfft, JOBS, HOPS[hops], "V3 nfft %d %s" % (nfft, hops))


@pytest.mark.parametrize("net", ["FullyCNN", "FullyCNNV2"])
def test_r_ced_lanes_match_oracle_chain_and_denoise_pcm(built, net):
    check_jobs(net, engine(net), 512, [[1357], [300], [1357]], HOPS["mixed"], net)


def test_v3_bf16_stream_matches_denoise_pcm_under_the_same_option(built):
    """Under "v3_bf16" only the device's own whole-utterance chain under the same option is the reference.  The bound is what
    tests/test_v3_bf16_gpu.py allows between the bf16 and the fp32 masks (1.5e-2 of the largest), carried through the rebuild:
    the rebuild is linear in the masks, so the audio of the two offline chains differs by the rebuild of the mask difference,
    measured here per signal as max|denoise_pcm(v3_bf16) - denoise_pcm(fp32)|; twice that is allowed between the stream and
    denoise_pcm, both under v3_bf16, the factor for the de-emphasis' order.
    Measured on an MI355X (signals of 1357, 3000, 300, 200 samples): offline bf16 against offline fp32 9.9e-3, 5.8e-3, 4.8e-3,
    2.4e-2 of the largest fp32 sample; the stream against offline bf16 8.6e-8, 1.7e-7, 7.2e-8, 1.8e-7 of it."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    e16, e32 = engine("FullyCNNV3", v3_bf16=1), engine("FullyCNNV3")
    jobs = [[1357], [3000], [300, 200]]
    sigs = [[signal(n, 100 * lane + i) for i, n in enumerate(lens)] for lane, lens in enumerate(jobs)]
    stream = StreamingDenoiser(e16, 3, max_hops=8)
    done = stream_np.run_lanes(stream, sigs, HOPS["mixed"])
    stream.close()
    for lane in range(3):
        for sig, (out, pushed) in zip(sigs[lane], done[lane]):
            out = drop_delay(out, pushed, len(sig))
            off16, off32 = e16.denoise_pcm(sig), e32.denoise_pcm(sig)
            allowed = 2.0 * np.abs(off16 - off32).max()
            err = np.abs(out - off16).max()
            print("[stream v3_bf16] L %d: offline bf16 vs offline fp32 %.2e of the scale; stream vs offline bf16 %.2e of the scale"
                  % (len(sig), np.abs(off16 - off32).max() / np.abs(off32).max(), err / np.abs(off32).max()))
            assert err <= allowed, (len(sig), err, allowed)


def test_duplicate_lanes_are_bit_equal_and_the_first_640_samples_are_zero(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    a, b = signal(1357, 1), signal(1357, 2)
    stream = StreamingDenoiser(engine("FullyCNNV3"), 4, max_hops=8)
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
        stream = StreamingDenoiser(eng, 3, max_hops=8)
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

    def run(stream, first=0):
        """a through lane 0 and b through lane 1 in pushes of 3 hops, from push `first` on, then both finish."""
        out = [stream.push(np.stack([a[at:at + 384], b[at:at + 384]])) for at in range(384 * first, 1152, 384)]
        rest = stream.finish([0, 1], [a[1152:], b[1152:]])
        return [np.concatenate([o[s] for o in out] + [rest[s]]) for s in range(2)]

    fresh = StreamingDenoiser(eng, 2, max_hops=3)
    want = run(fresh)
    fresh.close()
    assert len(want[0]) == 640 + 1200 and len(want[1]) == 640 + 1279
    used = StreamingDenoiser(eng, 2, max_hops=3)
    used.push(np.stack([b[:384], a[:384]]))
    used.push(np.stack([b[384:512], a[384:512]]))
    used.reset()                                                   # every lane, mid-utterance, nothing handed out
    got = run(used)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # one lane: the other goes on where it was
    head = used.push(np.stack([b[:384], b[:384]]))
    used.reset(0)
    used.push(np.stack([a[:384], b[:384]]), [1, 0])                # lane 0 catches up from the start, lane 1 waits
    got = run(used, first=1)
    assert np.array_equal(got[0], want[0][384:])
    assert np.array_equal(np.concatenate([head[1], got[1]]), want[1])
    used.close()


def test_pushes_back_to_back_need_no_synchronisation(built):
    import torch
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    sig = np.stack([signal(2048, 8), signal(2048, 9), signal(2048, 10)])
    dev = torch.from_numpy(sig).cuda()
    eng = engine("FullyCNNV3")

    def run(sync):
        stream = StreamingDenoiser(eng, 3, max_hops=8)
        outs = []
        for at, k in ((0, 8), (1024, 1), (1152, 7)):
            outs.append(stream.push(dev[:, at:at + 128 * k]))       # device tensors in, device tensors out: nothing waits
            if sync:
                torch.cuda.synchronize()
        out = torch.cat(outs, dim=1).cpu().numpy()
        stream.close()
        return out

    queued, stepped = run(False), run(True)
    assert queued[:, 640:].any() and np.array_equal(queued, stepped)


def test_denoise_stream_of_odd_pieces_equals_denoise_pcm(built):
    eng = engine("FullyCNNV3")
    sig = signal(3000, 11)
    cuts = [0, 50, 1050, 1127, 1128, 1500, 2900, 3000]              # pieces of 50, 1000, 77, 1, 372, 1400, 100 samples
    pieces = list(eng.denoise_stream(sig[a:b] for a, b in zip(cuts, cuts[1:])))
    out = np.concatenate(pieces)
    assert out.dtype == np.float32 and len(out) == 640 + 3000 and not out[:640].any()
    off = eng.denoise_pcm(sig)
    assert np.abs(out[640:] - off).max() <= BOUND * np.abs(off).max()
    ref = oracle_chain("FullyCNNV3", sig, 512)
    assert np.abs(out[640:] - ref).max() <= BOUND * np.abs(ref).max()


def test_hop_count_and_model_lifetime_errors(built):
    from fullycnnspeechenhancement_amd import FullyCNNSEModelV3, StreamingDenoiser, _lib
    model = FullyCNNSEModelV3(False, weights=weights("FullyCNNV3"))
    stream = StreamingDenoiser(model, 2, max_hops=2)
    with pytest.raises(_lib.RcedError) as e:
        stream.push(np.zeros((2, 384), np.float32))                # K = 3 > max_hops
    assert e.value.code == _lib.RCED_ERR_ARG
    with pytest.raises(ValueError):
        stream.push(np.zeros((2, 100), np.float32))                # not whole hops
    assert stream.push(np.zeros((2, 256), np.float32)).shape == (2, 256)
    model.close()                                                  # rced_destroy under the stream
    with pytest.raises(_lib.RcedError) as e:
        stream.push(np.zeros((2, 128), np.float32))
    assert e.value.code == _lib.RCED_ERR_STATE
    stream.close()
