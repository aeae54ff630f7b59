"""GPU tests of the denoiser lanes at a framing (rced_stream_create_fr, audio.StreamingDenoiser(framing=...),
InferenceEngine.denoise_stream(framing=...)): lanes that finish at different pushes and are reused, against the
device's own whole-utterance chain at that framing and against the fp64 chain of tests/framing_np.py; the general kernels against
the specialised ones at 256 / 128 / hamming; and the contract's invariants bit for bit -- a lane among others equals the lane
alone in three slot layouts, leading zeros, duplicate and idle lanes, reset, two runs, no synchronisation.

The bar is the streaming suite's (tests/test_stream_gpu.py): 1e-4 of the largest sample.  For overlap-add it is relaxed per sample
exactly as tests/test_framing_gpu.py::ola_bar relaxes its 2e-5 -- times max(1, A[n] / A0), A the conditioning of the sample
(framing_np.ola_conditioning), A0 = 229.7 that of 256 / 128 / hamming's worst sample -- and never by more than 64: the uncapped
factor of (200, 80, blackman) reaches 75.2 at the utterance's first and last samples, where a Blackman window is all but zero, so
there the cap binds and the bar is tighter than ola_bar's.  test_the_bar_cannot_widen checks on the CPU that the hamming framings
get no relaxation, that no factor is above 64, and that in each other framing's longest case at least 70 % of the samples sit at
the unrelaxed bar."""

import ctypes

import numpy as np
import pytest

import framing_np as fnp
import stream_fr_np as sfr
from test_stream_gpu import BOUND, engine, signal, weights

gpu = pytest.mark.gpu

OLA_FRAMINGS = [(160, 80, "hamming"), (256, 64, "hanning"), (64, 16, "hamming"), (255, 100, "hanning"), (200, 80, "blackman"),
                (256, 256, "bartlett"), (256, 128, "hamming")]
REF_FRAMINGS = [(160, 80, "hamming"), (64, 16, "hamming")]
IDS = lambda fs: ["%d-%d-%s" % f for f in fs]      # noqa: E731
HOPS = {"all-1": [1], "all-3": [3], "all-8": [8], "mixed": [1, 8, 2, 5, 3, 7]}
A0 = fnp.ola_conditioning(8, 256, 128, "hamming").max()        # 229.7 (tests/test_framing_host.py)
MAX_RELAX = 64.0
_cache = {}
_worst = {}


def relax(L, W, S, name, rebuild):
    """The factor on the bar per sample of an utterance of L samples: 1 for the reference rebuild and for every hamming framing
    (their conditioning is that of 256 / 128 / hamming or better: at most 1.0006 A0, test_the_bar_cannot_widen)."""
    if rebuild != "ola" or name == "hamming":
        return np.ones(L)
    A = fnp.ola_conditioning(sfr.num_frames(L, W, S), W, S, name)[:L]
    return np.minimum(MAX_RELAX, np.maximum(1.0, A / A0))


def test_the_bar_cannot_widen():
    for W, S, name in OLA_FRAMINGS:
        lens = sfr.lengths(W, S)
        assert max(lens) == 12 * S + W + 7
        worst = max(relax(L, W, S, name, "ola").max() for L in lens)
        share = float(np.mean(relax(max(lens), W, S, name, "ola") == 1.0))
        print("%d / %d / %s: relaxation at most %.2f, %.1f %% of the longest case unrelaxed" % (W, S, name, worst, 100 * share))
        assert worst <= MAX_RELAX
        if name == "hamming":
            assert worst == 1.0 and max(fnp.ola_conditioning(sfr.num_frames(L, W, S), W, S, name)[:L].max() for L in lens) <= 1.001 * A0
        else:
            assert share >= 0.70


def framing_of(f):
    from fullycnnspeechenhancement_amd import audio
    return audio.Framing(*f)


def jobs_of(W, S):
    """The lengths of a framing over five lanes: they finish at different pushes and take their next signal."""
    sigs = [signal(L, 7 * L + W) for L in sfr.lengths(W, S)]
    return [sigs[i::5] for i in range(5)]


def fp64_chain(net, sig, W, S, name, rebuild, nfft):
    key = (net, sig.tobytes(), W, S, name, rebuild, nfft)
    if key not in _cache:
        _cache[key] = sfr.offline(net, weights(net), sig, W, S, name, rebuild, nfft)
    return _cache[key]


def ratio(out, ref, factor):
    """max over samples of |out - ref| / (the sample's bar)"""
    scale = np.abs(ref).max()
    if scale == 0.0:
        return 0.0 if not np.abs(out).any() else np.inf
    return float((np.abs(out - ref) / (BOUND * scale * factor)).max())


def open_lanes(eng, lanes, nfft, rebuild, fr):
    """StreamingDenoiser at the framing.  At 256 / 128 / hamming that is the specialised stream (Framing() takes today's path), so
    there the general lanes are opened themselves: rced_stream_create_fr always runs the general kernels."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser, audio
    from fullycnnspeechenhancement_amd.streaming import _DenoiserLanes
    if not fr.is_default:
        return StreamingDenoiser(eng, lanes, max_hops=8, nfft=nfft, rebuild=rebuild, framing=fr)
    stream = _DenoiserLanes(eng.model, lanes, 8, nfft, rebuild, fr)
    stream.hop, stream.delay = fr.stride, audio.stream_delay_fr(fr)
    return stream


def check_jobs(net, framing, rebuild, nfft, hops, what):
    W, S, name = framing
    eng, fr = engine(net), framing_of(framing)
    jobs = jobs_of(W, S)
    stream = open_lanes(eng, len(jobs), nfft, rebuild, fr)
    assert stream.hop == S and stream.delay == sfr.delay(W, S)
    done = sfr.run_lanes(stream, jobs, hops)
    stream.close()
    worst_off = worst_ref = 0.0
    for lane, sigs in enumerate(jobs):
        assert len(done[lane]) == len(sigs)
        for sig, (out, pushed) in zip(sigs, done[lane]):
            out = sfr.drop_delay(out, pushed, len(sig), W, S)
            factor = relax(len(sig), W, S, name, rebuild)
            off = eng.denoise_pcm(sig, nfft, rebuild=rebuild, framing=fr)
            ref = fp64_chain(net, sig, W, S, name, rebuild, nfft)
            assert off.shape == ref.shape == out.shape
            r_off, r_ref = ratio(out, off, factor), ratio(out, ref, factor)
            worst_off, worst_ref = max(worst_off, r_off), max(worst_ref, r_ref)
            msg = "[stream_fr %s] lane %d L %d: %.2e of the bar vs denoise_pcm, %.2e vs the fp64 chain" % (what, lane, len(sig), r_off, r_ref)
            assert r_off <= 1.0 and r_ref <= 1.0, msg
    key = "%d / %d / %s %s" % (W, S, name, rebuild)
    _worst[key] = max(_worst.get(key, 0.0), worst_off, worst_ref)
    print("[stream_fr %s] worst: %.2e of the bar vs denoise_pcm, %.2e vs the fp64 chain; this framing so far %.2e"
          % (what, worst_off, worst_ref, _worst[key]))


@gpu
@pytest.mark.parametrize("hops", sorted(HOPS))
@pytest.mark.parametrize("framing", OLA_FRAMINGS, ids=IDS(OLA_FRAMINGS))
def test_overlap_add_lanes_match_denoise_pcm_and_the_fp64_chain(built, framing, hops):
    check_jobs("FullyCNNV3", framing, "ola", 512, HOPS[hops], "%d/%d/%s ola %s" % (framing + (hops,)))


@gpu
@pytest.mark.parametrize("hops", sorted(HOPS))
@pytest.mark.parametrize("nfft", [512, 256])
@pytest.mark.parametrize("framing", REF_FRAMINGS, ids=IDS(REF_FRAMINGS))
def test_reference_lanes_match_denoise_pcm_and_the_fp64_chain(built, framing, nfft, hops):
    check_jobs("FullyCNNV3", framing, "reference", nfft, HOPS[hops], "%d/%d/%s reference nfft %d %s" % (framing + (nfft, hops)))


@gpu
@pytest.mark.parametrize("rebuild", ["ola", "reference"])
@pytest.mark.parametrize("net", ["FullyCNN", "FullyCNNV2"])
def test_r_ced_lanes_at_160_80(built, net, rebuild):
    check_jobs(net, (160, 80, "hamming"), rebuild, 512, HOPS["mixed"], "%s 160/80 %s" % (net, rebuild))


def raw_stream(model, lanes, max_hops, rebuild, framing=None, nfft=512):
    """A handle of the C ABI: rced_stream_create_fr at a framing, rced_stream_create_ex without."""
    from fullycnnspeechenhancement_amd import _lib
    lib, h = _lib.load(), ctypes.c_void_p()
    code = ["reference", "ola"].index(rebuild)
    if framing is None:
        rc = lib.rced_stream_create_ex(model._handle, lanes, max_hops, nfft, code, ctypes.byref(h))
    else:
        W, S, name = framing
        rc = lib.rced_stream_create_fr(model._handle, lanes, max_hops, nfft, code, W, S, fnp.CODES[name], ctypes.byref(h))
    return rc, h


def run_raw(h, sigs, hop, ks, finish_max):
    """sigs [lanes, n] through the handle in pushes of ks hops (cycled), then every lane finishes: [lanes, delay + n]."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    lanes, n = sigs.shape
    dev = torch.from_numpy(np.ascontiguousarray(sigs)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    outs, at, i = [], 0, 0
    while n - at >= hop:
        k = min(ks[i % len(ks)], (n - at) // hop)
        x = dev[:, at:at + k * hop].contiguous()
        y = torch.empty_like(x)
        assert lib.rced_stream_push(h, x.data_ptr(), None, k, y.data_ptr(), st) == 0
        outs.append(y)
        at, i = at + k * hop, i + 1
    tail = torch.zeros((lanes, hop), dtype=torch.float32, device="cuda")
    tail[:, :n - at] = dev[:, at:]
    counts = torch.full((lanes,), n - at, dtype=torch.int32, device="cuda")
    rest = torch.empty((lanes, finish_max), dtype=torch.float32, device="cuda")
    owed = torch.empty((lanes,), dtype=torch.int32, device="cuda")
    assert lib.rced_stream_finish(h, tail.data_ptr(), counts.data_ptr(), rest.data_ptr(), owed.data_ptr(), st) == 0
    owed = owed.cpu().numpy()
    assert len(set(owed)) == 1
    return torch.cat(outs + [rest[:, :owed[0]]], dim=1).cpu().numpy()


@gpu
@pytest.mark.parametrize("rebuild", ["reference", "ola"])
def test_general_kernels_against_the_specialised_ones_at_the_default_framing(built, rebuild):
    """rced_stream_create_fr at 256 / 128 / hamming against rced_stream_create_ex on the same pushes: delay 640, within 1e-4 of the
    scale; and the specialised stream gives the same bits before and after a general one has lived."""
    from fullycnnspeechenhancement_amd import _lib
    lib, model = _lib.load(), engine("FullyCNNV3").model
    assert lib.rced_stream_delay_fr(256, 128) == 640 == lib.rced_stream_delay() and lib.rced_stream_finish_max_fr(256, 128) == 768
    sigs = np.stack([signal(1357, 21), signal(1357, 22), signal(1357, 23)])
    ks = HOPS["mixed"]

    def special():
        rc, h = raw_stream(model, 3, 8, rebuild)
        assert rc == 0
        out = run_raw(h, sigs, 128, ks, 768)
        lib.rced_stream_destroy(h)
        return out

    before = special()
    rc, h = raw_stream(model, 3, 8, rebuild, (256, 128, "hamming"))
    assert rc == 0
    general = run_raw(h, sigs, 128, ks, 768)
    lib.rced_stream_destroy(h)
    after = special()
    assert np.array_equal(before, after)
    assert general.shape == before.shape == (3, 640 + 1357) and not general[:, :640].any() and general[:, 640:].any()
    err = np.abs(general - before).max(axis=1) / np.abs(before).max(axis=1)
    print("[stream_fr general vs specialised, %s] %s of the scale" % (rebuild, ", ".join("%.2e" % e for e in err)))
    assert err.max() <= BOUND


LAYOUT = (256, 64, "hanning")


@gpu
@pytest.mark.parametrize("lanes,k,max_hops", [(65, 1, 8), (23, 3, 8), (2, 64, 64)], ids=["65-lanes-of-1-hop", "23-lanes-of-3-hops", "2-lanes-of-64-hops"])
def test_a_lane_among_others_equals_the_lane_alone(built, lanes, k, max_hops):
    """Slots of 64 a workgroup: 65 lanes of one hop spill into a second one, 23 lanes of 3 hops cut a lane across two, and 2
    lanes of 64 hops (two steps of the rebuild's walk) fill one each."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    W, S, name = LAYOUT
    eng, fr = engine("FullyCNNV3"), framing_of(LAYOUT)
    n = {1: 14, 3: 9, 64: 128}[k] * S + 37                          # 14, 3 and 2 pushes, more hops than the delay's 7
    mine, probe = signal(n, 31), ([0, lanes // 2, lanes - 1] if lanes > 2 else [1])

    def run(count, rows):
        stream = StreamingDenoiser(eng, count, max_hops=max_hops, rebuild="ola", framing=fr)
        sigs = np.stack([mine if i in rows else signal(n, 500 + i) for i in range(count)])
        outs = [stream.push(sigs[:, at:at + k * S]) for at in range(0, n - k * S + 1, k * S)]
        at = (n // (k * S)) * k * S
        rest = stream.finish(list(range(count)), [s[at:] for s in sigs])
        stream.close()
        return [np.concatenate([o[i] for o in outs] + [rest[i]]) for i in range(count)]

    alone = run(1, [0])[0]
    among = run(lanes, probe)
    assert len(alone) == sfr.delay(W, S) + n and alone[sfr.delay(W, S):].any()
    for i in probe:
        assert np.array_equal(among[i], alone), i
    assert not np.array_equal(among[1 if lanes > 2 else 0], alone)


@gpu
def test_leading_zeros_duplicate_lanes_and_two_runs(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    eng = engine("FullyCNNV3")
    for framing, rebuild in (((256, 64, "hanning"), "ola"), ((160, 80, "hamming"), "reference")):
        W, S, name = framing
        D, n = sfr.delay(W, S), 12 * S + W + 7
        a, b = signal(n, 1), signal(n, 2)

        def run():
            stream = StreamingDenoiser(eng, 4, max_hops=8, rebuild=rebuild, framing=framing_of(framing))
            outs, at = [], 0
            for k in (1, 3, 2, 4, 8):
                k = min(k, (n - at) // S)
                outs.append(stream.push(np.stack([a[at:at + k * S], b[at:at + k * S], a[at:at + k * S], a[at:at + k * S]])))
                at += k * S
            rest = stream.finish([0, 1, 2, 3], [a[at:], b[at:], a[at:], a[at:]])
            stream.close()
            return [np.concatenate([o[s] for o in outs] + [rest[s]]) for s in range(4)]

        out, again = run(), run()
        assert all(len(o) == D + n for o in out)
        for o in out:
            # zeros for exactly D samples; the signal follows at once (a Hann window starts at zero: sample 0 alone is the 1e-10 rule's)
            assert not o[:D].any() and o[D + 1] != 0.0 and (o[D] != 0.0 or name == "hanning")
        assert np.array_equal(out[0], out[2]) and np.array_equal(out[0], out[3]) and not np.array_equal(out[0], out[1])
        assert all(np.array_equal(x, y) for x, y in zip(out, again))


@gpu
def test_idle_pushes_leave_a_lane_untouched(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    W, S, name = LAYOUT
    n = 12 * S + W + 7
    a, b = signal(n, 3), signal(3 * n, 4)
    eng = engine("FullyCNNV3")

    def run(idle_between):
        stream = StreamingDenoiser(eng, 3, max_hops=8, rebuild="ola", framing=framing_of(LAYOUT))
        got, fed = [], 0
        for i, at in enumerate(range(0, n - 2 * S + 1, 2 * S)):
            pcm = np.zeros((3, 2 * S), np.float32)
            pcm[1] = a[at:at + 2 * S]
            got.append(stream.push(pcm, [0, 1, 0])[1])
            if idle_between:                                       # the others talk, lane 1 is idle: with other hop counts too
                k = 1 + i % 3
                pcm = np.full((3, S * k), 7.0, np.float32)
                pcm[0] = b[fed:fed + S * k]
                out = stream.push(pcm, [1, 0, 1])
                assert not out[1].any()
                fed += S * k
        got.append(stream.finish([1], [a[n // (2 * S) * 2 * S:]])[0])
        stream.close()
        return np.concatenate(got)

    quiet, busy = run(False), run(True)
    assert len(quiet) == sfr.delay(W, S) + n and np.array_equal(quiet, busy)


@gpu
def test_reset_without_finish_equals_a_fresh_object(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    W, S, name = LAYOUT
    whole = 15 * S                                                 # five pushes of 3 hops
    a, b = signal(whole + S - 1, 5), signal(whole + 20, 6)
    eng = engine("FullyCNNV3")

    def run(stream):
        out = [stream.push(np.stack([a[at:at + 3 * S], b[at:at + 3 * S]])) for at in range(0, whole, 3 * S)]
        rest = stream.finish([0, 1], [a[whole:], b[whole:]])
        return [np.concatenate([o[s] for o in out] + [rest[s]]) for s in range(2)]

    fresh = StreamingDenoiser(eng, 2, max_hops=3, rebuild="ola", framing=framing_of(LAYOUT))
    want = run(fresh)
    fresh.close()
    used = StreamingDenoiser(eng, 2, max_hops=3, rebuild="ola", framing=framing_of(LAYOUT))
    used.push(np.stack([b[:3 * S], a[:3 * S]]))
    used.push(np.stack([b[3 * S:4 * S], a[3 * S:4 * S]]))
    used.reset()                                                   # every lane, mid-utterance, nothing handed out
    got = run(used)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    used.push(np.stack([b[:3 * S], a[:3 * S]]))
    used.reset(0)                                                  # one lane: a finish of the other still owes its hops
    rest = used.finish([0, 1], [a[:0], a[:0]])
    assert len(rest[0]) == 0 and len(rest[1]) == 3 * S
    used.close()


@gpu
def test_pushes_back_to_back_need_no_synchronisation(built):
    import torch
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    W, S, name = LAYOUT
    sig = np.stack([signal(16 * S, 8), signal(16 * S, 9), signal(16 * S, 10)])
    dev = torch.from_numpy(sig).cuda()
    eng = engine("FullyCNNV3")

    def run(sync):
        stream = StreamingDenoiser(eng, 3, max_hops=8, rebuild="ola", framing=framing_of(LAYOUT))
        outs = []
        for at, k in ((0, 8), (8 * S, 1), (9 * S, 7)):
            outs.append(stream.push(dev[:, at:at + S * k]))         # device tensors in, device tensors out: nothing waits
            if sync:
                torch.cuda.synchronize()
        out = torch.cat(outs, dim=1).cpu().numpy()
        stream.close()
        return out

    queued, stepped = run(False), run(True)
    assert queued[:, sfr.delay(W, S):].any() and np.array_equal(queued, stepped)


@gpu
def test_denoise_stream_of_odd_pieces_equals_denoise_pcm(built):
    from fullycnnspeechenhancement_amd import audio
    eng, fr = engine("FullyCNNV3"), framing_of((160, 80, "hamming"))
    sig = signal(12 * 80 + 160 + 7, 11)
    cuts = [0, 50, 450, 527, 528, 700, 1100, len(sig)]
    for rebuild in ("ola", "reference"):
        pieces = list(eng.denoise_stream((sig[a:b] for a, b in zip(cuts, cuts[1:])), hops=3, rebuild=rebuild, framing=fr))
        out = np.concatenate(pieces)
        assert out.dtype == np.float32 and len(out) == 400 + len(sig) and not out[:400].any() and audio.stream_delay_fr(fr) == 400
        off = eng.denoise_pcm(sig, rebuild=rebuild, framing=fr)
        assert ratio(out[400:], off, np.ones(len(sig))) <= 1.0
        ref = fp64_chain("FullyCNNV3", sig, 160, 80, "hamming", rebuild, 512)
        assert ratio(out[400:], ref, np.ones(len(sig))) <= 1.0
    # Framing() and None are today's lanes: today's bits
    a = np.concatenate(list(eng.denoise_stream([sig[:500], sig[500:]], framing=audio.Framing())))
    b = np.concatenate(list(eng.denoise_stream([sig[:500], sig[500:]])))
    assert len(a) == 640 + len(sig) and np.array_equal(a, b)


@gpu
def test_create_refuses_through_the_abi_and_push_checks_its_hops(built):
    from fullycnnspeechenhancement_amd import StreamingDenoiser, _lib
    lib, eng = _lib.load(), engine("FullyCNNV3")
    for args in (((160, 80, "hamming"), 2), ((256, 16, "hamming"), 1), ((160, 80, "hanning"), 0)):
        h = ctypes.c_void_p()
        W, S, name = args[0]
        rc = lib.rced_stream_create_fr(eng.model._handle, 2, 8, 512, args[1], W, S, fnp.CODES[name], ctypes.byref(h))
        assert rc == _lib.RCED_ERR_ARG and not h and lib.rced_last_error()
    h = ctypes.c_void_p()
    assert lib.rced_stream_create_fr(eng.model._handle, 2, 8, 500, 1, 160, 80, 0, ctypes.byref(h)) == _lib.RCED_ERR_ARG     # nfft is checked
    assert lib.rced_stream_create_fr(eng.model._handle, 2, 65, 512, 1, 160, 80, 0, ctypes.byref(h)) == _lib.RCED_ERR_ARG
    stream = StreamingDenoiser(eng, 2, max_hops=2, rebuild="ola", framing=framing_of((160, 80, "hamming")))
    with pytest.raises(_lib.RcedError) as e:
        stream.push(np.zeros((2, 240), np.float32))                # K = 3 > max_hops
    assert e.value.code == _lib.RCED_ERR_ARG
    with pytest.raises(ValueError):
        stream.push(np.zeros((2, 128), np.float32))                # not whole hops of 80
    assert stream.push(np.zeros((2, 160), np.float32)).shape == (2, 160)
    stream.close()
