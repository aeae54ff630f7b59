"""GPU tests of the resampler lanes (rced_rstream_*, audio.StreamingResampler) and of audio.StreamingDenoiser /
InferenceEngine.denoise_stream at the device's rate.  A lane's output is audio.resample_batch of everything pushed, delayed by
`.delay`, bit for bit: lanes of different lengths that finish at different pushes and are reused, every source and output format;
the contract's invariants (leading zeros, duplicate lanes, idle lanes, reset, push sizes, no synchronisation, a captured graph)
bit for bit as well."""

import numpy as np
import pytest

import rstream_np as S
from oracle import rced_np
from test_rstream_host import CONVERSIONS

pytestmark = pytest.mark.gpu

FORMATS = [("int16", 1), ("int16", 2), ("float32", 1)]
_cache = {}


def signal(frames, channels, dtype, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None]
    x = (0.3 + 0.2 * np.sin(2 * np.pi * t / 700.0)) * rng.standard_normal((frames, channels))
    x = x[:, 0] if channels == 1 else x
    return np.clip(np.rint(x * 8000.0), -32768, 32767).astype(np.int16) if dtype == "int16" else x.astype(np.float32)


def offline(x, sr_in, sr_out, out_dtype):
    from fullycnnspeechenhancement_amd import audio
    rows, lens = audio.resample_batch(x[None], sr_in, sr_out, dtype=out_dtype)
    return rows[0, :lens[0]].cpu().numpy()


@pytest.mark.parametrize("sr_in,sr_out,unit_in,unit_out", CONVERSIONS)
def test_lanes_equal_resample_batch_delayed_bit_for_bit(built, sr_in, sr_out, unit_in, unit_out):
    from fullycnnspeechenhancement_amd import StreamingResampler
    # four lanes; lengths around the unit, a long one that spans several staging passes, lanes that take a second signal
    lens = [[5 * unit_in + 7, unit_in - 1], [3000, unit_in + 1], [1, unit_in, 2 * unit_in + 3], [3000]]
    for dtype, channels in FORMATS:
        jobs = [[signal(n, channels, dtype, 10 * lane + i) for i, n in enumerate(row)] for lane, row in enumerate(lens)]
        jobs[3] = [jobs[1][0]]                                                    # a duplicate of lane 1's first signal
        for out_dtype in ("float32", "int16"):
            stream = StreamingResampler(sr_in, sr_out, 4, unit_in=unit_in, unit_out=unit_out, channels=channels, dtype=dtype,
                                        out_dtype=out_dtype, max_units=4)
            done = S.run_lanes(stream, jobs, [2, 1, 4, 3])
            delay = stream.delay
            stream.close()
            for lane in range(4):
                assert len(done[lane]) == len(jobs[lane])
                for x, (out, units) in zip(jobs[lane], done[lane]):
                    want = S.delayed(offline(x, sr_in, sr_out, out_dtype), delay, units, unit_out)
                    zeros = min(delay, units * unit_out)
                    assert out.dtype == want.dtype and out.shape == want.shape, (dtype, channels, out_dtype, len(x), out.shape, want.shape)
                    assert not out[:zeros].any()
                    assert np.array_equal(out, want), "%s x%d -> %s, lane %d, %d frames: %d samples differ, first at %d" % (
                        dtype, channels, out_dtype, lane, len(x), int((out != want).sum()), int(np.argmax(out != want)))
            assert np.array_equal(done[3][0][0], done[1][0][0]) and done[1][0][0].any()


def test_long_pushes_span_several_staging_passes(built):
    """48 kHz -> 8 kHz stages 768 outputs at a time, 8 kHz -> 48 kHz 3072: pushes of 16 units (2048 and 12288 outputs) take several
    passes over a lane's history and input; pushes of one unit give the same stream."""
    from fullycnnspeechenhancement_amd import StreamingResampler
    for sr_in, sr_out, unit_in, unit_out in ((48000, 8000, 768, 128), (8000, 48000, 128, 768)):
        x = np.stack([signal(33 * unit_in + 5, 1, "float32", 40 + s) for s in range(3)])
        outs = {}
        for k in (1, 16):
            stream = StreamingResampler(sr_in, sr_out, 3, unit_in=unit_in, max_units=16)
            pieces = [stream.push(x[:, at:at + k * unit_in]) for at in range(0, 32 * unit_in, k * unit_in)]
            pieces.append(stream.push(x[:, 32 * unit_in:33 * unit_in]))
            rest = stream.finish([0, 1, 2], [x[s, 33 * unit_in:] for s in range(3)])
            outs[k] = [np.concatenate([p[s] for p in pieces] + [rest[s]]) for s in range(3)]
            delay = stream.delay
            stream.close()
        for s in range(3):
            assert np.array_equal(outs[1][s], outs[16][s])
            assert np.array_equal(outs[16][s], S.delayed(offline(x[s], sr_in, sr_out, "float32"), delay, 33, unit_out))


def test_idle_pushes_leave_a_lane_and_its_neighbours_untouched(built):
    from fullycnnspeechenhancement_amd import StreamingResampler
    a, b = signal(256 * 9 + 100, 2, "int16", 3), signal(256 * 30, 2, "int16", 4)

    def run(idle_between):
        stream = StreamingResampler(16000, 8000, 3, unit_out=128, channels=2, dtype="int16", max_units=4)
        got, others, fed = [], [], 0
        for i, at in enumerate(range(0, 256 * 9, 256 * 3)):
            pcm = np.zeros((3, 256 * 3, 2), np.int16)
            pcm[1] = a[at:at + 256 * 3]
            got.append(stream.push(pcm, [0, 1, 0])[1])
            if idle_between:                                       # the others talk, lane 1 is idle: with other unit counts too
                k = 1 + i % 3
                pcm = np.full((3, 256 * k, 2), 7, np.int16)
                pcm[0] = pcm[2] = b[fed:fed + 256 * k]
                out = stream.push(pcm, [1, 0, 1])
                assert not out[1].any()
                others.append(out[[0, 2]])
                fed += 256 * k
        got.append(stream.finish([1], [a[256 * 9:]])[0])
        stream.close()
        return np.concatenate(got), (np.concatenate(others, axis=1) if others else None)

    alone, _ = run(False)
    mixed, others = run(True)
    assert np.array_equal(alone, mixed) and alone.any()
    assert np.array_equal(others[0], others[1])
    assert np.array_equal(others[0], S.delayed(offline(b, 16000, 8000, "float32"), 63, 30, 128)[:others.shape[1]])


def test_reset_without_finish_equals_a_fresh_object(built):
    from fullycnnspeechenhancement_amd import StreamingResampler
    a, b = signal(128 * 9 + 50, 1, "float32", 5), signal(128 * 9 + 127, 1, "float32", 6)

    def run(stream, first=0):
        out = [stream.push(np.stack([a[at:at + 384], b[at:at + 384]])) for at in range(384 * first, 1152, 384)]
        rest = stream.finish([0, 1], [a[1152:], b[1152:]])
        return [np.concatenate([o[s] for o in out] + [rest[s]]) for s in range(2)]

    fresh = StreamingResampler(8000, 48000, 2, unit_in=128, max_units=3)
    want = run(fresh)
    fresh.close()
    used = StreamingResampler(8000, 48000, 2, unit_in=128, max_units=3)
    used.push(np.stack([b[:384], a[:384]]))
    used.push(np.stack([b[384:512], a[384:512]]))
    used.reset()                                                   # every lane, mid-utterance, nothing handed out
    got = run(used)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    head = used.push(np.stack([b[:384], b[:384]]))                 # one lane: the other goes on where it was
    used.reset(0)
    used.push(np.stack([a[:384], b[:384]]), [1, 0])
    got = run(used, first=1)
    assert np.array_equal(got[0], want[0][384 * 6:])
    assert np.array_equal(np.concatenate([head[1], got[1]]), want[1])
    used.close()


def test_pushes_back_to_back_need_no_synchronisation(built):
    import torch
    from fullycnnspeechenhancement_amd import StreamingResampler
    dev = torch.from_numpy(np.stack([signal(768 * 16, 1, "float32", 8 + s) for s in range(3)])).cuda()

    def run(sync):
        stream = StreamingResampler(48000, 8000, 3, unit_out=128, max_units=8)
        outs = []
        for at, k in ((0, 8), (8, 1), (9, 7)):
            outs.append(stream.push(dev[:, 768 * at:768 * (at + k)]))   # device tensors in, device tensors out: nothing waits
            if sync:
                torch.cuda.synchronize()
        out = torch.cat(outs, dim=1).cpu().numpy()
        stream.close()
        return out

    queued, stepped = run(False), run(True)
    assert queued[:, 63:].any() and not queued[:, :63].any() and np.array_equal(queued, stepped)


def test_a_push_replayed_from_a_captured_graph(built):
    """One push is one kernel launch and nothing else, so its capture is a single node without branches (the node count itself is
    not asserted here: torch does not expose it): captured once, replayed for every later push of the stream, against the same
    pushes launched directly."""
    import torch
    from fullycnnspeechenhancement_amd import StreamingResampler, _lib
    x = torch.from_numpy(np.stack([signal(256 * 2 * 6, 1, "float32", 20 + s) for s in range(3)])).cuda()
    eager = StreamingResampler(16000, 8000, 3, unit_out=128, max_units=2)
    want = torch.cat([eager.push(x[:, at:at + 512]) for at in range(0, 512 * 6, 512)], dim=1).cpu().numpy()
    eager.close()
    stream = StreamingResampler(16000, 8000, 3, unit_out=128, max_units=2)
    src = torch.zeros((3, 512), dtype=torch.float32, device="cuda")
    dst = torch.zeros((3, 256), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().rced_rstream_push(stream._h, src.data_ptr(), None, 2, dst.data_ptr(), st))
    got = []
    for at in range(0, 512 * 6, 512):
        src.copy_(x[:, at:at + 512])
        graph.replay()
        got.append(dst.clone())
    got = torch.cat(got, dim=1).cpu().numpy()
    stream.close()
    assert np.array_equal(got, want) and want[:, 63:].any()


# ---- audio.StreamingDenoiser and InferenceEngine.denoise_stream at the device's rate ----

def engine(net="FullyCNNV3"):
    from fullycnnspeechenhancement_amd import InferenceEngine
    if net not in _cache:
        _cache[net] = InferenceEngine(net_work=net, weights=rced_np.make_weights(net, seed=42))
    return _cache[net]


def composite(net, rate, dtype, channels, counts=(2, 1, 4, 3)):
    """Three lanes of StreamingDenoiser(sample_rate=rate, output_rate=rate) over signals of different lengths that finish at
    different pushes, one lane reused, in pushes of counts[i] hops (cycled); once per case for the whole module: (signals per
    lane, (output, hops) per signal, delay, the hop count and flags of every 8 kHz push the object issued)."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    key = ("composite", net, rate, dtype, channels, tuple(counts))
    if key not in _cache:
        hop = 128 * rate // 8000
        lens = [[23 * hop + 11], [10 * hop + hop - 1, 7 * hop], [12 * hop + 1]]
        jobs = [[signal(n, channels, dtype, 60 + 10 * lane + i) for i, n in enumerate(row)] for lane, row in enumerate(lens)]
        stream = StreamingDenoiser(engine(net), 3, max_hops=4, sample_rate=rate, channels=channels, dtype=dtype, output_rate=rate)
        stream.unit_in = stream.hop_in                              # the driver's name for it
        issued, push8 = [], stream._push8

        def logged(pcm, active=None):
            flags = [1, 1, 1] if active is None else [int(v) for v in (active.tolist() if hasattr(active, "tolist") else active)]
            issued.append((int(pcm.shape[1]) // 128, flags))
            return push8(pcm, active)
        stream._push8 = logged
        done = S.run_lanes(stream, jobs, list(counts))
        _cache[key] = (jobs, done, stream.delay, issued)
        stream.close()
    return _cache[key]


def by_hand(net, rate, x, hop_counts):
    """The three stages by hand for one signal: resample_batch(x -> 8 kHz) through a plain 8 kHz StreamingDenoiser in pushes of
    hop_counts hops (consumed from the front), then its finish; that whole output stream (640 zeros and the tail included) behind
    the hop of zeros the down lanes' delay puts in front of it, through resample_batch(8 kHz -> rate); behind the up lanes' delay."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser, audio
    x8 = offline(x, rate, 8000, "float32")
    plain = StreamingDenoiser(engine(net), 1, max_hops=8)
    z8, at = [], 0
    while len(x8) - at >= 128:
        k = hop_counts.pop(0)
        z8.append(plain.push(x8[None, at:at + 128 * k])[0])
        at += 128 * k
    z8.append(plain.finish([0], [x8[at:]])[0])
    plain.close()
    up = audio.resampler_delay(8000, rate)
    return np.concatenate([np.zeros(up, np.float32), offline(np.concatenate([np.zeros(128, np.float32)] + z8), 8000, rate, "float32")])


CASES = [("FullyCNNV3", 48000, "float32", 1), ("FullyCNNV3", 16000, "float32", 1), ("FullyCNNV3", 48000, "int16", 2),
         ("FullyCNN", 16000, "float32", 1)]


@pytest.mark.parametrize("net,rate,dtype,channels", CASES)
def test_composite_equals_the_three_stages_by_hand_bit_for_bit(built, net, rate, dtype, channels):
    """By hand: resample_batch(x -> 8 kHz) fed hop by hop to a plain 8 kHz StreamingDenoiser, that whole output stream through
    resample_batch(8 kHz -> rate), all delayed by the lanes' delays (by_hand above).  The object is pushed a hop at a time, as
    the plain denoiser is: the 8 kHz denoiser's own last bits depend on how many hops a push carries (measured on an MI355X: the
    same signal pushed 1 hop at a time and 2, 1, 4, 3 at a time differs in 6 to 8 % of the samples by one float32 rounding, 6e-8
    to 2.4e-7), so hop by hop is only equal to hop by hop; test_composite_in_longer_pushes_... covers the longer pushes."""
    from fullycnnspeechenhancement_amd import audio
    jobs, done, delay, _ = composite(net, rate, dtype, channels, counts=(1,))
    assert delay == audio.stream_delay(rate, rate, channels, dtype) == 768 * rate // 8000 + audio.resampler_delay(8000, rate)
    for lane in range(3):
        for x, (out, hops) in zip(jobs[lane], done[lane]):
            want = by_hand(net, rate, x, [1] * 1000)
            assert hops == len(x) // (128 * rate // 8000) and out.dtype == np.float32 and out.shape == want.shape, (out.shape, want.shape)
            diff = out != want
            print("[composite hop by hop %s %d Hz %s x%d] lane %d, %d frames: %d of %d samples differ, worst %.2e"
                  % (net, rate, dtype, channels, lane, len(x), int(diff.sum()), out.size, np.abs(out - want).max()))
            assert not diff.any()


@pytest.mark.parametrize("net,rate,dtype,channels", CASES)
def test_composite_in_longer_pushes_equals_the_stages_by_hand_in_the_same_pushes(built, net, rate, dtype, channels):
    """Pushes of 2, 1, 4, 3 hops: bit for bit the stages by hand with the plain denoiser fed the hops in the portions the object
    issued for that lane (the first hop of a push apart from the others, nothing for the void first hop of a lane's first push,
    a hop at a time while finish drains)."""
    jobs, done, delay, issued = composite(net, rate, dtype, channels)
    for lane in range(3):
        portions = [k for k, flags in issued if flags[lane]]
        for x, (out, hops) in zip(jobs[lane], done[lane]):
            want = by_hand(net, rate, x, portions)
            assert out.shape == want.shape, (out.shape, want.shape)
            diff = out != want
            print("[composite 2, 1, 4, 3 %s %d Hz %s x%d] lane %d, %d frames: %d of %d samples differ" % (net, rate, dtype, channels, lane, len(x),
                                                                                                     int(diff.sum()), out.size))
            assert not diff.any()
        assert not portions                                          # every 8 kHz push of the lane is accounted for


def plain8(net, x8, hop_counts):
    """The whole output stream of a plain 8 kHz StreamingDenoiser for the 8 kHz signal x8: pushes of hop_counts hops (consumed
    from the front), then its finish."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    plain = StreamingDenoiser(engine(net), 1, max_hops=8)
    z8, at = [], 0
    while len(x8) - at >= 128:
        k = hop_counts.pop(0)
        z8.append(plain.push(x8[None, at:at + 128 * k])[0])
        at += 128 * k
    z8.append(plain.finish([0], [x8[at:]])[0])
    plain.close()
    return np.concatenate(z8)


@pytest.mark.parametrize("sample_rate,output_rate", [(16000, None), (8000, 16000)], ids=["down_lanes_only", "up_lanes_only"])
def test_half_chain_equals_its_stages_by_hand_bit_for_bit(built, sample_rate, output_rate):
    """A chain of two stages.  Down lanes only (16 kHz in, 8 kHz out): the plain 8 kHz denoiser fed resample_batch(x -> 8 kHz)
    hop by hop, then its finish, behind the hop of zeros the down lanes' delay puts in front.  Up lanes only (8 kHz in, 16 kHz
    out): the plain denoiser's whole output stream through resample_batch(8 kHz -> 16 kHz), behind the up lanes' delay.  Two
    lanes pushed a hop at a time (as in test_composite_equals_the_three_stages_by_hand_bit_for_bit) that finish at different
    pushes: one signal of 6 hops and 11 frames; one of 2 hops and hop - 1 frames, then on the same lane one of exactly 3 hops,
    whose tail is empty."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser, audio
    hop = 128 * sample_rate // 8000
    jobs = [[signal(6 * hop + 11, 1, "float32", 90)], [signal(2 * hop + hop - 1, 1, "float32", 91), signal(3 * hop, 1, "float32", 92)]]
    stream = StreamingDenoiser(engine("FullyCNN"), 2, max_hops=4, sample_rate=sample_rate, output_rate=output_rate)
    stream.unit_in = stream.hop_in                                  # the driver's name for it
    done = S.run_lanes(stream, jobs, [1])
    delay = stream.delay
    stream.close()
    assert delay == audio.stream_delay(sample_rate, output_rate) == (768 if output_rate is None else 1280 + audio.resampler_delay(8000, 16000))
    for lane in range(2):
        assert len(done[lane]) == len(jobs[lane])
        for x, (out, hops) in zip(jobs[lane], done[lane]):
            if output_rate is None:
                x8 = offline(x, sample_rate, 8000, "float32")
                want = np.concatenate([np.zeros(128, np.float32), plain8("FullyCNN", x8, [1] * 100)])
            else:
                x8 = x
                up = np.zeros(audio.resampler_delay(8000, output_rate), np.float32)
                want = np.concatenate([up, offline(plain8("FullyCNN", x, [1] * 100), 8000, output_rate, "float32")])
            # `.delay` zeros, then the result; less the zeros of its 640 that a denoiser lane of under 5 hops never handed out
            short = max(0, 640 - len(x8) // 128 * 128)
            length = (delay + len(x8) - short if output_rate is None
                      else delay + audio.resample_length(len(x8), 8000, output_rate) - short * output_rate // 8000)
            assert hops == len(x) // hop and out.dtype == np.float32 and len(out) == length and out.shape == want.shape, (out.shape, want.shape)
            diff = out != want
            print("[half chain %d -> %s Hz] lane %d, %d frames: %d of %d samples differ" % (sample_rate, output_rate or 8000, lane, len(x),
                                                                                          int(diff.sum()), out.size))
            assert not diff.any() and out.any()


@pytest.mark.parametrize("rate", [48000, 16000])
def test_composite_against_the_offline_chain(built, rate):
    """The reference is resample_batch(denoise_pcm(x, sample_rate=rate), 8 kHz -> rate) delayed by `.delay`.  The up lanes are
    linear and what they are fed differs from denoise_pcm's result by at most DESIGN.md 3.4d's streaming bar, 1e-4 max|off|:
    the bound is that times the interpolator's worst-case gain max_r sum_i |table_up[r][i]|, plus one float32 rounding of the
    result.  The delay's samples are zeros up to where the interpolator first reaches the denoiser's first sample."""
    from fullycnnspeechenhancement_amd import audio
    jobs, done, delay, _ = composite("FullyCNNV3", rate, "float32", 1)
    p, q, left, table = audio.resample_taps(8000, rate)
    gain = np.abs(table).sum(axis=1).max()
    quiet = (768 - (table.shape[1] - 1 - left)) * p // q
    for lane in range(3):
        for x, (out, _) in zip(jobs[lane], done[lane]):
            off = engine().denoise_pcm(x, sample_rate=rate)
            ref = offline(off, 8000, rate, "float32")
            assert len(out) == delay + len(ref) and not out[:quiet].any()
            bound = 1e-4 * np.abs(off).max() * gain + 2.0 ** -24 * np.abs(ref).max()
            err = np.abs(out[delay:] - ref).max()
            print("[composite vs offline %d Hz] lane %d, %d frames: delay %d, gain %.4f, worst error %.3e, bound %.3e"
                  % (rate, lane, len(x), delay, gain, err, bound))
            assert err <= bound


def test_default_arguments_are_the_plain_8_khz_lanes(built):
    """StreamingDenoiser with the new arguments at their defaults holds no resampler lanes and gives the bits of the object
    built without them; denoise_stream with its defaults yields the pieces of that lane driven by hand."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    eng = engine()
    x = np.stack([signal(1357, 1, "float32", 1), signal(1357, 1, "float32", 2)])
    outs = []
    for kw in ({}, {"sample_rate": 8000, "channels": 1, "dtype": "float32", "output_rate": None}, {"output_rate": 8000}):
        stream = StreamingDenoiser(eng, 2, max_hops=8, **kw)
        assert stream._down is None and stream._up is None and stream.delay == 640 and stream.hop_in == 128
        got = [stream.push(x[:, at:at + 128 * k]) for at, k in ((0, 1), (128, 3), (512, 2), (768, 4))]
        rest = stream.finish([0, 1], [x[0, 1280:], x[1, 1280:]])
        outs.append([np.concatenate([g[s] for g in got] + [rest[s]]) for s in range(2)])
        stream.close()
    for other in outs[1:]:
        assert all(np.array_equal(a, b) and a[640:].any() for a, b in zip(outs[0], other))
    sig = signal(3000, 1, "float32", 11)
    cuts = [0, 50, 1050, 1127, 1128, 1500, 2900, 3000]
    got = list(eng.denoise_stream(sig[a:b] for a, b in zip(cuts, cuts[1:])))
    lane = StreamingDenoiser(eng.model, 1, max_hops=8)
    want, held = [], np.zeros(0, np.float32)
    for a, b in zip(cuts, cuts[1:]):
        held = np.concatenate([held, sig[a:b]])
        while held.size >= 128:
            k = min(held.size // 128, 8)
            want.append(lane.push(held[None, :k * 128])[0])
            held = held[k * 128:]
    want.append(lane.finish([0], [held])[0])
    lane.close()
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert sum(len(g) for g in got) == 640 + 3000


def test_denoise_stream_at_the_devices_rate_against_the_offline_chain(built):
    """Ragged pieces at 16 kHz in and out; joined and with the leading `.delay` samples dropped, the offline chain of
    test_composite_against_the_offline_chain within its bound."""
    from fullycnnspeechenhancement_amd import audio
    eng, rate = engine(), 16000
    n = 3000 * rate // 8000 + 37
    sig = signal(n, 1, "float32", 12)
    cuts = [0, 50, 1050, 1127, 1128, 2 * n // 3, n - 100, n]         # ragged pieces, one of a single sample
    out = np.concatenate(list(eng.denoise_stream((sig[a:b] for a, b in zip(cuts, cuts[1:])), sample_rate=rate, output_rate=rate)))
    delay = audio.stream_delay(rate, rate)
    off = eng.denoise_pcm(sig, sample_rate=rate)
    ref = offline(off, 8000, rate, "float32")
    assert out.dtype == np.float32 and len(out) == delay + len(ref)
    gain = np.abs(audio.resample_taps(8000, rate)[3]).sum(axis=1).max()
    bound = 1e-4 * np.abs(off).max() * gain + 2.0 ** -24 * np.abs(ref).max()
    err = np.abs(out[delay:] - ref).max()
    print("[denoise_stream %d Hz] delay %d, worst error %.3e, bound %.3e" % (rate, delay, err, bound))
    assert err <= bound
