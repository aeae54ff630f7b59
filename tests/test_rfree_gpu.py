"""GPU tests of the free-running resampler lanes (rced_rfree_*, audio.FreeResampler), of audio.BlockDenoiser and of
InferenceEngine.denoise_stream(block=...).  Everything a lane hands out is audio.resample_batch of everything it
was given, bit for bit and without a delay, whatever the pushes and takes; a BlockDenoiser's stream is its three stages by hand,
bit for bit, behind `.delay` samples, for 44.1 kHz as for any other rate."""

import numpy as np
import pytest

import rfree_np as S
from test_rstream_gpu import engine, offline, signal

pytestmark = pytest.mark.gpu

_cache = {}


# ---- audio.FreeResampler ----

# (sr_in, sr_out, dtype, channels, out_dtype)
LANE_CASES = [(44100, 8000, "float32", 1, "float32"), (44100, 8000, "int16", 2, "float32"), (8000, 44100, "float32", 1, "float32"),
              (48000, 8000, "float32", 1, "int16"), (8000, 8000, "float32", 1, "float32")]


@pytest.mark.parametrize("sr_in,sr_out,dtype,channels,out_dtype", LANE_CASES)
def test_lanes_equal_resample_batch_bit_for_bit_without_delay(built, sr_in, sr_out, dtype, channels, out_dtype):
    """Three lanes, signals of 2,000 to 5,000 frames, the first and last lane reused for a second signal; per lane and push 0, 1,
    7, 441, 480 or 1023 frames or an idle call, and a random take of what the mirror says is there (S.run_free, which also holds
    the mirror against `.in_ring` and against the counts finish reports).  A second chunking gives the same bits."""
    from fullycnnspeechenhancement_amd import FreeResampler, audio
    lens = [[4999, 2001], [3456], [2750, 2000]]
    jobs = [[signal(n, channels, dtype, 300 + 10 * lane + i) for i, n in enumerate(row)] for lane, row in enumerate(lens)]
    runs = []
    for seed, prefill in ((5, 0), (6, 0), (7, 29)):
        stream = FreeResampler(sr_in, sr_out, 3, channels=channels, dtype=dtype, out_dtype=out_dtype, max_frames=1023, prefill=prefill)
        runs.append(S.run_free(stream, jobs, seed))
        stream.close()
    for lane in range(3):
        for i, x in enumerate(jobs[lane]):
            want = offline(x, sr_in, sr_out, out_dtype)
            assert len(want) == audio.resample_length(len(x), sr_in, sr_out)
            for done, prefill in zip(runs, (0, 0, 29)):
                out = done[lane][i]
                assert out.dtype == want.dtype and len(out) == prefill + len(want) and not out[:prefill].any()
                assert np.array_equal(out[prefill:], want), "%d -> %d %s x%d -> %s, lane %d: %d samples differ, first at %d" % (
                    sr_in, sr_out, dtype, channels, out_dtype, lane, int((out[prefill:] != want).sum()), int(np.argmax(out[prefill:] != want)))
            assert want.any()


def test_a_push_of_several_staging_passes_equals_441_frames_at_a_time(built):
    """44.1 kHz -> 8 kHz stages 987 outputs a pass: 40,000 frames in one push are eight passes."""
    from fullycnnspeechenhancement_amd import FreeResampler
    x = np.stack([signal(40000, 1, "float32", 330), signal(40000, 1, "float32", 331)])
    stream = FreeResampler(44100, 8000, 2, max_frames=40000)
    whole = stream.push(x, counts=[40000, 39000])
    taken = list(stream.taken)
    rest = stream.finish([0, 1], [x[0, :0], x[1, 39000:]])
    stream.close()
    whole = [np.concatenate([whole[s, :taken[s]], rest[s]]) for s in range(2)]
    stream = FreeResampler(44100, 8000, 2, max_frames=441)
    parts = [[], []]
    for at in range(0, 39690, 441):
        out = stream.push(x[:, at:at + 441])
        for s in range(2):
            parts[s].append(out[s, :stream.taken[s]])
    rest = stream.finish([0, 1], [x[0, 39690:], x[1, 39690:]])
    stream.close()
    for s in range(2):
        want = offline(x[s], 44100, 8000, "float32")
        assert taken[s] > 6000 and np.array_equal(whole[s], want) and np.array_equal(np.concatenate(parts[s] + [rest[s]]), want)


def test_idle_calls_reset_and_reuse(built):
    """Idle calls leave a lane and its neighbours untouched; reset without finish equals a fresh object; a finished lane is reused."""
    from fullycnnspeechenhancement_amd import FreeResampler
    x = np.stack([signal(3000, 1, "float32", 340 + s) for s in range(3)])

    def run(stream, idle_between):
        got = [[] for _ in range(3)]
        for i, at in enumerate(range(0, 2400, 480)):
            if idle_between:
                counts = [-1, -1, -1]
                counts[i % 3] = 7                                   # one lane takes 7 frames of the block early, the others sit it out
                out = stream.push(x[:, at:at + 7], counts, [0, 0, 0])
                assert out.shape == (3, 0)
                counts = [480 - 7 if c == 7 else 480 for c in counts]
                pcm = np.stack([np.concatenate([x[s, at + 480 - c:at + 480], np.zeros(480 - c, np.float32)]) for s, c in enumerate(counts)])
                out = stream.push(pcm, counts)
            else:
                out = stream.push(x[:, at:at + 480])
            for s in range(3):
                got[s].append(out[s, :stream.taken[s]])
        rest = stream.finish([0, 1, 2], [x[s, 2400:] for s in range(3)])
        return [np.concatenate(g + [r]) for g, r in zip(got, rest)]

    stream = FreeResampler(44100, 8000, 3, max_frames=480)
    plain = run(stream, False)
    assert all(np.array_equal(a, b) for a, b in zip(plain, run(stream, True)))          # the finished lanes, reused
    for s in range(3):
        assert np.array_equal(plain[s], offline(x[s], 44100, 8000, "float32"))
    # lanes left in the middle of an utterance: reset one, then all, and start over
    stream.push(x[:, 100:580], take=0)
    stream.reset(1)
    assert stream.in_ring[1] == 0 and stream.in_ring[0] > 0
    stream.reset()
    assert stream.in_ring == [0, 0, 0]
    assert all(np.array_equal(a, b) for a, b in zip(plain, run(stream, False)))
    stream.close()


# ---- audio.BlockDenoiser ----

def run_blocks(lanes, jobs, late):
    """jobs[lane]: the signals that lane takes one after the other; lane s sits out the first late[s] calls.  Every call hands each
    lane that has a whole block left its next block; a lane with less is finished with the others like it and goes on to its next
    signal.  Returns per lane the list of outputs, one per signal."""
    n, block = lanes.lanes, lanes.block
    which, at = [0] * n, [0] * n
    pieces = [[] for _ in range(n)]
    done = [[] for _ in range(n)]
    tail_shape, dtype = jobs[0][0].shape[1:], jobs[0][0].dtype
    calls = 0
    while any(which[s] < len(jobs[s]) for s in range(n)):
        live = [which[s] < len(jobs[s]) and calls >= late[s] for s in range(n)]
        ending = [s for s in range(n) if live[s] and len(jobs[s][which[s]]) - at[s] < block]
        if ending:
            for s, rest in zip(ending, lanes.finish(ending, [jobs[s][which[s]][at[s]:] for s in ending])):
                done[s].append(np.concatenate(pieces[s] + [np.asarray(rest)]))
                pieces[s], at[s], which[s] = [], 0, which[s] + 1
            continue
        pcm = np.full((n, block) + tail_shape, 77, dtype)                  # an idle lane's row is not read
        for s in range(n):
            if live[s]:
                pcm[s] = jobs[s][which[s]][at[s]:at[s] + block]
        out = lanes.process(pcm, [int(v) for v in live])
        assert out.shape == (n, lanes.block_out) and out.dtype == np.float32
        for s in range(n):
            if live[s]:
                pieces[s].append(out[s])
                at[s] += block
            else:
                assert not out[s].any()                                      # an idle lane's row is zeros
        calls += 1
    return done


def logged(lanes, issued):
    """Routes every 8 kHz push of `lanes` through a logger: (hops, flags per lane)."""
    push8 = lanes._push8

    def push(pcm, active=None):
        flags = [1] * lanes.lanes if active is None else [int(v) for v in (active.tolist() if hasattr(active, "tolist") else active)]
        issued.append((int(pcm.shape[1]) // 128, flags))
        return push8(pcm, active)
    lanes._push8 = push


def blocks(net, rate, out_rate, dtype, channels, block, rebuild="reference"):
    """Three lanes of BlockDenoiser over signals of 0.25 to 0.4 s of different lengths: lane 2 starts three calls late, they finish at
    different calls, lane 1 is reused; once per case for the whole module: (signals per lane, output per signal, the object's
    numbers, the hop count and flags of every 8 kHz push it issued)."""
    from fullycnnspeechenhancement_amd import BlockDenoiser
    key = (net, rate, out_rate, dtype, channels, block, rebuild)
    if key not in _cache:
        lens = [[int(0.4 * rate) + 11], [int(0.25 * rate) + block - 1, int(0.27 * rate) // block * block], [int(0.3 * rate) + 1]]
        jobs = [[signal(n, channels, dtype, 400 + 10 * lane + i) for i, n in enumerate(row)] for lane, row in enumerate(lens)]
        lanes = BlockDenoiser(engine(net), 3, block, sample_rate=rate, output_rate=out_rate, channels=channels, dtype=dtype, rebuild=rebuild)
        issued = []
        logged(lanes, issued)
        done = run_blocks(lanes, jobs, [0, 0, 3])
        _cache[key] = (jobs, done, (lanes.delay, lanes.prefill, lanes.block_out), issued)
        lanes.close()
    return _cache[key]


def by_hand(net, rate, out_rate, x, portions, rebuild):
    """The three stages by hand for one signal: resample_batch(x -> 8 kHz) through a plain one-lane 8 kHz StreamingDenoiser in
    pushes of `portions` hops (consumed from the front), then its finish; that whole stream, its 640 zeros included, through
    resample_batch(8 kHz -> out_rate).  Returns (the 8 kHz signal, the result)."""
    from fullycnnspeechenhancement_amd import StreamingDenoiser
    x8 = offline(x, rate, 8000, "float32")
    plain = StreamingDenoiser(engine(net), 1, max_hops=8, rebuild=rebuild)
    z8, at = [], 0
    while len(x8) - at >= 128:
        k = portions.pop(0)
        z8.append(plain.push(x8[None, at:at + 128 * k])[0])
        at += 128 * k
    z8.append(plain.finish([0], [x8[at:]])[0])
    plain.close()
    return x8, offline(np.concatenate(z8), 8000, out_rate, "float32")


BLOCK_CASES = [("FullyCNN", 44100, 44100, "float32", 1, 441, "reference"), ("FullyCNNV3", 44100, 44100, "int16", 2, 512, "reference"),
               ("FullyCNN", 48000, 48000, "float32", 1, 480, "reference"), ("FullyCNN", 8000, 8000, "float32", 1, 100, "reference"),
               ("FullyCNN", 44100, None, "float32", 1, 441, "reference"), ("FullyCNN", 44100, 44100, "float32", 1, 441, "ola"),
               # blocks of 1 and 2 hops: with lane 2 three calls late most calls hold lanes of either count, and issue two 8 kHz pushes
               ("FullyCNN", 44100, 44100, "float32", 1, 1024, "reference")]


@pytest.mark.parametrize("net,rate,out_rate,dtype,channels,block,rebuild", BLOCK_CASES)
def test_block_denoiser_equals_the_three_stages_by_hand_bit_for_bit(built, net, rate, out_rate, dtype, channels, block, rebuild):
    """The plain denoiser is fed the hops in the portions the object issued for that lane (its last bit depends on the hops a push
    carries); Z zeros stand in front of the by-hand result."""
    from fullycnnspeechenhancement_amd import audio
    jobs, done, (delay, z, block_out), issued = blocks(net, rate, out_rate, dtype, channels, block, rebuild)
    rout = out_rate or 8000
    assert delay == audio.block_delay(block, rate, out_rate) == z + 640 * rout // 8000 and block_out * rate == block * rout
    assert {k for k, _ in issued} == ({1, 2} if block == 1024 else {1})
    if block == 1024:       # two pushes of one call: the lanes of one are the idle lanes of the other
        assert any(k1 != k2 and not any(f1[s] and f2[s] for s in range(3)) and any(f1) and any(f2)
                   for (k1, f1), (k2, f2) in zip(issued, issued[1:]))
    for lane in range(3):
        portions = [k for k, flags in issued if flags[lane]]
        assert len(done[lane]) == len(jobs[lane])
        for x, out in zip(jobs[lane], done[lane]):
            x8, up = by_hand(net, rate, rout, x, portions, rebuild)
            want = np.concatenate([np.zeros(z, np.float32), up])
            assert out.dtype == np.float32 and out.shape == want.shape, (out.shape, want.shape)
            assert len(out) == delay + audio.resample_length(len(x8), 8000, rout)
            diff = out != want
            print("[blocks %s %d -> %d Hz %s x%d block %d %s] lane %d, %d frames: delay %d, %d of %d samples differ"
                  % (net, rate, rout, dtype, channels, block, rebuild, lane, len(x), delay, int(diff.sum()), out.size))
            assert not diff.any() and out[delay:].any()
        assert not portions                                          # every 8 kHz push of the lane is accounted for


def test_a_lane_among_others_equals_the_same_lane_alone(built):
    """Lanes 0 and 1 take the same signal from the first call on, lane 2 another from the second call on: it is in another phase
    of the pattern of hops per call, so the same call holds lanes with one hop and lanes with none.  44.1 kHz in blocks of 441;
    out at 8 kHz, where the up lanes pass samples through and the first `.delay` samples are exactly zero, and out at 44.1 kHz,
    where the interpolator rings ahead of the denoiser's first sample: there the zeros end (640 - right) p / q
    samples behind Z, right = 64 the interpolator's reach, and the by-hand test holds what follows."""
    from fullycnnspeechenhancement_amd import BlockDenoiser, audio
    a, b = signal(12000, 1, "float32", 450), signal(11000, 1, "float32", 451)
    for out_rate in (None, 44100):
        three = BlockDenoiser(engine("FullyCNN"), 3, 441, sample_rate=44100, output_rate=out_rate)
        issued = []
        logged(three, issued)
        many = run_blocks(three, [[a], [a], [b]], [0, 0, 1])
        delay, z, block_out = three.delay, three.prefill, three.block_out
        three.close()
        alone = BlockDenoiser(engine("FullyCNN"), 1, 441, sample_rate=44100, output_rate=out_rate)
        one = run_blocks(alone, [[a]], [0])
        other = run_blocks(alone, [[b]], [0])                             # the finished lane, reused
        alone.close()
        assert any(flags[0] != flags[2] for _, flags in issued) and all(flags[0] == flags[1] for _, flags in issued)
        assert np.array_equal(many[0][0], one[0][0]) and np.array_equal(many[1][0], one[0][0]) and np.array_equal(many[2][0], other[0][0])
        p, q, left, table = audio.resample_taps(8000, out_rate or 8000)
        quiet = delay if out_rate is None else z + (640 - (table.shape[1] - 1 - left)) * p // q
        assert not one[0][0][:quiet].any() and one[0][0][delay:delay + block_out].any()


@pytest.mark.parametrize("rate,block", [(48000, 768), (16000, 256)])
def test_on_the_hop_grid_the_stream_is_the_streaming_denoisers(built, rate, block):
    """A block of one hop at the device's rate: StreamingDenoiser(rate, rate) pushed a hop at a time gives the same stream at the
    same delay, and both issue one-hop 8 kHz pushes.  The two finish differently (the existing object's down lanes hand the
    denoiser a last hop padded behind the signal's end where this one hands it the signal's true tail), so the streams are compared
    up to the last call's output; test_block_denoiser_equals_the_three_stages_by_hand_bit_for_bit is the authority on the end."""
    from fullycnnspeechenhancement_amd import BlockDenoiser, StreamingDenoiser, audio
    x = signal(20 * block + 5, 1, "float32", 460)
    new = BlockDenoiser(engine("FullyCNN"), 1, block, sample_rate=rate, output_rate=rate)
    old = StreamingDenoiser(engine("FullyCNN"), 1, max_hops=1, sample_rate=rate, output_rate=rate)
    logs = ([], [])
    logged(new, logs[0])
    logged(old, logs[1])
    assert new.delay == old.delay == audio.stream_delay(rate, rate)
    got = [[], []]
    for at in range(0, 20 * block, block):
        got[0].append(new.process(x[None, at:at + block])[0])
        got[1].append(old.push(x[None, at:at + block])[0])
    a, b = np.concatenate(got[0]), np.concatenate(got[1])
    # the existing object also issues the void first hop of a lane, with no lane active in it
    assert {k for k, _ in logs[0]} == {k for k, _ in logs[1]} == {1} and len(logs[0]) == sum(any(f) for _, f in logs[1]) == 19
    new.finish([0], [x[20 * block:]])
    old.finish([0], [x[20 * block:]])
    new.close()
    old.close()
    print("[hop grid %d Hz] delay %d, %d of %d samples differ" % (rate, new.delay, int((a != b).sum()), a.size))
    assert a.shape == b.shape and np.array_equal(a, b) and a[new.delay:].any()


def offline_bound(net, x, rate):
    """test_composite_against_the_offline_chain's reference and bound: resample_batch(denoise_pcm(x, sample_rate=rate), 8 kHz ->
    rate), and 1e-4 max|off| times the interpolator's gain plus one float32 rounding of the result."""
    from fullycnnspeechenhancement_amd import audio
    off = engine(net).denoise_pcm(x, sample_rate=rate)
    ref = offline(off, 8000, rate, "float32")
    gain = np.abs(audio.resample_taps(8000, rate)[3]).sum(axis=1).max()
    return ref, 1e-4 * np.abs(off).max() * gain + 2.0 ** -24 * np.abs(ref).max()


def test_block_denoiser_against_the_offline_chain_at_44100(built):
    jobs, done, (delay, _, _), _ = blocks("FullyCNN", 44100, 44100, "float32", 1, 441)
    for lane in range(3):
        for x, out in zip(jobs[lane], done[lane]):
            ref, bound = offline_bound("FullyCNN", x, 44100)
            assert len(out) == delay + len(ref)
            err = np.abs(out[delay:] - ref).max()
            print("[blocks vs offline 44100 Hz] lane %d, %d frames: delay %d, worst error %.3e, bound %.3e" % (lane, len(x), delay, err, bound))
            assert err <= bound


def test_calls_back_to_back_need_no_synchronisation(built):
    import torch
    from fullycnnspeechenhancement_amd import BlockDenoiser
    x = torch.as_tensor(np.stack([signal(20 * 441, 1, "float32", 470 + s) for s in range(4)]), device="cuda")

    def run(sync):
        lanes = BlockDenoiser(engine("FullyCNN"), 4, 441, sample_rate=44100, output_rate=44100)
        outs = []
        for at in range(0, 20 * 441, 441):
            outs.append(lanes.process(x[:, at:at + 441]))
            assert outs[-1].is_cuda and outs[-1].shape == (4, 441)
            if sync:
                torch.cuda.synchronize()
        out = torch.cat(outs, dim=1).cpu().numpy()
        lanes.close()
        return out
    queued, stepped = run(False), run(True)
    quiet = 1323 + (640 - 64) * 441 // 80                            # Z, and the denoiser's zeros up to where the interpolator reaches its first sample
    assert np.array_equal(queued, stepped) and queued[:, 4851:].any() and not queued[:, :quiet].any()


def test_denoise_stream_in_blocks_at_44100(built):
    from fullycnnspeechenhancement_amd import audio
    eng, rate = engine("FullyCNN"), 44100
    sig = signal(15000, 1, "float32", 480)
    cuts = [0, 50, 1050, 1127, 1128, 9000, 14900, 15000]             # ragged pieces, one of a single sample
    pieces = [sig[a:b] for a, b in zip(cuts, cuts[1:])]
    out = np.concatenate(list(eng.denoise_stream(iter(pieces), sample_rate=rate, output_rate=rate, block=441)))
    delay = audio.block_delay(441, rate, rate)
    ref, bound = offline_bound("FullyCNN", sig, rate)
    assert out.dtype == np.float32 and len(out) == delay + len(ref) and not out[:1323 + (640 - 64) * 441 // 80].any()
    err = np.abs(out[delay:] - ref).max()
    print("[denoise_stream block 441 at %d Hz] delay %d, worst error %.3e, bound %.3e" % (rate, delay, err, bound))
    assert err <= bound
    with pytest.raises(ValueError, match="44100"):
        next(eng.denoise_stream(iter(pieces), sample_rate=rate, output_rate=rate))
