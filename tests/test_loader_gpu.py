"""GPU tests of training from audio: the ragged crop-gather (rced_gather_pcm), the device loader's batches against REAL
reference output (tests/golden/loader_ref.npz: the reference's own DataSet + Sampler + DataLoader(num_works=1)), their
invariances, FullyCNNTrainer.train over the loader, and validation over it.  The gather is a copy with an exact
conversion, so it is compared bit for bit; the spectrogram bar is the suite's STFT bar, 2e-6 of the scale
(tests/test_audio_gpu.py); figures are printed before they are asserted."""

import os

import numpy as np
import pytest

import loader_np

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 7, 8, 9, 255, 256, 257, 2049)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def gold(built):
    return loader_np.load_fixture()


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.asarray(a, dtype) if dtype else a, device="cuda")


def raw_gather(arena, begins, counts, L, out, stride, stream=None):
    """The C entry as it is (audio.gather_pcm validates the ranges first; the clamping is the library's)."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().rced_gather_pcm(arena.data_ptr(), _lib.PCM_S16 if arena.dtype == torch.int16 else _lib.PCM_F32,
                                           int(arena.shape[0]), begins.data_ptr(), counts.data_ptr(), int(begins.shape[0]), L,
                                           out.data_ptr(), stride, 0, st))


def expected_rows(arena, begins, counts, L):
    """numpy: the header's contract, clamping included."""
    S = len(arena)
    out = np.zeros((len(begins), L), np.float32)
    for n, (b, c) in enumerate(zip(begins, counts)):
        b = min(max(int(b), 0), S)
        c = min(max(int(c), 0), L, S - b)
        row = arena[b:b + c]
        out[n, :c] = row.astype(np.float32) / np.float32(32768) if arena.dtype == np.int16 else row
    return out


def make_arena(dtype, size=40000, seed=5):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        a = rng.integers(-32768, 32768, size).astype(np.int16)
        a[:4] = [-32768, 32767, -1, 1]
        return a
    return rng.standard_normal(size).astype(np.float32)


# ---- 1. the gather, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["s16", "f32"])
def test_gather_bit_for_bit(built, dtype):
    """Every phase of the source (begin % 8 in 0..7: eight 16-byte phases of int16, two rounds of the four of float32),
    counts around one vector, one wave's worth and one column block (2048), L = count, count + 1, count + 9 and 2304 (two
    column blocks), a row stride wider than L (16-byte aligned rows and unaligned ones) whose columns past L must keep
    their sentinel, the same item in several rows, a row that ends at the arena's last sample, ranges that leave the arena
    at either end (clamped) -- all rows of a shape in one call."""
    import torch
    host = make_arena(dtype)
    S = len(host)
    arena = dev(host)
    checked = 0
    for count in COUNTS:
        for k, L in enumerate((count, count + 1, count + 9, 2304)):
            begins = [8 * (37 + 11 * p) + p for p in range(8)]       # phases 0..7 of distinct items
            counts = [count] * 8
            begins += [begins[3], begins[3], S - count, S - 5, -3, S + 10]     # twice the same item; ends at the end; clamped
            counts += [count, min(count, 3), count, min(L, 9), min(L, 6), min(L, 4)]
            counts += [L + 5, -2]                                     # a count past L, a negative one: clamped
            begins += [123, 456]
            stride = ((L + 3) // 4 * 4 + 4) if k % 2 == 0 else L + 5 + (L % 2 == 0)   # aligned rows / odd stride: unaligned rows
            n = len(begins)
            out = torch.full((n, stride), SENTINEL, dtype=torch.float32, device="cuda")
            raw_gather(arena, dev(begins, np.int64), dev(counts, np.int32), L, out, stride)
            got = out.cpu().numpy()
            want = expected_rows(host, begins, counts, L)
            assert np.array_equal(got[:, :L].view(np.uint32), want.view(np.uint32)), (count, L, stride)
            assert (got[:, L:] == SENTINEL).all(), (count, L, stride)
            checked += n
    print("gather %s: %d rows bit for bit" % (np.dtype(dtype).name, checked))


def test_gather_wrapper_validates(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib, audio, loader
    host = make_arena(np.int16, 5000)
    arena = dev(host)
    rows = audio.gather_pcm(arena, [3, 100], [10, 21])
    assert tuple(rows.shape) == (2, 24) and np.array_equal(rows.cpu().numpy(), expected_rows(host, [3, 100], [10, 21], 24))
    for begins, counts, L in (([4995], [10], None), ([-1], [4], None), ([0], [9], 8), ([0], [-1], 8)):
        with pytest.raises(ValueError):
            audio.gather_pcm(arena, begins, counts, L)
    with pytest.raises(ValueError):
        audio.gather_pcm(arena.double(), [0], [4])
    with pytest.raises(_lib.RcedError):
        raw_gather(arena, dev([0], np.int64), dev([4], np.int32), 8, torch.empty((1, 8), device="cuda"), 4)   # stride < L
    # the corpus: int16 in -> int16 arena, float in -> float32 arena, empty items raise
    c16 = loader.Corpus.from_arrays([host[:700], host[700:1000]])
    cf32 = loader.Corpus.from_arrays([host[:700] / 32768.0, (host[700:1000] / 32768.0).astype(np.float32)])
    assert c16.arena.dtype == torch.int16 and cf32.arena.dtype == torch.float32
    assert c16.offsets.tolist() == [0, 700] and c16.lengths.tolist() == [700, 300] and len(c16) == 2
    assert torch.equal(c16.gather([1, 0]), cf32.gather([1, 0]))       # / 32768 on the device = / 32768 on the host: exact
    assert torch.equal(c16.gather([0], [100], [50])[0, :50], dev(host[100:150].astype(np.float32) / 32768))
    with pytest.raises(ValueError):
        loader.Corpus.from_arrays([host[:10], host[:0]])
    with pytest.raises(ValueError):
        c16.gather([1], [250], [51])                                   # leaves the item, though not the arena


def test_corpus_from_manifest(built, tmp_path):
    import json
    import wave
    from fullycnnspeechenhancement_amd import loader
    host = make_arena(np.int16, 9000)
    sigs = [host[:4000], host[4000:9000]]
    with open(str(tmp_path / "m.json"), "w") as fh:
        for i, s in enumerate(sigs):
            p = str(tmp_path / ("u%d.wav" % i))
            w = wave.open(p, "wb")
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(8000)
            w.writeframes(s.tobytes())
            w.close()
            fh.write(json.dumps({"audio_filepath": p, "duration": len(s) / 8000.0}) + "\n")
    corpus = loader.Corpus.from_manifest(str(tmp_path / "m.json"), 8000)
    assert np.array_equal(corpus.arena.cpu().numpy(), host) and corpus.lengths.tolist() == [4000, 5000]


# ---- 2. every batch of the fixture -----------------------------------------------------------------------------------------

def fixture_loader(gold, c, **kw):
    from fullycnnspeechenhancement_amd import loader
    clean, noise = loader_np.signals(gold, "clean"), loader_np.signals(gold, "noise")
    clean_ids, noise_ids = gold["c%d_clean" % c].tolist(), gold["c%d_noise" % c].tolist()
    np.random.seed(int(gold["c%d_seed" % c]))
    ds = loader.DataSet(loader.Corpus.from_arrays([clean[i] for i in clean_ids]),
                        noise=loader.Corpus.from_arrays([noise[i] for i in noise_ids]), snr=0, **kw)
    bs = int(gold["c%d_batch_size" % c])
    return loader.DataLoader(ds, bs, sampler=loader.Sampler(ds, bs)), [len(clean[i]) for i in clean_ids]


@pytest.mark.parametrize("c", [0, 1])
def test_batches_match_the_reference(gold, c):
    from fullycnnspeechenhancement_amd.audio import num_frames
    dl, clean_len = fixture_loader(gold, c)
    worst = 0.0
    for e in range(2):
        dl.shuffle()
        b = -1
        for b, (batch_mix, batch_clean, mix_sig, clean_sig) in enumerate(dl):
            lens = clean_sig.lengths
            assert lens == [len(loader_np.signals(gold, "clean")[i]) for i in gold["c%d_ids_%d_%d" % (c, e, b)][:, 0]]
            assert len(mix_sig) == len(clean_sig) == len(lens) and tuple(mix_sig[0].shape) == (lens[0],)
            for got, key in ((batch_mix, "c%d_mix_%d_%d"), (batch_clean, "c%d_clean_%d_%d")):
                ref = gold[key % (c, e, b)].astype(np.float64)
                got = got.cpu().numpy()
                assert got.shape == ref.shape and got.dtype == np.float32
                err = np.abs(got - ref).max() / ref.max()
                worst = max(worst, err)
                assert err <= 2e-6, (key % (c, e, b), err)
                for i, n in enumerate(lens):
                    assert not got[i, num_frames(n):].any()          # frames past the utterance: exactly zero
        assert b + 1 == int(gold["c%d_batches" % c])
        assert np.random.random() == float(gold["c%d_next_%d" % (c, e)])
    print("device batches vs reference, case %d: worst %.3e of the scale (bar 2e-6)" % (c, worst))


# ---- 3. invariance, bit for bit --------------------------------------------------------------------------------------------

def test_rows_do_not_depend_on_offset_batch_or_neighbours(gold):
    import torch
    from fullycnnspeechenhancement_amd import audio, loader
    clean, noise = loader_np.signals(gold, "clean"), loader_np.signals(gold, "noise")
    pad = make_arena(np.int16, 64)

    def corpora(shift):
        """the same items behind `shift` extra samples: every offset moves through the 16-byte phases"""
        return (loader.Corpus.from_arrays([pad[:shift + 8]] + clean), loader.Corpus.from_arrays([pad[:shift + 8]] + noise))

    # utterance: clean 3 (901 samples) under noise 1 (450 samples, tiled: two gains) and under noise 0 (1500: cropped at 321)
    gains = np.asarray([0.7, 1.6])
    wanted = {}
    for shift in range(8):
        cc, nc = corpora(shift)
        ds = loader.DataSet(cc, noise=nc, snr=3)
        dl = loader.DataLoader(ds, 4)
        tiled, cropped = (1 + 3, 1 + 1, 0, gains), (1 + 3, 1 + 0, 321, np.zeros(0))
        other = [(1 + 4, 1 + 2, 0, np.asarray([1.1])), (1 + 0, 1 + 0, 77, np.zeros(0)), (1 + 2, 1 + 1, 0, np.asarray([0.4]))]
        plans = [[tiled], [cropped], [other[0], tiled, cropped], [cropped, other[1], other[2], tiled], [tiled, other[1]]]
        where = [(0, None), (None, 0), (1, 2), (3, 0), (0, None)]
        for plan, (it, ic) in zip(plans, where):
            batch_mix, batch_clean, mix_sig, clean_sig = dl.build(plan)
            t = audio.num_frames(901)
            for name, i in (("tiled", it), ("cropped", ic)):
                if i is None:
                    continue
                got = (batch_mix[i, :t].clone(), batch_clean[i, :t].clone(), mix_sig[i].clone(), clean_sig[i].clone())
                assert not batch_mix[i, t:].any() and not batch_clean[i, t:].any()
                if name not in wanted:
                    wanted[name] = got
                assert all(torch.equal(a, b) for a, b in zip(got, wanted[name])), (shift, len(plan), name)
    # the rows the gather wrote, fed to the existing entries directly
    cc, nc = corpora(5)
    speech = cc.gather([4])                                            # [1, 904]
    assert torch.equal(speech[0, :901], wanted["tiled"][3]) and not speech[0, 901:].any()
    for name, nrows, kw in (("tiled", nc.gather([2]), dict(noise_lengths=[450], gains=[gains])),
                            ("cropped", nc.gather([1], [321], [901]), dict(noise_lengths=[901]))):
        mix = audio.mix_snr_batch(speech, nrows, 3, speech_lengths=[901], **kw)
        assert torch.equal(mix[0, :901], wanted[name][2])
        mag, _ = audio.stft_batch(torch.cat([speech, mix]), [901, 901], with_phase=False)
        assert torch.equal(mag[1], wanted[name][0]) and torch.equal(mag[0], wanted[name][1])
    # and the cropped gather is the reference's crop: the whole noise with start = 321 gives the same mixture
    whole = audio.mix_snr_batch(speech, nc.gather([1]), 3, speech_lengths=[901], noise_lengths=[1500], starts=[321])
    assert torch.equal(whole[0, :901], wanted["cropped"][2])


# ---- 4. paired-corpus mode -------------------------------------------------------------------------------------------------

def test_paired_corpus_does_no_mixing(gold):
    import torch
    from fullycnnspeechenhancement_amd import audio, loader
    clean = loader_np.signals(gold, "clean")[:4]
    rng = np.random.default_rng(11)
    mixes = [np.clip(s.astype(np.int32) + rng.integers(-3000, 3000, len(s)), -32768, 32767).astype(np.int16) for s in clean]
    np.random.seed(3)
    ds = loader.DataSet(loader.Corpus.from_arrays(clean), mix=loader.Corpus.from_arrays(mixes))
    dl = loader.DataLoader(ds, 2, sampler=loader.Sampler(ds, 2))
    seen = 0
    for batch_mix, batch_clean, mix_sig, clean_sig in dl:
        ids = [[len(s) for s in clean].index(n) for n in clean_sig.lengths]    # the lengths are distinct
        for rows, sigs, batch in ((mix_sig, mixes, batch_mix), (clean_sig, clean, batch_clean)):
            width = max(clean_sig.lengths)
            host = np.zeros((len(ids), width), np.float32)
            for k, i in enumerate(ids):
                host[k, :len(sigs[i])] = sigs[i].astype(np.float32) / 32768
                assert torch.equal(rows[k], dev(host[k, :len(sigs[i])]))
            mag, _ = audio.stft_batch(dev(host), clean_sig.lengths, with_phase=False)
            assert torch.equal(batch, mag)
        seen += 1
    assert seen == len(dl) == 3
    with pytest.raises(ValueError):
        loader.DataSet(loader.Corpus.from_arrays(clean), mix=loader.Corpus.from_arrays(mixes[:3]))


# ---- 5. an epoch is the steps ------------------------------------------------------------------------------------------------

def test_train_is_the_steps(gold, tmp_path, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, loader, trainer as trainer_mod
    from oracle import rced_np
    clean, noise = loader_np.signals(gold, "clean")[:4], loader_np.signals(gold, "noise")
    w = rced_np.make_weights("FullyCNNV3", seed=42)
    cc, nc = loader.Corpus.from_arrays(clean), loader.Corpus.from_arrays(noise)

    def make_loader():
        np.random.seed(99)
        ds = loader.DataSet(cc, noise=nc, snr=5)
        return loader.DataLoader(ds, 2, sampler=loader.Sampler(ds, 2))

    class Recording(FullyCNNTrainer):
        def fit_step(self, x, y):
            out = FullyCNNTrainer.fit_step(self, x, y)
            self.losses.append(out[0])
            return out

    ckpts = str(tmp_path / "ckpts")
    a = Recording("FullyCNNV3", batch_size=2, lr=1e-3, weights=w)
    a.losses = []
    last = a.train(make_loader(), None, 2, checkpoints_path=ckpts, num_iter_print=2)
    assert "epoch: 1, batch: 2/3, TrainLoss: " in capsys.readouterr().out
    assert len(a.losses) == 6 and last == a.global_step == 6 and a.train_loss.count == a.batch_time.count == a.data_time.count == 6
    assert a.train_loss.val == a.losses[-1] and all(np.isfinite(a.losses))
    # the same batches drawn a second time after the same seed, stepped by hand
    b = FullyCNNTrainer("FullyCNNV3", batch_size=2, lr=1e-3, weights=w)
    dl, by_hand = make_loader(), []
    for _ in range(2):
        dl.shuffle()
        for batch_mix, batch_clean, _, _ in dl:
            by_hand.append(b.fit_step(batch_mix, batch_clean)[0])
    print("losses:", a.losses)
    assert a.losses == by_hand and b.global_step == 6
    va, vb = a.variables(), b.variables()
    assert sorted(va) == sorted(vb) and all(np.array_equal(va[k], vb[k]) for k in va)
    # one checkpoint per epoch, under the reference's name
    names = [trainer_mod.checkpoint_path(ckpts, "FullyCNN", "FullyCNNV3", e, 3 * (e + 1)) for e in range(2)]
    assert names[0].endswith(os.path.join("FullyCNN_FullyCNNV3", "FullyCNN_FullyCNNV3_0_2.ckpt"))
    assert sorted(f for f in os.listdir(os.path.dirname(names[0])) if f.endswith(".index")) == \
        [os.path.basename(n) + ".index" for n in names]
    # resuming from epoch 0's checkpoint runs epoch 1 only
    r = Recording.from_checkpoint(names[0], "FullyCNNV3", batch_size=2, lr=1e-3)
    r.losses = []
    assert r.global_step == 3 and r.continue_from == names[0]
    r.train(make_loader(), None, 2)
    assert len(r.losses) == 3 and r.global_step == 6
    r.losses = []
    r.train(make_loader(), None, 1)                                   # nothing left to do before epoch 1
    assert r.losses == []
    for t in (a, b, r):
        t.close()


# ---- 6. validation over the device loader ------------------------------------------------------------------------------------

def test_valid_over_the_device_loader(gold, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, loader
    from fullycnnspeechenhancement_amd.engine import evaluate_pcm
    from oracle import rced_np
    clean, noise = loader_np.signals(gold, "clean"), loader_np.signals(gold, "noise")
    cc, nc = loader.Corpus.from_arrays(clean), loader.Corpus.from_arrays(noise)
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=2, weights=rced_np.make_weights("FullyCNNV3", seed=42))

    def make_loader():
        np.random.seed(21)
        return loader.DataLoader(loader.DataSet(cc, noise=nc, snr=0, use_complex=True), 2)

    scores = []
    for batch_mix, batch_clean, mix_sig, clean_sig in make_loader():
        assert batch_mix is None and batch_clean is None
        den, sdr = evaluate_pcm(tr.valid_step, mix_sig, clean_sig)                    # the device rows, where they lie
        host_mix, host_clean = [m.cpu().numpy() for m in mix_sig], [c.cpu().numpy() for c in clean_sig]
        den_h, sdr_h = evaluate_pcm(tr.valid_step, host_mix, host_clean)               # host lists still work
        print("sdr device rows %s host lists %s" % (sdr, sdr_h))
        assert len(sdr) == len(clean_sig) and np.abs(sdr - sdr_h).max() <= 1e-9
        assert all(np.array_equal(x, y) for x, y in zip(den, den_h))
        scores.extend(sdr_h.tolist())
    avg = tr.valid(make_loader(), 4)
    assert tr.sdr_score.count == len(scores) == 5 and abs(avg - np.mean(scores)) <= 1e-9
    assert "Epoch: 4, Average sd_score: %.4f." % avg in capsys.readouterr().out
    tr.close()


# ---- 7. stream capture -------------------------------------------------------------------------------------------------------

def test_gather_replays_from_a_captured_graph(built):
    import torch
    host = make_arena(np.int16, 20000)
    arena = dev(host)
    begins_h, counts_h, L = [5, 4099, 9000, 19000], [2049, 300, 0, 1000], 2304
    begins, counts = dev(begins_h, np.int64), dev(counts_h, np.int32)
    out = torch.full((4, L), SENTINEL, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # one eager call first, as for the other entries: the library is loaded
        raw_gather(arena, begins, counts, L, out, L, stream=side.cuda_stream)
    side.synchronize()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        raw_gather(arena, begins, counts, L, out, L, stream=torch.cuda.current_stream().cuda_stream)
    arena.copy_(dev(host[::-1].copy()))                                 # the replay reads what is there when it runs
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), expected_rows(host[::-1], begins_h, counts_h, L))
    eager = torch.empty_like(out)
    raw_gather(arena, begins, counts, L, eager, L)
    assert torch.equal(out, eager)
