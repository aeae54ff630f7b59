"""CPU tests of the device loader's host half (loader.py: manifests, wav headers, the corpus index, DataSet / Sampler /
DataLoader order) against REAL reference outputs (tests/golden/loader_ref.npz: the reference's own DataSet + Sampler +
DataLoader(num_works=1) run for two epochs), of the float64 restatement the GPU tests use (tests/loader_np.py), and of the
checkpoint naming of FullyCNNTrainer.train."""

import json
import os
import wave

import numpy as np
import pytest

import loader_np


@pytest.fixture(scope="module")
def gold():
    return loader_np.load_fixture()


def case_dataset(gold, c):
    """DataSet / Sampler / DataLoader over host indices for case c, built right after the case's seed as the fixture's
    generator does; returns (loader, clean ids, noise ids) -- corpus position -> fixture signal id."""
    from fullycnnspeechenhancement_amd import loader
    clean_ids, noise_ids = gold["c%d_clean" % c].tolist(), gold["c%d_noise" % c].tolist()
    clean, noise = loader_np.signals(gold, "clean"), loader_np.signals(gold, "noise")
    np.random.seed(int(gold["c%d_seed" % c]))
    ds = loader.DataSet(loader.CorpusIndex([len(clean[i]) for i in clean_ids]),
                        noise=loader.CorpusIndex([len(noise[i]) for i in noise_ids]))
    bs = int(gold["c%d_batch_size" % c])
    return loader.DataLoader(ds, bs, sampler=loader.Sampler(ds, bs)), clean_ids, noise_ids


def epochs_of(gold, c):
    e = 0
    while "c%d_next_%d" % (c, e) in gold:
        e += 1
    return e


@pytest.mark.parametrize("c", [0, 1])
def test_order_and_random_stream_equal_the_reference(gold, c):
    dl, clean_ids, noise_ids = case_dataset(gold, c)
    nb = int(gold["c%d_batches" % c])
    assert len(dl) == nb
    if c == 1:          # 4 items, batch 2: the sampler appends a whole extra batch
        assert len(clean_ids) % dl.batch_size == 0 and nb == len(clean_ids) // dl.batch_size + 1
    for e in range(epochs_of(gold, c)):
        dl.shuffle()
        plans = list(dl.plans())
        assert len(plans) == nb
        for b, plan in enumerate(plans):
            ids = [(clean_ids[p[0]], noise_ids[p[1]]) for p in plan]
            assert ids == [tuple(r) for r in gold["c%d_ids_%d_%d" % (c, e, b)].tolist()], (e, b)
        assert np.random.random() == float(gold["c%d_next_%d" % (c, e)]), e


def test_short_noise_list_raises_index_error_like_the_reference(gold):
    from fullycnnspeechenhancement_amd import loader
    assert int(gold["short_noise_raises"]) == 1          # the reference did, for 8 items / 3 noises / batch 4
    for items, noises, bs in ((8, 3, 4), (10, 10, 4)):
        np.random.seed(7)
        ds = loader.DataSet(loader.CorpusIndex([400] * items), noise=loader.CorpusIndex([300] * noises))
        dl = loader.DataLoader(ds, bs, sampler=loader.Sampler(ds, bs))
        with pytest.raises(IndexError):
            for _ in dl.plans():
                pass


def test_sampler_without_drop_last_only(gold):
    from fullycnnspeechenhancement_amd import loader
    ds = loader.DataSet(loader.CorpusIndex([400] * 5), noise=loader.CorpusIndex([300] * 9))
    with pytest.raises(NotImplementedError):
        loader.Sampler(ds, 2, drop_last=True)
    assert ds.item_list == list(range(5))
    dl = loader.DataLoader(ds, 2)                         # no sampler: bins in order, the last one short
    assert dl.bins == [[0, 1], [2, 3], [4]] and len(dl) == 3
    with pytest.raises(ValueError):
        loader.DataSet(loader.CorpusIndex([400]))          # neither noise nor mix
    with pytest.raises(ValueError):
        loader.CorpusIndex([400, 0])                       # an empty item


@pytest.mark.parametrize("c", [0, 1])
def test_restatement_reproduces_the_reference_batches(gold, c):
    """tests/loader_np.py (gather / 32768, closed-form mix rounded to float32, oracle STFT, zero padding) against the
    batch_mix / batch_clean the reference yielded: within 2e-6 of the scale, the suite's STFT bar (tests/test_audio_gpu.py);
    the float32 rounding of the mixture moves the reference's own magnitudes by < 1e-7 of the scale."""
    dl, clean_ids, noise_ids = case_dataset(gold, c)
    clean, noise = loader_np.signals(gold, "clean"), loader_np.signals(gold, "noise")
    ca, co, cl = loader_np.arena_of([clean[i] for i in clean_ids])
    na, no, nl = loader_np.arena_of([noise[i] for i in noise_ids])
    worst = 0.0
    for e in range(epochs_of(gold, c)):
        dl.shuffle()
        for b, plan in enumerate(dl.plans()):
            mix, cln, _, _ = loader_np.build_batch(ca, (co, cl), na, (no, nl), plan, 0)
            for got, key in ((mix, "c%d_mix_%d_%d"), (cln, "c%d_clean_%d_%d")):
                ref = gold[key % (c, e, b)].astype(np.float64)
                assert got.shape == ref.shape
                err = np.abs(got - ref).max() / np.abs(ref).max()
                worst = max(worst, err)
                assert err <= 2e-6, (key % (c, e, b), err)
        assert np.random.random() == float(gold["c%d_next_%d" % (c, e)])
    print("restatement vs reference, case %d: worst %.3e of the scale" % (c, worst))


def write_wav(path, samples, rate=8000, channels=1, width=2):
    w = wave.open(str(path), "wb")
    w.setnchannels(channels)
    w.setsampwidth(width)
    w.setframerate(rate)
    w.writeframes(np.asarray(samples).tobytes())
    w.close()
    return str(path)


def test_manifest_index_and_wav_checks(tmp_path):
    from fullycnnspeechenhancement_amd import loader
    rng = np.random.default_rng(3)
    lengths = [4000, 1600, 5200, 3300]                                    # 0.5 s, 0.2 s, 0.65 s, 0.4125 s at 8 kHz
    sigs = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lengths]
    paths = [write_wav(tmp_path / ("u%d.wav" % i), s) for i, s in enumerate(sigs)]
    manifest = tmp_path / "m.json"
    with open(str(manifest), "w") as fh:
        for p, n in zip(paths, lengths):
            fh.write(json.dumps({"audio_filepath": p, "duration": n / 8000.0, "text": "x"}) + "\n")
    # the reference's duration filter (data_loader.py:105): min 0.4 s drops the second file
    idx = loader.CorpusIndex.from_manifest(str(manifest), 8000)
    assert idx.paths == [paths[0], paths[2], paths[3]]
    assert idx.lengths.tolist() == [4000, 5200, 3300] and idx.offsets.tolist() == [0, 4000, 9200] and idx.total == 12500
    assert len(loader.CorpusIndex.from_manifest(str(manifest), 8000, min_duration=0.0)) == 4
    assert loader.CorpusIndex.from_manifest(str(manifest), 8000, max_duration=0.5).lengths.tolist() == [4000, 3300]
    assert [d["audio_filepath"] for d in loader.read_manifest(str(manifest), 0.0, 0.45)] == [paths[1], paths[3]]
    for p, s in zip(paths, sigs):
        assert loader.wav_length(p, 8000) == len(s)
        got = loader.read_wav(p, 8000)
        assert got.dtype == np.int16 and np.array_equal(got, s)
    # a paired manifest picks its field by key
    paired = tmp_path / "p.json"
    with open(str(paired), "w") as fh:
        fh.write(json.dumps({"clean_audio_filepath": paths[0], "mix_audio_filepath": paths[2], "duration": 0.5}) + "\n")
    assert loader.CorpusIndex.from_manifest(str(paired), 8000, key="mix_audio_filepath").lengths.tolist() == [5200]
    # anything but mono PCM16 at the corpus rate raises
    bad = [write_wav(tmp_path / "stereo.wav", np.zeros(8000, np.int16), channels=2),
           write_wav(tmp_path / "u8.wav", np.zeros(4000, np.uint8), width=1),
           write_wav(tmp_path / "rate.wav", np.zeros(8000, np.int16), rate=16000)]
    for p in bad:
        with pytest.raises(ValueError):
            loader.wav_length(p, 8000)
        with pytest.raises(ValueError):
            loader.read_wav(p, 8000)
        m = tmp_path / "bad.json"
        with open(str(m), "w") as fh:
            fh.write(json.dumps({"audio_filepath": p, "duration": 1.0}) + "\n")
        with pytest.raises(ValueError):
            loader.CorpusIndex.from_manifest(str(m), 8000)
    with open(str(tmp_path / "broken.json"), "w") as fh:
        fh.write("{not json\n")
    with pytest.raises(IOError):
        loader.read_manifest(str(tmp_path / "broken.json"))


def test_checkpoint_name_and_start_epoch():
    from fullycnnspeechenhancement_amd import trainer
    path = trainer.checkpoint_path("ckpts", "FullyCNN", "FullyCNNV3", 7, 1201)
    assert path == os.path.join("ckpts/FullyCNN_FullyCNNV3", "FullyCNN_FullyCNNV3_7_1200.ckpt")     # trainer.py:232-238
    assert trainer.start_epoch(path) == 8 and trainer.start_epoch(None) == 0                         # trainer.py:198-201
    assert trainer.start_epoch(trainer.checkpoint_path("/a_b/c", "FullyCNN", "FullyCNN", 0, 3)) == 1
