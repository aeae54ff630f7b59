"""Generates tests/golden/loader_ref.npz from the REFERENCE'S OWN loader (data_utils/data_loader.py): DataSet + Sampler +
DataLoader(num_works=1), two epochs with shuffle() before each, over a tiny corpus of seeded int16 signals.  Nothing of
the reference's source is copied: the script imports it from the reference checkout named on the command line, feeds
seeded signals through temporary manifests and stores data only.

The one replacement: DataSet.load_audio (librosa) becomes a lookup that returns the stored int16 signal / 32768 WIDENED TO
FLOAT64 (the project's convention, make_golden_eval.py), so every stored spectrogram is the float64 answer for exactly
representable inputs.  The lookup also records which files each batch asked for: the (clean id, noise id) pairs.

Environment shims as in make_golden_eval.py (np.mat alias; empty stand-ins for librosa / pypesq / pystoi; joblib, which the
reference's DataLoader calls, gets a sequential stand-in only where it is absent -- with n_jobs=1 joblib runs the calls in
order in this process, which is what the stand-in does).

Stored: clean_<i>, noise_<i> (int16); per case c (c0: 5 clean, 3 noise, batch 2; c1: 4 clean -- a multiple of the batch
size, the sampler's extra-batch quirk --, 3 noise, batch 2): c<c>_seed, c<c>_clean / c<c>_noise (corpus ids), c<c>_batches
(batches per epoch), and per epoch e and batch b c<c>_ids_<e>_<b> ([N, 2] int32: clean id, noise id, in batch order),
c<c>_mix_<e>_<b> / c<c>_clean_<e>_<b> (batch_mix / batch_clean as yielded, [N, T, 129, 1], cast to float32: a rounding of
6e-8 relative, against the suite's STFT bar of 2e-6 of the scale), c<c>_next_<e> (np.random.random() right after the epoch:
where the reference leaves the stream; the draw is part of the sequence, a replay must make it too).
short_noise_raises: 1 if the reference raised IndexError for 8 items / 3 noises / batch 4 (its noise list, replicated to
9, is shorter than the item list the sampler extended to 12).

Run from the repo root:  python tests/golden/make_golden_loader.py <path to the reference checkout>
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SR = 8000
CLEAN_LENGTHS = [300, 517, 640, 901, 1100]
NOISE_LENGTHS = [1500, 450, 777]          # longer than every speech; shorter than most; in between
CASES = [(101, [0, 1, 2, 3, 4], [0, 1, 2], 2), (202, [0, 1, 2, 3], [0, 1, 2], 2)]
EPOCHS = 2


def signals():
    rng = np.random.default_rng(2026)
    clean = []
    for i, n in enumerate(CLEAN_LENGTHS):
        t = np.arange(n) / SR
        x = 0.3 * np.sin(2 * np.pi * (180 + 70 * i) * t) * (1 + 0.5 * np.sin(2 * np.pi * 5 * t)) + 0.02 * rng.standard_normal(n)
        clean.append(np.round(x * 32768).astype(np.int16))
    noise = [np.round(0.1 * rng.standard_normal(n) * 32768).astype(np.int16) for n in NOISE_LENGTHS]
    return clean, noise


def write_manifest(path, names):
    with open(path, "w") as fh:
        for name in names:
            fh.write(json.dumps({"audio_filepath": name, "duration": 1.0}) + "\n")


def main():
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix
    for name, attrs in (("librosa", ()), ("pypesq", ("pesq",)), ("pystoi", ("stoi",))):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, None)
            sys.modules[name] = m
    try:
        __import__("joblib")
    except ImportError:
        m = types.ModuleType("joblib")
        m.delayed = lambda f: (lambda *a, **k: (f, a, k))
        m.Parallel = lambda n_jobs=1: (lambda calls: [f(*a, **k) for f, a, k in calls])
        sys.modules["joblib"] = m
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from data_utils import data_loader as ref

    clean, noise = signals()
    table = {"clean_%d" % i: s for i, s in enumerate(clean)}
    table.update({"noise_%d" % i: s for i, s in enumerate(noise)})
    asked = []

    def load_audio(self, audio_filepath):
        asked.append(audio_filepath)
        return table[audio_filepath].astype(np.float64) / 32768.0, SR

    ref.DataSet.load_audio = load_audio
    out = dict(table)
    tmp = tempfile.mkdtemp()

    def dataset(clean_ids, noise_ids):
        cm, nm = os.path.join(tmp, "clean.json"), os.path.join(tmp, "noise.json")
        write_manifest(cm, ["clean_%d" % i for i in clean_ids])
        write_manifest(nm, ["noise_%d" % i for i in noise_ids])
        return ref.DataSet(cm, nm, sample_rate=SR, window_ms=32, stride_ms=16, snr=0)

    for c, (seed, clean_ids, noise_ids, batch_size) in enumerate(CASES):
        np.random.seed(seed)
        ds = dataset(clean_ids, noise_ids)
        sampler = ref.Sampler(ds, batch_size)
        loader = ref.DataLoader(ds, batch_size, sampler=sampler, num_works=1)
        out["c%d_seed" % c] = np.asarray(seed, np.int64)
        out["c%d_clean" % c], out["c%d_noise" % c] = np.asarray(clean_ids, np.int32), np.asarray(noise_ids, np.int32)
        out["c%d_batch_size" % c] = np.asarray(batch_size, np.int32)
        out["c%d_batches" % c] = np.asarray(len(loader), np.int32)
        for e in range(EPOCHS):
            loader.shuffle()
            b = 0
            for batch_mix, batch_clean, mix_sig, clean_sig in loader:
                ids = [(int(asked[k].split("_")[1]), int(asked[k + 1].split("_")[1])) for k in range(0, len(asked), 2)]
                assert all(asked[k].startswith("clean") and asked[k + 1].startswith("noise") for k in range(0, len(asked), 2))
                assert len(ids) == len(clean_sig) == batch_mix.shape[0]
                del asked[:]
                out["c%d_ids_%d_%d" % (c, e, b)] = np.asarray(ids, np.int32)
                out["c%d_mix_%d_%d" % (c, e, b)] = np.asarray(batch_mix, np.float32)
                out["c%d_clean_%d_%d" % (c, e, b)] = np.asarray(batch_clean, np.float32)
                print("case %d epoch %d batch %d ids %s shape %s" % (c, e, b, ids, batch_mix.shape))
                b += 1
            assert b == len(loader)
            out["c%d_next_%d" % (c, e)] = np.asarray(np.random.random(), np.float64)

    # the short-noise case: 8 items, 3 noises, batch 4
    np.random.seed(7)
    ds = dataset([0, 1, 2, 3, 4, 0, 1, 2], [0, 1, 2])
    loader = ref.DataLoader(ds, 4, sampler=ref.Sampler(ds, 4), num_works=1)
    try:
        for _ in loader:
            pass
        raised = 0
    except IndexError:
        raised = 1
    out["short_noise_raises"] = np.asarray(raised, np.int32)
    print("8 items / 3 noises / batch 4 raises IndexError:", bool(raised))

    path = os.path.join(HERE, "loader_ref.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
