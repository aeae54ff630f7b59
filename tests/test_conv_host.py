"""CPU tests of the reverberation path: the float64 restatement of the ragged FIR (tests/conv_np.py) against a literal double
loop and scipy, the C entry's refusals (made before any device work, so they need no GPU), the loader's plans and draw
order with and without rir=, RirCorpus on an index-only build, and synthetic_rirs."""

import ctypes
import inspect
import os
import warnings

import numpy as np
import pytest

import conv_np
from conftest import ROOT


def state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- the restatement -------------------------------------------------------------------------------------------------------

def test_restatement_is_the_double_loop_bit_for_bit():
    rng = np.random.default_rng(1)
    checked = 0
    for length in (0, 1, 2, 7, 16, 33):
        for taps in (1, 2, 5, 17, 40):
            x = rng.standard_normal(length + 3).astype(np.float32)
            h = rng.standard_normal(taps).astype(np.float32)
            for d in sorted({0, 1 % taps, taps // 2, taps - 1}):
                ref, bound = conv_np.convolve_ref(x, h, d, length)
                loop = conv_np.convolve_loop(x, h, d, length)
                assert ref.shape == loop.shape == bound.shape == (length,)
                # bit for bit where every sum is exact (small integers), whatever order np.convolve takes; within the
                # accumulation bound on the Gaussian values
                xi, hi = np.rint(8 * x), np.rint(8 * h)
                assert np.array_equal(conv_np.convolve_ref(xi, hi, d, length)[0], conv_np.convolve_loop(xi, hi, d, length))
                assert np.all(np.abs(ref - loop) <= taps * 2.0 ** -52 * bound)
                assert np.all(bound >= np.abs(ref))
                checked += 1
    assert checked > 50
    assert np.array_equal(conv_np.convolve_ref([1.0, 2.0, 3.0], [], 0, 3)[0], np.zeros(3))


def test_restatement_against_fftconvolve_at_full_size():
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(2)
    x = rng.standard_normal(9000).astype(np.float32)
    h = (rng.standard_normal(8192) * np.exp(-np.arange(8192) / 1500.0)).astype(np.float32)
    for d in (0, 4096, 8191):
        ref, _ = conv_np.convolve_ref(x, h, d, 9000)
        fft = fftconvolve(x.astype(np.float64), h.astype(np.float64))[d:d + 9000]
        err = np.abs(ref - fft).max() / np.abs(ref).max()
        print("shift %d: restatement vs fftconvolve %.3e of the scale" % (d, err))
        assert err <= 1e-12


# ---- the C entry -------------------------------------------------------------------------------------------------------------

def test_symbol_and_python_surface(built):
    import fullycnnspeechenhancement_amd as pkg
    from fullycnnspeechenhancement_amd import _lib, evaluation
    assert len(_lib.SYMBOLS["rced_convolve"][1]) == 13
    assert pkg.audio.convolve_batch is evaluation.convolve_batch and pkg.audio.CONV_MAX_TAPS == conv_np.MAX_TAPS == 8192
    sig = inspect.signature(pkg.audio.convolve_batch).parameters
    assert list(sig) == ["signal", "filters", "lengths", "filter_lengths", "shifts", "out"]
    assert all(sig[k].default is None for k in list(sig)[2:])
    header = open(os.path.join(ROOT, "include", "rced.h")).read()
    assert "#define RCED_CONV_MAX_TAPS 8192" in header
    with pytest.raises(ValueError):
        pkg.audio.convolve_batch(np.zeros((1, 4), np.float32), np.zeros((1, 1), np.float32))     # host arrays: refused


def test_symbol_refuses_bad_arguments(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    ARG = _lib.RCED_ERR_ARG

    def call(x=p, xs=8, xl=None, h=p, hs=4, hl=None, sh=None, N=1, L=8, y=p, ys=8):
        return lib.rced_convolve(x, xs, xl, h, hs, hl, sh, N, L, y, ys, 0, None)

    for kw, word in ((dict(x=None), b"x_dev"), (dict(h=None), b"h_dev"), (dict(y=None), b"y_dev"),
                     (dict(xs=-8), b"x_stride"), (dict(hs=-1), b"h_stride"), (dict(ys=-8), b"y_stride"),
                     (dict(L=9), b"x_stride"), (dict(xs=16, L=9), b"y_stride"),
                     (dict(hs=8193), b"h_stride"), (dict(N=-1), b"N"), (dict(N=65536), b"N"), (dict(L=-1), b"L")):
        assert call(**kw) == ARG, kw
        assert word in lib.rced_last_error(), (kw, lib.rced_last_error())
        assert call(N=0, **{k: v for k, v in kw.items() if k != "N"}) == (ARG if "N" not in kw else 0)   # checked before N = 0 passes
    assert call(N=0) == 0 and call(N=0, hs=8192) == 0
    assert call(N=0, hs=9000, hl=p) == 0                  # with filter lengths the stride may be wider than the bound


# ---- the loader's plans ----------------------------------------------------------------------------------------------------

CLEAN_LEN = [1200, 300, 2000, 777, 1500]
NOISE_LEN = [500, 4000]


def index_only():
    from fullycnnspeechenhancement_amd import loader
    return loader.CorpusIndex(CLEAN_LEN), loader.CorpusIndex(NOISE_LEN)


def rir_index(count=3):
    from fullycnnspeechenhancement_amd import loader
    return loader.RirCorpus.from_arrays(loader.synthetic_rirs(count, rt60=(0.01, 0.08), seed=4), index_only=True)


def same_plan(got, want):
    assert len(got) == len(want) and tuple(got[:3]) == tuple(want[:3]) and got[4:] == want[4:]
    gains = np.asarray(want[3], np.float64)
    assert np.array_equal(got[3], gains[:len(got[3])]) and got[3].dtype == np.float64


def test_without_rir_nothing_changes(built):
    from fullycnnspeechenhancement_amd import loader
    cc, nc = index_only()
    np.random.seed(17)
    ds = loader.DataSet(cc, noise=nc, snr=0)
    assert ds.rir is None and list(inspect.signature(loader.DataSet).parameters)[6:] == ["rir", "rir_prob", "target", "early_ms"]
    noise_list = [0, 1, 0, 1, 0, 1]
    got = [ds.plan(i) for i in range(5)]
    after = np.random.get_state()
    np.random.seed(17)
    want = [conv_np.plan(i, noise_list[i], CLEAN_LEN, NOISE_LEN) for i in range(5)]
    assert state_equal(after, np.random.get_state())
    for g, w in zip(got, want):
        assert len(g) == 4
        same_plan(g, w)
    # an epoch of the loader, sampler included: the parent's behaviour restated -- Sampler's permutation, then per bin its shuffle
    # and add_noise's draws item by item
    np.random.seed(23)
    ds = loader.DataSet(cc, noise=nc, snr=0)
    dl = loader.DataLoader(ds, 2, sampler=loader.Sampler(ds, 2))
    dl.shuffle()
    got = list(dl.plans())
    after = np.random.get_state()
    np.random.seed(23)
    items = list(range(5))
    items.extend(items[-1:])                                        # (5 // 2 + 1) * 2 - 5 = 1
    bins = [[0, 1], [2, 3], [4, 5]]
    order = np.random.permutation(3).tolist()
    np.random.shuffle(items)
    want = []
    for b in order:
        np.random.shuffle(bins[b])
        want.append([conv_np.plan(items[i], noise_list[i], CLEAN_LEN, NOISE_LEN) for i in bins[b]])
    assert state_equal(after, np.random.get_state())
    assert len(got) == 3
    for gb, wb in zip(got, want):
        assert len(gb) == len(wb) == 2
        for g, w in zip(gb, wb):
            assert len(g) == 4
            same_plan(g, w)


@pytest.mark.parametrize("prob", [0.0, 0.5, 1.0])
def test_with_rir_the_draws_come_first(built, prob):
    from fullycnnspeechenhancement_amd import loader
    cc, nc = index_only()
    rc = rir_index()
    np.random.seed(31)
    ds = loader.DataSet(cc, noise=nc, snr=0, rir=rc, rir_prob=prob)
    dl = loader.DataLoader(ds, 2)
    got = [p for batch in dl.plans() for p in batch]
    after = np.random.get_state()
    np.random.seed(31)
    noise_list = [0, 1, 0, 1, 0, 1]
    want = [conv_np.plan(i, noise_list[i], CLEAN_LEN, NOISE_LEN, len(rc), prob) for i in range(5)]
    assert state_equal(after, np.random.get_state())
    for g, w in zip(got, want):
        assert len(g) == 5 and (g[4] is None or (type(g[4]) is int and 0 <= g[4] < 3))
        same_plan(g, w)
    rids = [g[4] for g in got]
    assert (prob != 0.0 or rids == [None] * 5) and (prob != 1.0 or None not in rids)
    # the noise draws are those of the same seed without rir=, two draws later per item
    if prob == 0.5:
        np.random.seed(31)
        for i, g in enumerate(got):
            np.random.uniform(0, 1), np.random.randint(0, 3)
            same_plan(g[:4], conv_np.plan(i, noise_list[i], CLEAN_LEN, NOISE_LEN))


def test_dataset_refusals(built):
    from fullycnnspeechenhancement_amd import loader
    cc, nc = index_only()
    rc = rir_index()
    with pytest.raises(ValueError, match="mix="):
        loader.DataSet(cc, mix=loader.CorpusIndex(CLEAN_LEN), rir=rc)
    with pytest.raises(ValueError, match="target"):
        loader.DataSet(cc, noise=nc, rir=rc, target="wet")
    with pytest.raises(ValueError, match="target"):
        loader.DataSet(cc, noise=nc, target=None)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="rir_prob"):
            loader.DataSet(cc, noise=nc, rir=rc, rir_prob=bad)
    for target in ("reverberant", "early", "dry"):
        assert loader.DataSet(cc, noise=nc, rir=rc, target=target, rir_prob=1).target == target
    with pytest.raises(ValueError, match="index-only"):
        rc.filters([0])


# ---- RirCorpus, synthetic_rirs ---------------------------------------------------------------------------------------------

def test_rir_corpus_direct_normalisation_truncation(built):
    from fullycnnspeechenhancement_amd import loader
    a = np.float32([0.0, 0.1, -0.5, 0.5, 0.25])                     # first of the two maxima of |h|: index 2, negative
    b = np.int16([100, 16384, -200])
    rc = loader.RirCorpus.from_arrays([a, b], index_only=True)
    assert rc.direct.tolist() == [2, 1] and rc.direct.dtype == np.int64 and rc.lengths.tolist() == [5, 3] and len(rc) == 2
    assert rc.arena is None and rc.sample_rate == 8000
    rows, direct = loader.RirCorpus.prepare([a, b])
    assert rows[0].dtype == rows[1].dtype == np.float32 and direct.tolist() == [2, 1]
    assert rows[0][2] == 1.0 and rows[1][1] == 1.0                    # exactly +1
    assert np.array_equal(rows[0], (a.astype(np.float64) / -0.5).astype(np.float32))
    assert np.array_equal(rows[1], (b.astype(np.float32) / np.float32(32768)).astype(np.float64) / 0.5)
    raw, _ = loader.RirCorpus.prepare([a, b], normalize=False)
    assert np.array_equal(raw[0], a) and np.array_equal(raw[1], b.astype(np.float32) / np.float32(32768))
    assert rc.early_taps(0, 50.0) == 5 and rc.early_taps(0, 0.125) == 4 and rc.early_taps(1, 0.0) == 2
    assert rc.early_taps(0, 0.25) == conv_np.early_taps(5, 2, 0.25, 8000) == 5
    long = np.zeros(9000, np.float32)
    long[[10, 8500]] = 0.5, 2.0                                     # the larger peak lies behind the cut
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        cut = loader.RirCorpus.from_arrays([a, long, long[:8192], long], index_only=True)
    assert len(seen) == 1 and "2 of 4" in str(seen[0].message) and "8192" in str(seen[0].message)
    assert cut.lengths.tolist() == [5, 8192, 8192, 8192] and cut.direct.tolist() == [2, 10, 10, 10]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loader.RirCorpus.from_arrays([a, long[:8192]], index_only=True)            # nothing to cut: no warning
    for bad in ([np.zeros(4, np.float32)], [np.zeros((2, 2), np.float32)], [np.zeros(0, np.float32)], [np.float32([1, np.inf])]):
        with pytest.raises(ValueError):
            loader.RirCorpus.from_arrays(bad, index_only=True)


def test_rir_corpus_from_manifest_index_only(built, tmp_path):
    import json
    import wave
    from fullycnnspeechenhancement_amd import loader
    sigs = [np.int16([0, 0, 20000, -5000, 300]), np.int16([-30000, 1000])]
    with open(str(tmp_path / "m.json"), "w") as fh:
        for i, s in enumerate(sigs):
            p = str(tmp_path / ("h%d.wav" % i))
            w = wave.open(p, "wb")
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(8000)
            w.writeframes(s.tobytes())
            w.close()
            fh.write(json.dumps({"audio_filepath": p, "duration": len(s) / 8000.0}) + "\n")
    rc = loader.RirCorpus.from_manifest(str(tmp_path / "m.json"), 8000, index_only=True)
    assert rc.direct.tolist() == [2, 0] and rc.lengths.tolist() == [5, 2] and rc.sample_rate == 8000
    with pytest.raises(ValueError):
        loader.RirCorpus.from_manifest(str(tmp_path / "m.json"), 16000, index_only=True)      # the files are at 8 kHz


def test_synthetic_rirs_are_seeded_and_leave_np_random_alone(built):
    from fullycnnspeechenhancement_amd import loader
    np.random.seed(5)
    before = np.random.get_state()
    a = loader.synthetic_rirs(4, seed=3)
    b = loader.synthetic_rirs(4, seed=3)
    c = loader.synthetic_rirs(4, seed=4)
    assert state_equal(before, np.random.get_state())
    assert len(a) == 4 and all(x.dtype == np.float32 and x.ndim == 1 for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not all(x.size == y.size and np.array_equal(x, y) for x, y in zip(a, c))
    for h in a:
        d = int(np.argmax(np.abs(h)))
        assert h[d] == 1.0 and not h[:d].any() and d <= 32 and 0.2 * 8000 <= h.size - d - 1 <= 0.8 * 8000
        tail = np.abs(h[d + 1:])
        assert tail.max() < 1.0 and tail[-50:].max() <= 2e-3           # about -60 dB of sigma 0.3, clipped at 0.9
    assert [h.size for h in loader.synthetic_rirs(2, sample_rate=16000, rt60=(2.0, 2.0))] == [8192, 8192]     # capped at the bound
    assert "not a room simulator" in " ".join(loader.synthetic_rirs.__doc__.lower().split())
    assert loader.synthetic_rirs(0) == []
