"""GPU tests of the sample-rate conversion (rced_resample) against the float64 restatement in
tests/resample_np.py, which tests/test_resample_host.py pins to scipy.

The parity bound is derived, not measured: for float32 output |gpu - ref| <= 2^-24 |ref| + 1e-10 max|x|.  The device rounds
a float64 sum once (2^-24 |ref|); that sum's own error is at most 1,538 terms * 2^-53 * sum|w| * max|x| ~ 4e-13 max|x| (769 taps
with sum|w| ~ 2 the worst case), the two Bessel evaluations differ at 1e-14: 1e-10 leaves 250 times that.  Every figure is
printed before it is asserted."""

import json
import wave

import numpy as np
import pytest

import resample_np as R

pytestmark = pytest.mark.gpu

CASES = {
    (16000, 8000): (1, 2, 5, 254, 255, 256, 257, 1000, 4099),
    (48000, 8000): (1, 5, 6, 7, 768, 769, 770, 4801),
    (44100, 8000): (1, 441, 442, 4410, 9001),
    (8000, 16000): (1, 64, 65, 1501),
}
KINDS = ("s16", "s16x2", "f32")
S16_GUARD = 32767          # what lies around every int16 range: read by mistake it moves a sample by up to 1


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.asarray(a, dtype) if dtype else a, device="cuda")


def make_source(kind, counts, seed):
    """(arena [frames, channels], begins, channels): every range starts at an odd frame and has guards on both sides: NaN in
    float32, full scale in int16."""
    rng = np.random.RandomState(seed)
    channels = 2 if kind == "s16x2" else 1
    gaps = [3 + 2 * (i % 3) for i in range(len(counts) + 1)]
    begins, at = [], 0
    for g, c in zip(gaps, counts):
        at += g
        at += (at + 1) % 2                      # odd
        begins.append(at)
        at += c
    frames = at + gaps[-1]
    if kind == "f32":
        arena = np.full((frames, 1), np.nan, np.float32)
        for b, c in zip(begins, counts):
            arena[b:b + c, 0] = rng.uniform(-1, 1, c).astype(np.float32)
    else:
        arena = np.full((frames, channels), S16_GUARD, np.int16)
        for b, c in zip(begins, counts):
            arena[b:b + c] = rng.randint(-32768, 32768, (c, channels)).astype(np.int16)
    return arena, begins, channels


_refs = {}


def reference(kind, ratio):
    """The source of a (kind, ratio) and the restatement of every row, computed once and never written to."""
    key = (kind, ratio)
    if key not in _refs:
        counts = CASES[ratio]
        arena, begins, channels = make_source(kind, counts, seed=ratio[0] // 100 + len(kind))
        rows = [R.resample(arena[b:b + c] if channels > 1 else arena[b:b + c, 0], *ratio) for b, c in zip(begins, counts)]
        xmax = [float(np.abs(R.to_mono(arena[b:b + c])).max()) for b, c in zip(begins, counts)]
        _refs[key] = (arena, begins, channels, rows, xmax)
    return _refs[key]


def check_rows(got, rows, xmax, what):
    worst = 0.0
    for n, (ref, xm) in enumerate(zip(rows, xmax)):
        y = got[n, :ref.size].astype(np.float64)
        assert np.isfinite(y).all(), "%s row %d: a guard was read" % (what, n)
        bound = 2.0 ** -24 * np.abs(ref) + 1e-10 * xm
        over = (np.abs(y - ref) / bound).max() if ref.size else 0.0
        worst = max(worst, over)
        assert over <= 1.0, "%s row %d: error %.3f of the bound" % (what, n, over)
    print("%s: worst error %.3f of the bound" % (what, worst))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ratio", sorted(CASES), ids=lambda r: "%d-%d" % r)
def test_ragged_rows_against_the_restatement(built, ratio, kind):
    """All counts of a ratio as the rows of one call, L = the longest output and 9 more, in a buffer 5 columns wider than L
    whose columns past L hold NaN: the padding is exactly 0 and the NaNs stay."""
    import torch
    from fullycnnspeechenhancement_amd import audio
    arena, begins, channels, rows, xmax = reference(kind, ratio)
    counts = CASES[ratio]
    src = dev(arena)
    longest = max(r.size for r in rows)
    assert [r.size for r in rows] == [R.length(c, *ratio) for c in counts]
    for L in (longest, longest + 9):
        buf = torch.full((len(counts), L + 5), float("nan"), dtype=torch.float32, device="cuda")
        out, lens = audio.resample_arena(src, begins, counts, channels, ratio[0], ratio[1], L=L, out=buf)
        assert lens == [r.size for r in rows] and tuple(out.shape) == (len(counts), L)
        got = buf.cpu().numpy()
        assert np.isnan(got[:, L:]).all(), "columns past L were written"
        for n, ref in enumerate(rows):
            assert (got[n, ref.size:L] == 0).all() and not np.signbit(got[n, ref.size:L]).any(), "row %d: padding" % n
        check_rows(got, rows, xmax, "%d -> %d %s L = %d" % (ratio + (kind, L)))


def test_same_rate_is_the_downmixing_copy(built):
    from fullycnnspeechenhancement_amd import audio
    rng = np.random.RandomState(3)
    x = rng.randint(-32768, 32768, (3, 1001, 2)).astype(np.int16)
    rows, lens = audio.resample_batch(x, 8000, 8000, lengths=[1001, 7, 0])
    got = rows.cpu().numpy()
    assert lens == [1001, 7, 0]
    for n, c in enumerate(lens):
        assert np.array_equal(got[n, :c], R.to_mono(x[n, :c]).astype(np.float32)) and (got[n, c:] == 0).all()
    f = rng.uniform(-1, 1, (2, 300)).astype(np.float32)
    assert np.array_equal(audio.resample_batch(f, 16000, 16000)[0].cpu().numpy(), f)


@pytest.mark.parametrize("ratio", [(16000, 8000), (44100, 8000)], ids=lambda r: "%d-%d" % r)
def test_int16_output(built, ratio):
    """clip(rint(ref * 32768)) exactly wherever ref * 32768 is more than 1e-6 from a half-integer, +-1 elsewhere; fewer than 1 in
    10,000 samples may be exempt (about 2e-6 are expected).  The last row is scaled to clip at both ends."""
    from fullycnnspeechenhancement_amd import audio
    rng = np.random.RandomState(11)
    n, length = 4, 12000
    x = rng.uniform(-0.9, 0.9, (n, length)).astype(np.float32)
    x[-1] *= 3.0
    rows, lens = audio.resample_batch(x, ratio[0], ratio[1], dtype="int16")
    got = rows.cpu().numpy()
    assert got.dtype == np.int16
    exempt = total = 0
    for i in range(n):
        ref = R.resample(x[i], *ratio) * 32768.0
        want = R.to_int16(ref / 32768.0)
        near = np.abs(ref - np.floor(ref) - 0.5) <= 1e-6
        y = got[i, :lens[i]].astype(np.int64)
        assert np.array_equal(y[~near], want[~near].astype(np.int64))
        assert (np.abs(y[near] - want[near]) <= 1).all()
        exempt, total = exempt + int(near.sum()), total + ref.size
    print("%d -> %d int16: %d of %d samples within 1e-6 of a tie" % (ratio + (exempt, total)))
    assert exempt * 10000 < total
    assert got[-1].max() == 32767 and got[-1].min() == -32768


def raw_resample(src, channels, begins, counts, ratio, out, out_begins, stride, L, stream=None):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    return _lib.load().rced_resample(src.data_ptr(), _lib.PCM_S16 if src.dtype == torch.int16 else _lib.PCM_F32, channels,
                                     int(src.numel()) // max(channels, 1), begins.data_ptr(), counts.data_ptr(),
                                     int(begins.shape[0]), ratio[0], ratio[1], out.data_ptr(),
                                     _lib.PCM_F32 if out.dtype == torch.float32 else _lib.PCM_S16,
                                     out_begins.data_ptr() if out_begins is not None else None, stride, L, 0, st)


@pytest.mark.parametrize("ratio", [(16000, 8000), (44100, 8000), (8000, 16000)], ids=lambda r: "%d-%d" % r)
def test_invariance_bit_for_bit(built, ratio):
    """One utterance gives the same bits alone, as row 0 of 3, as row 200 of 256, from two begin alignments, in row mode and
    packed, in two calls in a row, and replayed from a graph captured on one stream."""
    import torch
    from fullycnnspeechenhancement_amd import _lib, audio
    rng = np.random.RandomState(17)
    c = 9001
    M = R.length(c, *ratio)
    item = rng.randint(-32768, 32768, c).astype(np.int16)
    other = rng.randint(-32768, 32768, 4 * c + 64).astype(np.int16)
    alone = audio.resample_arena(dev(item), [0], [c], 1, *ratio)[0][0].cpu().numpy()
    assert alone.shape == (M,)

    host = other.copy()
    host[1:1 + c] = item                     # odd
    host[2 * c + 6:3 * c + 6] = item         # even
    src = dev(host)
    of3, _ = audio.resample_arena(src, [1, c + 3, 2 * c + 6], [c, c - 5, c], 1, *ratio)
    of3 = of3.cpu().numpy()
    assert np.array_equal(of3[0], alone) and np.array_equal(of3[2], alone)

    begins = [(7 * i) % (3 * c) for i in range(256)]
    counts = [1 + (131 * i) % c for i in range(256)]
    begins[200], counts[200] = 2 * c + 6, c
    rows, lens = audio.resample_arena(src, begins, counts, 1, *ratio)
    assert np.array_equal(rows[200, :M].cpu().numpy(), alone)
    again, _ = audio.resample_arena(src, begins, counts, 1, *ratio)
    assert torch.equal(rows, again)

    offs = np.concatenate([[3], 3 + np.cumsum(np.asarray(lens[:-1]) + 1)])      # packed, one guard sample between rows
    packed = torch.full((int(offs[-1]) + lens[-1] + 1,), float("nan"), dtype=torch.float32, device="cuda")
    audio.resample_arena(src, begins, counts, 1, *ratio, out=packed, out_begins=offs.tolist())
    p = packed.cpu().numpy()
    r = rows.cpu().numpy()
    written = np.zeros(p.size, bool)
    for n in range(256):
        assert np.array_equal(p[offs[n]:offs[n] + lens[n]], r[n, :lens[n]]), n
        written[offs[n]:offs[n] + lens[n]] = True
    assert np.isnan(p[~written]).all(), "packed mode wrote outside the rows"

    # the ratio has been used: this call allocates nothing and can be captured
    b3, c3 = dev([1, c + 3, 2 * c + 6], np.int64), dev([c, c - 5, c], np.int32)
    L = of3.shape[1]
    out = torch.full((3, L), float("nan"), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert raw_resample(src, 1, b3, c3, ratio, out, None, L, L, stream=torch.cuda.current_stream().cuda_stream) == _lib.RCED_OK
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), of3)


def write_wav(path, sig, rate):
    sig = np.asarray(sig, np.int16)
    w = wave.open(str(path), "wb")
    w.setnchannels(1 if sig.ndim == 1 else sig.shape[1])
    w.setsampwidth(2)
    w.setframerate(rate)
    w.writeframes(sig.astype("<i2").tobytes())
    w.close()
    return str(path)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wavs")
    rng = np.random.RandomState(23)
    files = [(rng.randint(-20000, 20000, 8001).astype(np.int16), 16000),
             (rng.randint(-20000, 20000, (24007, 2)).astype(np.int16), 48000),
             (rng.randint(-20000, 20000, 3333).astype(np.int16), 8000)]
    paths = [write_wav(d / ("f%d.wav" % i), sig, rate) for i, (sig, rate) in enumerate(files)]
    manifest = d / "manifest.json"
    with open(str(manifest), "w") as fh:
        for p, (sig, rate) in zip(paths, files):
            fh.write(json.dumps({"audio_filepath": p, "duration": sig.shape[0] / float(rate)}) + "\n")
    return str(manifest), paths, files


def test_corpus_from_files_of_any_rate(built, wavs):
    from fullycnnspeechenhancement_amd import audio, loader
    manifest, paths, files = wavs
    corpus = loader.Corpus.from_manifest(manifest, 8000, resample=True)
    assert str(corpus.arena.dtype) == "torch.float32"
    assert corpus.lengths.tolist() == [R.length(sig.shape[0], rate, 8000) for sig, rate in files]
    arena = corpus.arena.cpu().numpy()
    c16 = loader.Corpus.from_manifest(manifest, 8000, resample=True, arena_dtype="int16")
    a16 = c16.arena.cpu().numpy()
    assert a16.dtype == np.int16 and c16.lengths.tolist() == corpus.lengths.tolist()
    for (sig, rate), off, n in zip(files, corpus.offsets, corpus.lengths):
        item = arena[off:off + n]
        rows, lens = audio.resample_batch(sig[None], rate, 8000)
        assert lens == [n] and np.array_equal(rows[0].cpu().numpy(), item)
        ref = R.resample(sig, rate, 8000)
        check_rows(item[None], [ref], [float(np.abs(R.to_mono(sig)).max())], "corpus item from %d Hz" % rate)
        want, scaled = R.to_int16(ref), ref * 32768.0
        near = np.abs(scaled - np.floor(scaled) - 0.5) <= 1e-6
        got = a16[off:off + n].astype(np.int64)
        assert np.array_equal(got[~near], want[~near].astype(np.int64)) and (np.abs(got[near] - want[near]) <= 1).all()
        assert near.sum() * 10000 < max(n, 10000)
    assert np.array_equal(a16[corpus.offsets[2]:], files[2][0])          # the file already at 8 kHz: its own samples
    assert np.array_equal(loader.read_wav(paths[1], 8000, resample=True), a16[corpus.offsets[1]:corpus.offsets[2]])
    with pytest.raises(ValueError, match="resample=True"):
        loader.Corpus.from_manifest(manifest, 8000)
    # two uploads instead of one give the same arena
    old = loader.STAGING_BYTES
    loader.STAGING_BYTES = 2 * 2 * 24007 + 8
    try:
        split = loader.Corpus.from_manifest(manifest, 8000, resample=True)
    finally:
        loader.STAGING_BYTES = old
    assert np.array_equal(split.arena.cpu().numpy(), arena)


def test_engine_takes_any_rate(built, wavs, tmp_path):
    from fullycnnspeechenhancement_amd import audio, loader
    from fullycnnspeechenhancement_amd.engine import InferenceEngine
    from oracle import rced_np
    engine = InferenceEngine(net_work="FullyCNNV3", weights=rced_np.make_weights("FullyCNNV3", seed=42))
    rng = np.random.RandomState(29)
    sig = rng.uniform(-0.5, 0.5, 16001).astype(np.float32)
    rows, lens = audio.resample_batch(sig, 16000, 8000)
    at8k = rows[0, :lens[0]].cpu().numpy()
    out = engine.denoise_pcm(sig, sample_rate=16000)
    assert out.shape == (R.length(16001, 16000, 8000),) and out.dtype == np.float32
    assert np.array_equal(out, engine.denoise_pcm(at8k))

    manifest, paths, files = wavs
    got = engine.denoise_file(paths[1], save_dir=str(tmp_path))
    n = R.length(24007, 48000, 8000)
    assert got.shape == (n,) and got.dtype == np.float32
    written = str(tmp_path / "f1_de.wav")
    assert loader.wav_info(written) == (8000, 1, n)
    assert np.array_equal(loader.read_wav(written, 8000), R.to_int16(got))
    frames, rate = loader.read_wav_frames(paths[1])
    assert np.array_equal(got, engine.denoise_pcm(audio.resample_batch(frames[None], rate, 8000)[0][0].cpu().numpy()))


def test_prepare_corpus_tool(built, wavs, tmp_path):
    """tools/prepare_corpus.py over a directory: mono PCM16 at 8 kHz under the output root, the reference's manifest lines, files
    of fewer than 100 frames skipped.  Its function is called as it is: the command line only parses arguments."""
    import importlib.util
    import os
    from conftest import ROOT
    from fullycnnspeechenhancement_amd import loader
    spec = importlib.util.spec_from_file_location("prepare_corpus", os.path.join(ROOT, "tools", "prepare_corpus.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    manifest, paths, files = wavs
    src = os.path.dirname(paths[0])
    write_wav(os.path.join(src, "tiny.wav"), np.zeros(99, np.int16), 16000)
    try:
        res = tool.prepare(src, str(tmp_path / "out"), str(tmp_path / "lists" / "manifest.train"), 8000)
    finally:
        os.remove(os.path.join(src, "tiny.wav"))
    assert res["files"] == 3 and res["skipped"] == 1
    items = loader.read_manifest(str(tmp_path / "lists" / "manifest.train"), min_duration=0.0)
    assert [os.path.basename(i["audio_filepath"]) for i in items] == ["f0.wav", "f1.wav", "f2.wav"]
    for item, path, (sig, rate) in zip(items, paths, files):
        n = R.length(sig.shape[0], rate, 8000)
        assert loader.wav_info(item["audio_filepath"]) == (8000, 1, n) and item["duration"] == n / 8000.0
        assert np.array_equal(loader.read_wav(item["audio_filepath"], 8000), loader.read_wav(path, 8000, resample=True))


def test_bad_arguments_launch_nothing(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib, audio
    src = dev(np.zeros(64, np.int16))
    b, c = dev([0], np.int64), dev([64], np.int32)
    out = torch.full((1, 40), float("nan"), dtype=torch.float32, device="cuda")
    lib = _lib.load()
    for channels, ratio, word in ((0, (16000, 8000), b"channels"), (1, (0, 8000), b"rates"), (1, (16000, 0), b"rates"),
                                  (1, (8001, 8000), b"8001")):
        assert raw_resample(src, channels, b, c, ratio, out, None, 40, 40) == _lib.RCED_ERR_ARG
        assert word in lib.rced_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    for kwargs in (dict(begins=[0], counts=[65]), dict(begins=[-1], counts=[4]), dict(begins=[0], counts=[64], L=31)):
        with pytest.raises(ValueError):
            audio.resample_arena(src, channels=1, sr_orig=16000, sr_new=8000, **kwargs)
    with pytest.raises(ValueError):
        audio.resample_arena(src, [0], [64], 1, 16000, 8000, dtype="float64")
