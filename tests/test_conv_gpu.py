"""GPU tests of the ragged batched FIR (rced_convolve, audio.convolve_batch) and of the loader's reverberant batches
(DataSet(rir=...)).  The pin is the float64 restatement of tests/conv_np.py; the elementwise bar is derived, not measured:
    |dev - ref| <= 2^-24 |ref| + K 2^-52 abs_bound
-- the one fp32 rounding at the store, plus the worst case of an fp64 accumulation of K terms in any order, doubled
(abs_bound: the same convolution over |x|, |h|).  Figures are printed before they are asserted."""

import os
import re

import numpy as np
import pytest

import conv_np
import loader_np
from conftest import ROOT

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
TAPS = (1, 2, 15, 16, 17, 31, 33, 65, 513, 8192)
SMALL = (0, 1, 15, 16, 17, 63, 64, 65)


def kernel_constants():
    """The constexpr ints of csrc/kernels_conv.h, evaluated in order (kWaves: kernels_eval.h's kThreads / 64)."""
    src = open(os.path.join(ROOT, "fullycnnspeechenhancement_amd", "csrc", "kernels_conv.h")).read()
    ev = open(os.path.join(ROOT, "fullycnnspeechenhancement_amd", "csrc", "kernels_eval.h")).read()
    env = {"kWaves": int(re.search(r"constexpr int kThreads = (\d+);", ev).group(1)) // 64}
    for name, expr in re.findall(r"^constexpr int (\w+) = ([^;]+);", src, flags=re.M):
        env[name] = int(eval(expr.replace("/", "//"), {}, env))
    return env


K_ = kernel_constants()


def slice_lengths():
    """One below, at and one above the kernel's own sizes: a 256-output tile, the history a chunk stages before its slice,
    an output slice, a staged window, two slices; then about 9,000."""
    sizes = (256, K_["kBack"], K_["kOutSlice"], K_["kWindow"], 2 * K_["kOutSlice"])
    return tuple(sorted({s + e for s in sizes for e in (-1, 0, 1)} | {9000}))


def shifts_of(K):
    return sorted({0, min(1, K - 1), K // 2, K - 1})


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.asarray(a, dtype) if dtype else a, device="cuda")


def raw_convolve(x, xlen, h, hlen, shift, L, y, stream=None):
    """The C entry as it is: x [N, xs], h [N, hs], y [N, ys] float32 device matrices, the rest int32 device vectors or None."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.check(_lib.load().rced_convolve(x.data_ptr(), int(x.stride(0)), ptr(xlen), h.data_ptr(), int(h.stride(0)), ptr(hlen),
                                         ptr(shift), int(x.shape[0]), L, y.data_ptr(), int(y.stride(0)), 0, st))


def gaussian(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def filters():
    """One seeded Gaussian filter per tap count, shared by the tests; never written to."""
    out = {K: gaussian(K, 1000 + K) for K in TAPS}
    for h in out.values():
        h.setflags(write=False)
    return out


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------

def test_constants_are_the_ones_the_cases_assume():
    assert K_["kMaxTaps"] == 8192 and K_["kMaxBlockLags"] == 513 and K_["kOutSlice"] == 4096
    assert K_["kWindow"] == K_["kOutSlice"] + K_["kBack"] and 9000 > 2 * K_["kOutSlice"] + 1
    assert len(slice_lengths()) == 16


@pytest.mark.parametrize("length", SMALL + slice_lengths())
def test_parity(built, filters, length):
    """Every tap count x every shift of it at one signal length, all rows in one launch (the rows share the signal; each has
    its own filter, tap count and shift).  The buffer is 3 columns wider than the signal: they must come back zero."""
    import torch
    x = gaussian(length + 3, 77 + length)
    rows = [(K, d) for K in TAPS for d in shifts_of(K)]
    n, L = len(rows), length + 3
    hmat = np.zeros((n, max(TAPS)), np.float32)
    for i, (K, _) in enumerate(rows):
        hmat[i, :K] = filters[K]
    y = torch.full((n, L), SENTINEL, dtype=torch.float32, device="cuda")
    raw_convolve(dev(np.tile(x, (n, 1))), dev([length] * n, np.int32), dev(hmat), dev([K for K, _ in rows], np.int32),
                 dev([d for _, d in rows], np.int32), L, y)
    got = y.cpu().numpy().astype(np.float64)
    worst, full = 0.0, {}
    for i, (K, d) in enumerate(rows):
        if K not in full:
            full[K] = conv_np.convolve_full(x, filters[K], length)
        ref, bound = conv_np.cut(full[K][0], d, length), conv_np.cut(full[K][1], d, length)
        bar = conv_np.bar(ref, bound, K)
        err = np.abs(got[i, :length] - ref)
        if length:
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
        assert np.all(err <= bar), (length, K, d, float(err.max()))
        assert not got[i, length:].any(), (length, K, d)
    print("length %d: %d rows, worst error %.3f of the bar" % (length, n, worst))


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", (1, 17, 300, 4097, 9000))
def test_exact_cases(built, length):
    import torch
    from fullycnnspeechenhancement_amd import audio
    x = gaussian(length, 5 + length)
    xd = dev(x)[None]
    # h = [1] returns x
    assert np.array_equal(bits(audio.convolve_batch(xd, dev(np.float32([[1.0]]))).cpu().numpy()[0]), bits(x))
    for j in (0, 1, 15, 16, 17, 511, 512, 513, 8191):
        imp = np.zeros((1, j + 1), np.float32)
        imp[0, j] = 1.0
        # a unit impulse at j with shift j returns x
        same = audio.convolve_batch(xd, dev(imp), shifts=[j]).cpu().numpy()[0]
        assert np.array_equal(bits(same), bits(x)), (length, j)
        # with shift 0 it returns x delayed by j, zeros before
        late = audio.convolve_batch(xd, dev(imp)).cpu().numpy()[0]
        want = np.zeros(length, np.float32)
        want[j:] = x[:max(length - j, 0)]
        assert np.array_equal(bits(late), bits(want)), (length, j)
    # an all-zero x gives +0.0 everywhere, whatever the signs of the taps
    h = gaussian(700, 9)[None]
    zero = audio.convolve_batch(torch.zeros((1, length), device="cuda"), dev(h), shifts=[350]).cpu().numpy()
    assert not bits(zero).any()
    # K = 0 gives zeros
    none = audio.convolve_batch(xd, dev(h), filter_lengths=[0]).cpu().numpy()
    assert not bits(none).any()


# ---- 3. invariants ---------------------------------------------------------------------------------------------------------------

def test_a_row_does_not_depend_on_the_batch_around_it(built, filters):
    """The same row alone, among 5 rows at two row indices, with strides wider than L / K, twice: the same bits.  Columns
    len .. L are zero, columns L .. y_stride keep their sentinel."""
    import torch
    length, L, K, d = 4700, 4704, 513, 256
    x, h = gaussian(length, 41), filters[K]

    def run(n, at, xs, hs, ys):
        xm, hm = np.full((n, xs), 3.0, np.float32), np.full((n, hs), -2.0, np.float32)
        lens, taps, shifts = [], [], []
        for i in range(n):
            li, ki = (length, K) if i == at else (1000 + 531 * i, (1, 17, 65, 8192, 33)[i])
            xm[i, :li] = x[:li] if i == at else gaussian(li, 50 + i)
            hm[i, :ki] = h[:ki] if i == at else gaussian(ki, 60 + i)
            lens.append(li), taps.append(ki), shifts.append(d if i == at else ki // 3)
        y = torch.full((n, ys), SENTINEL, dtype=torch.float32, device="cuda")
        raw_convolve(dev(xm), dev(lens, np.int32), dev(hm), dev(taps, np.int32), dev(shifts, np.int32), L, y)
        out = y.cpu().numpy()
        assert (out[:, L:] == SENTINEL).all()
        for i in range(n):
            assert not out[i, lens[i]:L].any()
        return out[at, :L].copy()

    alone = run(1, 0, L, K, L)
    ref, bound = conv_np.convolve_ref(x, h, d, length)
    assert np.all(np.abs(alone[:length].astype(np.float64) - ref) <= conv_np.bar(ref, bound, K))
    for n, at, xs, hs, ys in ((1, 0, L, K, L), (5, 1, L, 8192, L), (5, 4, L, 8192, L), (5, 2, L + 9, 8192 + 5, L + 13), (1, 0, L + 1, K + 3, L + 2)):
        assert np.array_equal(bits(run(n, at, xs, hs, ys)), bits(alone)), (n, at, xs, hs, ys)


def test_filters_of_very_different_lengths_in_one_launch(built, filters):
    from fullycnnspeechenhancement_amd import audio
    L = 9000
    xs = np.stack([gaussian(L, 71), gaussian(L, 72)])
    hm = np.zeros((2, 8192), np.float32)
    hm[0, 0], hm[1] = filters[1][0], filters[8192]
    lens, taps, shifts = [9000, 8999], [1, 8192], [0, 4000]
    both = audio.convolve_batch(dev(xs), dev(hm), lens, taps, shifts).cpu().numpy()
    for i in range(2):
        alone = audio.convolve_batch(dev(xs[i:i + 1]), dev(hm[i:i + 1, :taps[i]]), lens[i:i + 1], None, shifts[i:i + 1]).cpu().numpy()
        assert np.array_equal(bits(both[i]), bits(alone[0])), i
    assert np.array_equal(bits(both[0]), bits((xs[0].astype(np.float64) * np.float64(hm[0, 0])).astype(np.float32)))


def test_padding_is_never_read(built, filters):
    """NaN past len_n in x and past K_n in h never reaches the output."""
    import torch
    rows = [(0, 1, 0), (1, 16, 15), (17, 17, 8), (300, 513, 100), (4096, 33, 0), (4097, 8192, 8191), (9000, 65, 64), (8191, 8191, 1)]
    n, L = len(rows), 9003
    xm, hm = np.full((n, L + 5), np.nan, np.float32), np.full((n, 8200), np.nan, np.float32)
    for i, (length, K, _) in enumerate(rows):
        xm[i, :length] = gaussian(length, 80 + i)
        hm[i, :K] = filters[K] if K in filters else gaussian(K, 90 + i)
    y = torch.full((n, L + 2), SENTINEL, dtype=torch.float32, device="cuda")
    raw_convolve(dev(xm), dev([r[0] for r in rows], np.int32), dev(hm), dev([r[1] for r in rows], np.int32),
                 dev([r[2] for r in rows], np.int32), L, y)
    got = y.cpu().numpy()
    assert np.isfinite(got).all() and (got[:, L:] == SENTINEL).all()
    for i, (length, K, d) in enumerate(rows):
        ref, bound = conv_np.convolve_ref(xm[i, :length], hm[i, :K], d, length)
        assert np.all(np.abs(got[i, :length].astype(np.float64) - ref) <= conv_np.bar(ref, bound, K)), rows[i]
        assert not got[i, length:L].any()
    # the library's clamping: lengths, tap counts and shifts outside their rows are clamped into them, nothing outside is read
    xs, hs = dev(xm[3:4, :300].copy()), dev(hm[3:4, :513].copy())
    want = torch.empty((1, 300), device="cuda")
    raw_convolve(xs, None, hs, None, dev([512], np.int32), 300, want)
    for xl, hl, sh in ((301, 514, 512), (10 ** 9, 10 ** 9, 10 ** 9), (300, 513, 513)):
        out = torch.empty((1, 300), device="cuda")
        raw_convolve(xs, dev([xl], np.int32), hs, dev([hl], np.int32), dev([sh], np.int32), 300, out)
        assert torch.equal(out, want)
    out = torch.full((1, 300), SENTINEL, device="cuda")
    raw_convolve(xs, dev([-5], np.int32), hs, dev([-1], np.int32), dev([-3], np.int32), 300, out)
    assert not out.any()


def test_wrapper_validates(built):
    import torch
    from fullycnnspeechenhancement_amd import audio
    x, h = dev(gaussian(64, 1).reshape(2, 32)), dev(gaussian(16, 2).reshape(2, 8))
    y = audio.convolve_batch(x, h, [32, 20], [8, 3], [7, 2])
    assert tuple(y.shape) == (2, 32) and y.dtype == torch.float32 and not y[1, 20:].any()
    one = audio.convolve_batch(x[1, :20], h[1, :3], shifts=[2])                   # a 1-D signal is one row
    assert tuple(one.shape) == (20,) and torch.equal(one, y[1, :20])
    wide = torch.full((4, 40), SENTINEL, device="cuda")
    wide[:2, :32] = x
    assert torch.equal(audio.convolve_batch(wide[:2, :32], h, [32, 20], [8, 3], [7, 2]), y)      # a view of a wider buffer
    out = torch.empty((2, 32), device="cuda")
    assert audio.convolve_batch(x, h, [32, 20], [8, 3], [7, 2], out=out) is out and torch.equal(out, y)
    both = torch.empty((4, 32), device="cuda")
    both[:2] = x
    for bad in (dict(shifts=[8, 0]), dict(shifts=[0, -1]), dict(filter_lengths=[8, 3], shifts=[0, 3]), dict(lengths=[33, 0]),
                dict(lengths=[-1, 0]), dict(filter_lengths=[9, 0]), dict(lengths=[1]), dict(out=x),
                dict(out=torch.empty((2, 33), device="cuda")), dict(out=torch.empty((2, 32), device="cuda", dtype=torch.float64))):
        with pytest.raises(ValueError):
            audio.convolve_batch(x, h, **bad)
    for out in (both[:2], both[1:3]):                                             # the signal itself; its second row
        with pytest.raises(ValueError, match="overlap"):
            audio.convolve_batch(both[:2], h, out=out)
    audio.convolve_batch(both[:2], h, out=both[2:])                               # the other half of one buffer is fine
    assert torch.equal(both[2:], audio.convolve_batch(x, h))
    with pytest.raises(ValueError):
        audio.convolve_batch(x, h[:1])                                            # mismatched N
    with pytest.raises(ValueError, match="8192"):
        audio.convolve_batch(x, torch.zeros((2, 8193), device="cuda"))            # more than 8192 taps
    with pytest.raises(ValueError):
        audio.convolve_batch(x, h.cpu())                                          # another device
    assert tuple(audio.convolve_batch(torch.zeros((0, 8), device="cuda"), torch.zeros((0, 4), device="cuda")).shape) == (0, 8)


# ---- 4. the loader -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(built):
    """5 utterances of 300 .. 2,000 samples, 3 synthetic responses of 40 .. 700 taps, 2 noises: one shorter, one longer than
    every utterance."""
    from fullycnnspeechenhancement_amd import loader
    rng = np.random.default_rng(12)
    clean = [rng.integers(-9000, 9000, n).astype(np.int16) for n in (300, 2000, 777, 1501, 1024)]
    noise = [rng.integers(-5000, 5000, n).astype(np.int16) for n in (200, 2500)]
    rirs = [h[:k] for h, k in zip(loader.synthetic_rirs(3, rt60=(0.09, 0.2), seed=8), (40, 333, 700))]
    return dict(clean=clean, noise=noise, rirs=rirs, cc=loader.Corpus.from_arrays(clean), nc=loader.Corpus.from_arrays(noise),
                rc=loader.RirCorpus.from_arrays(rirs))


PLAN = [(1, 0, 0, np.asarray([0.7, 1.6, 0.9, 1.2]), 2), (0, 1, 411, np.zeros(0), 0), (3, 0, 0, np.asarray([1.1, 0.3, 1.9]), None),
        (2, 1, 0, np.zeros(0), 1), (4, 1, 1476, np.zeros(0), 2)]


@pytest.mark.parametrize("target", ["reverberant", "early", "dry"])
def test_batches_are_the_stages_by_hand_and_the_restatement(small, target):
    import torch
    from fullycnnspeechenhancement_amd import audio, loader
    cc, nc, rc = small["cc"], small["nc"], small["rc"]
    assert all(40 <= k <= 700 for k in rc.lengths) and rc.direct.tolist() == [int(np.argmax(np.abs(h))) for h in small["rirs"]]
    ds = loader.DataSet(cc, noise=nc, snr=3, rir=rc, target=target, early_ms=12.5)
    batch_mix, batch_clean, mix_sig, clean_sig = loader.DataLoader(ds, 5).build(PLAN)
    # by hand: gather, convolve_batch, mix_snr_batch, stft_batch
    cids, rids = [p[0] for p in PLAN], [p[4] for p in PLAN]
    ls = [len(small["clean"][c]) for c in cids]
    dry = cc.gather(cids)
    kmax = 700
    hm = np.zeros((5, kmax), np.float32)
    taps, shifts, early = [], [], []
    for i, r in enumerate(rids):
        h = small["rirs"][r] if r is not None else np.ones(1, np.float32)
        d = int(np.argmax(np.abs(h)))
        hm[i, :len(h)] = h / h[d]                                     # the direct path is already exactly 1: a no-op
        taps.append(len(h)), shifts.append(d), early.append(min(len(h), d + 100 + 1))
    wet = audio.convolve_batch(dry, dev(hm), ls, taps, shifts)
    tgt = {"reverberant": wet, "dry": dry, "early": audio.convolve_batch(dry, dev(hm), ls, early, shifts)}[target]
    nz = nc.gather([p[1] for p in PLAN], [p[2] for p in PLAN], [min(n, len(small["noise"][p[1]])) for p, n in zip(PLAN, ls)])
    mixed = audio.mix_snr_batch(wet, nz, 3, speech_lengths=ls, noise_lengths=[min(n, len(small["noise"][p[1]])) for p, n in zip(PLAN, ls)],
                                gains=[p[3] for p in PLAN])
    mag, _ = audio.stft_batch(torch.cat([tgt, mixed]), ls + ls, with_phase=False)
    assert torch.equal(batch_clean, mag[:5]) and torch.equal(batch_mix, mag[5:])
    assert clean_sig.lengths == mix_sig.lengths == ls
    assert torch.equal(clean_sig.rows, tgt) and torch.equal(mix_sig.rows, mixed)
    assert torch.equal(wet[2], dry[2])                                 # the row that stays dry: the identity, bit for bit
    # the float64 restatement
    ref_mix, ref_clean, mixes, targets, bounds = conv_np.build_batch(small["clean"], small["noise"], small["rirs"], rc.direct, PLAN, 3,
                                                                      target, early_ms=12.5)
    worst = 0.0
    for i, n in enumerate(ls):
        got = clean_sig[i].cpu().numpy().astype(np.float64)
        if bounds[i] is None:
            assert np.array_equal(got, targets[i])
        else:
            ref, bound, K = bounds[i]
            bar = conv_np.bar(ref, bound, K)
            worst = max(worst, float((np.abs(got - ref) / bar).max()))
            assert np.all(np.abs(got - ref) <= bar), (i, K)
    for got, ref, name in ((batch_mix, ref_mix, "mix"), (batch_clean, ref_clean, "clean")):
        got = got.cpu().numpy()
        assert got.shape == ref.shape
        err = np.abs(got - ref).max() / ref.max()
        print("%s, %s spectrograms vs the restatement: %.3e of the scale (bar 2e-6); target rows %.3f of their bar" % (target, name, err, worst))
        assert err <= 2e-6


def test_rir_prob_zero_is_the_loader_without_rir(small):
    """The same plans (rir= draws two more numbers per item, so the noise draws of one seed differ; the plans are carried over)."""
    import torch
    from fullycnnspeechenhancement_amd import loader
    np.random.seed(7)
    base = loader.DataLoader(loader.DataSet(small["cc"], noise=small["nc"], snr=2), 3)
    plans = list(base.plans())
    want = [base.build(p) for p in plans]
    assert len(plans) == 2 and all(len(p) == 4 for batch in plans for p in batch)
    for target in ("reverberant", "early", "dry"):
        dl = loader.DataLoader(loader.DataSet(small["cc"], noise=small["nc"], snr=2, rir=small["rc"], rir_prob=0.0, target=target), 3)
        assert all(len(p) == 5 and p[4] is None for batch in dl.plans() for p in batch)
        for plan, a in zip(plans, want):
            b = dl.build([p + (None,) for p in plan])
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert torch.equal(a[2].rows, b[2].rows) and torch.equal(a[3].rows, b[3].rows) and a[2].lengths == b[2].lengths


def test_one_training_step_on_a_reverberant_batch(small):
    """A smoke test of the whole path, not a parity claim."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, loader
    from oracle import rced_np
    np.random.seed(3)
    ds = loader.DataSet(small["cc"], noise=small["nc"], snr=5, rir=small["rc"], rir_prob=0.7, target="early")
    dl = loader.DataLoader(ds, 5)
    batch_mix, batch_clean, _, _ = next(iter(dl))
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=5, lr=1e-3, weights=rced_np.make_weights("FullyCNNV3", seed=42))
    loss = tr.train_step(batch_mix, batch_clean)[0]
    tr.close()
    print("loss of one step on a reverberant batch: %r" % (loss,))
    assert np.isfinite(loss)


# ---- 5. stream capture ---------------------------------------------------------------------------------------------------------------

def test_convolve_replays_from_a_captured_graph(built, filters):
    """The entry allocates nothing: captured after one eager call, a replay reads what lies in the buffers when it runs."""
    import torch
    n, L, K = 3, 4700, 513
    xh = np.stack([gaussian(L, 200 + i) for i in range(n)])
    hm = np.zeros((n, K), np.float32)
    hm[0, :K], hm[1, :65], hm[2, :1] = filters[K], filters[65], filters[1]
    x, h = dev(xh), dev(hm)
    lens, taps, shifts = dev([4700, 4097, 300], np.int32), dev([K, 65, 1], np.int32), dev([256, 64, 0], np.int32)
    out = torch.full((n, L), SENTINEL, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw_convolve(x, lens, h, taps, shifts, L, out, stream=side.cuda_stream)
    side.synchronize()
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        raw_convolve(x, lens, h, taps, shifts, L, out, stream=torch.cuda.current_stream().cuda_stream)
    x.copy_(dev(xh[:, ::-1].copy()))
    graph.replay()
    torch.cuda.synchronize()
    eager = torch.empty_like(out)
    raw_convolve(x, lens, h, taps, shifts, L, eager)
    assert torch.equal(out, eager)
    ref, bound = conv_np.convolve_ref(xh[1, ::-1], hm[1, :65], 64, 4097)
    assert np.all(np.abs(out[1, :4097].cpu().numpy().astype(np.float64) - ref) <= conv_np.bar(ref, bound, 65))
