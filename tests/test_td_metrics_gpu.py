"""GPU tests of rced_si_sdr / rced_seg_snr (audio.si_sdr_batch, audio.seg_snr_batch) against the float64 restatements of
their definitions (tests/td_metrics_np.py), and of the evaluation loop's `extra` argument.

The bar is 1e-9 dB, derived, not measured: the products of fp32 values are exact in fp64; an fp64 sum of n <= 65,664 terms
in any order is off by at most n 2^-53 relative, about 3e-11 dB (the one longer row here, 524,289 samples, 2.5e-10 dB); an
error in alpha enters the residual at second order only.  Every comparison prints its figure."""

import functools
import math

import numpy as np
import pytest

import stoi_np as sn
import td_metrics_np as td
import test_stoi_gpu as tg
from test_stoi_gpu import dev, padded, strided

pytestmark = pytest.mark.gpu

BAR = 1e-9
SLICE = 2048                                    # kernels_eval.h: kSlice
# a frame short, one frame, two frames, the frame kernel's 16 frames per workgroup and one more, the slice and its neighbours
LENS = (0, 1, 239, 240, 299, 300, 1140, 1199, 1200, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE, 24000, 9001, 6001)
SNRS = (-5, 5, 20, 60)


@functools.lru_cache(maxsize=None)
def ragged():
    """Gated-harmonic rows (tests/stoi_np.speechlike) against mixtures at -5, 5, 20, 60 dB, with their references."""
    clean = [sn.speechlike(L, 300 + i).astype(np.float32) for i, L in enumerate(LENS)]
    est = [sn.add_white(c.astype(np.float64), SNRS[i % 4], 400 + i).astype(np.float32) if len(c) > 1 else c.copy()
           for i, c in enumerate(clean)]
    est[1] = 2 * clean[1]                         # one sample: alpha = 2, no residual
    ref_si = [td.si_sdr(c, e) for c, e in zip(clean, est)]
    ref_seg = [td.seg_snr_detail(c, e, 8000) for c, e in zip(clean, est)]
    return clean, est, ref_si, ref_seg


def close(got, want, what):
    """Both finite and within BAR, or the same non-finite value."""
    if math.isfinite(want):
        print("%s: device %.12f restatement %.12f |diff| %.2e" % (what, got, want, abs(got - want)))
        assert math.isfinite(got) and abs(got - want) <= BAR, what
    else:
        print("%s: device %r restatement %r" % (what, got, want))
        assert (math.isnan(got) and math.isnan(want)) or got == want, what


def test_parity_with_the_restatements(built):
    from fullycnnspeechenhancement_amd.audio import seg_snr_batch, si_sdr_batch
    clean, est, ref_si, ref_seg = ragged()
    c, e = strided(clean, 24000 + 7), strided(est, 24000 + 13, fill=-3.0)
    si = si_sdr_batch(c, e, LENS).cpu().numpy()
    seg, nf = seg_snr_batch(c, e, LENS, detail=True)
    seg, nf = seg.cpu().numpy(), nf.cpu().numpy()
    for i, L in enumerate(LENS):
        close(float(si[i]), ref_si[i], "SI-SDR L %d" % L)
        close(float(seg[i]), ref_seg[i][0], "SegSNR L %d (%d frames)" % (L, ref_seg[i][1]))
        assert int(nf[i]) == ref_seg[i][1] == ((L - 240) // 60 + 1 if L >= 240 else 0)
    assert math.isnan(ref_si[0]) and ref_si[1] == math.inf and all(math.isfinite(v) for v in ref_si[2:])
    assert [math.isnan(r[0]) for r in ref_seg] == [L < 240 for L in LENS]


def test_a_row_of_more_than_256_slices(built):
    """524,289 samples: 257 slices, the second stride of the sums over the partials; beside it a short row."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    from fullycnnspeechenhancement_amd.audio import seg_snr_batch
    L = 256 * SLICE + 1
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal(L)).astype(np.float32)
    y = (x + 0.01 * rng.standard_normal(L)).astype(np.float32)
    c, e = dev(np.stack([x, x])), dev(np.stack([y, y]))
    lens = dev([L, 3000], np.int32)
    out, parts = torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty((2, 3), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().rced_si_sdr(c.data_ptr(), L, e.data_ptr(), L, lens.data_ptr(), 2, out.data_ptr(), parts.data_ptr(), 0,
                                       torch.cuda.current_stream().cuda_stream))
    out, parts = out.cpu().numpy(), parts.cpu().numpy()
    for i, n in enumerate((L, 3000)):
        close(float(out[i]), td.si_sdr(x[:n], y[:n]), "SI-SDR L %d" % n)
        alpha, target, residual = td.si_sdr_parts(x[:n], y[:n])
        assert abs(parts[i, 0] - alpha) <= 1e-12 and abs(parts[i, 1] / target - 1) <= 1e-12 and abs(parts[i, 2] / residual - 1) <= 1e-9
        assert abs(out[i] - 10 * np.log10(parts[i, 1] / parts[i, 2])) <= 1e-12
    seg = seg_snr_batch(c, e, [L, 3000]).cpu().numpy()
    for i, n in enumerate((L, 3000)):
        close(float(seg[i]), td.seg_snr(x[:n], y[:n], 8000), "SegSNR L %d" % n)


@pytest.mark.parametrize("fs", (117, 16000, 48016))
def test_seg_snr_at_other_rates(built, fs):
    """Frames of 4 (hop 1), 480 and 1440 samples: the ends of the range the library takes, and one between."""
    from fullycnnspeechenhancement_amd.audio import seg_snr_batch
    W = td.seg_window(fs)
    lens = (W - 1, W, W + W // 4 - 1, W + W // 4, 5 * W + 3)
    rng = np.random.default_rng(fs)
    clean = [rng.standard_normal(L).astype(np.float32) for L in lens]
    est = [(c + 0.2 * rng.standard_normal(len(c))).astype(np.float32) for c in clean]
    seg, nf = seg_snr_batch(dev(padded(clean, lens[-1])), dev(padded(est, lens[-1] + 1)), lens, sample_rate=fs, detail=True)
    seg, nf = seg.cpu().numpy(), nf.cpu().numpy()
    assert nf.tolist() == [0, 1, 1, 2, (4 * W + 3) // (W // 4) + 1]
    for i, L in enumerate(lens):
        want, frames = td.seg_snr_detail(clean[i], est[i], fs)
        assert frames == int(nf[i])
        close(float(seg[i]), want, "SegSNR fs %d L %d" % (fs, L))


def test_special_values(built):
    from fullycnnspeechenhancement_amd.audio import seg_snr_batch, si_sdr_batch
    x = sn.speechlike(5000, 9).astype(np.float32)
    noisy = sn.add_white(x.astype(np.float64), 5, 10).astype(np.float32)
    zero = np.zeros_like(x)
    rows = dev(np.stack([x, (0.5 * x).astype(np.float32), zero, noisy, (4 * noisy).astype(np.float32), np.ones_like(x)]))
    clean = rows[[0, 0, 2, 0, 2, 0, 0, 0]]
    est = rows[[0, 1, 0, 2, 2, 3, 4, 0]]
    lens = [5000, 5000, 5000, 5000, 5000, 5000, 5000, 0]
    si = si_sdr_batch(clean, est, lens).cpu().numpy()
    print("SI-SDR:", si.tolist())
    assert si[0] == math.inf and si[1] == math.inf              # y = x and y = 0.5 x: alpha exact, the residual exactly zero
    assert all(math.isnan(v) for v in si[[2, 3, 4, 7]])         # a zero clean row, a zero estimate, both, a length of 0
    assert si[5] == si[6] and math.isfinite(si[5])              # a gain of 4 on the estimate: the same bits
    seg, nf = seg_snr_batch(clean, est, lens, detail=True)
    seg, nf = seg.cpu().numpy(), nf.cpu().numpy()
    print("SegSNR:", seg.tolist())
    assert nf.tolist() == [80] * 7 + [0]
    assert seg[0] == 35 and math.isnan(seg[7])
    assert seg[2] == -10                                         # x = 0: every frame at the floor
    # x = 0, y = 1 over 300 samples: -10 from 2 frames; y = 0 over one frame: 10 log10(1 + EPS)
    seg, nf = seg_snr_batch(rows[[2, 0]], rows[[5, 2]], [300, 240], detail=True)
    assert nf.tolist() == [2, 1] and float(seg[0]) == -10 and abs(float(seg[1]) - 10 * np.log10(1 + td.EPS)) <= BAR


def test_scores_do_not_depend_on_the_batch_around_them(built):
    from fullycnnspeechenhancement_amd.audio import seg_snr_batch, si_sdr_batch
    clean, est, _, _ = ragged()
    pick = [13, 9, 10, 11, 14, 5]
    lens = [LENS[i] for i in pick]
    clean, est = [clean[i] for i in pick], [est[i] for i in pick]
    width = max(lens)
    for fn in (si_sdr_batch, seg_snr_batch):
        full = fn(dev(padded(clean, width)), dev(padded(est, width)), lens).cpu().numpy()
        again = fn(dev(padded(clean, width)), dev(padded(est, width)), lens).cpu().numpy()
        assert full.tobytes() == again.tobytes()                                             # run to run
        order = [3, 0, 5, 2, 1, 4]                                                           # other rows, strides, junk
        moved = fn(strided([clean[i] for i in order], width + 5, fill=-1e3), strided([est[i] for i in order], width + 10, fill=9e9),
                   [lens[i] for i in order]).cpu().numpy()
        assert moved.tobytes() == full[order].tobytes()
        for i in (0, 2):                                                                     # alone, exactly as long as itself
            alone = fn(dev(clean[i][None]), dev(est[i][None])).cpu().numpy()
            assert alone.tobytes() == full[i:i + 1].tobytes()


def test_second_call_allocates_nothing_and_replays_from_a_captured_graph(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lens_host = [20000, 14321, 100]
    clean = [sn.speechlike(L, 60 + i).astype(np.float32) for i, L in enumerate(lens_host)]
    est = [sn.add_white(c.astype(np.float64), 5, 70 + i).astype(np.float32) for i, c in enumerate(clean)]
    ref, e = dev(padded(clean, 20003)), dev(padded(est, 20001))
    lens = dev(lens_host, np.int32)
    si, seg = torch.empty(3, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
    parts, nf = torch.empty((3, 3), dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call():
        lib = _lib.load()
        _lib.check(lib.rced_si_sdr(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, si.data_ptr(), parts.data_ptr(), 0,
                                   side.cuda_stream))
        _lib.check(lib.rced_seg_snr(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, 8000, seg.data_ptr(), nf.data_ptr(),
                                    0, side.cuda_stream))

    call()                                             # sizes the stream's workspaces
    side.synchronize()
    first = si.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches
        call()
    for scale in (1.0, 4.0):
        e.mul_(scale)
        for t in (si, seg, parts, nf):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (si, seg, parts, nf)]
        call()                                         # the eager call on the changed input: the same bits
        side.synchronize()
        assert all(torch.equal(a, b) or bool((torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(), b.nan_to_num()))
                   for a, b in zip(got, (si, seg, parts, nf)))
        assert torch.equal(got[0], first)              # a gain of 4 on the estimate leaves SI-SDR's bits
    assert nf.tolist() == [330, 235, 0] and math.isnan(float(seg[2]))
    for i in range(3):
        close(float(si[i]), td.si_sdr(clean[i], est[i]), "SI-SDR after replay, row %d" % i)


def test_evaluation_loop_with_extra_scores(built, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTester, FullyCNNTrainer
    from fullycnnspeechenhancement_amd.audio import seg_snr_batch, si_sdr_batch, stoi_batch
    from fullycnnspeechenhancement_amd.engine import evaluate_pcm
    from fullycnnspeechenhancement_amd.metrics import ESTOI, SISDR, SegSNR
    from oracle import rced_np
    names = ("estoi", "si_sdr", "seg_snr")
    weights = rced_np.make_weights("FullyCNNV3", seed=42)
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=weights)
    batches = tg.ragged_batches()
    scores = {name: [] for name in names}
    for _, _, mix, clean in batches:
        pair = eng.evaluate_pcm(mix, clean)
        triple = eng.evaluate_pcm(mix, clean, stoi=True)
        assert len(pair) == 2 and len(triple) == 3               # the default calls return today's tuples
        den, sdr, st, more = eng.evaluate_pcm(mix, clean, stoi=True, extra=names)
        assert all(np.array_equal(a, b) for a, b in zip(den, pair[0])) and np.array_equal(sdr, pair[1]) and np.array_equal(st, triple[2])
        without = eng.evaluate_pcm(mix, clean, extra=("seg_snr", "estoi"))
        assert len(without) == 3 and list(without[2]) == ["seg_snr", "estoi"]
        lens = [len(c) for c in clean]
        c, d = dev(padded(clean, max(lens))), dev(padded(den, max(lens) + 3))
        by_hand = {"estoi": stoi_batch(c, d, lens, extended=True), "si_sdr": si_sdr_batch(c, d, lens), "seg_snr": seg_snr_batch(c, d, lens)}
        assert list(more) == list(names)
        for name in names:
            assert more[name].dtype == np.float64 and more[name].shape == (len(lens),)
            assert np.array_equal(more[name], by_hand[name].cpu().numpy())
            scores[name].extend(more[name].tolist())
        assert np.array_equal(without[2]["estoi"], more["estoi"]) and np.array_equal(without[2]["seg_snr"], more["seg_snr"])
        assert ESTOI()(clean[0], den[0]) == more["estoi"][0] and SISDR()(clean[0], den[0]) == more["si_sdr"][0]
        assert SegSNR()(clean[0], den[0]) == more["seg_snr"][0] and isinstance(SegSNR()(clean[0], den[0]), float)
        assert abs(more["si_sdr"][0] - td.si_sdr(clean[0], den[0])) <= BAR
        assert abs(more["seg_snr"][0] - td.seg_snr(clean[0], den[0], 8000)) <= BAR
    assert all(np.isfinite(v).all() for v in scores.values())
    assert all(eng.extra_scores[name].count == 0 for name in names)
    capsys.readouterr()

    avg = eng.test(batches)                                        # the default line is today's, and the only one
    printed = capsys.readouterr().out
    assert printed == "Average sd_score: %.4f.\n\n" % avg and all(eng.extra_scores[name].count == 0 for name in names)
    avg = eng.test(batches, stoi=True, extra=names)
    printed = capsys.readouterr().out
    assert all(eng.extra_scores[name].count == 5 for name in names) and avg == eng.sdr_score.avg
    for name in names:
        assert abs(eng.extra_scores[name].avg - np.mean(scores[name])) <= 1e-12
    more_line = "Average estoi: %.4f; Average si_sdr: %.4f; Average seg_snr: %.4f.\n" % tuple(eng.extra_scores[n].avg for n in names)
    assert printed == "Average st_score: %.4f; Average sd_score: %.4f.\n\n" % (eng.stoi_score.avg, avg) + more_line + "\n"

    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, weights=weights)
    want = {name: [] for name in names}
    for _, _, mix, clean in batches:
        more = evaluate_pcm(tr.valid_step, mix, clean, 512, 0, extra=names)[2]
        for name in names:
            want[name].extend(more[name].tolist())

    class Log(object):
        lines = []

        def info(self, msg):
            self.lines.append(msg)

    avg = tr.valid(batches, 4, Log())
    assert capsys.readouterr().out == "Epoch: 4, Average sd_score: %.4f.\n\n" % avg and len(Log.lines) == 1
    avg = tr.valid(batches, 5, Log(), extra=names)
    for name in names:
        assert tr.extra_scores[name].count == 5 and abs(tr.extra_scores[name].avg - np.mean(want[name])) <= 1e-12
    line = "Epoch: 5, Average sd_score: %.4f.\n" % avg
    more_line = "Epoch: 5, Average estoi: %.4f; Average si_sdr: %.4f; Average seg_snr: %.4f.\n" % tuple(tr.extra_scores[n].avg for n in names)
    assert capsys.readouterr().out == line + "\n" + more_line + "\n"
    assert Log.lines[1:] == [line, more_line]
    tr.close()
