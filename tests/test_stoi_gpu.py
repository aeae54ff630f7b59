"""GPU tests of rced_stoi / audio.stoi_batch against the float64 restatement of the published algorithm (tests/stoi_np.py;
the reference's pystoi is not available to this project, so parity is with the restatement and with analytic properties).

The score error has a hard cap of 5e-5 (half a unit of the fourth decimal the reference prints).  The bar asserted is BAR.
Only the DFT products are below float64 -- operands rounded to fp32 and split into three bf16 parts, fp32 accumulation --
so the error is of the order of fp32 sums of 256 terms: a numpy emulation of exactly that arithmetic (fp32 operands, fp32
dot products, everything else float64) lands 8e-9 .. 2.2e-8 from the restatement on signals of this kind.  BAR is ten
times the emulation's worst: room for another summation order inside the matrix pipe, and still 250 times under the cap.
Every comparison prints its figure (DESIGN.md "STOI")."""

import numpy as np
import pytest

import eval_closed_form as cf
import stoi_np as sn

pytestmark = pytest.mark.gpu

CAP = 5e-5
BAR = 2e-7


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.asarray(a, dtype=dtype) if dtype else a, device="cuda")


def padded(rows, width, fill=7.0):
    """Rows of ragged float32 signals in a [N, width] matrix with junk past each length."""
    out = np.full((len(rows), width), fill, np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def strided(rows, stride, fill=7.0):
    """A device view [N, stride - 1] of a [N, stride] buffer: the row stride is wider than the row."""
    return dev(padded(rows, stride, fill))[:, :stride - 1]


def batch(seed=11):
    """Seeded ragged speech-like pairs: gated harmonics with silences; clean against clean + white noise at several SNRs."""
    lens = (65664, 24000, 24001, 30123, 9001, 6001, 13579, 65664)
    snrs = (5, 20, 10, 0, -5, 15, None, -5)                    # None: the estimate is the clean signal
    clean = [sn.speechlike(L, seed + i).astype(np.float32) for i, L in enumerate(lens)]
    est = [(c if s is None else sn.add_white(c.astype(np.float64), s, seed + 100 + i)).astype(np.float32)
           for i, (c, s) in enumerate(zip(clean, snrs))]
    return lens, clean, est


def reference(clean, est, fs=8000):
    """The restatement on the float32 signals the device sees; asserts the condition on the inputs first: no frame's
    energy within 0.01 dB of its utterance's threshold, so a rounding-flipped mask cannot hide as a tolerance."""
    out = []
    for c, e in zip(clean, est):
        d, det, en = sn.stoi_detail(c, e, fs)
        if len(en):
            clearance = np.abs(en - (en.max() - sn.DYN_RANGE)).min()
            assert clearance > 0.01, "a frame sits %.4f dB from the threshold: pick another input" % clearance
        out.append((d, det))
    return out


def test_parity_with_the_restatement(built):
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    lens, clean, est = batch()
    ref = reference(clean, est)
    assert any(det[1] < det[0] for _, det in ref)               # frames really are removed
    d, det = stoi_batch(strided(clean, 65664 + 7), strided(est, 65664 + 13, fill=-3.0), lens, detail=True)
    d, det = d.cpu().numpy(), det.cpu().numpy()
    worst = 0.0
    for i, (r, counts) in enumerate(ref):
        err = abs(d[i] - r)
        worst = max(worst, err)
        print("utterance %d (L %d): F, K, M = %s  stoi %.9f  restatement %.9f  |diff| %.2e" % (i, lens[i], tuple(det[i]), d[i], r, err))
        assert tuple(det[i]) == counts
    print("worst |d_gpu - d_ref| = %.3e (bar %.1e, cap %.1e)" % (worst, BAR, CAP))
    assert worst <= CAP
    assert worst <= BAR


def test_10_khz_skips_the_resampler(built):
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    lens = (12000, 30001, 4097)
    clean = [sn.speechlike(L, 40 + i, fs=10000).astype(np.float32) for i, L in enumerate(lens)]
    est = [sn.add_white(c.astype(np.float64), 3, 50 + i).astype(np.float32) for i, c in enumerate(clean)]
    ref = reference(clean, est, 10000)
    d, det = stoi_batch(dev(padded(clean, 30001)), dev(padded(est, 30001)), lens, sample_rate=10000, detail=True)
    for i, (r, counts) in enumerate(ref):
        err = abs(float(d[i]) - r)
        print("10 kHz utterance %d: %s |diff| %.2e" % (i, counts, err))
        assert tuple(det[i].tolist()) == counts and err <= BAR


def test_edge_values(built):
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    rng = np.random.default_rng(6)
    x = sn.speechlike(24000, 7).astype(np.float32)
    noisy = sn.add_white(x.astype(np.float64), 5, 8).astype(np.float32)
    rows = dev(np.stack([x, noisy, 0.5 * noisy, np.zeros_like(x)]))
    # lengths 0 and 204 (255 samples at 10 kHz: no frame) give exactly 1e-5
    d, det = stoi_batch(rows[:2], rows[:2], [0, 204], detail=True)
    assert d.tolist() == [1e-5, 1e-5] and det.tolist() == [[0, 0, 0], [0, 0, 0]]
    # stoi(x, x) = 1; a gain on the estimate is taken out; an all-zero clean signal scores 0
    d = stoi_batch(rows[[0, 0, 0, 3]], rows[[0, 1, 2, 1]]).cpu().numpy()
    print("self %.12f, noisy %.12f, half %.12f, zero clean %r" % tuple(d))
    assert d[0] >= 1 - 1e-9 and d[0] <= 1 + 1e-9
    assert abs(d[1] - d[2]) <= 1e-9
    assert d[3] == 0
    # 30 frames, all kept -> 29 spectral frames: exactly 1e-5; one more sample -> one segment
    w = rng.standard_normal(4097).astype(np.float32)
    v = (w + 0.3 * rng.standard_normal(4097)).astype(np.float32)
    both = dev(np.stack([w, v]))
    d, det = stoi_batch(both[0:1].repeat(2, 1), both[1:2].repeat(2, 1), [4096, 4097], sample_rate=10000, detail=True)
    assert det.tolist() == [[30, 30, 0], [31, 31, 1]] and float(d[0]) == 1e-5
    assert sn.stoi_detail(w[:4096], v[:4096], 10000)[:2] == (1e-5, (30, 30, 0))
    assert abs(float(d[1]) - sn.stoi(w, v, 10000)) <= BAR


def test_fixture_pairs(built):
    """The reference's own rebuilt signals (tests/golden/eval_ref.npz): cases 0 and 3 are long enough, the rest give 1e-5."""
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    gold = cf.load_fixture()
    long_enough = []
    for i in range(len(gold["cases"])):
        clean = gold["speech_%d" % i].astype(np.float32)
        for nfft in cf.NFFTS:
            est = cf.rebuilt(gold, i, nfft, 1.0)
            (r, counts), = reference([clean], [est])
            d, det = stoi_batch(dev(clean[None]), dev(est[None]), detail=True)
            err = abs(float(d[0]) - r)
            print("fixture case %d nfft %d: %s stoi %.6f |diff| %.2e" % (i, nfft, counts, float(d[0]), err))
            assert tuple(det[0].tolist()) == counts and err <= BAR
            if counts[2]:
                long_enough.append(i)
            else:
                assert float(d[0]) == 1e-5 == r
    assert sorted(set(long_enough)) == [0, 3]


def test_scores_do_not_depend_on_the_batch_around_them(built):
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    lens, clean, est = batch(seed=23)
    lens, clean, est = lens[1:6], clean[1:6], est[1:6]
    width = max(lens)
    full = stoi_batch(dev(padded(clean, width)), dev(padded(est, width)), lens)
    again = stoi_batch(dev(padded(clean, width)), dev(padded(est, width)), lens)
    assert full.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()                    # run to run
    order = [3, 0, 4, 2, 1]                                                          # other rows, other strides, other junk
    moved = stoi_batch(strided([clean[i] for i in order], width + 5, fill=-1e3), strided([est[i] for i in order], width + 10, fill=9e9),
                       [lens[i] for i in order])
    for k, i in enumerate(order):
        assert float(moved[k]) == float(full[i])
    for i in (0, 3):                                                                      # alone, exactly as long as itself
        alone = stoi_batch(dev(clean[i][None]), dev(est[i][None]))
        assert float(alone[0]) == float(full[i])


def test_second_call_allocates_nothing_and_replays_from_a_captured_graph(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lens_host = [20000, 14321, 9000]
    clean = [sn.speechlike(L, 60 + i).astype(np.float32) for i, L in enumerate(lens_host)]
    est = [sn.add_white(c.astype(np.float64), 5, 70 + i).astype(np.float32) for i, c in enumerate(clean)]
    ref, e = dev(padded(clean, 20003)), dev(padded(est, 20001))
    lens = dev(lens_host, np.int32)
    out, det = torch.empty(3, dtype=torch.float64, device="cuda"), torch.empty((3, 3), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call():
        _lib.check(_lib.load().rced_stoi(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, 8000, out.data_ptr(),
                                         det.data_ptr(), 0, side.cuda_stream))

    call()                                             # sizes the stream's workspace, uploads the tables
    side.synchronize()
    first = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, no parallel branches.  An allocation or a copy from the
        call()                                         # host inside a capture is an error: the second call made neither
    for scale in (1.0, 0.25):
        e.mul_(scale)
        out.zero_()
        det.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got, got_det = out.clone(), det.clone()
        call()                                         # the eager call on the changed input: the same bits
        side.synchronize()
        assert torch.equal(out, got) and torch.equal(det, got_det)
        assert (got - first).abs().max().item() <= 1e-9            # a gain on the estimate is normalised out
        assert scale != 1.0 or torch.equal(got, first)
    for i in range(3):
        assert abs(float(out[i]) - sn.stoi(clean[i], est[i], 8000)) <= BAR


def ragged_batches(seed=31):
    out = []
    for j, lens in enumerate(((9000, 4000, 12000), (7000, 10001))):
        clean = [(0.2 * sn.speechlike(L, seed + 10 * j + i)).astype(np.float32) for i, L in enumerate(lens)]
        mix = [sn.add_white(c.astype(np.float64), 5, seed + 50 + 10 * j + i).astype(np.float32) for i, c in enumerate(clean)]
        out.append((None, None, mix, clean))
    return out


def test_evaluate_pcm_with_stoi(built, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTester
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    from fullycnnspeechenhancement_amd.metrics import STOI
    from oracle import rced_np
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=rced_np.make_weights("FullyCNNV3", seed=42))
    batches = ragged_batches()
    scores = []
    for _, _, mix, clean in batches:
        pair = eng.evaluate_pcm(mix, clean)
        assert len(pair) == 2                                      # the default call returns today's pair
        den, sdr, st = eng.evaluate_pcm(mix, clean, stoi=True)
        assert all(np.array_equal(a, b) for a, b in zip(den, pair[0])) and np.array_equal(sdr, pair[1])
        lens = [len(c) for c in clean]
        assert st.dtype == np.float64 and st.shape == (len(lens),)
        by_hand = stoi_batch(dev(padded(clean, max(lens))), dev(padded(den, max(lens) + 3)), lens).cpu().numpy()
        assert np.array_equal(st, by_hand)
        for i in range(len(lens)):
            assert abs(st[i] - sn.stoi(clean[i], den[i], 8000)) <= BAR
        assert STOI()(clean[0], den[0]) == st[0] and isinstance(STOI()(clean[0], den[0]), float)
        scores.extend(st.tolist())
    assert eng.stoi_score.count == 0
    capsys.readouterr()
    avg = eng.test(batches, stoi=True)
    assert eng.stoi_score.count == eng.sdr_score.count == 5
    assert abs(eng.stoi_score.avg - np.mean(scores)) <= 1e-12 and avg == eng.sdr_score.avg
    assert "Average st_score: %.4f; Average sd_score: %.4f." % (eng.stoi_score.avg, avg) in capsys.readouterr().out
    avg = eng.test(batches)                                        # the default line is today's
    printed = capsys.readouterr().out
    assert "Average sd_score: %.4f." % avg in printed and "st_score" not in printed and eng.stoi_score.count == 5


def test_trainer_valid_with_stoi(built, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd.engine import evaluate_pcm
    from oracle import rced_np
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, weights=rced_np.make_weights("FullyCNNV3", seed=42))
    batches = ragged_batches()
    scores = []
    for _, _, mix, clean in batches:
        scores.extend(evaluate_pcm(tr.valid_step, mix, clean, 512, 0, stoi=True)[2].tolist())

    class Log(object):
        lines = []

        def info(self, msg):
            self.lines.append(msg)

    avg = tr.valid(batches, 4, Log(), stoi=True)
    assert tr.stoi_score.count == tr.sdr_score.count == 5 and avg == tr.sdr_score.avg
    assert abs(tr.stoi_score.avg - np.mean(scores)) <= 1e-12
    line = "Epoch: 4, Average st_score: %.4f; Average sd_score: %.4f." % (tr.stoi_score.avg, avg)
    assert line in capsys.readouterr().out and line in Log.lines[0]
    tr.close()
