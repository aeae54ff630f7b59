"""GPU tests of rced_bss_sdr (audio.bss_sdr_batch) against the float64 restatement of its definition (tests/bsseval_np.py,
form (a): the normal equations), and of the evaluation loop's `extra` name "bss_sdr".  mir_eval is not available here:
parity with bss_eval_sources is unpinned.

The bar follows the family's rule (tests/test_sepm_gpu.py): ten times the worst distance, on the same batch, between two
correct float64 evaluations of the definition -- form (a) against (b), direct sums and scipy's Toeplitz solver, and against
(c), the least-squares problem itself, where the utterance is short enough -- with a floor of 1e-12 dB and a hard cap of
5e-5 dB, half a unit of the fourth decimal the loop prints.  Every test asserts cond(toeplitz(r)) < 1e7 on the CPU for
every utterance it uses before it trusts the bar ("pick another seed" otherwise).  The energies carry the same bar from dB
to a relative distance (ln 10 / 10); the filters are compared where cond < 10 only, relative to their largest tap, against
ten times the restatements' own distance with a floor of 10 * (cond 10) * (512 roundings) * 2^-52 = 1.1e-11.
Every comparison prints its figure; DESIGN.md 3.4c records the measured ones."""

import functools
import math

import numpy as np
import pytest

import bsseval_np as bn
import stoi_np as sn
import td_metrics_np as td
import test_stoi_gpu as tg
from test_stoi_gpu import dev, padded, strided

pytestmark = pytest.mark.gpu

CAP = 5e-5
FLOOR = 1e-12
COND_MAX = 1e7
TO_REL = math.log(10.0) / 10.0
FILTER_FLOOR = 10 * 10 * 512 * 2.0 ** -52
SNRS = (-5, 5, 20)
# 0, 1, 2; the 16-sample block; the matrix instruction's four blocks; 512 taps; 3585 + 511 = 4096, one slice of the projection's
# outputs at 512 taps, and 3586, two; 4095 .. 4097 around a slice of 4096 samples of the correlations (and of the outputs at one
# tap); 8192, two slices, 8200, three; 70,000
LENS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 511, 512, 513, 3585, 3586, 4095, 4096, 4097, 8192, 8200, 70000)
WHITE = (9000, 20001, 30000)              # white-noise references: cond < 10 at every filter length
FILTERS = (1, 2, 15, 16, 17, 33, 512)


def signals():
    clean = [sn.speechlike(L, 500 + i, 8000).astype(np.float32) for i, L in enumerate(LENS)]
    est = [sn.add_white(c.astype(np.float64), SNRS[i % 3], 600 + i).astype(np.float32) if len(c) else c.copy() for i, c in enumerate(clean)]
    for j, L in enumerate(WHITE):
        rng = np.random.default_rng(900 + j)
        x = (0.1 * rng.standard_normal(L)).astype(np.float32)
        h = np.array([0.5, 0.0, -0.25, 0.125])
        clean.append(x)
        est.append(sn.add_white(np.convolve(x.astype(np.float64), h)[:L], SNRS[j % 3], 950 + j).astype(np.float32))
    return clean, est


class Reference(object):
    """Form (a) of every pair at one filter length, its distances to (b) and (c), cond(G): computed once per filter length."""

    def __init__(self, F, clean, est):
        self.F, self.clean, self.est = F, clean, est
        self.lens = [len(c) for c in clean]
        self.want, self.cond = [], []
        gap = gap_energy = gap_filter = 0.0
        for c, e in zip(clean, est):
            a = bn.normal(c, e, F)
            self.want.append(a)
            self.cond.append(bn.cond(c, F))
            if len(c) < 2:                           # nan, or an exact fit: compared by rule, not by distance
                continue
            others = [bn.direct(c, e, F)] + ([bn.lstsq(c, e, F)] if len(c) <= bn.LSTSQ_MAX else [])
            for o in others:
                gap = max(gap, abs(a[0] - o[0]))
                gap_energy = max(gap_energy, abs(a[2][0] / o[2][0] - 1), abs(a[2][1] / o[2][1] - 1))
                if self.cond[-1] < 10:
                    gap_filter = max(gap_filter, np.abs(a[1] - o[1]).max() / np.abs(a[1]).max())
        self.gap, self.gap_energy, self.gap_filter = gap, gap_energy, gap_filter
        self.bar = min(max(10 * gap, FLOOR), CAP)
        self.bar_energy = min(max(10 * gap_energy, FLOOR * TO_REL), CAP * TO_REL)
        self.bar_filter = max(10 * gap_filter, FILTER_FLOOR)

    def check_cond(self, rows=None):
        worst = max(self.cond[i] for i in (rows if rows is not None else range(len(self.lens))) if self.lens[i] > 0)
        print("F = %d: largest cond(G) of the batch %.3e" % (self.F, worst))
        assert worst < COND_MAX, "cond(G) = %.3e: pick another seed" % worst


@functools.lru_cache(maxsize=None)
def the_signals():
    return signals()


@functools.lru_cache(maxsize=None)
def reference(F):
    return Reference(F, *the_signals())


def compare(ref, score, filt, energies):
    worst = worst_energy = worst_filter = 0.0
    compared_filters = 0
    for i, L in enumerate(ref.lens):
        want, c, (ss, se) = ref.want[i]
        got = float(score[i])
        if L == 0:
            assert math.isnan(got) and math.isnan(want) and energies[i].tolist() == [0.0, 0.0]
            continue
        if L == 1:                                   # the one sample is matched up to a rounding: 2^-104 in energy, 313 dB
            print("L = 1: %r dB (restatement %r)" % (got, want))
            assert got > 250.0 and want > 250.0
            assert abs(filt[i, 0] / c[0] - 1) <= 4 * 2.0 ** -52 and not filt[i, 1:].any()
            continue
        worst = max(worst, abs(got - want))
        worst_energy = max(worst_energy, abs(energies[i, 0] / ss - 1), abs(energies[i, 1] / se - 1))
        if ref.cond[i] < 10:
            compared_filters += 1
            worst_filter = max(worst_filter, np.abs(filt[i] - c).max() / np.abs(c).max())
    print("F = %d: restatement (a) against (b), (c): %.3e dB, energies %.3e, filters %.3e" % (ref.F, ref.gap, ref.gap_energy, ref.gap_filter))
    print("F = %d: device against (a): worst score distance %.3e dB (bar %.3e, cap %.1e), energies %.3e relative (bar %.3e), "
          "filters of %d well-conditioned references %.3e of the largest tap (bar %.3e)"
          % (ref.F, worst, ref.bar, CAP, worst_energy, ref.bar_energy, compared_filters, worst_filter, ref.bar_filter))
    assert compared_filters >= len(WHITE)
    assert worst <= ref.bar <= CAP
    assert worst_energy <= ref.bar_energy
    assert worst_filter <= ref.bar_filter


@pytest.mark.parametrize("F", FILTERS)
def test_parity_with_the_restatement(built, F):
    """Measured on an MI355X (DESIGN.md 3.4c records the run): see the printed figures."""
    from fullycnnspeechenhancement_amd.audio import bss_sdr_batch
    ref = reference(F)
    ref.check_cond()                                                              # before any device call
    width = max(ref.lens)
    c, e = strided(ref.clean, width + 7), strided(ref.est, width + 13, fill=-3.0)    # two unequal strides, junk past every length
    score, filt, energies = (t.cpu().numpy() for t in bss_sdr_batch(c, e, list(ref.lens), F, detail=True))
    assert score.dtype == np.float64 and score.shape == (len(ref.lens),) and filt.shape == (len(ref.lens), F) and energies.shape == (len(ref.lens), 2)
    compare(ref, score, filt, energies)
    plain = bss_sdr_batch(c, e, list(ref.lens), F).cpu().numpy()
    assert plain.tobytes() == score.tobytes()                                     # the detail changes no bit of the score


def test_one_tap_is_si_sdr(built):
    from fullycnnspeechenhancement_amd.audio import bss_sdr_batch, si_sdr_batch
    ref = reference(1)
    ref.check_cond()
    width = max(ref.lens)
    c, e = dev(padded(ref.clean, width)), dev(padded(ref.est, width))
    a, b = bss_sdr_batch(c, e, list(ref.lens), 1).cpu().numpy(), si_sdr_batch(c, e, list(ref.lens)).cpu().numpy()
    worst = 0.0
    for i, L in enumerate(ref.lens):
        if L == 0:
            assert math.isnan(a[i]) and math.isnan(b[i])
        elif L == 1:
            assert a[i] > 250.0 and b[i] > 250.0
        else:
            worst = max(worst, abs(a[i] - b[i]), abs(a[i] - td.si_sdr(ref.clean[i], ref.est[i])))
    print("one tap against si_sdr_batch and its restatement: worst distance %.3e dB (bar %.3e)" % (worst, ref.bar))
    assert worst <= ref.bar


def test_special_values(built):
    from fullycnnspeechenhancement_amd.audio import bss_sdr_batch
    clean, est = the_signals()
    i = LENS.index(4097)
    x, y = clean[i], est[i]
    nan_y = y.copy()
    nan_y[77] = np.nan
    rows_x = [x, np.zeros(4097, np.float32), x, x, x]
    rows_y = [y, y, np.zeros(4097, np.float32), nan_y, (8.0 * x).astype(np.float32)]
    for F in (1, 17, 512):
        s, filt, en = (t.cpu().numpy() for t in bss_sdr_batch(dev(np.stack(rows_x)), dev(np.stack(rows_y)), None, F, detail=True))
        assert math.isfinite(s[0]) and math.isnan(s[1]) and math.isnan(s[2]) and math.isnan(s[3])      # x = 0, y = 0, a nan
        assert not filt[2].any() and en[2].tolist() == [0.0, 0.0]                                      # y = 0: c = 0, 0 / 0
        assert s[4] > 250.0 and abs(filt[4, 0] - 8.0) <= 1e-9 and np.abs(filt[4, 1:]).max(initial=0.0) <= 1e-9      # y = 8 x
    empty = bss_sdr_batch(dev(np.stack(rows_x)), dev(np.stack(rows_y)), [0] * 5)
    assert empty.shape == (5,) and bool(empty.isnan().all())                                           # L = 0


def test_scores_do_not_depend_on_the_batch_around_them(built):
    from fullycnnspeechenhancement_amd.audio import bss_sdr_batch
    clean, est = the_signals()
    pick = [LENS.index(L) for L in (8200, 17, 3586, 4096, 513, 2, 4097)]
    lens = [LENS[i] for i in pick]
    c7, e7 = [clean[i] for i in pick], [est[i] for i in pick]
    width = max(lens)

    def bits(out):
        score, filt, en = (t.cpu().numpy() for t in out)
        return [(score[i].tobytes(), filt[i].tobytes(), en[i].tobytes()) for i in range(len(score))]

    for F in (512, 17, 1):
        full = bits(bss_sdr_batch(dev(padded(c7, width)), dev(padded(e7, width)), lens, F, detail=True))
        again = bits(bss_sdr_batch(dev(padded(c7, width)), dev(padded(e7, width)), lens, F, detail=True))
        assert full == again                                                                 # run to run
        order = [3, 0, 5, 2, 6, 1, 4]                                                        # other rows, strides, junk
        moved = bits(bss_sdr_batch(strided([c7[i] for i in order], width + 5, fill=-1e3), strided([e7[i] for i in order], width + 10, fill=9e9),
                                   [lens[i] for i in order], F, detail=True))
        assert moved == [full[i] for i in order]
        for i in (0, 2, 3, 6):                                                               # alone, exactly as long as itself
            assert bits(bss_sdr_batch(dev(c7[i][None]), dev(e7[i][None]), None, F, detail=True)) == full[i:i + 1]
            assert bits(bss_sdr_batch(dev(c7[i][None]), dev(e7[i][None]), [lens[i]], F, detail=True)) == full[i:i + 1]


def test_second_call_allocates_nothing_and_nothing_past_a_length_is_read(built):
    """The C ABI on a side stream: after one call of the shape a capture succeeds (an allocation inside a capture is an
    error) and replays to the eager call's bits; the rows carry nan past every length."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lens_host = [9000, 4321, 0]
    clean = [sn.speechlike(L, 60 + i).astype(np.float32) for i, L in enumerate(lens_host)]
    est = [sn.add_white(c.astype(np.float64), 5, 70 + i).astype(np.float32) if len(c) else c.copy() for i, c in enumerate(clean)]
    assert max(bn.cond(c, 512) for c in clean[:2]) < COND_MAX
    ref, e = dev(padded(clean, 9003, fill=np.nan)), dev(padded(est, 9001, fill=np.nan))
    lens = dev(lens_host, np.int32)
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    filt = torch.empty((3, 512), dtype=torch.float64, device="cuda")
    en = torch.empty((3, 2), dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call():
        _lib.check(_lib.load().rced_bss_sdr(ref.data_ptr(), 9003, e.data_ptr(), 9001, lens.data_ptr(), 3, 512, out.data_ptr(), filt.data_ptr(),
                                            en.data_ptr(), 0, side.cuda_stream))

    call()                                             # sizes the stream's workspace
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches
        call()
    e.mul_(0.5)                                        # another input: the replay computes, it does not repeat
    for t in (out, filt, en):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (out, filt, en)]
    call()
    side.synchronize()
    same = lambda a, b: torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0))      # noqa: E731
    assert all(same(a, b) for a, b in zip(got, (out, filt, en)))
    assert torch.isfinite(out[:2]).all() and math.isnan(float(out[2]))
    for i in range(2):                                 # scored on 0.5 y: the score keeps its value under the gain
        half = (0.5 * est[i]).astype(np.float32)
        bar = min(max(10 * abs(bn.bss_sdr(clean[i], half) - bn.direct(clean[i], half)[0]), FLOOR), CAP)
        assert abs(float(out[i]) - bn.bss_sdr(clean[i], half)) <= bar and abs(float(out[i]) - bn.bss_sdr(clean[i], est[i])) <= 1e-9


def test_evaluation_loop_with_the_projection_score(built, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTester, FullyCNNTrainer
    from fullycnnspeechenhancement_amd.audio import bss_sdr_batch, si_sdr_batch
    from fullycnnspeechenhancement_amd.engine import evaluate_pcm
    from fullycnnspeechenhancement_amd.metrics import BSSSDR
    from oracle import rced_np
    names = ("bss_sdr", "si_sdr")
    weights = rced_np.make_weights("FullyCNNV3", seed=42)
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=weights)
    batches = tg.ragged_batches()                                  # five short utterances in two batches
    scores = {name: [] for name in names}
    figures = []                                                   # printed last: capsys.readouterr() below swallows what came before
    for _, _, mix, clean in batches:
        worst_cond = max(bn.cond(c, 512) for c in clean)
        figures.append("largest cond(G) of the batch %.3e" % worst_cond)
        assert worst_cond < COND_MAX                               # before the bar is trusted
        den, sdr = eng.evaluate_pcm(mix, clean)
        den2, sdr2, more = eng.evaluate_pcm(mix, clean, extra=names)
        assert all(np.array_equal(a, b) for a, b in zip(den, den2)) and np.array_equal(sdr, sdr2) and list(more) == list(names)
        gap = max(abs(bn.normal(c, d)[0] - bn.direct(c, d)[0]) for c, d in zip(clean, den))
        bar = min(max(10 * gap, FLOOR), CAP)
        worst = max(abs(more["bss_sdr"][i] - bn.bss_sdr(c, d)) for i, (c, d) in enumerate(zip(clean, den)))
        figures.append("the loop's bss_sdr against the restatement on the returned audio: %.3e dB (bar %.3e)" % (worst, bar))
        assert worst <= bar <= CAP
        lens = [len(c) for c in clean]
        c, d = dev(padded(clean, max(lens))), dev(padded(den, max(lens) + 3))
        by_hand = {"bss_sdr": bss_sdr_batch(c, d, lens), "si_sdr": si_sdr_batch(c, d, lens)}
        for name in names:
            assert more[name].dtype == np.float64 and more[name].shape == (len(lens),)
            assert np.array_equal(more[name], by_hand[name].cpu().numpy())
            scores[name].extend(more[name].tolist())
        assert BSSSDR()(clean[0], den[0]) == more["bss_sdr"][0] and isinstance(BSSSDR(16)(clean[0], den[0]), float)
        assert (more["bss_sdr"] >= more["si_sdr"] - 1e-9).all()                  # 512 taps never fit worse than one
    assert all(np.isfinite(v).all() for v in scores.values()) and len(scores["bss_sdr"]) == 5
    assert all(m.count == 0 for m in eng.extra_scores.values()) and "bss_sdr" in eng.extra_scores
    capsys.readouterr()
    plain = FullyCNNTester(net_work="FullyCNNV3", weights=weights)
    avg0 = plain.test(batches)
    assert capsys.readouterr().out == "Average sd_score: %.4f.\n\n" % avg0      # the default call prints today's line alone
    avg = eng.test(batches, extra=names)
    printed = capsys.readouterr().out
    assert avg == avg0 and all(eng.extra_scores[name].count == 5 for name in names)
    for name in names:
        assert abs(eng.extra_scores[name].avg - np.mean(scores[name])) <= 1e-12 * max(1.0, abs(np.mean(scores[name])))
    more_line = "Average bss_sdr: %.4f; Average si_sdr: %.4f.\n" % tuple(eng.extra_scores[n].avg for n in names)
    assert printed == "Average sd_score: %.4f.\n\n" % avg + more_line + "\n"

    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, weights=weights)
    want = {name: [] for name in names}
    for _, _, mix, clean in batches:
        den, _, more = evaluate_pcm(tr.valid_step, mix, clean, 512, 0, extra=names)
        gap = max(abs(bn.normal(c, d)[0] - bn.direct(c, d)[0]) for c, d in zip(clean, den))
        worst = max(abs(more["bss_sdr"][i] - bn.bss_sdr(c, d)) for i, (c, d) in enumerate(zip(clean, den)))
        figures.append("valid's bss_sdr against the restatement on the returned audio: %.3e dB (bar %.3e)" % (worst, min(max(10 * gap, FLOOR), CAP)))
        assert worst <= min(max(10 * gap, FLOOR), CAP)
        for name in names:
            want[name].extend(more[name].tolist())

    class Log(object):
        lines = []

        def info(self, msg):
            self.lines.append(msg)

    capsys.readouterr()
    avg = tr.valid(batches, 5, Log(), extra=names)
    for name in names:
        assert tr.extra_scores[name].count == 5 and abs(tr.extra_scores[name].avg - np.mean(want[name])) <= 1e-12 * max(1.0, abs(np.mean(want[name])))
    line = "Epoch: 5, Average sd_score: %.4f.\n" % avg
    more_line = "Epoch: 5, Average bss_sdr: %.4f; Average si_sdr: %.4f.\n" % tuple(tr.extra_scores[n].avg for n in names)
    assert capsys.readouterr().out == line + "\n" + more_line + "\n" and Log.lines == [line, more_line]
    tr.close()
    print("\n".join(figures))
