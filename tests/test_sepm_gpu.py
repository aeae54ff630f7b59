"""GPU tests of rced_llr / rced_wss (audio.llr_batch, audio.wss_batch) against the float64 restatement of their definitions
(tests/sepm_np.py), and of the evaluation loop's `extra` names "llr" and "wss".

Clearance.  A slope's sign decides which peak a band is weighed by, so every test first asserts, on the CPU, that no slope
of any frame of either signal in its batch lies within 1e-8 dB of zero: the device's energies land some 1e-12 dB from the
restatement's, and a flipped decision cannot hide as a tolerance.  The seeds below were picked so that this holds (white
noise under every band keeps the slopes of these signals some 1e-5 dB and more from zero).

The bar is not a constant.  It is ten times the worst distance, on the same batch, between the restatement and its own
second evaluation -- the DFT by np.fft.rfft instead of the matrix product, the autocorrelation sums from the other end --
with a floor of 1e-12: how far two correct float64 evaluations of one definition lie apart, times the factor of ten DESIGN.md
3.4c uses.  Hard caps: 5e-5 for LLR, 5e-5 relative for WSS, half a unit of the fourth decimal the loop prints.
Every comparison prints its figure."""

import functools
import math

import numpy as np
import pytest

import sepm_np as sp
import stoi_np as sn
import test_stoi_gpu as tg
from test_stoi_gpu import dev, padded, strided

pytestmark = pytest.mark.gpu

CAP = 5e-5
CLEARANCE = 1e-8
SNRS = (-5, 5, 20)


def length_for(nf, fs, more=0):
    w, h = sp.framing(fs)
    return w + (nf - 1) * h + more


# 8 kHz: no frame, one, two; 10 .. 17 around the LLR frame kernel's 16 frames per workgroup; 31 .. 33 around the WSS GEMM's
# tile of 32 frames; 63 .. 65 (two tiles, four LLR workgroups); 255 .. 257 around the 256 frames a workgroup of the
# recursion, slope and ranking kernels takes, and a ranking pass; 70,000 samples (1,163 frames: five passes)
LENS_8K = (0, 239, 240, 299, 300) + tuple(length_for(nf, 8000, more) for nf, more in (
    (10, 0), (11, 7), (15, 59), (16, 0), (17, 1), (31, 0), (32, 30), (33, 0), (63, 0), (64, 59), (65, 0), (255, 0), (256, 13), (257, 0))) \
    + (70000,)
# 16 kHz: one frame; 15 .. 17 around the GEMM's tile of 16 frames; about 200
LENS_16K = tuple(length_for(nf, 16000, more) for nf, more in ((1, 0), (15, 0), (16, 119), (17, 0), (200, 40)))


def rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got - want)


class Reference(object):
    """The restatement, twice, of ragged gated-harmonic rows against mixtures at -5, 5, 20 dB; computed once per batch."""

    def __init__(self, lens, fs, seed):
        self.lens, self.fs = lens, fs
        self.clean = [sn.speechlike(L, seed + i, fs).astype(np.float32) for i, L in enumerate(lens)]
        self.est = [sn.add_white(c.astype(np.float64), SNRS[i % 3], seed + 100 + i).astype(np.float32) if len(c) else c.copy()
                    for i, c in enumerate(self.clean)]
        self.nf = [sp.num_frames(L, fs) for L in lens]
        self.llr_frames, self.wss_frames, self.clearance = [], [], np.inf
        gap_llr = gap_wss = 0.0
        for c, e in zip(self.clean, self.est):
            d1, d2 = sp.llr_frames(c, e, fs), sp.llr_frames(c, e, fs, reverse=True)
            (w1, clear), (w2, _) = sp.wss_frames(c, e, fs), sp.wss_frames(c, e, fs, "rfft")
            self.llr_frames.append(d1)
            self.wss_frames.append(w1)
            self.clearance = min(self.clearance, clear)
            if len(d1):
                gap_llr = max(gap_llr, np.abs(d1 - d2).max(), abs(sp.llr_from_frames(d1) - sp.llr_from_frames(d2)),
                              abs(sp.llr_from_frames(d1, None) - sp.llr_from_frames(d2, None)))
                gap_wss = max(gap_wss, np.abs(w1 / w2 - 1).max(), rel(sp.lowest_mean(w1), sp.lowest_mean(w2)))
        self.llr = [sp.llr_from_frames(d) for d in self.llr_frames]
        self.llr_unlimited = [sp.llr_from_frames(d, None) for d in self.llr_frames]
        self.wss = [sp.lowest_mean(d) for d in self.wss_frames]
        self.gap_llr, self.gap_wss = gap_llr, gap_wss
        self.bar_llr, self.bar_wss = min(max(10 * gap_llr, 1e-12), CAP), min(max(10 * gap_wss, 1e-12), CAP)

    def check_clearance(self):
        print("smallest |slope| of the batch: %.3e dB" % self.clearance)
        assert self.clearance >= CLEARANCE, "a slope sits %.3e dB from zero: pick another seed" % self.clearance


@functools.lru_cache(maxsize=None)
def batch_8k():
    return Reference(LENS_8K, 8000, 500)


@functools.lru_cache(maxsize=None)
def batch_16k():
    return Reference(LENS_16K, 16000, 700)


def compare(ref, scores, nf, frames, want_scores, want_frames, bar, dist, what):
    worst_score = worst_frame = 0.0
    for i, L in enumerate(ref.lens):
        assert int(nf[i]) == ref.nf[i] == len(want_frames[i])
        if ref.nf[i] == 0:
            assert math.isnan(scores[i]) and math.isnan(want_scores[i])
            continue
        worst_score = max(worst_score, dist(float(scores[i]), want_scores[i]))
        worst_frame = max(worst_frame, max(dist(float(g), float(w)) for g, w in zip(frames[i, :ref.nf[i]], want_frames[i])))
        assert not frames[i, ref.nf[i]:].any()                                    # past nf: as the wrapper left it
    print("%s at %d Hz: worst score distance %.3e, worst frame distance %.3e, bar %.3e, cap %.1e"
          % (what, ref.fs, worst_score, worst_frame, bar, CAP))
    assert worst_score <= bar <= CAP and worst_frame <= bar, what


@pytest.mark.parametrize("make", (batch_8k, batch_16k))
def test_parity_with_the_restatement(built, make):
    """Measured on an MI355X (DESIGN.md 3.4c records the run): see the printed figures."""
    from fullycnnspeechenhancement_amd.audio import llr_batch, wss_batch
    ref = make()
    ref.check_clearance()                                                         # before any device call
    print("restatement against its second evaluation: LLR %.3e, WSS %.3e relative" % (ref.gap_llr, ref.gap_wss))
    width = max(ref.lens)
    c, e = strided(ref.clean, width + 7), strided(ref.est, width + 13, fill=-3.0)    # two unequal strides, junk past every length
    lens = list(ref.lens)
    score, nf, frames = (t.cpu().numpy() for t in llr_batch(c, e, lens, ref.fs, detail=True))
    assert frames.shape[0] == len(lens) and frames.shape[1] >= max(ref.nf)
    compare(ref, score, nf, frames, ref.llr, ref.llr_frames, ref.bar_llr, lambda a, b: abs(a - b), "LLR")
    unlimited = llr_batch(c, e, lens, ref.fs, limit=None).cpu().numpy()
    worst = max(abs(float(unlimited[i]) - ref.llr_unlimited[i]) for i in range(len(lens)) if ref.nf[i])
    print("LLR without the limit: worst score distance %.3e" % worst)
    assert worst <= ref.bar_llr
    assert any(a < b for a, b in zip(ref.llr, ref.llr_unlimited) if not math.isnan(a))       # the limit is active somewhere
    score, nf, frames = (t.cpu().numpy() for t in wss_batch(c, e, lens, ref.fs, detail=True))
    compare(ref, score, nf, frames, ref.wss, ref.wss_frames, ref.bar_wss, rel, "WSS")


def test_identity_and_special_values(built):
    from fullycnnspeechenhancement_amd.audio import llr_batch, wss_batch
    ref = batch_8k()
    i = LENS_8K.index(length_for(65, 8000))
    x = dev(np.stack([ref.clean[i], ref.est[i]]))
    for fn in (llr_batch, wss_batch):
        same = fn(x, x).cpu().numpy()
        assert same.tolist() == [0.0, 0.0]                                        # y = x: exactly 0
    zero = dev(np.zeros((1, 600), np.float32))                                    # digital silence: the + eps keeps LLR finite
    assert float(llr_batch(zero, zero)[0]) == 0.0
    score, nf, frames = llr_batch(x[:1], x[1:], [100], detail=True)
    assert math.isnan(float(score[0])) and int(nf[0]) == 0 and frames.shape == (1, 65) and not frames.cpu().numpy().any()


def test_scores_do_not_depend_on_the_batch_around_them(built):
    from fullycnnspeechenhancement_amd.audio import llr_batch, wss_batch
    ref = batch_8k()
    ref.check_clearance()
    pick = [LENS_8K.index(length_for(nf, 8000, more)) for nf, more in ((257, 0), (33, 0), (64, 59), (17, 1), (256, 13), (2, 0))]
    lens = [LENS_8K[i] for i in pick]
    clean, est = [ref.clean[i] for i in pick], [ref.est[i] for i in pick]
    width = max(lens)

    def bits(out):
        score, nf, frames = (t.cpu().numpy() for t in out)
        return [(score[i].tobytes(), int(nf[i]), frames[i, :nf[i]].tobytes()) for i in range(len(score))]

    for fn in (llr_batch, wss_batch):
        full = bits(fn(dev(padded(clean, width)), dev(padded(est, width)), lens, detail=True))
        again = bits(fn(dev(padded(clean, width)), dev(padded(est, width)), lens, detail=True))
        assert full == again                                                                 # run to run
        order = [3, 0, 5, 2, 1, 4]                                                           # other rows, strides, junk
        moved = bits(fn(strided([clean[i] for i in order], width + 5, fill=-1e3), strided([est[i] for i in order], width + 10, fill=9e9),
                        [lens[i] for i in order], detail=True))
        assert moved == [full[i] for i in order]
        for i in (0, 2, 3):                                                                  # alone, exactly as long as itself
            assert bits(fn(dev(clean[i][None]), dev(est[i][None]), detail=True)) == full[i:i + 1]
    r16 = batch_16k()
    r16.check_clearance()
    c, e = dev(padded(r16.clean, max(LENS_16K))), dev(padded(r16.est, max(LENS_16K)))
    for fn in (llr_batch, wss_batch):
        full = bits(fn(c, e, list(LENS_16K), 16000, detail=True))
        assert bits(fn(dev(r16.clean[3][None]), dev(r16.est[3][None]), None, 16000, detail=True)) == full[3:4]


def test_second_call_allocates_nothing_and_nothing_past_a_length_is_read(built):
    """The C ABI on a side stream: after one call of the shape, a capture of both entries succeeds (an allocation or a copy
    from the host inside a capture is an error) and replays to the eager call's bits.  The rows carry nan past every
    length and the per-frame buffers a sentinel past every nf: no score sees the one, no store reaches the other."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lens_host = [20000, 14321, 100]
    clean = [sn.speechlike(L, 60 + i).astype(np.float32) for i, L in enumerate(lens_host)]
    est = [sn.add_white(c.astype(np.float64), 5, 70 + i).astype(np.float32) for i, c in enumerate(clean)]
    clear = min(sp.wss_frames(c, e, 8000)[1] for c, e in zip(clean[:2], est[:2]))
    assert clear >= CLEARANCE, "a slope sits %.3e dB from zero: pick another seed" % clear       # before any device call
    want_llr = [sp.llr(c, e, 8000) for c, e in zip(clean, est)]
    want_wss = [sp.wss(c, e, 8000) for c, e in zip(clean, est)]
    ref, e = dev(padded(clean, 20003, fill=np.nan)), dev(padded(est, 20001, fill=np.nan))
    lens = dev(lens_host, np.int32)
    most = sp.num_frames(20001, 8000)
    llr, wss = torch.empty(3, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
    fl, fw = (torch.full((3, most + 2), -77.0, dtype=torch.float64, device="cuda") for _ in range(2))
    nl, nw = (torch.empty(3, dtype=torch.int32, device="cuda") for _ in range(2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call():
        lib = _lib.load()
        _lib.check(lib.rced_llr(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, 8000, 2.0, llr.data_ptr(), fl.data_ptr(),
                                most + 2, nl.data_ptr(), 0, side.cuda_stream))
        _lib.check(lib.rced_wss(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, 8000, wss.data_ptr(), fw.data_ptr(),
                                most + 2, nw.data_ptr(), 0, side.cuda_stream))

    call()                                             # sizes the stream's workspaces, uploads the tables
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches
        call()
    e.mul_(0.5)                                        # another input: the replay computes, it does not repeat
    for t in (llr, wss, nl, nw):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (llr, wss, fl, fw, nl, nw)]
    call()
    side.synchronize()
    same = lambda a, b: torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0))      # noqa: E731
    assert all(same(a, b) for a, b in zip(got, (llr, wss, fl, fw, nl, nw)))
    nf = [sp.num_frames(L, 8000) for L in lens_host]
    assert nl.tolist() == nw.tolist() == nf == [330, 235, 0]
    for scores, frames in ((llr, fl), (wss, fw)):
        assert torch.isfinite(scores[:2]).all() and math.isnan(float(scores[2]))
        for i in range(3):
            assert torch.isfinite(frames[i, :nf[i]]).all() and bool((frames[i, nf[i]:] == -77.0).all())
    # scored on 0.5 y: LLR keeps its value under the gain (up to the eps term), WSS does not
    half = [(0.5 * v).astype(np.float32) for v in est[:2]]
    for i in range(2):
        assert abs(float(llr[i]) - sp.llr(clean[i], half[i], 8000)) <= CAP and abs(float(llr[i]) - want_llr[i]) <= 1e-9
        assert rel(float(wss[i]), sp.wss(clean[i], half[i], 8000)) <= CAP
    assert want_wss[0] > 0


def test_evaluation_loop_with_the_spectral_scores(built, capsys):
    """Through the overlap-add rebuild: the reference rebuild opens every row with a run of zeros, the first frame of some rows
    then has neighbouring bands on the 1e-10 floor, a slope of exactly 0, and the clearance precondition does not hold."""
    from fullycnnspeechenhancement_amd import FullyCNNTester
    from fullycnnspeechenhancement_amd.audio import llr_batch, seg_snr_batch, wss_batch
    from fullycnnspeechenhancement_amd.metrics import LLR, WSS, composite
    from oracle import rced_np
    names = ("llr", "wss", "seg_snr")
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=rced_np.make_weights("FullyCNNV3", seed=42))
    batches = tg.ragged_batches()                                  # five short utterances in two batches
    scores = {name: [] for name in names}
    unlimited = []
    for _, _, mix, clean in batches:
        den, sdr = eng.evaluate_pcm(mix, clean, rebuild="ola")     # the audio first: the clearance is asserted on the CPU
        clear = min(sp.wss_frames(c, d, 8000)[1] for c, d in zip(clean, den))
        print("smallest |slope| of the batch: %.3e dB" % clear)
        assert clear >= CLEARANCE
        den2, sdr2, more = eng.evaluate_pcm(mix, clean, extra=names, rebuild="ola")
        assert all(np.array_equal(a, b) for a, b in zip(den, den2)) and np.array_equal(sdr, sdr2) and list(more) == list(names)
        lens = [len(c) for c in clean]
        c, d = dev(padded(clean, max(lens))), dev(padded(den, max(lens) + 3))
        by_hand = {"llr": llr_batch(c, d, lens), "wss": wss_batch(c, d, lens), "seg_snr": seg_snr_batch(c, d, lens)}
        for name in names:
            assert more[name].dtype == np.float64 and more[name].shape == (len(lens),)
            assert np.array_equal(more[name], by_hand[name].cpu().numpy())
            scores[name].extend(more[name].tolist())
        unlimited.extend(llr_batch(c, d, lens, limit=None).cpu().numpy().tolist())
        assert LLR()(clean[0], den[0]) == more["llr"][0] and WSS()(clean[0], den[0]) == more["wss"][0]
        assert LLR(limit=None)(clean[0], den[0]) == unlimited[-len(lens)] and isinstance(WSS()(clean[0], den[0]), float)
        assert abs(more["llr"][0] - sp.llr(clean[0], den[0], 8000)) <= CAP        # the loop's "llr" is the limited form
        assert rel(more["wss"][0], sp.wss(clean[0], den[0], 8000)) <= CAP
    assert all(np.isfinite(v).all() for v in scores.values()) and len(scores["llr"]) == 5
    assert all(eng.extra_scores[name].count == 0 for name in names)
    capsys.readouterr()
    avg = eng.test(batches, extra=names, rebuild="ola")
    printed = capsys.readouterr().out
    assert all(eng.extra_scores[name].count == 5 for name in names)
    for name in names:
        assert abs(eng.extra_scores[name].avg - np.mean(scores[name])) <= 1e-12 * max(1.0, abs(np.mean(scores[name])))
    more_line = "Average llr: %.4f; Average wss: %.4f; Average seg_snr: %.4f.\n" % tuple(eng.extra_scores[n].avg for n in names)
    assert printed == "Average sd_score: %.4f.\n\n" % avg + more_line + "\n"

    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd.engine import evaluate_pcm
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, weights=rced_np.make_weights("FullyCNNV3", seed=42))
    want = {name: [] for name in names}
    for _, _, mix, clean in batches:
        more = evaluate_pcm(tr.valid_step, mix, clean, 512, 0, extra=names, rebuild="ola")[2]
        for name in names:
            want[name].extend(more[name].tolist())

    class Log(object):
        lines = []

        def info(self, msg):
            self.lines.append(msg)

    avg = tr.valid(batches, 5, Log(), extra=names, rebuild="ola")
    for name in names:
        assert tr.extra_scores[name].count == 5 and abs(tr.extra_scores[name].avg - np.mean(want[name])) <= 1e-12 * max(1.0, abs(np.mean(want[name])))
    line = "Epoch: 5, Average sd_score: %.4f.\n" % avg
    more_line = "Epoch: 5, Average llr: %.4f; Average wss: %.4f; Average seg_snr: %.4f.\n" % tuple(tr.extra_scores[n].avg for n in names)
    assert capsys.readouterr().out == line + "\n" + more_line + "\n" and Log.lines == [line, more_line]
    tr.close()

    pesq = np.array([1.5, 2.0, 2.5, 3.0, 3.5])                     # made up: this project does not compute PESQ
    llr_u, wss, seg = np.array(unlimited), np.array(scores["wss"]), np.array(scores["seg_snr"])
    csig, cbak, covl = composite(pesq, llr_u, wss, seg)
    assert np.array_equal(csig, np.clip(3.093 - 1.029 * llr_u + 0.603 * pesq - 0.009 * wss, 1, 5))
    assert np.array_equal(cbak, np.clip(1.634 + 0.478 * pesq - 0.007 * wss + 0.063 * seg, 1, 5))
    assert np.array_equal(covl, np.clip(1.594 + 0.805 * pesq - 0.512 * llr_u - 0.007 * wss, 1, 5))
