"""GPU tests of rced_fwseg / rced_cepd (audio.fw_seg_snr_batch, audio.cep_dist_batch) against the float64 restatement of their
definitions (tests/sepm2_np.py), and of the evaluation loop's `extra` names "fw_seg_snr" and "cd".  The harness is
tests/test_sepm_gpu.py's: its lengths, its signals (gated harmonics against mixtures at -5, 5, 20 dB), padded and strided rows.

The bar is not a constant.  It is ten times the worst distance, on the same batch, between the restatement and its own second
evaluation -- the DFT by np.fft.rfft instead of the matrix product, the autocorrelation sums from the other end -- with a
floor of 1e-12: how far two correct float64 evaluations of one definition lie apart, times the factor of ten DESIGN.md 3.4c
uses.  Hard caps: 5e-5 absolute for CD (LLR's), 5e-4 dB for fwSNRseg (half a unit of the third decimal over a 45 dB range).
Every Reference asserts, on the CPU and before any device call, that its own two evaluations stay a factor of ten inside
both caps.  Every comparison prints its figure."""

import functools
import math

import numpy as np
import pytest

import sepm2_np as s2
import sepm_np as sp
import stoi_np as sn
import test_stoi_gpu as tg
from test_sepm2_host import U, eps_term_bound, weighted_mean_slack
from test_sepm_gpu import LENS_8K, LENS_16K, SNRS, length_for
from test_stoi_gpu import dev, padded, strided

pytestmark = pytest.mark.gpu

CAP_CD = 5e-5
CAP_FW = 5e-4

# 8 kHz (tests/test_sepm_gpu.py): 0, 239, 240, 299, 300 samples; 15 .. 17 frames around the autocorrelation kernel's 16 per
# workgroup; 31 .. 33 and 63 .. 65 around the GEMM's tile of 32; 255 .. 257 around the 256 frames a workgroup of the recursion,
# band and ranking kernels takes; 70,000 samples (1,163 frames: five ranking passes).  16 kHz: 1, 15, 16, 17 and 200 frames:
# the 512-bin sum in two passes, tiles of 16 frames, P = 16.


class Reference(object):
    """The restatement, twice, of ragged gated-harmonic rows against mixtures at -5, 5, 20 dB; computed once per batch."""

    def __init__(self, lens, fs, seed, orders=(None,)):
        self.lens, self.fs = lens, fs
        self.clean = [sn.speechlike(L, seed + i, fs).astype(np.float32) for i, L in enumerate(lens)]
        self.est = [sn.add_white(c.astype(np.float64), SNRS[i % 3], seed + 100 + i).astype(np.float32) if len(c) else c.copy()
                    for i, c in enumerate(self.clean)]
        self.nf = [sp.num_frames(L, fs) for L in lens]
        self.fw_frames = [s2.fwseg_frames(c, e, fs) for c, e in zip(self.clean, self.est)]
        self.fw = [s2.plain_mean(d) for d in self.fw_frames]
        self.gap_fw = 0.0
        for c, e, d1 in zip(self.clean, self.est, self.fw_frames):
            if len(d1):
                d2 = s2.fwseg_frames(c, e, fs, "rfft")
                self.gap_fw = max(self.gap_fw, np.abs(d1 - d2).max(), abs(s2.plain_mean(d1) - s2.plain_mean(d2)))
        self.cd_frames, self.cd, self.gap_cd = {}, {}, 0.0
        for order in orders:
            self.cd_frames[order] = [s2.cd_frames(c, e, fs, order) for c, e in zip(self.clean, self.est)]
            self.cd[order] = [sp.lowest_mean(d) for d in self.cd_frames[order]]
            for c, e, d1 in zip(self.clean, self.est, self.cd_frames[order]):
                if len(d1):
                    d2 = s2.cd_frames(c, e, fs, order, reverse=True)
                    self.gap_cd = max(self.gap_cd, np.abs(d1 - d2).max(), abs(sp.lowest_mean(d1) - sp.lowest_mean(d2)))
        print("%d Hz: the restatement against its second evaluation: fwSNRseg %.3e dB, CD %.3e" % (fs, self.gap_fw, self.gap_cd))
        assert 10 * self.gap_fw <= CAP_FW and 10 * self.gap_cd <= CAP_CD, "the two evaluations lie too far apart: pick another seed"
        self.bar_fw, self.bar_cd = max(10 * self.gap_fw, 1e-12), max(10 * self.gap_cd, 1e-12)


@functools.lru_cache(maxsize=None)
def batch_8k():
    return Reference(LENS_8K, 8000, 500, orders=(None, 16))


@functools.lru_cache(maxsize=None)
def batch_16k():
    return Reference(LENS_16K, 16000, 700, orders=(None, 10))


def compare(ref, scores, nf, frames, want_scores, want_frames, bar, cap, what):
    worst_score = worst_frame = 0.0
    for i, L in enumerate(ref.lens):
        assert int(nf[i]) == ref.nf[i] == len(want_frames[i]) == sp.num_frames(L, ref.fs)
        if ref.nf[i] == 0:
            assert math.isnan(scores[i]) and math.isnan(want_scores[i])
            continue
        worst_score = max(worst_score, abs(float(scores[i]) - want_scores[i]))
        worst_frame = max(worst_frame, float(np.abs(frames[i, :ref.nf[i]] - want_frames[i]).max()))
        assert not frames[i, ref.nf[i]:].any()                                    # past nf: as the wrapper left it
    print("%s at %d Hz: worst score distance %.3e, worst frame distance %.3e, bar %.3e, cap %.1e"
          % (what, ref.fs, worst_score, worst_frame, bar, cap))
    assert worst_score <= bar <= cap and worst_frame <= bar, what


def device_rows(ref):
    width = max(ref.lens)
    return strided(ref.clean, width + 7), strided(ref.est, width + 13, fill=-3.0), list(ref.lens)    # two unequal strides, junk past every length


@pytest.mark.parametrize("make", (batch_8k, batch_16k))
def test_parity_with_the_restatement(built, make):
    """Measured on an MI355X (DESIGN.md 3.4c records the run): see the printed figures."""
    from fullycnnspeechenhancement_amd.audio import cep_dist_batch, fw_seg_snr_batch
    ref = make()                                                                  # asserts the restatement's own gap first
    c, e, lens = device_rows(ref)
    score, nf, frames = (t.cpu().numpy() for t in fw_seg_snr_batch(c, e, lens, ref.fs, detail=True))
    assert frames.shape[0] == len(lens) and frames.shape[1] >= max(ref.nf)
    compare(ref, score, nf, frames, ref.fw, ref.fw_frames, ref.bar_fw, CAP_FW, "fwSNRseg")
    assert min(d.min() for d in ref.fw_frames if len(d)) < 0 and max(d.max() for d in ref.fw_frames if len(d)) > 15   # both ends of the range
    score, nf, frames = (t.cpu().numpy() for t in cep_dist_batch(c, e, lens, ref.fs, detail=True))
    compare(ref, score, nf, frames, ref.cd[None], ref.cd_frames[None], ref.bar_cd, CAP_CD, "CD")
    at_limit = sum(int((d == s2.CD_MAX).sum()) for d in ref.cd_frames[None])
    print("frames at CD's limit of 10: %d" % at_limit)
    assert at_limit > 0 and frames.max() == s2.CD_MAX and frames.min() >= 0.0                # the limit is active, and exact
    assert np.array_equal(cep_dist_batch(c, e, lens, ref.fs).cpu().numpy(), score, equal_nan=True)   # without detail: the same bits


@pytest.mark.parametrize("make,order", ((batch_16k, 10), (batch_8k, 16)))
def test_order_argument(built, make, order):
    from fullycnnspeechenhancement_amd import _lib
    from fullycnnspeechenhancement_amd.audio import cep_dist_batch
    ref = make()
    c, e, lens = device_rows(ref)
    score, nf, frames = (t.cpu().numpy() for t in cep_dist_batch(c, e, lens, ref.fs, order=order, detail=True))
    compare(ref, score, nf, frames, ref.cd[order], ref.cd_frames[order], ref.bar_cd, CAP_CD, "CD at order %d" % order)
    default = cep_dist_batch(c, e, lens, ref.fs).cpu().numpy()
    assert not np.array_equal(default, score, equal_nan=True)
    assert np.array_equal(default, cep_dist_batch(c, e, lens, ref.fs, order=sp.lpc_order(ref.fs)).cpu().numpy(), equal_nan=True)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            cep_dist_batch(c, e, lens, ref.fs, order=bad)
        out = dev(np.zeros(len(lens)))
        rc = _lib.load().rced_cepd(c.data_ptr(), c.stride(0), e.data_ptr(), e.stride(0), None, len(lens), ref.fs, bad, out.data_ptr(),
                                   None, 0, None, 0, None)
        assert rc == _lib.RCED_ERR_ARG and not out.cpu().numpy().any()


def test_identity_and_special_values(built):
    """0.5 x: every band of every frame at 35 dB, the frame value their weighted mean -- 35.0 up to that mean's own rounding
    (tests/test_sepm2_host.py, weighted_mean_slack), the score the mean of those.  CD: exactly 0.0 against itself; against
    0.5 x the definition's eps term is left (x + EPS against 0.5 x + EPS): the restatement is held against that term's first-order
    bound per frame, the device against the restatement."""
    from fullycnnspeechenhancement_amd.audio import cep_dist_batch, fw_seg_snr_batch
    ref = batch_8k()
    i = LENS_8K.index(length_for(65, 8000))
    x = ref.clean[i]
    half = (0.5 * x).astype(np.float32)
    rows, halves = dev(np.stack([x, ref.est[i]])), dev(np.stack([half, (0.5 * ref.est[i]).astype(np.float32)]))
    score, nf, frames = (t.cpu().numpy() for t in fw_seg_snr_batch(rows, halves, detail=True))
    slack = weighted_mean_slack()
    print("fwSNRseg of x against 0.5 x: frames within %.3e of 35, scores within %.3e" % (np.abs(frames - 35).max(), np.abs(score - 35).max()))
    assert nf.tolist() == [65, 65] and np.abs(frames - 35.0).max() <= slack and np.abs(score - 35.0).max() <= slack + 65 * U * 35.0
    same = fw_seg_snr_batch(rows, rows).cpu().numpy()
    assert np.abs(same - 35.0).max() <= slack + 65 * U * 35.0
    score, nf, frames = (t.cpu().numpy() for t in cep_dist_batch(rows, rows, detail=True))
    assert score.tolist() == [0.0, 0.0] and not frames.any()                      # y = x: exactly 0
    score, nf, frames = (t.cpu().numpy() for t in cep_dist_batch(rows[:1], halves[:1], detail=True))
    bound = eps_term_bound(x, 8000)
    want = s2.cd_frames(x, half, 8000)
    print("CD of x against 0.5 x: largest frame %.3e (restatement %.3e), score %.3e" % (frames.max(), want.max(), score[0]))
    assert (want <= bound).all() and (frames[0] >= 0).all() and np.abs(frames[0] - want).max() <= ref.bar_cd and 0.0 <= score[0] <= bound.max() + ref.bar_cd
    # no frame: nan, 0 frames, nothing written
    for fn in (fw_seg_snr_batch, cep_dist_batch):
        for fs, short in ((8000, 239), (16000, 479), (8000, 0)):
            score, nf, frames = fn(rows[:1], rows[1:], [short], fs, detail=True)
            assert math.isnan(float(score[0])) and int(nf[0]) == 0 and not frames.cpu().numpy().any()
    # a digitally silent stretch: fwSNRseg is nan in the frames the restatement names, and so is the utterance; CD stays finite
    quiet = x.copy()
    quiet[600:1100] = 0.0
    est = ref.est[i]
    for a, b in ((quiet, est), (est, quiet)):
        want = s2.fwseg_frames(a, b, 8000)
        assert np.flatnonzero(np.isnan(want)).tolist() == [10, 11, 12, 13, 14]
        score, nf, frames = (t.cpu().numpy() for t in fw_seg_snr_batch(dev(np.stack([a, x])), dev(np.stack([b, est])), detail=True))
        assert np.array_equal(np.isnan(frames[0]), np.isnan(want)) and math.isnan(score[0]) and math.isnan(s2.fwseg(a, b, 8000))
        ok = ~np.isnan(want)
        assert np.abs(frames[0][ok] - want[ok]).max() <= ref.bar_fw
        assert np.isfinite(frames[1]).all() and score[1] == fw_seg_snr_batch(dev(x[None]), dev(est[None])).cpu().numpy()[0]   # the neighbour is untouched
        score, nf, frames = (t.cpu().numpy() for t in cep_dist_batch(dev(a[None]), dev(b[None]), detail=True))
        assert np.isfinite(frames).all() and abs(score[0] - s2.cd(a, b, 8000)) <= CAP_CD


def test_scores_do_not_depend_on_the_batch_around_them(built):
    from fullycnnspeechenhancement_amd.audio import cep_dist_batch, fw_seg_snr_batch
    ref = batch_8k()
    pick = [LENS_8K.index(length_for(nf, 8000, more)) for nf, more in ((257, 0), (33, 0), (64, 59), (17, 1), (256, 13), (2, 0))]
    lens = [LENS_8K[i] for i in pick]
    clean, est = [ref.clean[i] for i in pick], [ref.est[i] for i in pick]
    width = max(lens)

    def bits(out):
        score, nf, frames = (t.cpu().numpy() for t in out)
        return [(score[i].tobytes(), int(nf[i]), frames[i, :nf[i]].tobytes()) for i in range(len(score))]

    fns = (fw_seg_snr_batch, cep_dist_batch, functools.partial(cep_dist_batch, order=7))
    for fn in fns:
        full = bits(fn(dev(padded(clean, width)), dev(padded(est, width)), lens, detail=True))
        again = bits(fn(dev(padded(clean, width)), dev(padded(est, width)), lens, detail=True))
        assert full == again                                                                 # run to run
        order = [3, 0, 5, 2, 1, 4]                                                           # other rows, strides, nan past every length
        moved = bits(fn(strided([clean[i] for i in order], width + 5, fill=np.nan), strided([est[i] for i in order], width + 10, fill=np.nan),
                        [lens[i] for i in order], detail=True))
        assert moved == [full[i] for i in order]
        fewer = bits(fn(strided(clean[1:4], width + 1, fill=np.nan), strided(est[1:4], width + 2, fill=9e9), lens[1:4], detail=True))
        assert fewer == full[1:4]                                                            # another N
        for i in (0, 2, 3):                                                                  # alone, exactly as long as itself
            assert bits(fn(dev(clean[i][None]), dev(est[i][None]), detail=True)) == full[i:i + 1]
        assert all(math.isfinite(np.frombuffer(s, np.float64)[0]) for s, _, _ in full)
    r16 = batch_16k()
    c, e = dev(padded(r16.clean, max(LENS_16K), fill=np.nan)), dev(padded(r16.est, max(LENS_16K), fill=np.nan))
    for fn in fns:
        full = bits(fn(c, e, list(LENS_16K), 16000, detail=True))
        for i in (3, 4):
            assert bits(fn(dev(r16.clean[i][None]), dev(r16.est[i][None]), None, 16000, detail=True)) == full[i:i + 1]


def test_second_call_allocates_nothing_and_nothing_past_a_length_is_read(built):
    """The C ABI on a side stream: after one call of the shape, a capture of both entries succeeds (an allocation or a copy
    from the host inside a capture is an error) and replays to the eager call's bits.  The rows carry nan past every
    length and the per-frame buffers a sentinel past every nf: no score sees the one, no store reaches the other."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lens_host = [20000, 14321, 100]
    clean = [sn.speechlike(L, 60 + i).astype(np.float32) for i, L in enumerate(lens_host)]
    est = [sn.add_white(c.astype(np.float64), 5, 70 + i).astype(np.float32) for i, c in enumerate(clean)]
    ref, e = dev(padded(clean, 20003, fill=np.nan)), dev(padded(est, 20001, fill=np.nan))
    lens = dev(lens_host, np.int32)
    most = sp.num_frames(20001, 8000)
    fw, cd = torch.empty(3, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
    ff, fc = (torch.full((3, most + 2), -77.0, dtype=torch.float64, device="cuda") for _ in range(2))
    nw, nc = (torch.empty(3, dtype=torch.int32, device="cuda") for _ in range(2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call():
        lib = _lib.load()
        _lib.check(lib.rced_fwseg(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, 8000, fw.data_ptr(), ff.data_ptr(),
                                  most + 2, nw.data_ptr(), 0, side.cuda_stream))
        _lib.check(lib.rced_cepd(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, 8000, 10, cd.data_ptr(), fc.data_ptr(),
                                 most + 2, nc.data_ptr(), 0, side.cuda_stream))

    call()                                             # sizes the stream's workspaces, uploads the tables
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches
        call()
    e.mul_(0.75)                                       # another input: the replay computes, it does not repeat
    for t in (fw, cd, nw, nc):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (fw, cd, ff, fc, nw, nc)]
    call()
    side.synchronize()
    same = lambda a, b: torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0))      # noqa: E731
    assert all(same(a, b) for a, b in zip(got, (fw, cd, ff, fc, nw, nc)))
    nf = [sp.num_frames(L, 8000) for L in lens_host]
    assert nw.tolist() == nc.tolist() == nf == [330, 235, 0]
    for scores, frames in ((fw, ff), (cd, fc)):
        assert torch.isfinite(scores[:2]).all() and math.isnan(float(scores[2]))
        for i in range(3):
            assert torch.isfinite(frames[i, :nf[i]]).all() and bool((frames[i, nf[i]:] == -77.0).all())
    scaled = [(0.75 * v).astype(np.float32) for v in est[:2]]
    for i in range(2):
        assert abs(float(fw[i]) - s2.fwseg(clean[i], scaled[i], 8000)) <= CAP_FW
        assert abs(float(cd[i]) - s2.cd(clean[i], scaled[i], 8000)) <= CAP_CD


def test_evaluation_loop_with_the_new_scores(built, capsys):
    """N = 3 ragged through a small V3 model and the overlap-add rebuild (the reference rebuild opens every row with a run of
    zeros: a digitally silent first frame, and fwSNRseg is nan as defined)."""
    from fullycnnspeechenhancement_amd import FullyCNNTester, FullyCNNTrainer
    from fullycnnspeechenhancement_amd.audio import cep_dist_batch, fw_seg_snr_batch
    from fullycnnspeechenhancement_amd.metrics import CepDist, FwSegSNR
    from oracle import rced_np
    new, old = ("fw_seg_snr", "cd"), ("llr", "wss")
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=rced_np.make_weights("FullyCNNV3", seed=42))
    batches = tg.ragged_batches()[:1]
    (_, _, mix, clean), = batches
    assert [len(c) for c in clean] == [9000, 4000, 12000]
    den, sdr, more = eng.evaluate_pcm(mix, clean, extra=new, rebuild="ola")
    assert list(more) == list(new)
    lens = [len(c) for c in clean]
    c, d = dev(padded(clean, max(lens))), dev(padded(den, max(lens) + 3))
    by_hand = {"fw_seg_snr": fw_seg_snr_batch(c, d, lens), "cd": cep_dist_batch(c, d, lens)}
    for name in new:
        assert more[name].dtype == np.float64 and more[name].shape == (3,) and np.isfinite(more[name]).all()
        assert np.array_equal(more[name], by_hand[name].cpu().numpy())
    assert FwSegSNR()(clean[0], den[0]) == more["fw_seg_snr"][0] and CepDist()(clean[0], den[0]) == more["cd"][0]
    assert abs(more["fw_seg_snr"][0] - s2.fwseg(clean[0], den[0], 8000)) <= CAP_FW
    assert abs(more["cd"][0] - s2.cd(clean[0], den[0], 8000)) <= CAP_CD
    # together with the two spectral terms: every column keeps its bits
    den2, sdr2, all4 = eng.evaluate_pcm(mix, clean, extra=new + old, rebuild="ola")
    den3, sdr3, only_old = eng.evaluate_pcm(mix, clean, extra=old, rebuild="ola")
    assert all(np.array_equal(a, b) and np.array_equal(a, e) for a, b, e in zip(den, den2, den3))
    assert np.array_equal(sdr, sdr2) and np.array_equal(sdr, sdr3) and list(all4) == list(new + old)
    for name in new:
        assert np.array_equal(all4[name], more[name])
    for name in old:
        assert np.array_equal(all4[name], only_old[name]) and np.isfinite(only_old[name]).all()
    assert all(eng.extra_scores[name].count == 0 for name in new + old)
    capsys.readouterr()
    avg = eng.test(batches, extra=new + old, rebuild="ola")
    printed = capsys.readouterr().out
    assert all(eng.extra_scores[name].count == 3 for name in new + old)
    for name in new + old:
        assert abs(eng.extra_scores[name].avg - np.mean(all4[name])) <= 1e-12 * max(1.0, abs(np.mean(all4[name])))
    more_line = "Average fw_seg_snr: %.4f; Average cd: %.4f; Average llr: %.4f; Average wss: %.4f.\n" % tuple(
        eng.extra_scores[n].avg for n in new + old)
    assert printed == "Average sd_score: %.4f.\n\n" % avg + more_line + "\n"

    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, weights=rced_np.make_weights("FullyCNNV3", seed=42))

    class Log(object):
        lines = []

        def info(self, msg):
            self.lines.append(msg)

    avg = tr.valid(batches, 2, Log(), extra=new, rebuild="ola")
    assert all(tr.extra_scores[name].count == 3 and math.isfinite(tr.extra_scores[name].avg) for name in new)
    line = "Epoch: 2, Average sd_score: %.4f.\n" % avg
    more_line = "Epoch: 2, Average fw_seg_snr: %.4f; Average cd: %.4f.\n" % tuple(tr.extra_scores[n].avg for n in new)
    assert capsys.readouterr().out == line + "\n" + more_line + "\n" and Log.lines == [line, more_line]
    tr.close()
    with pytest.raises(ValueError):
        eng.evaluate_pcm(mix, clean, extra=("fw_seg_snr", "fwsnrseg"), rebuild="ola")
