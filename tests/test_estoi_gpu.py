"""GPU tests of rced_stoi_ex / audio.stoi_batch(extended=...) against the float64 restatement of ESTOI (tests/estoi_np.py;
pystoi is not available to this project, so parity is with the restatement and with analytic properties).

The score error has the project's hard cap of 5e-5 (half a unit of the fourth decimal the reference prints).  The bar
asserted is derived, not measured: only the DFT products are below float64, so ten times the worst distance of the
f32_dft emulation (frames rounded to fp32, fp32 dot products of 256 terms, everything else float64) from the restatement ON
THE SAME INPUTS, computed here -- the margin of ten is DESIGN.md 3.4c's, room for another summation order inside the
matrix pipe.  Every comparison prints its figure (DESIGN.md "ESTOI")."""

import functools

import numpy as np
import pytest

import estoi_np as en
import stoi_np as sn
import test_stoi_gpu as tg
from test_stoi_gpu import dev, padded, strided

pytestmark = pytest.mark.gpu

CAP = 5e-5
MARGIN = 10


def restated(clean, est, fs=8000):
    """[(d, counts)] of the restatement on the float32 signals the device sees, and the bar: MARGIN times the emulation's
    worst distance from it on these inputs."""
    ref, worst = [], 0.0
    for c, e in zip(clean, est):
        d, counts, _ = en.estoi_detail(c, e, fs)
        worst = max(worst, abs(en.estoi(c, e, fs, f32_dft=True) - d))
        ref.append((d, counts))
    return ref, MARGIN * worst


@functools.lru_cache(maxsize=None)
def parity_batch():
    """tests/test_stoi_gpu.batch(seed=11) with its references, computed once: 8 ragged rows of 6,001 .. 65,664 samples."""
    lens, clean, est = tg.batch(seed=11)
    classic = tg.reference(clean, est)            # asserts the 0.01 dB clearance from the silent-frame threshold first
    ref, bar = restated(clean, est)
    return lens, clean, est, classic, ref, bar


def white_pair(L, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(L).astype(np.float32)
    return w, (w + 0.3 * rng.standard_normal(L)).astype(np.float32)


def test_parity_with_the_restatement(built):
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    lens, clean, est, classic, ref, bar = parity_batch()
    assert [counts[2] for _, counts in ref] == [335, 100, 101, 139, 20, 3, 41, 335]
    assert [counts for _, counts in ref] == [counts for _, counts in classic]
    assert min(d for d, _ in ref) < 0.19 and max(d for d, _ in ref) > 1 - 1e-12
    assert 0 < bar < CAP / 10
    st, d, det = stoi_batch(strided(clean, 65664 + 7), strided(est, 65664 + 13, fill=-3.0), lens, detail=True, extended="both")
    st, d, det = st.cpu().numpy(), d.cpu().numpy(), det.cpu().numpy()
    worst = 0.0
    for i, (r, counts) in enumerate(ref):
        err = abs(d[i] - r)
        worst = max(worst, err)
        print("utterance %d (L %d): F, K, M = %s  estoi %.9f  restatement %.9f  |diff| %.2e" % (i, lens[i], tuple(det[i]), d[i], r, err))
        assert tuple(det[i]) == counts
        assert abs(st[i] - classic[i][0]) <= tg.BAR
    print("worst |d_gpu - d_ref| = %.3e (bar %.3e = %d x the emulation's worst, cap %.1e)" % (worst, bar, MARGIN, CAP))
    assert worst <= CAP
    assert worst <= bar


def test_segment_counts_at_the_workgroup_seams(built):
    """10 kHz white noise, every frame kept: no segment, one, one workgroup's 16, one more; a too-short row between two long
    ones.  (The 65,664-sample rows of the parity batch have M = 335 > 256: the final sum's second stride.)"""
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    lens = (6145, 4096, 6017, 4097, 0, 256)
    want = ((47, 47, 17), (30, 30, 0), (46, 46, 16), (31, 31, 1), (0, 0, 0), (0, 0, 0))
    pairs = [white_pair(L, 90 + i) for i, L in enumerate(lens)]
    clean, est = [p[0] for p in pairs], [p[1] for p in pairs]
    ref, bar = restated(clean, est, 10000)
    assert tuple(counts for _, counts in ref) == want
    d, det = stoi_batch(dev(padded(clean, 6145)), dev(padded(est, 6150)), lens, sample_rate=10000, detail=True, extended=True)
    d, det = d.cpu().numpy(), det.cpu().numpy()
    for i, (r, counts) in enumerate(ref):
        print("L %d: %s estoi %.9f restatement %.9f |diff| %.2e (bar %.2e)" % (lens[i], counts, d[i], r, abs(d[i] - r), bar))
        assert tuple(det[i]) == counts
        if counts[2] == 0:
            assert d[i] == 1e-5 == r
        else:
            assert abs(d[i] - r) <= min(bar, CAP)


def test_analytic_properties(built):
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    x = sn.speechlike(24000, 7).astype(np.float32)
    noisy = (8 * sn.add_white(x.astype(np.float64), 5, 8)).astype(np.float32)
    quarter = (0.25 * noisy).astype(np.float32)                 # exact: a power of two
    # `norm + EPS` of a row is the one step a power-of-two gain does not pass through exactly; it does where both norms
    # are at least 4 (EPS under a quarter of an ulp), which the restatement confirms for these inputs with room to spare
    assert min(en.min_row_norm(noisy, x, 8000), en.min_row_norm(quarter, x, 8000)) >= 5
    rows = dev(np.stack([x, noisy, quarter, np.zeros_like(x)]))
    d = stoi_batch(rows[[0, 0, 0, 3, 0]], rows[[0, 1, 2, 1, 3]], extended=True).cpu().numpy()
    print("self %.15f, noisy %.12f, quarter %.12f, zero clean %r, zero estimate %r" % tuple(d))
    assert abs(d[0] - 1) <= 1e-9
    assert d[1] == d[2]
    assert d[3] == 0 and d[4] == 0
    assert abs(d[1] - en.estoi(x, noisy, 8000)) <= CAP


def test_both_gives_the_bits_of_each_alone(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    lens, clean, est, _, _, _ = parity_batch()
    c, e = strided(clean, 65664 + 7), strided(est, 65664 + 13, fill=-3.0)
    alone, det0 = stoi_batch(c, e, lens, detail=True)                              # rced_stoi
    ext, det2 = stoi_batch(c, e, lens, detail=True, extended=True)
    st, both, det3 = stoi_batch(c, e, lens, detail=True, extended="both")
    assert torch.equal(st, alone) and torch.equal(both, ext)
    assert torch.equal(det0, det2) and torch.equal(det0, det3)
    # which = CLASSIC through rced_stoi_ex, the extended output left alone
    out, keep = torch.zeros(len(lens), dtype=torch.float64, device="cuda"), torch.full((len(lens),), 7.0, dtype=torch.float64, device="cuda")
    ldev = dev(list(lens), np.int32)
    _lib.check(_lib.load().rced_stoi_ex(c.data_ptr(), 65664 + 7, e.data_ptr(), 65664 + 13, ldev.data_ptr(), len(lens), 8000,
                                        _lib.STOI_CLASSIC, out.data_ptr(), keep.data_ptr(), None, 0,
                                        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out, alone) and bool((keep == 7.0).all())


def test_scores_do_not_depend_on_the_batch_around_them(built):
    from fullycnnspeechenhancement_amd.audio import stoi_batch
    lens, clean, est = tg.batch(seed=23)
    lens, clean, est = lens[1:6], clean[1:6], est[1:6]
    width = max(lens)
    full = stoi_batch(dev(padded(clean, width)), dev(padded(est, width)), lens, extended=True)
    again = stoi_batch(dev(padded(clean, width)), dev(padded(est, width)), lens, extended=True)
    assert full.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()                    # run to run
    order = [3, 0, 4, 2, 1]                                                          # other rows, other strides, other junk
    moved = stoi_batch(strided([clean[i] for i in order], width + 5, fill=-1e3), strided([est[i] for i in order], width + 10, fill=9e9),
                       [lens[i] for i in order], extended=True)
    for k, i in enumerate(order):
        assert float(moved[k]) == float(full[i])
    for i in (0, 3):                                                                      # alone, exactly as long as itself
        alone = stoi_batch(dev(clean[i][None]), dev(est[i][None]), extended=True)
        assert float(alone[0]) == float(full[i])


def test_second_call_allocates_nothing_and_replays_from_a_captured_graph(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lens_host = [20000, 14321, 9000]
    clean = [sn.speechlike(L, 60 + i).astype(np.float32) for i, L in enumerate(lens_host)]
    est = [(8 * sn.add_white(c.astype(np.float64), 5, 70 + i)).astype(np.float32) for i, c in enumerate(clean)]
    ref, e = dev(padded(clean, 20003)), dev(padded(est, 20001))
    lens = dev(lens_host, np.int32)
    st, out = torch.empty(3, dtype=torch.float64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
    det = torch.empty((3, 3), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call():
        _lib.check(_lib.load().rced_stoi_ex(ref.data_ptr(), 20003, e.data_ptr(), 20001, lens.data_ptr(), 3, 8000,
                                            _lib.STOI_CLASSIC | _lib.STOI_EXTENDED, st.data_ptr(), out.data_ptr(), det.data_ptr(), 0,
                                            side.cuda_stream))

    call()                                             # sizes the stream's workspace, uploads the tables
    side.synchronize()
    first = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches.  An allocation or a
        call()                                         # copy from the host inside a capture is an error: this call made neither
    for scale in (1.0, 0.25):
        e.mul_(scale)
        out.zero_()
        st.zero_()
        det.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got, got_st, got_det = out.clone(), st.clone(), det.clone()
        call()                                         # the eager call on the changed input: the same bits
        side.synchronize()
        assert torch.equal(out, got) and torch.equal(st, got_st) and torch.equal(det, got_det)
        assert (got - first).abs().max().item() <= 1e-9
        assert scale != 1.0 or torch.equal(got, first)
    for i in range(3):
        assert abs(float(out[i]) - en.estoi(clean[i], 0.25 * est[i], 8000)) <= CAP
