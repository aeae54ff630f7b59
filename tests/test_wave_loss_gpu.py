"""GPU tests of rced_wave_loss (kernels_wave_loss.h) through audio.wave_loss_batch: terms and gradient against the float64
restatement (tests/wave_loss_np.py) on one ragged batch (tests/wave_loss_cases.py), for wave_sse alone, si_sdr alone and both,
with and without skip_edges.  The bar on a row's gradient is 4x the error of the float32 restatements of the same chain on that
row and case (wave_loss_cases.reference; test_wave_loss_host.py guards it).  The terms are float64 sums of a float32 rebuild
that is itself held to d = 2e-5 of its scale (test_ola_gpu.py); what an error of d per sample can do to them over the n scored
samples is their bar (term_bars).  Invariants are asked for bit for bit.  Figures are printed before they are asserted."""

import numpy as np
import pytest

import wave_loss_cases as wc
import wave_loss_np as wl

pytestmark = pytest.mark.gpu


def term_bars(row, skip_edges):
    """(bar on wave_sse, bar on si_sdr in dB) for a rebuild off by at most d = 2e-5 max |y| per sample, n samples scored:
    |y' - c|^2 - |y - c|^2 <= 2 d sqrt(n) |y - c| + n d^2 (Cauchy-Schwarz); alpha moves by at most d sqrt(n) / |c|, so |alpha c| by
    d sqrt(n); r = y - alpha c moves by the part of the error orthogonal to c, at most d sqrt(n); si_sdr = k ln(|alpha c|^2 / |r|^2)
    to first order in both."""
    y, clean = wc.rebuilt(row, "f64"), wc.batch()[2][row]
    lo, hi = wl.scored_range(wc.LENGTHS[row], wc.FRAMES[row], skip_edges)
    sse, _, valid, _, target, resid = wl.terms(y, clean, wc.LENGTHS[row], wc.FRAMES[row], skip_edges)
    n, d = hi - lo, 2e-5 * float(np.abs(y).max()) if y.any() else 0.0
    move = lambda s: 2 * d * np.sqrt(n * s) + n * d * d
    return move(sse), (wl.K_DB * (move(target) / target + move(resid) / resid) if valid else 0.0)


def objective(weights, skip_edges):
    from fullycnnspeechenhancement_amd import audio
    return audio.WaveObjective(0.0 if any(weights) else 1.0, weights[0], weights[1], skip_edges)


@pytest.fixture(scope="module")
def on_device(built):
    """The batch on the device: the clean rows as a view of a wider buffer (a row stride that is no multiple of four floats)."""
    import torch
    mag, ph, clean = wc.batch()
    wide = torch.full((wc.N, wc.CLEAN_STRIDE), 7.0, device="cuda")
    wide[:, :wc.CLEAN_WIDTH] = torch.tensor(clean, device="cuda")
    view = wide[:, :wc.CLEAN_WIDTH]
    assert view.stride(0) == wc.CLEAN_STRIDE != (wc.T + 1) * 128
    return torch.tensor(mag, device="cuda"), torch.tensor(ph, device="cuda"), view


def run(dev, weights, skip_edges, rows=slice(None), frames=None, grad=True):
    from fullycnnspeechenhancement_amd import audio
    mag, ph, clean = (a[rows] for a in dev)
    terms, g = audio.wave_loss_batch(mag, ph, clean, list(wc.LENGTHS[rows]), objective(weights, skip_edges), wc.BATCH, frames=frames, grad=grad)
    return terms.cpu().numpy(), (g.cpu().numpy() if g is not None else None)


@pytest.mark.parametrize("weights,skip_edges", wc.CASES)
def test_terms_and_gradient_against_the_restatement(on_device, weights, skip_edges):
    terms, g = run(on_device, weights, skip_edges)
    assert terms.shape == (wc.N, 3) and terms.dtype == np.float64 and g.shape == (wc.N, wc.T, 129) and g.dtype == np.float32
    assert np.isfinite(terms).all() and np.isfinite(g).all()
    worst = 0.0
    for i, (ref_terms, ref_g, yard, bar) in enumerate(wc.reference(weights, skip_edges)):
        F = wc.FRAMES[i]
        assert not g[i, F:].any()                                         # frames at and past F: exactly zero
        assert terms[i, 2] == ref_terms[2]
        if not ref_terms[2]:                                              # invalid: flagged and zero
            assert terms[i, 1] == 0.0
        print("row %d (%4d samples, %2d frames): wave_sse %.6e (ref %.6e), si_sdr %.6f (ref %.6f), valid %d"
              % (i, wc.LENGTHS[i], F, terms[i, 0], ref_terms[0], terms[i, 1], ref_terms[1], terms[i, 2]))
        bar_sse, bar_si = term_bars(i, skip_edges)
        print("        off by %.2e (bar %.2e) and %.2e dB (bar %.2e)" % (abs(terms[i, 0] - ref_terms[0]), bar_sse, abs(terms[i, 1] - ref_terms[1]), bar_si))
        assert abs(terms[i, 0] - ref_terms[0]) <= bar_sse and abs(terms[i, 1] - ref_terms[1]) <= bar_si
        if not ref_g.any():
            assert not g[i].any()                                         # an empty range, no frames, an invalid term alone
            continue
        err = np.abs(g[i] - ref_g).max() / np.abs(ref_g).max()
        worst = max(worst, err / bar)
        print("        gradient: %.2e of the largest entry; yardsticks %.2e, %.2e; bar %.2e; %.2f of the bar" % ((err,) + yard + (bar, err / bar)))
    print("worst fraction of a bar %.2f" % worst)
    assert worst <= 1.0


def test_terms_do_not_depend_on_the_weights_or_on_asking_for_a_gradient(on_device):
    a, _ = run(on_device, (1.0, 0.0), True)
    b, g = run(on_device, (0.5, 1.0), True, grad=False)
    assert g is None and np.array_equal(a, b)


def test_frames_none_is_the_count_of_the_length(on_device):
    a = run(on_device, (0.5, 1.0), True)
    b = run(on_device, (0.5, 1.0), True, frames=list(wc.FRAMES))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a count outside [0, T] is clamped into it
    c = run(on_device, (0.5, 1.0), False, rows=slice(0, 1), frames=[999])
    d = run(on_device, (0.5, 1.0), False, rows=slice(0, 1), frames=[wc.T])
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])


@pytest.mark.parametrize("skip_edges", [True, False])
def test_each_row_alone_gives_the_bits_it_gives_in_the_batch(on_device, skip_edges):
    terms, g = run(on_device, (0.5, 1.0), skip_edges)
    for i in range(wc.N):
        t1, g1 = run(on_device, (0.5, 1.0), skip_edges, rows=slice(i, i + 1))
        assert np.array_equal(t1[0], terms[i]) and np.array_equal(g1[0], g[i]), i
    # ... and with fewer padded frames behind it: row 2 (3 frames) at T = 5
    from fullycnnspeechenhancement_amd import audio
    mag, ph, clean = on_device
    t2, g2 = audio.wave_loss_batch(mag[2:3, :5].contiguous(), ph[2:3, :5].contiguous(), clean[2:3], [wc.LENGTHS[2]],
                                   objective((0.5, 1.0), skip_edges), wc.BATCH)
    assert np.array_equal(t2.cpu().numpy()[0], terms[2]) and np.array_equal(g2.cpu().numpy()[0], g[2, :5])


def test_two_runs_are_bit_equal_and_the_second_replays_from_a_captured_graph(on_device):
    """A call that allocated, or synchronised, could not be captured: after the first call at a shape nothing is allocated."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    a = run(on_device, (0.5, 1.0), True)
    b = run(on_device, (0.5, 1.0), True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    mag, ph, clean = on_device
    phr = torch.view_as_real(ph).contiguous()
    lens = torch.tensor(wc.LENGTHS, dtype=torch.int32, device="cuda")
    terms = torch.empty((wc.N, 3), dtype=torch.float64, device="cuda")
    g = torch.empty((wc.N, wc.T, 129), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def call():
        _lib.check(_lib.load().rced_wave_loss(mag.data_ptr(), phr.data_ptr(), None, clean.data_ptr(), wc.CLEAN_STRIDE, lens.data_ptr(),
                                              wc.N, wc.T, 0.5, 1.0, 1, 1.0 / wc.BATCH, terms.data_ptr(), g.data_ptr(), 0, side.cuda_stream))

    call()                                             # sizes the stream's workspace
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches
        call()
    terms.zero_()
    g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(terms.cpu().numpy(), a[0]) and np.array_equal(g.cpu().numpy(), a[1])


def test_padded_frames_and_samples_past_the_length_are_not_read(on_device):
    """NaN in every frame at and past F and in every clean sample at and past the length: nothing changes."""
    from fullycnnspeechenhancement_amd import audio
    mag, ph, clean = (a.clone() for a in on_device)
    for i, (l, F) in enumerate(zip(wc.LENGTHS, wc.FRAMES)):
        mag[i, F:] = float("nan")
        ph[i, F:] = complex(float("nan"), float("nan"))
        clean[i, l:] = float("nan")
    obj = objective((0.5, 1.0), False)
    want = run(on_device, (0.5, 1.0), False)
    terms, g = audio.wave_loss_batch(mag, ph, clean, list(wc.LENGTHS), obj, wc.BATCH)
    assert np.array_equal(terms.cpu().numpy(), want[0]) and np.array_equal(g.cpu().numpy(), want[1])


def test_host_side_refusals(on_device):
    from fullycnnspeechenhancement_amd import audio
    mag, ph, clean = on_device
    obj = audio.WaveObjective(1, 1, 0)
    for kw in ({"lengths": list(wc.LENGTHS[:-1])}, {"lengths": [9000] * wc.N}, {"lengths": None}, {"batch_size": 0},
               {"objective": None}, {"frames": [1, 2]}):
        args = {"lengths": list(wc.LENGTHS), "objective": obj, "batch_size": wc.BATCH, "frames": None}
        args.update(kw)
        with pytest.raises(ValueError):
            audio.wave_loss_batch(mag, ph, clean, args["lengths"], args["objective"], args["batch_size"], frames=args["frames"])
    with pytest.raises(ValueError):
        audio.wave_loss_batch(mag[:, :, :100], ph, clean, list(wc.LENGTHS), obj, wc.BATCH)
