"""GPU tests of rced_wave_loss_fr (kernels_wave_loss_fr.h) and of the training step at a framing: terms and gradient against
the float64 restatement (tests/wave_loss_fr_np.py) on one ragged batch per framing (tests/wave_loss_fr_cases.py), for wave_sse
alone, si_sdr alone and both, with and without skip_edges.  The bar on a row's gradient is 4x the error of the float32
restatements of the same chain on that row and case, over the whole row and again over frames 1 .. F - 2 alone
(wave_loss_fr_cases.Batch.reference; test_wave_loss_fr_host.py guards what it rests on).  The terms are float64 sums of a float32
rebuild that is held per sample to d_i = 2e-5 max|y| max(1, A[i] / A0) (test_framing_gpu.ola_bar); what such an error can do to
them over the scored samples is their bar (term_bars).  Invariants are asked for bit for bit.  Figures are printed before they are
asserted.  At 256 / 128 / hamming audio.wave_loss_batch goes to the specialised entry, so that framing is run through the C entry.

Measured (one run): the gradient 3.5e-7 .. 1.9e-4 of a row's largest entry over 293 rows; the worst fraction of a
bar 1.00 (6.41e-6 against 6.44e-6: 256 / 64 / hanning, 65 frames, without skip_edges, weights (0.5, 1) -- frame 0 holds every
large entry of that row through 1 / D = 4e7 at sample 1), then 0.99, 0.98, 0.98, 0.87; frames 1 .. F - 2 alone at most 0.36.  At
the default framing the general and the specialised entry are 4.4e-6 .. 5.6e-5 of a row's largest entry apart.  The training step:
loss within 1.3e-8 / 5.9e-8, the worst gradient tensor 4.9e-6 (CR-CED) and 1.9e-6 (R-CED V1) of its largest entry."""

import ctypes

import numpy as np
import pytest

import framing_np as fn
import wave_loss_fr_cases as fc
import wave_loss_fr_np as wf

pytestmark = pytest.mark.gpu

A0 = fn.ola_conditioning(8, 256, 128, "hamming").max()


def term_bars(b, row, skip_edges):
    """(bar on wave_sse, bar on si_sdr in dB) for a rebuild off by at most d_i per sample: test_wave_loss_gpu.term_bars with
    sum d_i^2 over the scored samples in place of n d^2 (Cauchy-Schwarz)."""
    W, S, name = b.framing
    F, y, clean = b.frames[row], b.rebuilt(row, "f64"), b.clean[row]
    lo, hi = wf.scored_range(b.lengths[row], F, skip_edges, W, S)
    sse, _, valid, _, target, resid = wf.terms(y, clean, b.lengths[row], F, skip_edges, W, S)
    if hi <= lo:
        return 0.0, 0.0
    d = 2e-5 * float(np.abs(y).max()) * np.maximum(1.0, fn.ola_conditioning(F, W, S, name)[lo:hi] / A0)
    d2 = float(np.sum(d * d))
    move = lambda s: 2 * np.sqrt(d2 * s) + d2
    return move(sse), (wf.K_DB * (move(target) / target + move(resid) / resid) if valid else 0.0)


def objective(weights, skip_edges):
    from fullycnnspeechenhancement_amd import audio
    return audio.WaveObjective(0.0 if any(weights) else 1.0, weights[0], weights[1], skip_edges)


DEVICE = {}


def on_device(framing):
    """The batch on the device, once per framing: the clean rows as a view of a wider buffer at an odd stride."""
    import torch
    if framing not in DEVICE:
        b = fc.batch(framing)
        wide = torch.full((b.N, b.clean_stride), 7.0, device="cuda")
        wide[:, :b.clean_width] = torch.tensor(b.clean, device="cuda")
        view = wide[:, :b.clean_width]
        assert view.stride(0) == b.clean_stride and b.clean_stride % 2 == 1
        DEVICE[framing] = (torch.tensor(b.mag, device="cuda"), torch.tensor(b.ph, device="cuda"), view)
    return DEVICE[framing]


def run_c(framing, mag, ph, clean, lengths, weights, skip_edges, frames=None, grad=True, stream=None, out=None):
    """rced_wave_loss_fr itself (what audio.wave_loss_batch calls for every framing but the default)."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    n, t = int(mag.shape[0]), int(mag.shape[1])
    phr = torch.view_as_real(ph.contiguous()).contiguous()
    lens = torch.tensor(list(lengths), dtype=torch.int32, device="cuda")
    fdev = torch.tensor(list(frames), dtype=torch.int32, device="cuda") if frames is not None else None
    terms, g = out if out is not None else (torch.empty((n, 3), dtype=torch.float64, device="cuda"),
                                            torch.empty((n, t, 129), dtype=torch.float32, device="cuda") if grad else None)
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().rced_wave_loss_fr(mag.contiguous().data_ptr(), phr.data_ptr(), fdev.data_ptr() if fdev is not None else None,
                                             clean.data_ptr(), clean.stride(0), lens.data_ptr(), n, t, framing[0], framing[1],
                                             fn.CODES[framing[2]], weights[0], weights[1], int(skip_edges), 1.0 / fc.BATCH,
                                             terms.data_ptr(), g.data_ptr() if g is not None else None, 0, ctypes.c_void_p(st)))
    return terms, g


def run(framing, weights, skip_edges, rows=slice(None), frames=None, grad=True, dev=None):
    from fullycnnspeechenhancement_amd import audio
    b = fc.batch(framing)
    mag, ph, clean = (a[rows] for a in (dev or on_device(framing)))
    if framing == fc.DEFAULT:
        terms, g = run_c(framing, mag, ph, clean, b.lengths[rows], weights, skip_edges, frames, grad)
    else:
        terms, g = audio.wave_loss_batch(mag, ph, clean, list(b.lengths[rows]), objective(weights, skip_edges), fc.BATCH, frames=frames,
                                         grad=grad, framing=audio.Framing(*framing))
    return terms.cpu().numpy(), (g.cpu().numpy() if g is not None else None)


def check_against_reference(b, terms, g, weights, skip_edges, what=""):
    """Prints every figure, then returns the worst fraction of a bar (whole rows, interior frames)."""
    worst, worst_in = 0.0, 0.0
    for i, (ref_terms, ref_g, yard, bar, inner) in enumerate(b.reference(weights, skip_edges)):
        F = b.frames[i]
        assert not g[i, F:].any()                                         # frames at and past F: exactly zero
        assert terms[i, 2] == ref_terms[2]                                # the validity column is exact
        if not ref_terms[2]:
            assert terms[i, 1] == 0.0
        bar_sse, bar_si = term_bars(b, i, skip_edges)
        print("%s row %d (%5d samples, %3d frames): wave_sse %.6e (ref %.6e) off by %.2e (bar %.2e); si_sdr %.6f (ref %.6f) off by %.2e dB "
              "(bar %.2e); valid %d" % (what, i, b.lengths[i], F, terms[i, 0], ref_terms[0], abs(terms[i, 0] - ref_terms[0]), bar_sse,
                                        terms[i, 1], ref_terms[1], abs(terms[i, 1] - ref_terms[1]), bar_si, terms[i, 2]))
        assert abs(terms[i, 0] - ref_terms[0]) <= bar_sse and abs(terms[i, 1] - ref_terms[1]) <= bar_si
        if not ref_g.any():
            assert not g[i].any()                                         # an empty range, no frames, an invalid term alone
            continue
        err = np.abs(g[i] - ref_g).max() / np.abs(ref_g).max()
        worst = max(worst, err / bar)
        line = "        gradient: %.2e of the largest entry; yardsticks %.2e, %.2e; bar %.2e; %.2f of the bar" % ((err,) + yard + (bar, err / bar))
        if inner is not None:
            sl = slice(1, F - 1)
            err_in = np.abs(g[i, sl] - ref_g[sl]).max() / np.abs(ref_g[sl]).max()
            worst_in = max(worst_in, err_in / inner[1])
            line += "; frames 1 .. F - 2: %.2e, yardsticks %.2e, %.2e, %.2f of the bar" % ((err_in,) + inner[0] + (err_in / inner[1],))
        print(line)
    return worst, worst_in


@pytest.mark.parametrize("framing", fc.FRAMINGS, ids=fc.IDS)
@pytest.mark.parametrize("weights,skip_edges", fc.CASES)
def test_terms_and_gradient_against_the_restatement(built, framing, weights, skip_edges):
    b = fc.batch(framing)
    terms, g = run(framing, weights, skip_edges)
    assert terms.shape == (b.N, 3) and terms.dtype == np.float64 and g.shape == (b.N, b.T, 129) and g.dtype == np.float32
    assert np.isfinite(terms).all() and np.isfinite(g).all()
    worst, worst_in = check_against_reference(b, terms, g, weights, skip_edges)
    print("%s weights %s skip_edges %s: worst fraction of a bar %.2f (rows), %.2f (frames 1 .. F - 2)" % (framing, weights, skip_edges, worst, worst_in))
    assert worst <= 1.0 and worst_in <= 1.0


@pytest.mark.parametrize("weights,skip_edges", fc.CASES)
def test_at_the_default_framing_both_entries_lie_within_the_bars(built, weights, skip_edges):
    """The general kernels and the specialised ones against the same float64 gradient; their mutual distance is printed, not held."""
    from fullycnnspeechenhancement_amd import audio
    b = fc.batch(fc.DEFAULT)
    mag, ph, clean = on_device(fc.DEFAULT)
    ta, ga = run(fc.DEFAULT, weights, skip_edges)
    for framing in (None, audio.Framing()):
        tb, gb = audio.wave_loss_batch(mag, ph, clean, list(b.lengths), objective(weights, skip_edges), fc.BATCH, framing=framing)
    tb, gb = tb.cpu().numpy(), gb.cpu().numpy()
    wa = check_against_reference(b, ta, ga, weights, skip_edges, "general")
    wb = check_against_reference(b, tb, gb, weights, skip_edges, "specialised")
    scale = np.abs(ga).max(axis=(1, 2))
    dist = max(np.abs(ga[i] - gb[i]).max() / scale[i] for i in range(b.N) if scale[i])
    print("weights %s skip_edges %s: fractions of a bar %.2f / %.2f (general), %.2f / %.2f (specialised); mutual distance %.2e of a row's "
          "largest entry, terms %.2e" % ((weights, skip_edges) + wa + wb + (dist, np.abs(ta - tb).max())))
    assert max(wa + wb) <= 1.0


@pytest.mark.parametrize("framing", fc.FRAMINGS, ids=fc.IDS)
@pytest.mark.parametrize("skip_edges", [True, False])
def test_each_row_alone_gives_the_bits_it_gives_in_the_batch(built, framing, skip_edges):
    b = fc.batch(framing)
    terms, g = run(framing, (0.5, 1.0), skip_edges)
    for i in range(b.N):
        t1, g1 = run(framing, (0.5, 1.0), skip_edges, rows=slice(i, i + 1))
        assert np.array_equal(t1[0], terms[i]) and np.array_equal(g1[0], g[i]), i
    # ... and with fewer padded frames behind it: row 3 (3 frames) at T = 5
    dev = tuple(a[:, :5].contiguous() if k < 2 else a for k, a in enumerate(on_device(framing)))
    t2, g2 = run(framing, (0.5, 1.0), skip_edges, rows=slice(3, 4), dev=dev)
    assert np.array_equal(t2[0], terms[3]) and np.array_equal(g2[0], g[3, :5])


@pytest.mark.parametrize("framing", fc.FRAMINGS, ids=fc.IDS)
def test_frames_none_is_the_count_of_the_length_and_terms_need_no_gradient(built, framing):
    b = fc.batch(framing)
    a = run(framing, (0.5, 1.0), True)
    c = run(framing, (0.5, 1.0), True, frames=list(b.frames))
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    t, g = run(framing, (1.0, 0.0), True, grad=False)
    assert g is None and np.array_equal(t, a[0])
    c = run(framing, (0.5, 1.0), False, rows=slice(0, 1), frames=[9999])       # a count outside [0, T] is clamped into it
    d = run(framing, (0.5, 1.0), False, rows=slice(0, 1), frames=[b.T])
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1])


@pytest.mark.parametrize("framing", [(255, 100, "hanning"), (256, 64, "hanning"), (256, 128, "hamming")], ids=lambda f: "%d-%d-%s" % f)
def test_two_runs_are_bit_equal_and_the_second_replays_from_a_captured_graph(built, framing):
    """A call that allocated, or synchronised, could not be captured: after the first call at a shape nothing is allocated."""
    import torch
    b = fc.batch(framing)
    mag, ph, clean = on_device(framing)
    a = run(framing, (0.5, 1.0), True)
    a2 = run(framing, (0.5, 1.0), True)
    assert np.array_equal(a[0], a2[0]) and np.array_equal(a[1], a2[1])
    terms = torch.empty((b.N, 3), dtype=torch.float64, device="cuda")
    g = torch.empty((b.N, b.T, 129), dtype=torch.float32, device="cuda")
    lens = torch.tensor(b.lengths, dtype=torch.int32, device="cuda")
    phr = torch.view_as_real(ph).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    from fullycnnspeechenhancement_amd import _lib

    def call():
        _lib.check(_lib.load().rced_wave_loss_fr(mag.data_ptr(), phr.data_ptr(), None, clean.data_ptr(), b.clean_stride, lens.data_ptr(),
                                                 b.N, b.T, framing[0], framing[1], fn.CODES[framing[2]], 0.5, 1.0, 1, 1.0 / fc.BATCH,
                                                 terms.data_ptr(), g.data_ptr(), 0, side.cuda_stream))

    call()                                             # sizes the stream's workspace, builds the packs
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches
        call()
    terms.zero_()
    g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(terms.cpu().numpy(), a[0]) and np.array_equal(g.cpu().numpy(), a[1])


@pytest.mark.parametrize("framing", fc.FRAMINGS, ids=fc.IDS)
def test_padded_frames_and_samples_past_the_length_are_not_read(built, framing):
    """NaN in every frame at and past F and in every clean sample at and past the length: nothing changes."""
    b = fc.batch(framing)
    mag, ph, clean = (a.clone() for a in on_device(framing))
    for i, (l, F) in enumerate(zip(b.lengths, b.frames)):
        mag[i, F:] = float("nan")
        ph[i, F:] = complex(float("nan"), float("nan"))
        clean[i, l:] = float("nan")
    for skip in (True, False):
        want = run(framing, (0.5, 1.0), skip)
        got = run(framing, (0.5, 1.0), skip, dev=(mag, ph, clean))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_the_default_framing_is_todays_entry_bit_for_bit(built):
    """framing=None and Framing() against the call without a framing, on test_wave_loss_gpu.py's batch."""
    import torch
    import wave_loss_cases as wc
    from fullycnnspeechenhancement_amd import audio
    mag, ph, clean = (torch.tensor(a, device="cuda") for a in wc.batch())
    obj = objective((0.5, 1.0), True)
    t0, g0 = audio.wave_loss_batch(mag, ph, clean, list(wc.LENGTHS), obj, wc.BATCH)
    for framing in (None, audio.Framing(), audio.Framing(256, 128, "hamming")):
        t1, g1 = audio.wave_loss_batch(mag, ph, clean, list(wc.LENGTHS), obj, wc.BATCH, framing=framing)
        assert torch.equal(t0, t1) and torch.equal(g0, g1)


# ---- the training step at a framing ------------------------------------------------------------------------------------------------

TRAIN_FRAMING = (160, 80, "hamming")
N, T, BATCH = 2, 9, 4
LENGTHS = (800, 700)                            # F = (9, 8): one padded frame, a range that ends inside a hop
FRAMES = tuple(wf.num_frames(v, 160, 80) for v in LENGTHS)
WEIGHTS = (1.0, 0.5, 1.0)                       # spectral, wave_sse, si_sdr: all three weights in one step
TRAIN_CASES = {}


def train_case(net_work):
    """Weights, the screened input, the target, the phase, the clean rows and the float64 loss and gradients: once per net."""
    if net_work in TRAIN_CASES:
        return TRAIN_CASES[net_work]
    import torch
    from oracle import rced_np, train_ref
    from test_train_gpu import screened_input
    assert FRAMES == (9, 8)
    variant = {"FullyCNN": 1, "FullyCNNV2": 2, "FullyCNNV3": 3}[net_work]
    w = rced_np.make_weights(net_work, seed=11)
    ref = train_ref.TrainRef(net_work, w, batch_size=BATCH)
    x, seed = screened_input(ref, N, T, 7000 + 100 * variant)
    y = rced_np.make_input(N, T, seed=89 + variant)
    rng = np.random.default_rng(60 + variant)
    phase = np.exp(2j * np.pi * rng.random((N, T, 129))).astype(np.complex64)
    for k in ref.m:
        ref.vars[k].grad = None
    pred, _ = ref.forward_train(x)
    clean = np.zeros((N, max(LENGTHS)), np.float32)
    for n in range(N):                           # 0.7 of what the untrained net rebuilds, plus noise at half its rms
        yy = wf.rebuild(pred[n, :, :, 0].detach().numpy(), phase[n], FRAMES[n], *TRAIN_FRAMING)[:LENGTHS[n]]
        clean[n, :LENGTHS[n]] = 0.7 * yy + 0.5 * np.sqrt(np.mean(yy * yy)) * rng.standard_normal(LENGTHS[n])
    spectral = ((torch.as_tensor(y).to(pred.dtype) - pred) ** 2).sum()
    sse, si = 0.0, 0.0
    for n in range(N):
        a, b, valid = wf.torch_terms(pred[n, :, :, 0], phase[n], clean[n], LENGTHS[n], FRAMES[n], True, *TRAIN_FRAMING)
        assert valid == 1.0
        sse, si = sse + a, si + b
    loss = (WEIGHTS[0] * spectral + WEIGHTS[1] * sse - WEIGHTS[2] * si) / BATCH
    loss.backward()
    grads = {k: ref.vars[k].grad.clone().numpy() for k in ref.m}
    TRAIN_CASES[net_work] = (w, x, y, phase, clean, loss.item(), (spectral.item(), sse.item(), si.item()), grads)
    return TRAIN_CASES[net_work]


def wave_on_device(phase, clean):
    import torch
    return torch.tensor(phase, device="cuda"), torch.tensor(clean, device="cuda"), list(LENGTHS)


def trainer(net_work, w, **kw):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, audio
    return FullyCNNTrainer(net_work, batch_size=BATCH, lr=1e-4, weights=w, objective=audio.WaveObjective(*WEIGHTS), **kw)


@pytest.mark.parametrize("net_work", ["FullyCNNV3", "FullyCNN"])
def test_training_step_against_the_float64_composition(net_work, built, capsys):
    from fullycnnspeechenhancement_amd import audio
    from test_train_gpu import TIGHT
    w, x, y, phase, clean, loss_ref, parts_ref, grads_ref = train_case(net_work)
    tr = trainer(net_work, w)
    loss, _, step = tr.train_step(x, y, wave=wave_on_device(phase, clean), framing=audio.Framing(*TRAIN_FRAMING))
    assert step == 1
    g = tr.gradients()
    worst = {}
    for name, gr in grads_ref.items():
        if name.endswith("/bias") and (name[:-5] + "/batch_norm/gamma") in grads_ref:
            assert np.abs(g[name]).max() <= 1e-4 * max(np.abs(g[name[:-5] + "/kernel"]).max(), 1e-30), name
            continue
        worst[name] = np.abs(g[name].astype(np.float64) - gr).max() / np.abs(gr).max()
    k = max(worst, key=worst.get)
    with capsys.disabled():
        print("\n[train wave parity at %s] %s: loss %.8e (ref %.8e, rel err %.2e), parts %s (ref %s), worst gradient %s %.2e of its max "
              "(%d tensors)" % (TRAIN_FRAMING, net_work, loss, loss_ref, abs(loss - loss_ref) / abs(loss_ref), tr.loss_parts, parts_ref, k,
                                worst[k], len(worst)))
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref)
    for got, want in zip(tr.loss_parts, parts_ref):
        assert abs(got - want) <= 1e-5 * abs(want)
    assert worst[k] < TIGHT, (k, worst[k])
    tr.close()


def test_accumulation_at_a_framing_gives_loss_parts_that_add_up(built):
    import torch
    from fullycnnspeechenhancement_amd import audio
    w, x, y, phase, clean = train_case("FullyCNNV3")[:5]
    wave, fr = wave_on_device(phase, clean), audio.Framing(*TRAIN_FRAMING)
    acc, one = trainer("FullyCNNV3", w, accumulate=2), trainer("FullyCNNV3", w)
    loss = acc.train_step(x, y, wave=wave, framing=fr)[0]
    summed = acc.exchange_tensors()[0].clone()
    parts, losses, gs = [], [], []
    for a, b in ((0, 1), (1, 2)):
        losses.append(one.grad_step(x[a:b], y[a:b], wave=(wave[0][a:b], wave[1][a:b], wave[2][a:b]), framing=fr))
        parts.append(one.loss_parts)
        gs.append(one.exchange_tensors()[0].clone())
    assert loss == losses[0] + losses[1]
    assert acc.loss_parts == tuple(p + q for p, q in zip(*parts))
    assert torch.equal(summed, gs[0] + gs[1])
    # ... and they are not the default framing's
    other = trainer("FullyCNNV3", w)
    other.grad_step(x[0:1], y[0:1], wave=(wave[0][0:1], wave[1][0:1], wave[2][0:1]))
    assert other.loss_parts[0] == parts[0][0] and other.loss_parts[1:] != parts[0][1:]
    for tr in (acc, one, other):
        tr.close()


def test_the_default_framing_is_todays_training_step_bit_for_bit(built):
    import wave_loss_np as wl
    from fullycnnspeechenhancement_amd import audio
    w, x, y, phase, clean = train_case("FullyCNNV3")[:5]
    lengths = [wl.FRAME + 8 * wl.STEP - 40, wl.FRAME + 7 * wl.STEP]      # F = (9, 8) at 256 / 128
    assert tuple(wl.num_frames(v) for v in lengths) == FRAMES
    wide = np.zeros((N, max(lengths)), np.float32)
    wide[:, :clean.shape[1]] = clean
    import torch
    wave = (torch.tensor(phase, device="cuda"), torch.tensor(wide, device="cuda"), lengths)
    outs = []
    for kw in ({}, {"framing": None}, {"framing": audio.Framing()}):
        tr = trainer("FullyCNNV3", w)
        loss = tr.train_step(x, y, wave=wave, **kw)[0]
        outs.append((loss, tr.loss_parts, tr.gradients()))
        tr.close()
    for loss, parts, g in outs[1:]:
        assert loss == outs[0][0] and parts == outs[0][1] and all(np.array_equal(g[k], outs[0][2][k]) for k in g)
    assert outs[0][1][1] > 0


def test_train_runs_an_epoch_at_a_framing_and_a_repeated_batch_descends(built, capsys):
    import torch
    from oracle import rced_np
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, audio, loader
    from fullycnnspeechenhancement_amd.trainer import wave_of_batch
    fr = audio.Framing(*TRAIN_FRAMING)
    rng = np.random.default_rng(5)
    clean = [(3000 * rng.standard_normal(n)).astype(np.int16) for n in (1500, 1300, 1100, 900)]
    mixes = [np.clip(s.astype(np.int32) + rng.integers(-1000, 1000, len(s)), -32768, 32767).astype(np.int16) for s in clean]
    w = rced_np.make_weights("FullyCNNV3", seed=42)
    obj = audio.WaveObjective(1.0, 0.5, 0.1)

    def make_loader():
        np.random.seed(3)
        ds = loader.DataSet(loader.Corpus.from_arrays(clean), mix=loader.Corpus.from_arrays(mixes), framing=fr)
        return loader.DataLoader(ds, 2, sampler=loader.Sampler(ds, 2))

    class Recording(FullyCNNTrainer):
        def fit_step(self, x, y, wave=None, framing=None):
            out = FullyCNNTrainer.fit_step(self, x, y, wave=wave, framing=framing)
            self.seen.append((out[0], self.loss_parts, framing))
            return out

    a = Recording("FullyCNNV3", batch_size=2, lr=1e-3, weights=w, objective=obj)
    a.seen = []
    steps = len(make_loader())
    assert steps >= 2 and a.train(make_loader(), None, 1) == steps == len(a.seen)
    assert all(f == fr and np.isfinite(l) and p[1] > 0 for l, p, f in a.seen)
    # the steps by hand: the phase is the STFT's at the loader's framing, whose magnitudes are the loader's batch bit for bit
    b = FullyCNNTrainer("FullyCNNV3", batch_size=2, lr=1e-3, weights=w, objective=obj)
    dl, by_hand = make_loader(), []
    dl.shuffle()
    for batch_mix, batch_clean, mix_sig, clean_sig in dl:
        wave = wave_of_batch(dl, batch_mix, mix_sig, clean_sig)
        mag, phase = audio.stft_batch(mix_sig.rows, mix_sig.lengths, frames=int(batch_mix.shape[1]), framing=fr)
        assert torch.equal(mag, batch_mix) and torch.equal(phase, wave[0])
        by_hand.append((b.fit_step(batch_mix, batch_clean, wave=wave, framing=fr)[0], b.loss_parts))
    assert by_hand == [(l, p) for l, p, _ in a.seen]
    # a repeated toy batch: the objective goes down
    c = FullyCNNTrainer("FullyCNNV3", batch_size=2, lr=1e-3, weights=w, objective=audio.WaveObjective(1.0, 0.0, 1.0))
    losses = [c.train_step(batch_mix, batch_clean, wave=wave, framing=fr)[0] for _ in range(30)]
    with capsys.disabled():
        print("\n[train at %s] an epoch of %d steps; a repeated batch: loss %.5f -> %.5f over 30 steps" % (TRAIN_FRAMING, steps, losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    for tr in (a, b, c):
        tr.close()


def test_refusals_stay_by_name_at_a_framing(built):
    from fullycnnspeechenhancement_amd import audio, dist
    w, x, y, phase, clean = train_case("FullyCNNV3")[:5]
    wave, fr = wave_on_device(phase, clean), audio.Framing(*TRAIN_FRAMING)
    tr = trainer("FullyCNNV3", w)
    before = tr.variables()
    with pytest.raises(ValueError, match="sync_bn=True cannot be combined with an objective that has a wave term"):
        tr.train_step_sharded([(x[:1], y[:1], None), (x[1:], y[1:], None)], sync_bn=True, framing=fr)
    with pytest.raises(ValueError, match="DataParallelTrainer cannot be combined with an objective that has a wave term"):
        dist.DataParallelTrainer(tr)
    with pytest.raises(ValueError, match="wave=None"):
        tr.train_step(x, y, framing=fr)
    with pytest.raises(ValueError, match="wave=None"):
        tr.grad_step(x, y, framing=fr)
    with pytest.raises(ValueError, match="framing must be an audio.Framing"):
        tr.train_step(x, y, wave=wave, framing=TRAIN_FRAMING)
    after = tr.variables()
    assert tr.global_step == 0 and all(np.array_equal(before[k], after[k]) for k in before)      # a refused step changes nothing
    tr.close()
