"""CPU tests of the waveform objective at a framing: the restatement (tests/wave_loss_fr_np.py) against central differences, a
torch autograd form, the default framing's restatement and the evaluation loop's SI-SDR; the condition under which the float32
and float64 zero sets of the 1e-10 rule agree for the batches tests/test_wave_loss_fr_gpu.py runs (tests/wave_loss_fr_cases.py);
and the argument checks of the new entries and of the Python layer that come before any device work."""

import ctypes

import numpy as np
import pytest

import framing_np as fn
import td_metrics_np
import wave_loss_cases as wc
import wave_loss_fr_cases as fc
import wave_loss_fr_np as wf
import wave_loss_np as wl


def _utterance(F, framing, seed, frames_pad=2):
    W, S, name = framing
    rng = np.random.default_rng(seed)
    length = fc.length_of(F, W, S)
    T = F + frames_pad
    X = rng.standard_normal((T, 129)) + 1j * rng.standard_normal((T, 129))
    mag, ph = np.abs(X) + 0.01, np.exp(1j * np.angle(X))
    y = wf.rebuild(mag, ph, F, W, S, name)[:length]
    clean = 0.7 * y + 0.5 * np.sqrt(np.mean(y * y)) * rng.standard_normal(length)
    return mag, ph, clean, length


@pytest.mark.parametrize("framing", fc.FRAMINGS, ids=fc.IDS)
@pytest.mark.parametrize("weights", [(0.25, 0.0), (0.0, 0.25)])
def test_gradient_against_central_differences(framing, weights):
    """Entries of every kind -- first, last and padded frames, bins 0 and 128 --: 1e-9 of the largest entry, for both terms, for
    one, two, three and six frames.  Two step sizes, the h^2 term removed (test_wave_loss_host.py says why).  The steps are 4e-3 and
    2e-3: the difference of two objectives carries their rounding, 2^-53 |objective| / h, and under a window that ends in zero the
    gradient's largest entry is small against the objective (1 / D at the edge) -- at h = 5e-4 that rounding alone is 1e-9 of it,
    while the h^4 term left after the extrapolation is far below at either step."""
    W, S, name = framing
    for F in (1, 2, 3, 6):
        mag, ph, clean, length = _utterance(F, framing, 100 + F + W)
        for skip in (True, False):
            g = wf.gradient(wf.rebuild(mag, ph, F, W, S, name), ph, clean, length, F, weights[0], weights[1], skip, W, S, name)
            assert not g[F:].any()                                       # padded frames: exactly zero
            lo, hi = wf.scored_range(length, F, skip, W, S)
            if hi <= lo:
                assert not g.any()
                continue
            rng = np.random.default_rng(F)
            picks = [(0, 0), (0, 128), (F - 1, 0), (F - 1, 128), (F - 1, 64), (F, 5)] + \
                    [(int(rng.integers(F)), int(rng.integers(129))) for _ in range(10)]
            worst, scale = 0.0, np.abs(g).max()

            def central(t, b, h):
                up, dn = mag.copy(), mag.copy()
                up[t, b] += h
                dn[t, b] -= h
                return (wf.objective(up, ph, clean, length, F, weights[0], weights[1], skip, W, S, name) -
                        wf.objective(dn, ph, clean, length, F, weights[0], weights[1], skip, W, S, name)) / (2 * h)

            for t, b in picks:
                fd = (4 * central(t, b, 2e-3) - central(t, b, 4e-3)) / 3
                worst = max(worst, abs(fd - g[t, b]) / scale)
            print("%s, %d frames, weights %s, skip_edges %s: %.2e of the largest entry" % (framing, F, weights, skip, worst))
            assert worst <= 1e-9


@pytest.mark.parametrize("framing", fc.FRAMINGS, ids=fc.IDS)
def test_torch_form_equals_the_numpy_form(framing):
    import torch
    W, S, name = framing
    for F in (1, 2, 3, 6):
        mag, ph, clean, length = _utterance(F, framing, 50 + F + W)
        for skip in (True, False):
            m = torch.tensor(mag, dtype=torch.float64, requires_grad=True)
            sse, si, valid = wf.torch_terms(m, ph, clean, length, F, skip, W, S, name)
            y = wf.rebuild(mag, ph, F, W, S, name)
            ref = wf.terms(y, clean, length, F, skip, W, S)
            assert valid == ref[2]
            assert abs(float(sse.detach()) - ref[0]) <= 1e-12 * max(1.0, abs(ref[0]))
            assert abs(float(si.detach()) - ref[1]) <= 1e-12 * max(1.0, abs(ref[1]))
            g = wf.gradient(y, ph, clean, length, F, 0.3, 0.2 * valid, skip, W, S, name)
            if not valid and wf.scored_range(length, F, skip, W, S) == (0, 0):
                assert not g.any()
                continue
            (0.3 * sse - 0.2 * si).backward()
            assert np.abs(m.grad.numpy() - g).max() <= 1e-12 * max(1.0, np.abs(g).max())


def test_at_the_default_framing_it_is_wave_loss_np():
    mag, ph, clean = wc.batch()
    for i in range(wc.N):
        for skip in (True, False):
            a = wl.wave_loss(mag[i], ph[i], clean[i], wc.LENGTHS[i], wc.FRAMES[i], 0.3, 0.2, skip)
            b = wf.wave_loss(mag[i], ph[i], clean[i], wc.LENGTHS[i], wc.FRAMES[i], 0.3, 0.2, skip, 256, 128, "hamming")
            assert wf.scored_range(wc.LENGTHS[i], wc.FRAMES[i], skip, 256, 128) == wl.scored_range(wc.LENGTHS[i], wc.FRAMES[i], skip)
            assert wf.num_frames(wc.LENGTHS[i], 256, 128) == wl.num_frames(wc.LENGTHS[i])
            for p, q in zip(a[0], b[0]):
                assert abs(p - q) <= 1e-12 * max(1.0, abs(p))
            assert np.abs(a[1] - b[1]).max() <= 1e-12 * max(1.0, np.abs(a[1]).max())
            assert np.abs(a[2] - b[2]).max() <= 1e-12 * max(1.0, np.abs(a[2]).max())


@pytest.mark.parametrize("framing", fc.FRAMINGS, ids=fc.IDS)
def test_si_sdr_is_the_evaluation_loops_up_to_eps(framing):
    W, S, name = framing
    for F in (3, 6, 20):
        mag, ph, clean, length = _utterance(F, framing, 7 + F)
        y = fn.rebuild_ola(mag, ph, F, W, S, name)
        _, si, valid = wf.terms(y, clean, length, F, False, W, S)[:3]
        assert valid == 1.0 and min(length, wf.n_out(F, W, S)) == length
        assert abs(si - td_metrics_np.si_sdr(clean[:length], y[:length])) <= 1e-9      # eps = 1e-8 against sums of 1e2 and more
    assert wf.terms(y, np.zeros(length), length, F, False, W, S)[1:3] == (0.0, 0.0)     # a silent clean signal
    if S <= W - S:                                                                      # one frame: an empty range under skip_edges
        assert wf.terms(y, clean, W, 1, True, W, S)[:3] == (0.0, 0.0, 0.0)


def test_no_denominator_lies_near_the_floor_so_the_zero_sets_agree():
    """The device decides D[i] <= 1e-10 on a float32 sum, the reference on a float64 one.  For every framing and frame count the GPU
    tests use, no D[i] lies within a factor of 10 of 1e-10; then the two float32 sums (a few ulps from the float64 one) fall on its
    side of the floor, sample by sample.  A framing that failed this would be dropped; at least five remain."""
    kept = 0
    for framing in fc.FRAMINGS:
        W, S, name = framing
        for F in sorted(set(fc.counts(W, S)) | {9, 8}):                  # (9, 8: the training step's batch)
            if F == 0:
                continue
            d = wf.denominator(F, W, S, name)
            near = (d > wf.FLOOR / 10) & (d < wf.FLOOR * 10)
            assert not near.any(), (framing, F, d[near])
            for mode in wf.MODES[1:]:
                assert np.array_equal(wf.denominator(F, W, S, name, mode) > np.float32(wf.FLOOR), d > wf.FLOOR), (framing, F, mode)
        kept += 1
    assert kept >= 5
    # the rule does fire where the issue says it does: sample 0 under a window that ends in zero, every seam without overlap
    assert wf.denominator(5, 256, 64, "hanning")[0] <= wf.FLOOR
    d = wf.denominator(5, 256, 256, "bartlett")
    assert (d[0::256] <= wf.FLOOR).all() and (d[255::256] <= wf.FLOOR).all()
    assert (wf.denominator(5, 160, 80, "hamming") > 1e-3).all()


def test_the_batches_are_what_the_issue_asks_for():
    for framing in fc.FRAMINGS:
        W, S, _ = framing
        b = fc.batch(framing)
        assert b.frames[:2] == (65, 64) and b.frames[3:7] == (3, 2, 1, 0) and b.lengths[6] == 0 and not b.clean[fc.SILENT].any()
        assert wf.n_out(b.frames[2], W, S) > fc.CHUNK and wf.n_out(b.frames[2], W, S) % fc.CHUNK
        assert b.T == max(b.frames) + 2 and b.clean_stride % 2 == 1 and b.clean_stride > b.clean_width
        assert (wf.scored_range(b.lengths[5], 1, True, W, S) == (0, 0)) == (S <= W - S)


def test_argument_errors_come_before_any_device_work(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused on its arguments

    def call(N=1, T=1, stride=8, W=160, S=80, name=0, w_sse=1.0, w_si=0.0, skip=1, inv=1.0, mag=p, clean=p, lengths=p, terms=p):
        return lib.rced_wave_loss_fr(mag, p, None, clean, stride, lengths, N, T, W, S, name, w_sse, w_si, skip, inv, terms, None, 0, None)

    for kw, text in (({"W": 257}, b"window must lie"), ({"W": 1}, b"window must lie"), ({"S": 0}, b"stride must lie"),
                     ({"S": 161}, b"stride must lie"), ({"name": 4}, b"window name"), ({"W": 300, "N": -1}, b"window must lie"),
                     ({"N": -1}, b"negative"), ({"T": -1}, b"negative"), ({"stride": -1}, b"negative"),
                     ({"w_sse": -1.0}, b"weights"), ({"w_si": float("nan")}, b"weights"), ({"w_si": float("inf")}, b"weights"),
                     ({"inv": 0.0}, b"inv_batch"), ({"inv": float("nan")}, b"inv_batch"), ({"skip": 2}, b"skip_edges"),
                     ({"N": 65536}, b"65535"), ({"terms": None}, b"null"), ({"lengths": None}, b"null"), ({"clean": None}, b"null"),
                     ({"mag": None}, b"null")):
        assert call(**kw) == _lib.RCED_ERR_ARG, kw
        assert text in lib.rced_last_error(), (kw, lib.rced_last_error())
    assert call(N=0) == _lib.RCED_OK


def test_the_training_entries_refuse_a_framing_then_the_struct_then_the_trainer(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)     # never dereferenced
    W = _lib.WaveArgs
    good = W(0, 0, 1, 1, p, p, 8, p, None)

    def step(args, fr, grad):
        a = ctypes.byref(args) if args is not None else None
        if grad:
            return lib.rced_train_grad_wave_fr(None, p, p, 1, 1, p, p, 0, a, fr[0], fr[1], fr[2], None, None, None)
        return lib.rced_train_step_wave_fr(None, p, p, 1, 1, 0.0, a, fr[0], fr[1], fr[2], None, None, None)

    for grad in (False, True):
        for args, fr, text in ((good, (257, 80, 0), b"window must lie"), (None, (160, 161, 0), b"stride must lie"),
                               (good, (160, 80, 7), b"window name"), (None, (160, 80, 0), b"NULL"),
                               (W(0, 0, 0, 1, p, p, 8, p, None), (160, 80, 0), b"all zero"),
                               (W(0, 0, 1, 1, None, p, 8, p, None), (160, 80, 0), b"phase_dev"),
                               (good, (160, 80, 0), b"trainer is NULL"), (good, (256, 128, 0), b"trainer is NULL")):
            assert step(args, fr, grad) == _lib.RCED_ERR_ARG
            assert text in lib.rced_last_error(), (text, lib.rced_last_error())


def test_python_refusals_and_the_dispatch_of_the_default(built):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, audio
    from fullycnnspeechenhancement_amd.trainer import wave_of_batch
    obj = audio.WaveObjective(0, 1, 1)
    # framing=None and Framing() are today's entries; anything else is the Framing the _fr entries take
    fr = audio.Framing(160, 80, "hamming")
    for pick in (audio._general, FullyCNNTrainer._wave_framing):
        assert pick(None) is None and pick(audio.Framing()) is None and pick(audio.Framing(256, 128, "hamming")) is None
        assert pick(fr) is fr and pick(audio.Framing(256, 128, "hanning")) is not None
        with pytest.raises(ValueError, match="framing must be an audio.Framing"):
            pick((160, 80, "hamming"))
    # the framing is looked at before the tensors are (None stands for them: no device is touched)
    with pytest.raises(ValueError, match="framing must be an audio.Framing"):
        audio.wave_loss_batch(None, None, None, [1], obj, 1, framing="hanning")
    with pytest.raises(ValueError, match="mag must be a CUDA/HIP tensor"):
        audio.wave_loss_batch(None, None, None, [1], obj, 1, framing=fr)
    with pytest.raises(ValueError, match="window must lie"):
        audio.Framing(300, 80)

    class Loader(object):
        class dataset(object):
            framing = fr

    # a loader at a framing is no longer refused for its framing: what is missing here is the device rows
    with pytest.raises(ValueError, match="device rows"):
        wave_of_batch(Loader, None, None, None)
