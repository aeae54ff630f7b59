"""CPU tests of the waveform objective's restatement (tests/wave_loss_np.py), of the bars tests/test_wave_loss_gpu.py holds the
device to (tests/wave_loss_cases.py), and of rced_wave_loss's argument errors, which come before any device work."""

import ctypes

import numpy as np
import pytest

import td_metrics_np
import wave_loss_cases as wc
import wave_loss_np as wl


def _utterance(length, seed, frames_pad=2):
    rng = np.random.default_rng(seed)
    F = wl.num_frames(length)
    T = F + frames_pad
    X = rng.standard_normal((T, 129)) + 1j * rng.standard_normal((T, 129))
    mag, ph = np.abs(X) + 0.01, np.exp(1j * np.angle(X))
    y = wl.rebuild(mag, ph, F)[:length]
    clean = 0.7 * y + 0.5 * np.sqrt(np.mean(y * y)) * rng.standard_normal(length)
    return mag, ph, clean, F


@pytest.mark.parametrize("length", [130, 256, 257, 384, 385, 1000, 8327])
@pytest.mark.parametrize("weights", [(0.25, 0.0), (0.0, 0.25)])
def test_gradient_against_central_differences(length, weights):
    """Sixty entries of every kind -- first, last and padded frames, bins 0 and 128 --: 1e-9 of the largest entry, for both terms."""
    mag, ph, clean, F = _utterance(length, 100 + length)
    for skip in (True, False):
        g = wl.gradient(wl.rebuild(mag, ph, F), ph, clean, length, F, weights[0], weights[1], skip)
        assert not g[F:].any()                                       # padded frames: exactly zero
        lo, hi = wl.scored_range(length, F, skip)
        if hi <= lo:
            assert not g.any()
            continue
        rng = np.random.default_rng(length)
        picks = [(0, 0), (0, 128), (F - 1, 0), (F - 1, 128), (F - 1, 64), (F, 5)] + \
                [(int(rng.integers(F)), int(rng.integers(129))) for _ in range(54)]
        worst, scale = 0.0, np.abs(g).max()

        def central(t, b, h):
            up, dn = mag.copy(), mag.copy()
            up[t, b] += h
            dn[t, b] -= h
            return (wl.objective(up, ph, clean, length, F, weights[0], weights[1], skip) -
                    wl.objective(dn, ph, clean, length, F, weights[0], weights[1], skip)) / (2 * h)

        for t, b in picks:
            # two step sizes, the h^2 term removed: over a range of two samples the SI-SDR's third derivative is large enough for
            # a single central difference to miss 1e-9 by its own truncation at any step its rounding allows
            fd = (4 * central(t, b, 5e-4) - central(t, b, 1e-3)) / 3
            worst = max(worst, abs(fd - g[t, b]) / scale)
        print("length %d, weights %s, skip_edges %s: %.2e of the largest entry" % (length, weights, skip, worst))
        assert worst <= 1e-9


def test_si_sdr_is_the_evaluation_loops_up_to_eps():
    for length in (385, 1000, 8327):
        mag, ph, clean, F = _utterance(length, 7 + length)
        y = wl.rebuild(mag, ph, F)
        _, si, valid = wl.terms(y, clean, length, F, False)[:3]
        hi = min(length, 128 * (F + 1))
        assert valid == 1.0 and hi == length
        assert abs(si - td_metrics_np.si_sdr(clean[:hi], y[:hi])) <= 1e-9      # eps = 1e-8 against sums of 1e2 and more
    # the invalid row: a silent clean signal, an empty range
    assert wl.terms(y, np.zeros(length), length, F, False)[1:3] == (0.0, 0.0)
    mag, ph, clean, F = _utterance(256, 3)
    assert wl.terms(wl.rebuild(mag, ph, F), clean, 256, F, True)[:3] == (0.0, 0.0, 0.0)


@pytest.mark.parametrize("length", [130, 257, 1000])
def test_torch_form_equals_the_numpy_form(length):
    import torch
    mag, ph, clean, F = _utterance(length, 50 + length)
    for skip in (True, False):
        m = torch.tensor(mag, dtype=torch.float64, requires_grad=True)
        sse, si, valid = wl.torch_terms(m, ph, clean, length, F, skip)
        ref = wl.terms(wl.rebuild(mag, ph, F), clean, length, F, skip)
        assert valid == ref[2]
        assert abs(float(sse.detach()) - ref[0]) <= 1e-12 * max(1.0, abs(ref[0]))
        assert abs(float(si.detach()) - ref[1]) <= 1e-12 * max(1.0, abs(ref[1]))
        (0.3 * sse - 0.2 * si).backward()
        g = wl.gradient(wl.rebuild(mag, ph, F), ph, clean, length, F, 0.3, 0.2 * valid, skip)
        assert np.abs(m.grad.numpy() - g).max() <= 1e-12 * max(1.0, np.abs(g).max())


def test_the_two_yardstick_chains_lie_within_the_margin_of_each_other():
    """A bar of MARGIN x the larger error means something only if it is not a bar on which chain one happened to pick."""
    worst = 0.0
    for weights, skip in wc.CASES:
        for i, (terms, g, yard, bar) in enumerate(wc.reference(weights, skip)):
            if not g.any():
                assert yard == (0.0, 0.0)
                continue
            a, b = yard
            print("weights %s skip_edges %-5s row %d (%4d samples): plain %.2e, device order %.2e of the largest entry"
                  % (weights, skip, i, wc.LENGTHS[i], a, b))
            assert 0 < a < 1e-4 and 0 < b < 1e-4
            worst = max(worst, a / b, b / a)
    print("worst ratio %.2f" % worst)
    assert worst <= wc.MARGIN


def test_argument_errors_come_before_any_device_work(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused on its arguments

    def call(N=1, T=1, stride=8, w_sse=1.0, w_si=0.0, skip=1, inv=1.0, mag=p, clean=p, lengths=p, terms=p):
        return lib.rced_wave_loss(mag, p, None, clean, stride, lengths, N, T, w_sse, w_si, skip, inv, terms, None, 0, None)

    for kw, text in (({"N": -1}, b"negative"), ({"T": -1}, b"negative"), ({"stride": -1}, b"negative"),
                     ({"w_sse": -1.0}, b"weights"), ({"w_si": float("nan")}, b"weights"), ({"w_si": float("inf")}, b"weights"),
                     ({"inv": 0.0}, b"inv_batch"), ({"inv": float("nan")}, b"inv_batch"), ({"skip": 2}, b"skip_edges"),
                     ({"N": 65536}, b"65535"), ({"terms": None}, b"null"), ({"lengths": None}, b"null"), ({"clean": None}, b"null"),
                     ({"mag": None}, b"null")):
        assert call(**kw) == _lib.RCED_ERR_ARG, kw
        assert text in lib.rced_last_error(), (kw, lib.rced_last_error())
    assert call(N=0) == _lib.RCED_OK


def test_the_training_entries_refuse_a_bad_struct_before_they_look_at_the_trainer(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)     # never dereferenced

    def step(args, y=p, grad=False):
        a = ctypes.byref(args) if args is not None else None
        if grad:
            return lib.rced_train_grad_wave(None, p, y, 1, 1, p, p, 0, a, None, None, None)
        return lib.rced_train_step_wave(None, p, y, 1, 1, 0.0, a, None, None, None)

    W = _lib.WaveArgs
    for grad in (False, True):
        for args, y, text in ((None, p, b"NULL"), (W(0, 0, 0, 1, p, p, 8, p, None), p, b"all zero"),
                              (W(-1, 1, 0, 1, p, p, 8, p, None), p, b"weights"), (W(1, float("nan"), 0, 1, p, p, 8, p, None), p, b"weights"),
                              (W(1, 1, 0, 2, p, p, 8, p, None), p, b"skip_edges"), (W(1, 1, 0, 1, p, p, 8, p, None), None, b"target is NULL"),
                              (W(1, 1, 0, 1, None, p, 8, p, None), p, b"phase_dev"), (W(0, 0, 1, 1, p, None, 8, p, None), p, b"clean_dev"),
                              (W(0, 0, 1, 1, p, p, 8, None, None), p, b"lengths_dev"),
                              (W(0, 0, 1, 1, p, p, 8, p, None), None, b"trainer is NULL"),        # a good struct, no target needed
                              (W(2, 0, 0, 1, None, None, 0, None, None), p, b"trainer is NULL")):  # no wave term: no wave pointers needed
            assert step(args, y, grad) == _lib.RCED_ERR_ARG
            assert text in lib.rced_last_error(), (text, lib.rced_last_error())


def test_objective_value_checks(built):
    from fullycnnspeechenhancement_amd import audio
    o = audio.WaveObjective()
    assert (o.spectral, o.wave_sse, o.si_sdr, o.skip_edges) == (1.0, 0.0, 0.0, True) and not o.has_wave_term
    assert audio.WaveObjective(0, 0, 2).has_wave_term and audio.WaveObjective(1, 0.5, 0) == audio.WaveObjective(1.0, 0.5, 0.0)
    for bad in ((0, 0, 0), (-1, 1, 0), (1, float("nan"), 0), (1, 0, float("inf")), ("x", 0, 0)):
        with pytest.raises(ValueError):
            audio.WaveObjective(*bad)
    with pytest.raises(ValueError):
        audio.WaveObjective(skip_edges=2)
    with pytest.raises(AttributeError):
        o.si_sdr = 1.0
