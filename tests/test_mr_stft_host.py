"""CPU tests of the multi-resolution STFT term's restatement (tests/mr_stft_np.py), of the bars tests/test_mr_stft_gpu.py holds the
device to (tests/mr_stft_cases.py), of the argument errors of every entry that takes the term, which come before any device work,
and of WaveObjective's new fields."""

import ctypes

import numpy as np
import pytest

import framing_np as fn
import mr_stft_cases as mc
import mr_stft_np as mr
import wave_loss_fr_np as wf


def _pair(n, seed):
    """A reference with energy in every bin and an estimate near it: no magnitude of either comes close to zero by design of the test,
    only by chance."""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal(n + 8)
    ref = ref[8:] + 0.9 * ref[7:-1] + 0.5 * ref[4:-4]
    return 0.8 * ref + 0.3 * rng.standard_normal(n), ref


@pytest.mark.parametrize("key", mc.IDS)
@pytest.mark.parametrize("lo,hi", [(0, 700), (37, 612), (80, 336), (5, 5), (10, 60)])
def test_analytic_gradient_equals_autograd(key, lo, hi):
    """The pin: 1e-12 of the largest entry."""
    import torch
    est, ref = _pair(700, 11 + hi)
    (term, valid, _), g = mr.mr_stft(est, ref, lo, hi, mc.SETS[key], 0.3)
    y = torch.tensor(est, dtype=torch.float64, requires_grad=True)
    t, v = mr.torch_term(y, ref, lo, hi, mc.SETS[key])
    assert v == valid and abs(float(t.detach()) - term) <= 1e-12 * max(1.0, abs(term))
    if not valid:
        assert term == 0.0 and not g.any()
        return
    (0.3 * t).backward()
    assert not g[:lo].any() and not g[hi:].any()
    worst = np.abs(y.grad.numpy() - g).max() / np.abs(g).max()
    print("%s [%d, %d): %.2e of the largest entry" % (key, lo, hi, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("key", mc.IDS)
def test_gradient_against_central_differences(key):
    """Forty samples of every kind -- the range's first and last, the last whole frame's end, one behind it --: the two-step form of
    test_wave_loss_host.py at its 1e-9 of the largest entry.  The steps are its steps times 1e-2: the log-magnitude part's higher
    derivatives grow like 1 / |Y|^k at a bin whose magnitude happens to be small."""
    lo, hi = 21, 620
    est, ref = _pair(640, 5)
    res = mc.SETS[key]
    g = mr.mr_stft(est, ref, lo, hi, res, 0.25)[1]
    scale = np.abs(g).max()
    W, S, _ = res[0]
    last = lo + (mr.frames_in(lo, hi, W, S) - 1) * S + W       # the end of the last whole frame of the first resolution
    rng = np.random.default_rng(3)
    picks = [lo - 1, lo, hi - 1, hi, last - 1, min(last, hi - 1)] + [int(v) for v in rng.integers(lo, hi, 34)]

    def central(i, h):
        up, dn = est.copy(), est.copy()
        up[i] += h
        dn[i] -= h
        return 0.25 * (mr.mr_stft(up, ref, lo, hi, res, grad=False)[0][0] - mr.mr_stft(dn, ref, lo, hi, res, grad=False)[0][0]) / (2 * h)

    worst = 0.0
    for i in picks:
        fd = (4 * central(i, 5e-6) - central(i, 1e-5)) / 3
        worst = max(worst, abs(fd - g[i]) / scale)
    print("%s: %.2e of the largest entry" % (key, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("mode", mr.MODES)
def test_equal_signals_give_a_zero_term_and_an_exactly_zero_gradient(mode):
    est, _ = _pair(700, 9)
    est = est.astype(np.float32)
    for key in mc.IDS:
        (term, valid, detail), g = mr.mr_stft(est, est, 13, 655, mc.SETS[key], 0.5, mode)
        assert term == 0.0 and valid == 1.0 and all(sc == 0.0 and lsd == 0.0 for sc, lsd, _ in detail)
        assert not g.any()


def test_frames_are_whole_and_inside_the_range():
    """Samples behind the last whole frame, and everything outside [lo, hi), play no part: changing them changes nothing."""
    est, ref = _pair(700, 2)
    res = mc.SETS["odd"]
    lo, hi = 40, 597
    want = mr.mr_stft(est, ref, lo, hi, res)
    ends = [lo + (mr.frames_in(lo, hi, W, S) - 1) * S + W for W, S, _ in res]
    assert max(ends) < hi
    e2, r2 = est.copy(), ref.copy()
    for a in (e2, r2):
        a[:lo] = 1e6
        a[max(ends):] = -1e6
    got = mr.mr_stft(e2, r2, lo, hi, res)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and not want[1][max(ends):].any()
    assert [d[2] for d in want[0][2]] == [(hi - lo - W) // S + 1 for W, S, _ in res]


def test_without_the_term_the_wave_chain_is_wave_loss_fr_nps():
    """mr_stft_np.wave_loss_mr restates wave_loss_fr_np.gradient around one addition: with a zero weight they are the same arrays."""
    b = mc.wave_batch()
    for i in (2, 3, 5, 7):
        for mode in mr.MODES:
            for skip in (True, False):
                y = b.rebuilt(i, mode)
                terms, g, _ = mr.wave_loss_mr(b.mag[i], b.ph[i], b.clean[i], b.lengths[i], b.frames[i], 0.125, 0.25, 0.0, skip, *mc.FRAMING,
                                              resolutions=mc.WAVE_SETS["two"], mode=mode, y=y)
                want = wf.wave_loss(b.mag[i], b.ph[i], b.clean[i], b.lengths[i], b.frames[i], 0.125, 0.25, skip, *mc.FRAMING, mode=mode, y=y)
                assert terms[:3] == want[0] and np.array_equal(g, want[1])


def test_the_two_yardstick_chains_lie_within_the_margin_of_each_other():
    """A bar of MARGIN x the larger error means something only if it is not a bar on which chain one happened to pick."""
    worst = 0.0
    cases = [("direct %s" % key, mc.reference(key)) for key in mc.IDS]
    cases += [("wave %s %s skip_edges %s" % c, mc.wave_batch().reference(*c)) for c in mc.WAVE_CASES]
    for what, rows in cases:
        for i, row in enumerate(rows):
            g, yard = row[1], row[2]
            if not g.any():
                assert yard == (0.0, 0.0)
                continue
            a, b = yard
            print("%s row %d: plain %.2e, device order %.2e of the largest entry" % (what, i, a, b))
            # (1 / |Y|^2 at the smallest magnitude of a row conditions the log-magnitude part: a float32 spectrum moves such a bin's
            # entry by far more than 2^-24 of it, in either chain)
            assert 0 < a < 1e-2 and 0 < b < 1e-2
            worst = max(worst, a / b, b / a)
    print("worst ratio %.2f" % worst)
    assert worst <= mc.MARGIN


def test_the_cases_hold_the_ranges_they_are_there_for():
    J = lambda l, r: mr.frames_in(0, l, r[0], r[1])
    r8 = mc.MR_STFT_8K
    assert [J(200, r) for r in r8] == [0, 3, 9] and J(256, r8[0]) == 1 and J(576, r8[0]) == 6 and J(575, r8[0]) == 5
    assert J(1500, r8[2]) > 64 and all(J(63, r) == 0 for s in mc.SETS.values() for r in s)
    for key in mc.IDS:
        rows = mc.reference(key)
        assert rows[5][0][:2] == (0.0, 0.0) and rows[7][0][:2] == (0.0, 0.0) and rows[mc.SILENT][0][1] == 1.0
        assert not rows[5][1].any() and not rows[7][1].any()
    b = mc.wave_batch()
    rows = b.reference("8k", (0.0, 0.0, 1.0), True)
    assert rows[5][0][3:] == (0.0, 0.0) and rows[6][0][3:] == (0.0, 0.0)          # an empty range under skip_edges; no samples
    lo, hi = wf.scored_range(b.lengths[3], 3, True, 160, 80)
    assert hi - lo == 160 and b.reference("two", (0.0, 0.0, 1.0), True)[3][0][4] == 1.0 and rows[3][0][3] > 0
    assert max(b.frames) <= 67 and b.T <= 67


# ---- the entries' argument errors -----------------------------------------------------------------------------------------------

def _mr(w=1.0, n=2, window=(64, 32, 0, 0), stride=(16, 8, 0, 0), name=(0, 1, 0, 0)):
    from fullycnnspeechenhancement_amd import _lib
    return _lib.MrArgs(w, n, (ctypes.c_int * 4)(*window), (ctypes.c_int * 4)(*stride), (ctypes.c_int * 4)(*name))


BAD_MR = (({"w": -1.0}, b"w_mr"), ({"w": float("nan")}, b"w_mr"), ({"w": float("inf")}, b"w_mr"), ({"n": 0}, b"n_res"), ({"n": 5}, b"n_res"),
          ({"window": (64, 257, 0, 0)}, b"window"), ({"stride": (16, 33, 0, 0)}, b"stride"), ({"stride": (0, 8, 0, 0)}, b"stride"),
          ({"name": (0, 4, 0, 0)}, b"window name"))


def test_the_check_names_what_it_refuses(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    assert lib.rced_mr_stft_check(None) == _lib.RCED_ERR_ARG and b"NULL" in lib.rced_last_error()
    for kw, text in BAD_MR:
        assert lib.rced_mr_stft_check(ctypes.byref(_mr(**kw))) == _lib.RCED_ERR_ARG, kw
        assert text in lib.rced_last_error(), (kw, lib.rced_last_error())
    assert lib.rced_mr_stft_check(ctypes.byref(_mr())) == _lib.RCED_OK
    assert lib.rced_mr_stft_check(ctypes.byref(_mr(w=0.0, n=1, window=(2, 999, -1, 0), stride=(1, 0, 0, 0)))) == _lib.RCED_OK     # only n_res resolutions are looked at


def test_argument_errors_come_before_any_device_work(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)     # never dereferenced: every call below is refused on its arguments

    def direct(N=1, es=8, rs=8, inv=1.0, est=p, ref=p, lengths=p, terms=p, mr=None):
        m = ctypes.byref(mr if mr is not None else _mr())
        return lib.rced_mr_stft(est, es, ref, rs, lengths, N, m, inv, terms, None, 0, None)

    def wave(N=1, T=1, stride=8, w_sse=1.0, w_si=0.0, skip=1, inv=1.0, mag=p, clean=p, lengths=p, terms=p, W=160, S=80, name=0, mr=None):
        m = ctypes.byref(mr if mr is not None else _mr())
        return lib.rced_wave_loss_mr(mag, p, None, clean, stride, lengths, N, T, W, S, name, w_sse, w_si, skip, inv, m, terms, None, 0, None)

    for kw, text in (({"N": -1}, b"negative"), ({"es": -1}, b"negative"), ({"rs": -1}, b"negative"), ({"inv": 0.0}, b"inv_batch"),
                     ({"inv": float("nan")}, b"inv_batch"), ({"N": 65536}, b"65535"), ({"terms": None}, b"null"), ({"lengths": None}, b"null"),
                     ({"est": None}, b"null"), ({"ref": None}, b"null")) + tuple(({"mr": _mr(**kw)}, text) for kw, text in BAD_MR):
        assert direct(**kw) == _lib.RCED_ERR_ARG, kw
        assert text in lib.rced_last_error(), (kw, lib.rced_last_error())
    assert lib.rced_mr_stft(p, 8, p, 8, p, 1, None, 1.0, p, None, 0, None) == _lib.RCED_ERR_ARG and b"NULL" in lib.rced_last_error()
    assert direct(N=0) == _lib.RCED_OK
    for kw, text in (({"N": -1}, b"negative"), ({"T": -1}, b"negative"), ({"stride": -1}, b"negative"), ({"w_sse": -1.0}, b"weights"),
                     ({"w_si": float("nan")}, b"weights"), ({"inv": 0.0}, b"inv_batch"), ({"skip": 2}, b"skip_edges"), ({"N": 65536}, b"65535"),
                     ({"terms": None}, b"null"), ({"lengths": None}, b"null"), ({"clean": None}, b"null"), ({"mag": None}, b"null"),
                     ({"W": 257}, b"window"), ({"S": 161}, b"stride"), ({"name": 7}, b"window name")) + \
            tuple(({"mr": _mr(**kw)}, text) for kw, text in BAD_MR):
        assert wave(**kw) == _lib.RCED_ERR_ARG, kw
        assert text in lib.rced_last_error(), (kw, lib.rced_last_error())
    assert lib.rced_wave_loss_mr(p, p, None, p, 8, p, 1, 1, 160, 80, 0, 1.0, 0.0, 1, 1.0, None, p, None, 0, None) == _lib.RCED_ERR_ARG
    assert wave(N=0) == _lib.RCED_OK


def test_the_training_entries_refuse_bad_arguments_before_they_look_at_the_trainer(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)     # never dereferenced
    Wv = _lib.WaveArgs

    def step(args, mr, y=p, grad=False, fr=(160, 80, 0)):
        a = ctypes.byref(args) if args is not None else None
        m = ctypes.byref(mr) if mr is not None else None
        if grad:
            return lib.rced_train_grad_wave_mr(None, p, y, 1, 1, p, p, 0, a, fr[0], fr[1], fr[2], m, None, None, None)
        return lib.rced_train_step_wave_mr(None, p, y, 1, 1, 0.0, a, fr[0], fr[1], fr[2], m, None, None, None)

    good = Wv(0, 0, 0, 1, p, p, 8, p, None)        # every weight of the struct zero: the term's weight carries the objective
    for grad in (False, True):
        for args, mra, y, fr, text in ((good, _mr(), None, (300, 80, 0), b"window"), (good, None, None, (160, 80, 0), b"NULL"),
                                       (None, _mr(), p, (160, 80, 0), b"NULL"), (good, _mr(w=0.0), None, (160, 80, 0), b"all zero"),
                                       (Wv(-1, 0, 0, 1, p, p, 8, p, None), _mr(), p, (160, 80, 0), b"weights"),
                                       (Wv(1, 0, 0, 1, p, p, 8, p, None), _mr(), None, (160, 80, 0), b"target is NULL"),
                                       (Wv(0, 0, 0, 1, None, p, 8, p, None), _mr(), None, (160, 80, 0), b"phase_dev"),
                                       (Wv(0, 0, 0, 1, p, None, 8, p, None), _mr(), None, (160, 80, 0), b"clean_dev"),
                                       (Wv(0, 0, 0, 1, p, p, 8, None, None), _mr(), None, (160, 80, 0), b"lengths_dev"),
                                       (good, _mr(), None, (160, 80, 0), b"trainer is NULL")) + \
                tuple((good, _mr(**kw), None, (160, 80, 0), text) for kw, text in BAD_MR):
            assert step(args, mra, y, grad, fr) == _lib.RCED_ERR_ARG
            assert text in lib.rced_last_error(), (text, lib.rced_last_error())


# ---- WaveObjective ---------------------------------------------------------------------------------------------------------------

def test_objective_value_checks_and_the_unchanged_repr(built):
    from fullycnnspeechenhancement_amd import audio
    F = audio.Framing
    assert audio.MR_STFT_8K == (F(256, 64, "hanning"), F(128, 32, "hanning"), F(64, 16, "hanning"))
    o = audio.WaveObjective()
    assert (o.mr_stft, o.resolutions) == (0.0, None) and not o.has_wave_term
    assert repr(o) == "WaveObjective(spectral=1.0, wave_sse=0.0, si_sdr=0.0, skip_edges=True)"
    assert repr(audio.WaveObjective(0, 0.5, 2, False)) == "WaveObjective(spectral=0.0, wave_sse=0.5, si_sdr=2.0, skip_edges=False)"
    m = audio.WaveObjective(0, 0, 0, True, 0.5)
    assert m.has_wave_term and m.mr_stft == 0.5 and m.resolutions == audio.MR_STFT_8K
    assert m == audio.WaveObjective(0.0, 0.0, 0.0, True, mr_stft=0.5, resolutions=list(audio.MR_STFT_8K)) and hash(m) == hash(
        audio.WaveObjective(0, 0, 0, True, 0.5, audio.MR_STFT_8K))
    other = audio.WaveObjective(0, 0, 0, True, 0.5, (F(64, 16),))
    assert m != other and m != audio.WaveObjective(0, 0, 0, True, 0.25) and audio.WaveObjective(1, 0, 0) != audio.WaveObjective(1, 0, 0, True, 0.5)
    assert "mr_stft=0.5" in repr(other) and "Framing(window=64, stride=16" in repr(other)
    a = other.mr_args()
    assert (a.w_mr, a.n_res, a.window[0], a.stride[0], a.window_name[0]) == (0.5, 1, 64, 16, 0)
    with pytest.raises(ValueError, match="must not all be zero"):
        audio.WaveObjective(0, 0, 0, True, 0.0)
    for bad in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="mr_stft"):
            audio.WaveObjective(1, 0, 0, True, bad)
    for bad in ((), (F(),) * 5, (F(), (64, 16, "hamming")), 7):
        with pytest.raises(ValueError, match="resolutions"):
            audio.WaveObjective(1, 0, 0, True, 1.0, bad)
    with pytest.raises(AttributeError):
        m.mr_stft = 1.0
    assert fn.CODES["hanning"] == F(64, 16, "hanning").code
