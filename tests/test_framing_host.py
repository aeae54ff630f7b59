"""CPU tests of framing as a parameter: the float64 restatement (tests/framing_np.py) against the reference's own outputs
(tests/golden/framing_ref.npz, made by tests/golden/make_golden_framing.py) and against scipy.signal.istft; audio.Framing's
validation and its two rounding rules; the library's host-only entries.  Bounds: 1e-12 of the scale, float64 round-off."""

import os

import numpy as np
import pytest

import framing_np as fnp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "framing_ref.npz")
EXACT = 1e-12


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def spectra(T, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, 129)) + 1j * rng.standard_normal((T, 129))
    return np.abs(X), np.exp(1j * np.angle(X))


def test_golden_file_is_small_enough():
    assert os.path.getsize(GOLDEN) <= 631529


@pytest.mark.parametrize("framing", fnp.FRAMINGS, ids=fnp.FRAMING_IDS)
def test_restated_stft_equals_the_reference(framing, golden):
    W, S, name = framing
    key = fnp.tag(*framing)
    lengths = [int(v) for v in golden["lengths_" + key]]
    assert lengths == [1, W - 1, W, W + 1, W + 5 * S + 3]
    for i, L in enumerate(lengths):
        ref = golden["spec_%s_%d" % (key, i)]
        mag, ph = fnp.stft(golden["pcm_%s_%d" % (key, i)], W, S, name)
        assert ref.shape == (fnp.num_frames(L, W, S), 129) == mag.shape        # the frame count is the reference's
        # (a Hann window's first sample is zero: the spectrum of a one-sample signal is zero, and then so is the restatement's)
        err = np.abs(mag * ph - ref).max() / (np.abs(ref).max() or 1.0)
        print("%s L = %d: %d frames, restated STFT off by %.2e of the scale" % (key, L, ref.shape[0], err))
        assert err <= EXACT


@pytest.mark.parametrize("framing", fnp.HAMMING_FRAMINGS, ids=["%d-%d-%s" % f for f in fnp.HAMMING_FRAMINGS])
def test_restated_reference_rebuild_equals_the_reference(framing, golden):
    W, S, name = framing
    key = fnp.tag(*framing)
    for T in golden["rebuild_frames"]:
        for nfft in golden["rebuild_nfft"]:
            ref = golden["rb_audio_%s_%d_%d" % (key, T, nfft)]
            out = fnp.rebuild_reference(golden["rb_mag_%s_%d" % (key, T)], golden["rb_phase_%s_%d" % (key, T)], W, S, int(nfft))
            assert out.shape == ref.shape == (fnp.width(int(T), W, S),)
            err = np.abs(out - ref).max() / np.abs(ref).max()
            print("%s T = %d nfft = %d: restated rebuild off by %.2e of the scale" % (key, T, nfft, err))
            assert err <= EXACT


@pytest.mark.parametrize("framing", fnp.FRAMINGS, ids=fnp.FRAMING_IDS)
@pytest.mark.parametrize("T", [1, 3, 70])
def test_restated_overlap_add_equals_scipy_istft(framing, T):
    """scipy's weighted overlap-add inverse divides by the same sum of squared windows and leaves the same samples zero; it
    scales the spectrum by sum(w) (scaling='spectrum'), hence the division."""
    import scipy.signal as ss
    W, S, name = framing
    mag, ph = spectra(T, 7)
    w = fnp.window(name, W)
    y = fnp.rebuild_ola(mag, ph, T, W, S, name)
    e = np.append(y[0], y[1:] - fnp.PRE * y[:-1])
    _, x = ss.istft((mag * ph).T / w.sum(), window=w, nperseg=W, noverlap=W - S, nfft=256, boundary=False, input_onesided=True)
    assert x.shape == e.shape == (fnp.width(T, W, S),)
    err = np.abs(x - e).max() / np.abs(x).max()
    print("%s T = %d: restated overlap-add against scipy.signal.istft, %.2e of the scale" % (fnp.tag(*framing), T, err))
    assert err <= EXACT


def test_overlap_add_reads_its_own_frames_only():
    W, S, name = 200, 80, "blackman"
    mag, ph = spectra(9, 3)
    a = fnp.rebuild_ola(mag, ph, 5, W, S, name)
    junk = mag.copy()
    junk[5:] = np.nan
    b = fnp.rebuild_ola(junk, ph, 5, W, S, name)
    assert np.array_equal(a, b) and not a[4 * S + W:].any() and a[0] == 0.0      # blackman's first sample: denominator ~ 2e-34


def test_the_bar_of_the_fixed_framing():
    """A0 of the overlap-add bound (tests/test_framing_gpu.py): the conditioning of 256 / 128 / hamming, the framing the suite's
    2e-5 was set for."""
    a0 = fnp.ola_conditioning(8, 256, 128, "hamming").max()
    print("A0 = %.2f" % a0)
    assert abs(a0 - 229.7) < 0.1


# ---- audio.Framing and the host-only entries ----------------------------------------------------------------------------------------

def test_framing_is_a_validated_immutable_value(built):
    from fullycnnspeechenhancement_amd import audio
    f = audio.Framing()
    assert (f.window, f.stride, f.windows_name) == (256, 128, "hamming") and f.is_default
    g = audio.Framing(160, 80, "hanning")
    assert g == audio.Framing(160, 80, "hanning") and g != f and hash(g) == hash(audio.Framing(160, 80, "hanning"))
    assert not g.is_default and not audio.Framing(256, 128, "hanning").is_default
    assert g.width(7) == 80 + 7 * 80
    with pytest.raises(AttributeError):
        g.window = 200
    for bad in ((257, 128, "hamming"), (1, 1, "hamming"), (256, 0, "hamming"), (128, 129, "hamming"), (256, 128, "kaiser"),
                (256.5, 128, "hamming")):
        with pytest.raises(ValueError):
            audio.Framing(*bad)
    assert audio.Framing(2, 1).window == 2 and audio.Framing(256, 256, "bartlett").stride == 256


def test_framing_rounds_as_the_reference_does(built):
    from fullycnnspeechenhancement_amd import audio
    # en_frame: int(round(s * rate)); rebuild_audio: int(ms * rate / 1000) -- they differ, and each is kept where it is used
    assert audio.Framing.from_seconds(8000, 0.02, 0.01, "hanning") == audio.Framing(160, 80, "hanning")
    assert audio.Framing.from_seconds(8000, 0.0319, 0.016) == audio.Framing(255, 128)           # 255.2 rounds down
    assert audio.Framing.from_seconds(8000, 0.03195, 0.016) == audio.Framing(256, 128)          # 255.6 rounds up
    assert audio.Framing.from_ms(8000, 31.95, 16) == audio.Framing(255, 128)                    # 255.6 truncates
    assert audio.Framing.from_ms(8000, 32, 16) == audio.Framing() and audio.Framing.from_ms(8000, 20, 10) == audio.Framing(160, 80)
    with pytest.raises(ValueError):
        audio.Framing.from_seconds(16000, 0.02, 0.01)                                           # 320 samples


def test_num_frames_matches_the_reference(built, golden):
    from fullycnnspeechenhancement_amd import audio
    for W, S, name in fnp.FRAMINGS:
        key = fnp.tag(W, S, name)
        fr = audio.Framing(W, S, name)
        for i, L in enumerate(golden["lengths_" + key]):
            assert audio.num_frames(int(L), fr) == golden["spec_%s_%d" % (key, i)].shape[0]
        for L in (1, 2, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 8321):
            assert audio.num_frames(L, fr) == fnp.num_frames(L, W, S)
    assert audio.num_frames(8321, audio.Framing()) == audio.num_frames(8321) == 65


def test_library_refuses_bad_framings_without_a_device(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    assert lib.rced_framing_check(256, 128, 0) == _lib.RCED_OK and lib.rced_framing_check(2, 1, 3) == _lib.RCED_OK
    for W, S, name in ((257, 128, 0), (256, 0, 0), (128, 129, 0), (256, 128, 4), (1, 1, 0), (256, 128, -1)):
        assert lib.rced_framing_check(W, S, name) == _lib.RCED_ERR_ARG, (W, S, name)
        assert lib.rced_last_error()
        if 0 <= name <= 3:
            assert lib.rced_stft_num_frames_fr(1000, W, S) == -1
        assert lib.rced_stft_fr(None, None, 1, 1000, 4, W, S, name, None, None, 0, None) == _lib.RCED_ERR_ARG
        assert lib.rced_istft_ola_fr(None, None, None, 1, 4, W, S, name, None, 0, None) == _lib.RCED_ERR_ARG
    assert lib.rced_istft_fr(None, None, 1, 4, 512, 257, 128, None, 0, None) == _lib.RCED_ERR_ARG
    assert lib.rced_istft_fr(None, None, 1, 4, 300, 160, 80, None, 0, None) == _lib.RCED_ERR_ARG
    assert lib.rced_stft_num_frames_fr(1000, 160, 80) == 12 and lib.rced_stft_num_frames_fr(0, 160, 80) == 0


def test_reference_rebuild_is_refused_by_name(built):
    """hanning, blackman and bartlett end in zero (np.blackman: -1.4e-17): the reference divides by them.  Refused by the name."""
    from fullycnnspeechenhancement_amd import _lib, audio
    lib = _lib.load()
    assert lib.rced_istft_fr_check(160, 80, 0) == _lib.RCED_OK
    for name in ("hanning", "blackman", "bartlett"):
        assert lib.rced_istft_fr_check(160, 80, fnp.CODES[name]) == _lib.RCED_ERR_ARG
        assert name.encode() in lib.rced_last_error() and b"zero" in lib.rced_last_error()
        with pytest.raises(ValueError, match="zero"):
            audio.check_reference_rebuild(audio.Framing(160, 80, name))
        with pytest.raises(ValueError, match="zero"):
            audio.AudioReBuild(name)
        assert audio.AudioReBuild(name, rebuild="ola").windows_name == name
        assert audio.AudioFeature(name).windows_name == name
    with pytest.raises(ValueError):
        audio.AudioFeature("kaiser")
    # the reference's own result, for the record: not finite (hanning, bartlett) or off by 1e17 (blackman)
    mag, ph = spectra(2, 5)
    for name in ("hanning", "bartlett"):
        with np.errstate(divide="ignore", invalid="ignore"):
            assert not np.isfinite(fnp.rebuild_reference(mag, ph, 160, 80, 256, name)).all()
    with np.errstate(over="ignore"):
        assert np.abs(fnp.rebuild_reference(mag, ph, 160, 80, 256, "blackman")).max() > 1e14
