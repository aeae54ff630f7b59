"""CPU tests of the evaluation loop's host side: the two C entries exist, bind and refuse bad arguments without a device;
plan_noise consumes np.random exactly as the reference's add_noise does (tests/golden/eval_ref.npz records both the
draws and where the reference leaves the stream); the closed form the kernels compute reproduces the reference's
mixtures; AverageMeter / padding_batch / SDR's argument checks."""

import ctypes
import re

import numpy as np
import pytest

import eval_closed_form as cf
from conftest import ROOT


@pytest.fixture(scope="module")
def gold():
    return cf.load_fixture()


def n_cases(gold):
    return len(gold["cases"])


def test_entries_are_declared_exported_and_bound(built):
    import os
    from fullycnnspeechenhancement_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rced.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in ("rced_sdr", "rced_mix_snr"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS and getattr(_lib.load(), name).restype is ctypes.c_int


def test_bad_arguments_are_refused_before_any_device_is_touched(built):
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    p = 4096                      # never dereferenced on the host
    ARG = _lib.RCED_ERR_ARG
    assert lib.rced_sdr(None, 8, p, 8, None, 1, p, None, 0, None) == ARG
    assert lib.rced_sdr(p, 8, None, 8, None, 1, p, None, 0, None) == ARG
    assert lib.rced_sdr(p, 8, p, 8, None, 1, None, None, 0, None) == ARG
    assert lib.rced_sdr(p, 8, p, 8, None, -1, p, None, 0, None) == ARG
    assert lib.rced_sdr(p, -8, p, 8, None, 1, p, None, 0, None) == ARG
    assert b"null pointer" in lib.rced_last_error() or b"negative" in lib.rced_last_error()
    assert lib.rced_mix_snr(None, None, 1, 8, p, None, 8, None, None, 0, 0.0, p, 0, None) == ARG
    assert lib.rced_mix_snr(p, None, 1, 8, None, None, 8, None, None, 0, 0.0, p, 0, None) == ARG
    assert lib.rced_mix_snr(p, None, 1, 8, p, None, 8, None, None, 0, 0.0, None, 0, None) == ARG
    assert lib.rced_mix_snr(p, None, -1, 8, p, None, 8, None, None, 0, 0.0, p, 0, None) == ARG
    assert lib.rced_mix_snr(p, None, 1, 8, p, None, 8, None, None, -1, 0.0, p, 0, None) == ARG
    assert lib.rced_mix_snr(p, None, 1, 8, p, None, 8, None, None, 2, 0.0, p, 0, None) == ARG      # gains promised, none given
    assert lib.rced_sdr(p, 8, p, 8, None, 0, p, None, 0, None) == 0                                  # nothing to do
    assert lib.rced_mix_snr(p, None, 0, 8, p, None, 8, None, None, 0, 0.0, p, 0, None) == 0


def test_entries_fail_loudly_without_gpu(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    if torch.cuda.is_available():
        return                    # with a device these calls would run: tests/test_eval_gpu.py
    lib, p = _lib.load(), 4096
    assert lib.rced_sdr(p, 8, p, 8, None, 1, p, None, 0, None) == _lib.RCED_ERR_HIP
    assert b"no CPU fallback" in lib.rced_last_error()
    assert lib.rced_mix_snr(p, None, 1, 8, p, None, 8, None, None, 0, 0.0, p, 0, None) == _lib.RCED_ERR_HIP


def test_plan_noise_draws_what_the_reference_draws(gold):
    from fullycnnspeechenhancement_amd.loader import plan_noise
    for i, (ls, ln, _snr) in enumerate(gold["cases"]):
        np.random.seed(int(gold["seed_%d" % i]))
        start, gains = plan_noise(ls, ln)
        assert np.random.random() == float(gold["next_%d" % i]), "case %d leaves np.random elsewhere" % i
        assert start == int(gold["start_%d" % i])
        assert gains.dtype == np.float64 and np.array_equal(gains, gold["gains_%d" % i])
        assert len(gains) <= int(gold["draws_%d" % i])


def test_closed_form_reproduces_the_reference_mixtures(gold):
    """The formula the kernel computes, in numpy float64 with the recorded draws, against add_noise's own output."""
    for i, (ls, ln, snr) in enumerate(gold["cases"]):
        ref = gold["mix_%d" % i]
        got = cf.mix(gold["speech_%d" % i], gold["noise_%d" % i], int(snr), int(gold["start_%d" % i]), gold["gains_%d" % i])
        assert got.shape == ref.shape == (ls,)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("case %d (ls %d, ln %d): closed form vs reference %.2e of the scale" % (i, ls, ln, err))
        assert err <= 1e-12


def test_fixture_sanity_rows(gold):
    """nfft = 256 inverts the STFT, so with the identity mask the residual is the scaled noise: SDR = the configured SNR."""
    for i, (_ls, _ln, snr) in enumerate(gold["cases"]):
        assert abs(float(gold["sdr_%d_256_10" % i]) - snr) < 1e-3
        for nfft in cf.NFFTS:
            for g in cf.GAINS:
                stored = float(gold["sdr_%d_%d_%d" % (i, nfft, int(g * 10))])
                # the stored score is of the un-cast float64 signal: the float32 cast moves it by far less than 1e-5 dB
                assert abs(cf.sdr(gold["speech_%d" % i], cf.rebuilt(gold, i, nfft, g)) - stored) < 1e-5


def test_gains_needed():
    from fullycnnspeechenhancement_amd.audio import gains_needed
    assert [gains_needed(*a) for a in ((100, 200), (200, 200), (201, 200), (400, 200), (401, 200), (65536, 300), (8192, 1100))] \
        == [0, 0, 1, 1, 2, 8, 3]


def test_average_meter():
    from fullycnnspeechenhancement_amd.metrics import AverageMeter
    m = AverageMeter()
    assert (m.val, m.avg, m.sum, m.count) == (0, 0, 0, 0)
    m.update(2.0)
    m.update(4.0)
    assert (m.val, m.sum, m.count, m.avg) == (4.0, 6.0, 2, 3.0)
    m.update(3.0, n=2)                        # as the reference: sum += val, count += n
    assert (m.sum, m.count, m.avg) == (9.0, 4, 2.25)
    m.reset()
    assert (m.val, m.avg, m.sum, m.count) == (0, 0, 0, 0)


def test_padding_batch():
    from fullycnnspeechenhancement_amd.loader import padding_batch
    a = np.arange(6, dtype=np.float32).reshape(3, 2)          # [F = 3, T = 2]
    b = 10 + np.arange(12, dtype=np.float32).reshape(3, 4)    # [F = 3, T = 4]
    out = padding_batch([a, b])
    assert out.shape == (2, 4, 3, 1) and out.dtype == np.float32
    assert np.array_equal(out[0, :, :, 0], [[0, 2, 4], [1, 3, 5], [0, 0, 0], [0, 0, 0]])
    assert np.array_equal(out[1, :, :, 0], b.T)
    c = padding_batch([(a + 1j * a).astype(np.complex128)])
    assert c.dtype == np.complex128 and c.shape == (1, 2, 3, 1)


def test_sdr_argument_checks():
    from fullycnnspeechenhancement_amd.metrics import SDR
    with pytest.raises(ValueError):
        SDR()(np.zeros((2, 8)), np.zeros((2, 8)))             # utils.py:74
    with pytest.raises(ValueError):
        SDR()(np.zeros(8), np.zeros(9))                       # utils.py:75


def test_package_exports_the_evaluation_surface():
    import fullycnnspeechenhancement_amd as pkg
    assert hasattr(pkg.audio, "mix_snr_batch") and hasattr(pkg.audio, "sdr_batch")
    assert hasattr(pkg.loader, "AudioParser") and hasattr(pkg.loader, "plan_noise")
    assert hasattr(pkg.FullyCNNTester, "evaluate_pcm") and hasattr(pkg.FullyCNNTester, "test")
    assert hasattr(pkg.FullyCNNTrainer, "valid")
