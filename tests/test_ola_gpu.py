"""GPU tests of the overlap-add rebuild (rced_istft_ola, istft_ola_x6_kernel) against its float64 restatement (tests/ola_np.py,
pinned to scipy and to the reference's own rebuild by tests/test_ola_host.py), and of the `rebuild` keyword through every layer.
Bars: 2e-5 of the row's scale against the restatement -- the bar tests/test_audio_gpu.py holds the reference rebuild to; the
overlap-add coefficients are no larger than its 1 / w, so it is conditioned no worse --, 2e-4 of the peak for STFT -> ISTFT round
trips and 1e-4 for the pipeline with the net, as there.  Invariants (padding, neighbours, run to run) are asked for bit for bit.
Figures are printed before they are asserted."""

import numpy as np
import pytest

import ola_np
from oracle import audio_np

pytestmark = pytest.mark.gpu

N, T = 6, 70                                  # 70 frames: across the 64-frame block seam
FRAMES = [70, 64, 65, 1, 2, 0]                # the whole row; a full block (hop 64 alone in the next one); one frame past the seam; the edges


def dev(a):
    import torch
    return torch.tensor(a, device="cuda")


@pytest.fixture(scope="module")
def case(built):
    """Seeded complex spectra [N, T, 129], bins 0 and 128 non-real, and the restatement's rows: computed once, left unchanged."""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N, T, 129)) + 1j * rng.standard_normal((N, T, 129))
    mag, ph = np.abs(X).astype(np.float32), np.exp(1j * np.angle(X)).astype(np.complex64)
    ref = np.stack([ola_np.ola(mag[i], ph[i], frames=FRAMES[i]) for i in range(N)])
    for a in (mag, ph, ref):
        a.setflags(write=False)
    return mag, ph, ref


def run(mag, ph, frames):
    from fullycnnspeechenhancement_amd.audio import istft_batch
    return istft_batch(dev(mag), dev(ph), rebuild="ola", frames=frames).cpu().numpy()


def test_against_the_restatement(case):
    mag, ph, ref = case
    out = run(mag, ph, FRAMES)
    assert out.shape == ref.shape == (N, (T + 1) * 128) and out.dtype == np.float32
    worst = 0.0
    for i, F in enumerate(FRAMES):
        end = (F + 1) * 128 if F else 0
        assert not out[i, end:].any()                             # exactly 0 past the utterance; every column for F = 0
        if F:
            err = np.abs(out[i] - ref[i]).max() / np.abs(ref[i]).max()
            worst = max(worst, err)
            print("row %d, %d frames: %.2e of the scale (bar 2e-5)" % (i, F, err))
    print("worst %.2e" % worst)
    assert worst <= 2e-5
    # frames=None is T each; a count outside [0, T] is clamped into it
    full = run(mag, ph, None)
    assert np.array_equal(full[0], out[0]) and np.array_equal(run(mag, ph, [99, 64, 65, 1, 2, -3]), out)
    err = np.abs(full[1] - ola_np.ola(mag[1], ph[1])).max() / np.abs(ref[1]).max()
    assert err <= 2e-5


def test_padding_rows_and_neighbours_do_not_reach_the_bits(case):
    """Utterance n's result depends on its own F frames only: not on T, on what the frames at or past F hold (after the net a
    padded frame is not zero: here NaN), on its row, on N or on its neighbours."""
    mag, ph, _ = case
    base = run(mag, ph, FRAMES)
    assert np.isfinite(base).all()
    T2 = 130
    mag2 = np.full((N, T2, 129), np.nan, np.float32)
    ph2 = np.full((N, T2, 129), np.nan + 1j * np.nan, np.complex64)
    for i, F in enumerate(FRAMES):
        mag2[i, :F], ph2[i, :F] = mag[i, :F], ph[i, :F]
    wide = run(mag2, ph2, FRAMES)
    assert wide.shape == (N, (T2 + 1) * 128) and np.isfinite(wide).all()
    assert np.array_equal(wide[:, :(T + 1) * 128], base) and not wide[:, (T + 1) * 128:].any()
    order = [4, 0, 5, 2, 1, 3]
    shuffled = run(mag2[order, :T], ph2[order, :T], [FRAMES[i] for i in order])
    assert np.array_equal(shuffled, base[order])
    for i in range(N):
        alone = run(mag2[i:i + 1, :T], ph2[i:i + 1, :T], FRAMES[i:i + 1])
        assert np.array_equal(alone[0], base[i])


def test_run_to_run(case):
    mag, ph, _ = case
    assert np.array_equal(run(mag, ph, FRAMES), run(mag, ph, FRAMES))


def test_round_trip_on_ragged_signals(built):
    from fullycnnspeechenhancement_amd.audio import istft_batch, num_frames, stft_batch
    lens = [256, 300, 1000, 8321]                                  # 8,321 = 64 frames + 1 sample: 65 frames
    rng = np.random.default_rng(9)
    sigs = [(0.2 * rng.standard_normal(L)).astype(np.float32) for L in lens]
    pcm = np.zeros((len(lens), max(lens)), np.float32)
    for i, s in enumerate(sigs):
        pcm[i, :len(s)] = s
    frames = [num_frames(L) for L in lens]
    assert frames == [1, 2, 7, 65]
    mag, ph = stft_batch(dev(pcm), lens)
    back = istft_batch(mag, ph, rebuild="ola", frames=frames).cpu().numpy()
    for i, s in enumerate(sigs):
        err = np.abs(back[i, :len(s)] - s).max() / np.abs(s).max()
        print("L = %d (%d frames): round trip %.2e of the peak (bar 2e-4)" % (len(s), frames[i], err))
        assert err <= 2e-4
        assert not back[i, (frames[i] + 1) * 128:].any()
    # one frame: both hops are single-frame, overlap-add IS the reference rebuild at the matching nfft
    one_ola = istft_batch(mag[:1, :1], ph[:1, :1], rebuild="ola").cpu().numpy()
    one_ref = istft_batch(mag[:1, :1], ph[:1, :1], nfft=256).cpu().numpy()
    err = np.abs(one_ola - one_ref).max() / np.abs(one_ref).max()
    print("T = 1: overlap-add against the nfft = 256 reference rebuild %.2e (bar 2e-5)" % err)
    assert one_ola.shape == (1, 256) and err <= 2e-5
    # AudioReBuild derives the frame counts from the lengths
    from fullycnnspeechenhancement_amd.audio import AudioReBuild
    rows = AudioReBuild(rebuild="ola").rebuild_audio(lens, mag.cpu().numpy()[..., 0], ph.cpu().numpy(), 8000, 32, 16)
    assert all(np.array_equal(rows[i], back[i, :L]) for i, L in enumerate(lens))


def test_denoise_pcm_matches_the_oracle_chain(built):
    """STFT -> net -> overlap-add on the device against oracle STFT -> the oracle's masks -> the restatement: the pipeline bar."""
    from fullycnnspeechenhancement_amd import InferenceEngine
    from oracle import rced_c, rced_np
    w = rced_np.make_weights("FullyCNNV3", seed=42)
    eng = InferenceEngine(net_work="FullyCNNV3", weights=w)
    sig = (0.2 * np.random.default_rng(13).standard_normal(8321)).astype(np.float32)
    out = eng.denoise_pcm(sig, rebuild="ola")
    mag, phase = audio_np.stft(sig)
    pred = rced_c.forward("FullyCNNV3", w, mag.astype(np.float32)[None, :, :, None], np.float64)[0, :, :, 0]
    ref = ola_np.ola(pred, phase, length=len(sig))
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print("denoise_pcm(rebuild='ola'): %.2e of the scale (bar 1e-4)" % err)
    assert out.shape == sig.shape and out.dtype == np.float32 and err <= 1e-4
    assert not np.array_equal(out, eng.denoise_pcm(sig))           # the default is the other rebuild


def ragged(seed, lens):
    rng = np.random.default_rng(seed)
    clean = [(0.2 * rng.standard_normal(L)).astype(np.float32) for L in lens]
    return [c + (0.1 * rng.standard_normal(len(c))).astype(np.float32) for c in clean], clean


def test_evaluation_loop(built):
    from fullycnnspeechenhancement_amd import FullyCNNTester, FullyCNNTrainer, engine
    from oracle import rced_np
    w = rced_np.make_weights("FullyCNNV3", seed=42)
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=w)
    mix, clean = ragged(21, (3000, 8321, 300, 8192))             # 23, 65, 2 and 63 frames
    # the engine's own net, and a stand-in that leaves padded frames NON-zero element by element (its own bits cannot depend on
    # the batch, so what it shows is the rebuild's and the scores' independence alone)
    for name, net in (("net", None), ("stand-in", lambda m: 0.7 * m + 0.05)):
        den, sdr, more = eng.evaluate_pcm(mix, clean, model=net, rebuild="ola", extra=("si_sdr",))
        for i in range(4):
            d1, s1, m1 = eng.evaluate_pcm(mix[i:i + 1], clean[i:i + 1], model=net, rebuild="ola", extra=("si_sdr",))
            print("%s, utterance %d: alone / in the batch sdr %.17g / %.17g, si_sdr %.17g / %.17g, audio off by %.2e"
                  % (name, i, s1[0], sdr[i], m1["si_sdr"][0], more["si_sdr"][i], np.abs(d1[0] - den[i]).max()))
            assert np.array_equal(d1[0], den[i]) and den[i].shape == clean[i].shape
            assert s1[0] == sdr[i] and m1["si_sdr"][0] == more["si_sdr"][i]
            assert np.isfinite(den[i]).all() and np.isfinite(sdr[i])
    # test() and valid() hand the keyword down and average what evaluate_pcm scores
    batches = [(None, None) + ragged(22, (3000, 1800, 4096)), (None, None) + ragged(23, (2500, 5000))]
    scores = [s for _, _, m, c in batches for s in eng.evaluate_pcm(m, c, rebuild="ola")[1]]
    avg = eng.test(batches, rebuild="ola")
    assert eng.sdr_score.count == 5 and abs(avg - np.mean(scores)) <= 1e-12
    assert abs(avg - FullyCNNTester(net_work="FullyCNNV3", weights=w).test(batches)) > 1e-6     # not the reference rebuild's scores
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, weights=w)
    scores = [s for _, _, m, c in batches for s in engine.evaluate_pcm(tr.valid_step, m, c, rebuild="ola")[1]]
    avg = tr.valid(batches, 4, rebuild="ola")
    assert tr.sdr_score.count == 5 and abs(avg - np.mean(scores)) <= 1e-12
    tr.close()


def test_the_default_is_untouched(case):
    from fullycnnspeechenhancement_amd.audio import istft_batch
    mag, ph, _ = case
    m, p = dev(mag), dev(ph)
    for nfft in (512, 256):
        assert np.array_equal(istft_batch(m, p, nfft).cpu().numpy(), istft_batch(m, p, nfft, rebuild="reference").cpu().numpy())
    assert not np.array_equal(istft_batch(m, p, 256).cpu().numpy(), istft_batch(m, p, rebuild="ola").cpu().numpy())


def test_abi_refuses_bad_arguments(case):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    mag, ph, _ = case
    m, p = dev(mag), torch.view_as_real(dev(ph)).contiguous()
    out = torch.full((N, (T + 1) * 128), 3.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for n, t, o, word in ((-1, T, out.data_ptr(), b"negative"), (N, -1, out.data_ptr(), b"negative"), (N, T, None, b"null")):
        assert lib.rced_istft_ola(m.data_ptr(), p.data_ptr(), None, n, t, o, 0, st) == _lib.RCED_ERR_ARG
        assert word in lib.rced_last_error()
    assert lib.rced_istft_ola(None, p.data_ptr(), None, N, T, out.data_ptr(), 0, st) == _lib.RCED_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                               # a refused call writes nothing
    # T = 0: no frames to read, [N, 128] written as 0
    short = torch.full((2, 128), 3.0, device="cuda")
    assert lib.rced_istft_ola(None, None, None, 2, 0, short.data_ptr(), 0, st) == 0
    torch.cuda.synchronize()
    assert not bool(short.any())
