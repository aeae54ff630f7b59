"""GPU tests of framing as a parameter (kernels_framing.h behind rced_stft_fr / rced_istft_fr / rced_istft_ola_fr): the STFT and
the reference rebuild against the reference's own outputs (tests/golden/framing_ref.npz), the overlap-add rebuild against the
float64 restatement (tests/framing_np.py, pinned to scipy.signal.istft by tests/test_framing_host.py), the general kernels
against the specialised ones at 256 / 128 / hamming, and the framing's way through denoise_pcm, evaluate_pcm and the loader.
Bars: the suite's (2e-6 of the scale for magnitudes, 2e-5 for rebuilds, 5e-5 for a round trip); the overlap-add bar is the suite's
2e-5, relaxed per sample only where the framing itself is worse conditioned than 256 / 128 / hamming (see ola_bar).  Every test
prints the worst figure it measured before it asserts (pytest -s shows them)."""

import os

import numpy as np
import pytest

import framing_np as fnp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "framing_ref.npz")
BLOCK = 64            # frames per block of the kernels
MAG_BOUND = 2e-6      # of max(ref)
PHASE_BOUND = 2e-3    # where ref_mag > 1e-3 * scale: tests/test_audio_edges_gpu.py
REBUILD_BOUND = 2e-5  # of max|ref|
ISTFT_BOUND = 5e-5    # of max|x|, a round trip


@pytest.fixture(scope="module")
def golden(built):
    return np.load(GOLDEN)


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def framing_of(f):
    from fullycnnspeechenhancement_amd import audio
    return audio.Framing(*f)


def check_spectrum(mag, ph, ref_m, ref_p, what):
    """Device frames [T, 129] against reference magnitude and unit phase, as tests/test_audio_edges_gpu.py compares them."""
    scale = ref_m.max()
    if scale == 0.0:                                  # a Hann window's first sample is zero: one sample gives a zero spectrum
        assert not mag.any() and np.all(ph == 1.0 + 0.0j), what
        return 0.0, 0.0
    em = np.abs(mag - ref_m).max() / scale
    strong = ref_m > 1e-3 * scale
    ep = np.abs(ph - ref_p)[strong].max()
    assert em <= MAG_BOUND, "%s: magnitude off by %.3e of the scale" % (what, em)
    assert ep <= PHASE_BOUND, "%s: phase off by %.3e" % (what, ep)
    return em, ep


def seeded_spectra(N, T, seed):
    """Complex spectra that are not the STFT of a real signal (bins 0 and 128 non-real), as float32 magnitude and complex64 phase."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, T, 129)) + 1j * rng.standard_normal((N, T, 129))
    return np.abs(X).astype(np.float32), np.exp(1j * np.angle(X)).astype(np.complex64)


# ---- the _fr entries called directly: audio.stft_batch / istft_batch hand the default framing to the specialised ones -----------------

def stft_fr(pcm, lengths, T, W, S, name):
    import torch
    from fullycnnspeechenhancement_amd import _args, _lib
    n, L = pcm.shape
    mag = torch.empty((n, T, 129), dtype=torch.float32, device="cuda")
    ph = torch.empty((n, T, 129, 2), dtype=torch.float32, device="cuda")
    ldev = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().rced_stft_fr(pcm.data_ptr(), ldev.data_ptr(), n, L, T, W, S, fnp.CODES[name], mag.data_ptr(), ph.data_ptr(), 0,
                                        _args.current_stream(pcm.device)))
    return mag, torch.view_as_complex(ph)


def rebuild_fr(mag, ph, W, S, name, nfft=None, frames=None):
    """nfft given: rced_istft_fr; else rced_istft_ola_fr."""
    import torch
    from fullycnnspeechenhancement_amd import _args, _lib
    mag = mag.float().contiguous()
    phr = torch.view_as_real(ph.to(torch.complex64).contiguous()).contiguous()
    n, T = int(mag.shape[0]), int(mag.shape[1])
    out = torch.empty((n, fnp.width(T, W, S)), dtype=torch.float32, device="cuda")
    st = _args.current_stream(mag.device)
    if nfft is not None:
        _lib.check(_lib.load().rced_istft_fr(mag.data_ptr(), phr.data_ptr(), n, T, nfft, W, S, out.data_ptr(), 0, st))
    else:
        fdev = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
        _lib.check(_lib.load().rced_istft_ola_fr(mag.data_ptr(), phr.data_ptr(), fdev.data_ptr() if fdev is not None else None, n, T, W, S,
                                                 fnp.CODES[name], out.data_ptr(), 0, st))
    return out


# ---- 1. STFT against the reference's own output ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("framing", fnp.FRAMINGS, ids=fnp.FRAMING_IDS)
def test_stft_equals_the_reference(framing, golden):
    from fullycnnspeechenhancement_amd import audio
    key, fr = fnp.tag(*framing), framing_of(framing)
    for i, L in enumerate(golden["lengths_" + key]):
        ref = golden["spec_%s_%d" % (key, i)]
        mag, ph = audio.stft_batch(dev(golden["pcm_%s_%d" % (key, i)])[None], framing=fr)
        assert tuple(mag.shape) == (1, ref.shape[0], 129, 1) and tuple(ph.shape) == (1, ref.shape[0], 129)
        em, ep = check_spectrum(mag[0, :, :, 0].cpu().numpy(), ph[0].cpu().numpy(), np.abs(ref), np.exp(1j * np.angle(ref)),
                                "%s L = %d" % (key, L))
        print("%s L = %d (%d frames): magnitude %.2e of the scale, phase %.2e" % (key, L, ref.shape[0], em, ep))


# ---- 2. a ragged batch ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("framing", fnp.FRAMINGS, ids=fnp.FRAMING_IDS)
def test_stft_of_a_ragged_batch(framing):
    """Five lengths, one of 65 frames (one more than a block), frames= larger than any needs, junk past every length."""
    import torch
    from fullycnnspeechenhancement_amd import audio
    W, S, name = framing
    fr = framing_of(framing)
    lens = [W + BLOCK * S, 1, W - 1, W + 5 * S + 3, W + 30 * S + 7]
    counts = [fnp.num_frames(L, W, S) for L in lens]
    assert counts[0] == BLOCK + 1 and [audio.num_frames(L, fr) for L in lens] == counts
    T = BLOCK + 6
    rng = np.random.default_rng(W + S)
    pcm = np.full((len(lens), max(lens)), 7.0, np.float32)
    for i, L in enumerate(lens):
        pcm[i, :L] = 0.2 * rng.standard_normal(L)
    x = dev(pcm)
    mag, ph = audio.stft_batch(x, lens, frames=T, framing=fr)
    assert tuple(mag.shape) == (len(lens), T, 129, 1) and tuple(ph.shape) == (len(lens), T, 129)
    m, p = mag.cpu().numpy()[..., 0], ph.cpu().numpy()
    worst = (0.0, 0.0)
    for i, L in enumerate(lens):
        ref_m, ref_p = fnp.stft(pcm[i, :L], W, S, name)
        worst = max(worst, check_spectrum(m[i, :counts[i]], p[i, :counts[i]], ref_m, ref_p, "row %d (length %d)" % (i, L)))
        assert not m[i, counts[i]:].any(), "row %d: a frame past the utterance is not zero" % i
        assert np.all(p[i, counts[i]:] == 1.0 + 0.0j), "row %d: phase of a padding frame is not 1 + 0j" % i
    print("%s: worst (magnitude, phase) %.2e, %.2e" % (fnp.tag(*framing), worst[0], worst[1]))
    again = audio.stft_batch(x, lens, frames=T, framing=fr)
    assert torch.equal(again[0], mag) and torch.equal(torch.view_as_real(again[1]), torch.view_as_real(ph))
    for i in (0, 4):                                  # alone, in a row of its own length, with its own frame count
        m1, p1 = audio.stft_batch(x[i:i + 1, :lens[i]].contiguous(), framing=fr)
        assert m1.shape[1] == counts[i]
        assert torch.equal(m1[0], mag[i, :counts[i]]) and torch.equal(torch.view_as_real(p1[0]), torch.view_as_real(ph[i, :counts[i]]))


# ---- 3. the reference rebuild against the reference's own output -----------------------------------------------------------------------

@pytest.mark.parametrize("framing", fnp.HAMMING_FRAMINGS, ids=["%d-%d-%s" % f for f in fnp.HAMMING_FRAMINGS])
def test_reference_rebuild_equals_the_reference(framing, golden):
    import torch
    from fullycnnspeechenhancement_amd import audio
    W, S, name = framing
    key = fnp.tag(*framing)
    for T in golden["rebuild_frames"]:
        mag, ph = dev(golden["rb_mag_%s_%d" % (key, T)])[None], dev(golden["rb_phase_%s_%d" % (key, T)])[None]
        for nfft in golden["rebuild_nfft"]:
            ref = golden["rb_audio_%s_%d_%d" % (key, T, nfft)]
            out = rebuild_fr(mag, ph, W, S, name, nfft=int(nfft))           # the general kernels, at 256 / 128 too
            assert tuple(out.shape) == (1, fnp.width(int(T), W, S))
            err = np.abs(out[0].cpu().numpy() - ref).max() / np.abs(ref).max()
            print("%s T = %d nfft = %d: %.2e of max|ref|" % (key, T, nfft, err))
            assert err <= REBUILD_BOUND
            if (W, S) != (256, 128):                                        # the public way in reaches the same entry
                assert torch.equal(audio.istft_batch(mag, ph, int(nfft), framing=framing_of(framing)), out)


def test_reference_rebuild_is_refused_for_windows_that_end_in_zero(built):
    from fullycnnspeechenhancement_amd import _lib, audio
    mag, ph = seeded_spectra(1, 3, 1)
    for name in ("hanning", "blackman", "bartlett"):
        with pytest.raises(ValueError, match="zero"):
            audio.istft_batch(dev(mag), dev(ph), 256, framing=audio.Framing(160, 80, name))
        assert _lib.load().rced_istft_fr_check(160, 80, fnp.CODES[name]) == _lib.RCED_ERR_ARG
        out = audio.istft_batch(dev(mag), dev(ph), framing=audio.Framing(160, 80, name), rebuild="ola")
        assert tuple(out.shape) == (1, fnp.width(3, 160, 80))


# ---- 4. overlap-add against the restatement --------------------------------------------------------------------------------------------

A0 = fnp.ola_conditioning(8, 256, 128, "hamming").max()       # 229.7 (tests/test_framing_host.py)


def ola_bar(ref, F, W, S, name):
    """Per sample: 2e-5 of max|ref|, times how much worse than 256 / 128 / hamming's worst sample this sample is conditioned
    (A: the growth of one unit of error per frame sample through the division by sum w^2 and the de-emphasis), never less than 1."""
    A = fnp.ola_conditioning(F, W, S, name)
    return REBUILD_BOUND * np.abs(ref).max() * np.maximum(1.0, A / A0)


@pytest.mark.parametrize("framing", fnp.FRAMINGS, ids=fnp.FRAMING_IDS)
def test_overlap_add_equals_the_restatement(framing):
    import torch
    from fullycnnspeechenhancement_amd import audio
    W, S, name = framing
    fr = framing_of(framing)
    T, counts = BLOCK + 6, [BLOCK + 2, 5, BLOCK]                        # above a block, below one, exactly one
    mag, ph = seeded_spectra(len(counts), T, 100 + W + S)
    junk_m, junk_p = mag.copy(), ph.copy()
    for i, F in enumerate(counts):                                      # frames at or past the count must never be read
        junk_m[i, F:], junk_p[i, F:] = np.nan, np.nan
    out = audio.istft_batch(dev(junk_m), dev(junk_p), rebuild="ola", frames=counts, framing=fr)
    assert tuple(out.shape) == (len(counts), fnp.width(T, W, S))
    got = out.cpu().numpy()
    for i, F in enumerate(counts):
        ref = fnp.rebuild_ola(mag[i], ph[i], F, W, S, name)
        n = (F - 1) * S + W
        bar = ola_bar(ref[:n], F, W, S, name)
        ratio = np.abs(got[i, :n] - ref[:n]) / bar
        print("%s F = %d: worst sample at %.3f of its bar (sample %d of %d)" % (fnp.tag(*framing), F, ratio.max(), ratio.argmax(), n))
        assert np.isfinite(got[i]).all() and ratio.max() <= 1.0
        assert not got[i, n:].any(), "columns past (F - 1) S + W are not zero"
        # samples without a denominator: e is zero there, so y is 0.97 times the sample before (held by the bar above), and
        # exactly zero where nothing came before -- the first sample under every window that starts at zero
        dead = fnp.ola_sums(F, W, S, name)[1] <= fnp.DEN_FLOOR
        assert dead.any() == (name != "hamming") and dead[0] == (name != "hamming")
        assert not got[i, :int(np.argmin(dead))].any(), "a leading sample without a denominator is not zero"
    # other N, T and rows: the same bits
    T2 = BLOCK + 2
    swapped = audio.istft_batch(dev(junk_m[[1, 0], :T2]), dev(junk_p[[1, 0], :T2]), rebuild="ola", frames=[counts[1], counts[0]], framing=fr)
    w2 = fnp.width(T2, W, S)
    assert torch.equal(swapped[1], out[0, :w2]) and torch.equal(swapped[0], out[1, :w2])
    small = audio.istft_batch(dev(mag[1:2, :5]), dev(ph[1:2, :5]), rebuild="ola", framing=fr)       # T below a block, no counts
    assert torch.equal(small[0], out[1, :fnp.width(5, W, S)])
    assert torch.equal(audio.istft_batch(dev(junk_m), dev(junk_p), rebuild="ola", frames=counts, framing=fr), out)


# ---- 5. the general kernels against the specialised ones -------------------------------------------------------------------------------

def test_general_kernels_agree_with_the_specialised_ones_at_the_default_framing(built):
    from fullycnnspeechenhancement_amd import audio
    W, S, name = 256, 128, "hamming"
    lens = [W + BLOCK * S, 131, W + 30 * S + 7]
    T = BLOCK + 1
    rng = np.random.default_rng(17)
    pcm = np.zeros((len(lens), max(lens)), np.float32)
    for i, L in enumerate(lens):
        pcm[i, :L] = 0.2 * rng.standard_normal(L)
    mag0, ph0 = audio.stft_batch(dev(pcm), lens, frames=T)
    mag1, ph1 = stft_fr(dev(pcm), lens, T, W, S, name)
    m0, p0, m1, p1 = mag0.cpu().numpy()[..., 0], ph0.cpu().numpy(), mag1.cpu().numpy(), ph1.cpu().numpy()
    for i in range(len(lens)):
        em, ep = check_spectrum(m1[i], p1[i], m0[i], p0[i], "row %d" % i)
        print("STFT row %d: general against specialised, magnitude %.2e of the scale, phase %.2e" % (i, em, ep))
    smag, sph = seeded_spectra(2, T, 23)
    for nfft in (256, 512):
        a = audio.istft_batch(dev(smag), dev(sph), nfft).cpu().numpy()
        b = rebuild_fr(dev(smag), dev(sph), W, S, name, nfft=nfft).cpu().numpy()
        err = np.abs(a - b).max() / np.abs(a).max()
        print("reference rebuild nfft = %d: general against specialised, %.2e of the scale" % (nfft, err))
        assert a.shape == b.shape and err <= REBUILD_BOUND
    counts = [T, 7]
    a = audio.istft_batch(dev(smag), dev(sph), rebuild="ola", frames=counts).cpu().numpy()
    b = rebuild_fr(dev(smag), dev(sph), W, S, name, frames=counts).cpu().numpy()
    err = np.abs(a - b).max() / np.abs(a).max()
    print("overlap-add: general against specialised, %.2e of the scale" % err)
    assert a.shape == b.shape and err <= REBUILD_BOUND


# ---- 5b. the frame buffer between a rebuild's two launches: nothing allocated once it fits, grown when it does not ---------------------

def test_rebuilds_replay_from_a_captured_graph_and_the_frame_buffer_grows(built):
    """A call that allocated, or synchronised, could not be captured: after the first call at a shape on a stream nothing is
    allocated.  Both rebuilds share the stream's frame buffer; a longer batch grows it, and the call that grew it is still right."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    lib = _lib.load()
    N, T, T2, W, S = 2, 5, 9, 160, 80
    smag, sph = seeded_spectra(N, T2, 77)
    omag, oph = seeded_spectra(N, T, 78)

    def spectra(m, p, t):
        return dev(m[:, :t]), torch.view_as_real(dev(p[:, :t])).contiguous()

    def entry(which, mag, phr, t, out, stream):
        if which == "ola":
            return lambda: _lib.check(lib.rced_istft_ola_fr(mag.data_ptr(), phr.data_ptr(), None, N, t, W, S, fnp.CODES["hamming"],
                                                            out.data_ptr(), 0, stream))
        return lambda: _lib.check(lib.rced_istft_fr(mag.data_ptr(), phr.data_ptr(), N, t, 512, W, S, out.data_ptr(), 0, stream))

    side = torch.cuda.Stream()
    for which in ("ola", "ref512"):
        mag, phr = spectra(smag, sph, T)
        mag2, phr2 = spectra(omag, oph, T)
        out = torch.zeros((N, fnp.width(T, W, S)), dtype=torch.float32, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        call = entry(which, mag, phr, T, out, side.cuda_stream)
        call()                                             # sizes the stream's frame buffer
        call()
        side.synchronize()
        eager = out.clone()
        assert eager.abs().max() > 0
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):         # one stream, a linear chain, no parallel branches
            call()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), which
        mag.copy_(mag2)                                    # other inputs at the same addresses
        phr.copy_(phr2)
        torch.cuda.synchronize()
        call()
        side.synchronize()
        eager2 = out.clone()
        assert not torch.equal(eager2, eager)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager2), which
        del graph
    for which in ("ola", "ref512"):                        # T = 9: the first of the two grows the buffer (no graph is replayed after)
        mag, phr = spectra(smag, sph, T2)
        grown = torch.zeros((N, fnp.width(T2, W, S)), dtype=torch.float32, device="cuda")
        plain = torch.zeros_like(grown)
        torch.cuda.synchronize()
        entry(which, mag, phr, T2, grown, side.cuda_stream)()
        entry(which, mag, phr, T2, plain, torch.cuda.current_stream().cuda_stream)()
        torch.cuda.synchronize()
        assert plain.abs().max() > 0 and torch.equal(grown, plain), which


# ---- 6. the framing's way through the engine -------------------------------------------------------------------------------------------

def test_denoise_pcm_and_evaluate_pcm_at_a_framing(built):
    from fullycnnspeechenhancement_amd import InferenceEngine, audio
    from oracle import rced_np
    eng = InferenceEngine(net_work="FullyCNNV3", weights=rced_np.make_weights("FullyCNNV3", seed=42))
    fr = audio.Framing(160, 80)
    rng = np.random.default_rng(31)
    clean = (0.2 * rng.standard_normal(3001)).astype(np.float32)
    mix = (clean + 0.1 * rng.standard_normal(3001)).astype(np.float32)
    out = eng.denoise_pcm(mix, rebuild="ola", framing=fr)
    mag, ph = audio.stft_batch(dev(mix)[None], framing=fr)
    assert mag.shape[1] == fnp.num_frames(3001, 160, 80)
    by_hand = audio.istft_batch(eng.model(mag), ph, rebuild="ola", framing=fr)
    assert out.shape == (3001,) and np.array_equal(out, by_hand[0, :3001].cpu().numpy())
    assert not np.array_equal(out, eng.denoise_pcm(mix, rebuild="ola")[:3001])          # the framing is honoured, not dropped
    denoise, sdr = eng.evaluate_pcm([mix], [clean], rebuild="ola", framing=fr)
    assert np.array_equal(denoise[0], out)
    want = audio.sdr_batch(dev(clean)[None], by_hand, [3001]).cpu().numpy()
    print("SDR at %r: %.4f dB" % (fr, sdr[0]))
    assert sdr.shape == (1,) and sdr[0] == want[0]
    with pytest.raises(ValueError, match="zero"):
        eng.denoise_pcm(mix, framing=audio.Framing(160, 80, "hanning"))


# ---- 7. the loader ---------------------------------------------------------------------------------------------------------------------

def test_loader_batches_are_cut_by_the_datasets_framing(built):
    import torch
    from fullycnnspeechenhancement_amd import audio, engine, loader
    fr = audio.Framing(256, 64, "hanning")
    rng = np.random.default_rng(41)
    lens = [901, 5000, 300, 2222]
    clean = [(3000 * rng.standard_normal(L)).astype(np.int16) for L in lens]
    mixes = [np.clip(c.astype(np.int32) + rng.integers(-2000, 2000, len(c)), -32768, 32767).astype(np.int16) for c in clean]
    ds = loader.DataSet(loader.Corpus.from_arrays(clean), mix=loader.Corpus.from_arrays(mixes), framing=fr)
    assert ds.framing == fr and loader.DataSet(loader.Corpus.from_arrays(clean), mix=loader.Corpus.from_arrays(mixes)).framing is None
    dl = loader.DataLoader(ds, 2)
    assert engine.loader_framing(dl) == fr
    seen = 0
    for batch_mix, batch_clean, mix_sig, clean_sig in dl:
        T = max(audio.num_frames(L, fr) for L in clean_sig.lengths)
        assert tuple(batch_mix.shape) == tuple(batch_clean.shape) == (2, T, 129, 1)
        for batch, sig in ((batch_mix, mix_sig), (batch_clean, clean_sig)):
            want, _ = audio.stft_batch(sig.rows.contiguous(), sig.lengths, frames=T, with_phase=False, framing=fr)
            assert torch.equal(batch, want)
        seen += 1
    assert seen == 2
    with pytest.raises(ValueError):
        loader.DataSet(loader.Corpus.from_arrays(clean), mix=loader.Corpus.from_arrays(mixes), framing=(256, 64, "hanning"))


# ---- 7b. the reference's own classes, with the reference's own arguments ---------------------------------------------------------------

def test_reference_classes_honour_their_arguments(golden):
    from fullycnnspeechenhancement_amd import audio, loader
    # AudioFeature("hanning") at 32 ms / 8 ms, through AudioParser as the reference's data set calls it
    key = fnp.tag(256, 64, "hanning")
    sig, ref = golden["pcm_%s_4" % key], golden["spec_%s_4" % key]
    spec = loader.AudioParser(8000, window_ms=32, stride_ms=8, windows_name="hanning", use_complex=True).parse_audio(sig)
    assert spec.shape == ref.T.shape
    err = np.abs(np.abs(spec) - np.abs(ref.T)).max() / np.abs(ref).max()
    print("AudioParser(32 ms, 8 ms, hanning): magnitude %.2e of the scale" % err)
    assert err <= MAG_BOUND
    # compute_spectrogram's own defaults: 20 ms / 10 ms
    key = fnp.tag(160, 80, "hamming")
    sig, ref = golden["pcm_%s_4" % key], golden["spec_%s_4" % key]
    mag = audio.AudioFeature().compute_spectrogram(sig, 8000, nfft=256)
    assert mag.dtype == np.float32 and np.abs(mag - np.abs(ref.T)).max() <= MAG_BOUND * np.abs(ref).max()
    # AudioReBuild().rebuild_audio at 20 ms / 10 ms, nfft = 512 as the reference ships it
    T = 7
    out = audio.AudioReBuild().rebuild_audio([500], golden["rb_mag_%s_%d" % (key, T)][None], golden["rb_phase_%s_%d" % (key, T)][None],
                                             8000, 20, 10)
    want = golden["rb_audio_%s_%d_512" % (key, T)]
    assert len(out) == 1 and out[0].shape == (500,)
    assert np.abs(out[0] - want[:500]).max() <= REBUILD_BOUND * np.abs(want).max()


# ---- 7c. the corners of the definition's range -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("framing", [(2, 1, "hamming"), (256, 1, "hanning"), (3, 3, "bartlett")], ids=["2-1-hamming", "256-1-hanning", "3-3-bartlett"])
def test_smallest_window_and_smallest_stride(framing):
    """W = 2, S = 1 (299 frames of two samples), S = 1 under a full window (256 addends per sample), and a window with one live
    sample in three: the same bars as above."""
    from fullycnnspeechenhancement_amd import audio
    W, S, name = framing
    fr = framing_of(framing)
    L = 300
    sig = (0.2 * np.random.default_rng(W).standard_normal(L)).astype(np.float32)
    T = fnp.num_frames(L, W, S)
    mag, ph = audio.stft_batch(dev(sig)[None], framing=fr)
    assert mag.shape[1] == T
    ref_m, ref_p = fnp.stft(sig, W, S, name)
    em, ep = check_spectrum(mag[0, :, :, 0].cpu().numpy(), ph[0].cpu().numpy(), ref_m, ref_p, fnp.tag(*framing))
    smag, sph = seeded_spectra(1, T, 5)
    got = audio.istft_batch(dev(smag), dev(sph), rebuild="ola", framing=fr)[0].cpu().numpy()
    ref = fnp.rebuild_ola(smag[0], sph[0], T, W, S, name)
    ratio = np.abs(got - ref) / ola_bar(ref, T, W, S, name)
    print("%s (%d frames): magnitude %.2e of the scale, phase %.2e; overlap-add at %.3f of its bar" % (fnp.tag(*framing), T, em, ep, ratio.max()))
    assert got.shape == ref.shape == (fnp.width(T, W, S),) and ratio.max() <= 1.0


# ---- 8. round trip ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("framing", fnp.HAMMING_FRAMINGS, ids=["%d-%d-%s" % f for f in fnp.HAMMING_FRAMINGS])
def test_overlap_add_inverts_the_stft(framing):
    W, S, name = framing
    L = W + (BLOCK + 5) * S + 13                                            # 71 frames: past one block
    rng = np.random.default_rng(L)
    x = np.convolve(rng.standard_normal(L), np.ones(8) / 8, "same").astype(np.float32)      # tests/test_ola_host.py's signal
    mag, ph = stft_fr(dev(x)[None], [L], fnp.num_frames(L, W, S), W, S, name)
    back = rebuild_fr(mag, ph, W, S, name, frames=[fnp.num_frames(L, W, S)])[0, :L].cpu().numpy()
    err = np.abs(back - x).max() / np.abs(x).max()
    print("%s L = %d: OLA(STFT(x)) off by %.2e of max|x|" % (fnp.tag(*framing), L, err))
    assert err <= ISTFT_BOUND
