"""GPU tests of the evaluation loop: SNR mixing (rced_mix_snr), ragged SDR (rced_sdr) and the STFT -> net -> ISTFT -> SDR
chain, against REAL reference outputs (tests/golden/eval_ref.npz: the reference's own add_noise / AudioReBuild / SDR run
on float32 signals widened to float64) and, where the reference cannot run, against its closed form in numpy float64
(tests/eval_closed_form.py, itself checked against the fixture by tests/test_eval_host.py).  Every bar is derived from
the number formats or from bounds the suite already holds, and stated where it is used; figures are printed before
they are asserted."""

import numpy as np
import pytest

import eval_closed_form as cf

pytestmark = pytest.mark.gpu

DB = 10 / np.log(10)          # d(10 log10 x) = DB * dx / x


@pytest.fixture(scope="module")
def gold(built):
    return cf.load_fixture()


@pytest.fixture(params=["x6", "f32"], ids=["x6", "fp32-mfma"])
def K(request, built):
    """Both STFT / ISTFT kernel families, as in tests/test_audio_gpu.py."""
    return request.param


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.asarray(a, dtype) if dtype else a, device="cuda")


def padded(rows, width, fill=7.0):
    """float32 [N, width] holding rows[i] from column 0 and junk after it (junk past a length must not leak in)."""
    out = np.full((len(rows), width), fill, np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def pairs(gold):
    """Every (clean, rebuilt, stored score) of the fixture, float32 signals."""
    out = []
    for i in range(len(gold["cases"])):
        for nfft in cf.NFFTS:
            for g in cf.GAINS:
                out.append((gold["speech_%d" % i], cf.rebuilt(gold, i, nfft, g), float(gold["sdr_%d_%d_%d" % (i, nfft, int(g * 10))])))
    return out


# ---- SDR ----------------------------------------------------------------------------------------------------------

def test_sdr_pinned_to_the_reference(gold):
    from fullycnnspeechenhancement_amd.audio import sdr_batch
    ps = pairs(gold)
    lens = [len(y) for y, _, _ in ps]
    # one ragged batch, two different padded strides (neither a multiple of 4: rows start unaligned)
    clean, est = padded([y for y, _, _ in ps], max(lens) + 5), padded([e for _, e, _ in ps], max(lens) + 131, fill=-3.0)
    got = sdr_batch(dev(clean), dev(est), lens).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (len(ps),)
    for k, (y, e, stored) in enumerate(ps):
        want = cf.sdr(y, e)                        # the reference formula on the same float32 arrays widened to float64
        # against the fixture's score (of the un-cast float64 signals) the bar is the float32 cast's
        cast_bar = 8.69 * 2.0 ** -24 * (np.linalg.norm(y.astype(np.float64)) / np.linalg.norm(e.astype(np.float64) - y) + 1) * 2
        print("pair %2d L %5d: sdr %+.10f dB, vs formula %.2e (bar 1e-9), vs stored %.2e (bar %.2e)"
              % (k, len(y), got[k], abs(got[k] - want), abs(got[k] - stored), cast_bar))
        # fp64 sums of <= 8192 exactly widened terms: relative error <= ~1e-13, times 10 / ln 10; room for the device log10
        assert abs(got[k] - want) <= 1e-9
        assert abs(got[k] - stored) <= cast_bar


def test_sdr_edge_values(gold):
    from fullycnnspeechenhancement_amd.audio import sdr_batch
    from fullycnnspeechenhancement_amd.metrics import SDR
    y = gold["speech_0"]
    clean = padded([y, np.zeros(3000, np.float32), y], 4000)
    est = padded([y, gold["speech_0"][:3000], y], 4100)
    got = sdr_batch(dev(clean), dev(est), [4000, 3000, 0]).cpu().numpy()
    perfect = 10 * np.log10(np.sum(y.astype(np.float64) ** 2) / cf.EPS32)       # y_pred == y
    assert abs(got[0] - perfect) <= 1e-9
    assert got[1] == -np.inf and got[2] == -np.inf                              # all-zero clean; a length of 0
    assert abs(SDR()(y, cf.rebuilt(gold, 0, 512, 1.0)) - cf.sdr(y, cf.rebuilt(gold, 0, 512, 1.0))) <= 1e-9
    assert isinstance(SDR()(y, y), float)
    with pytest.raises(ValueError):
        sdr_batch(dev(clean), dev(est), [4001, 1, 1])
    with pytest.raises(ValueError):
        sdr_batch(dev(clean), dev(est), [1, -1, 1])


# ---- add_noise ----------------------------------------------------------------------------------------------------

def mix_bar(speech, ref):
    """One fp32 rounding is 2^-24 of the result; a factor 2 for the fp64 scale."""
    return 2.0 ** -23 * (np.abs(speech.astype(np.float64)) + np.abs(ref - speech))


def fixture_batch(gold):
    n = len(gold["cases"])
    speech, noise = [gold["speech_%d" % i] for i in range(n)], [gold["noise_%d" % i] for i in range(n)]
    return dict(speech=speech, noise=noise, sl=[len(s) for s in speech], nl=[len(v) for v in noise],
                starts=[int(gold["start_%d" % i]) for i in range(n)], gains=[gold["gains_%d" % i] for i in range(n)])


def test_mix_pinned_to_the_reference(gold):
    from fullycnnspeechenhancement_amd.audio import mix_snr_batch
    from fullycnnspeechenhancement_amd.loader import AudioParser
    b = fixture_batch(gold)
    Ls, Ln = max(b["sl"]) + 3, max(b["nl"]) + 1
    speech, noise = dev(padded(b["speech"], Ls)), dev(padded(b["noise"], Ln, fill=-9.0))
    for snr in sorted(set(int(c[2]) for c in gold["cases"])):      # the SNR is one value per call: one batch per value
        mix = mix_snr_batch(speech, noise, snr, b["sl"], b["nl"], b["starts"], b["gains"]).cpu().numpy()
        assert mix.shape == (len(b["sl"]), Ls) and mix.dtype == np.float32
        for i, (ls, ln, case_snr) in enumerate(gold["cases"]):
            assert not mix[i, ls:].any()                           # columns past each length are 0
            if case_snr != snr:
                continue
            ref = gold["mix_%d" % i]
            excess = np.abs(mix[i, :ls] - ref) - mix_bar(b["speech"][i], ref)
            print("case %d (ls %d, ln %d, %d dB): worst |mix - ref| / bar = %.3f"
                  % (i, ls, ln, snr, (np.abs(mix[i, :ls] - ref) / np.maximum(mix_bar(b["speech"][i], ref), 1e-300)).max()))
            assert excess.max() <= 0
            np.random.seed(int(gold["seed_%d" % i]))
            alone = AudioParser(snr=snr).add_noise(b["speech"][i], b["noise"][i])
            assert np.random.random() == float(gold["next_%d" % i])
            assert alone.dtype == np.float32 and np.array_equal(alone, mix[i, :ls])


def test_mix_where_the_reference_cannot_run():
    """ls = 65536 over ln = 300: the reference's buffer would double 218 times.  Eight of the 218 draws are used."""
    from fullycnnspeechenhancement_amd.audio import mix_snr_batch
    from fullycnnspeechenhancement_amd.loader import plan_noise
    rng = np.random.default_rng(77)
    ls, ln = 65536, 300
    speech, noise = (0.2 * rng.standard_normal(ls)).astype(np.float32), (0.05 * rng.standard_normal(ln)).astype(np.float32)
    np.random.seed(9)
    start, gains = plan_noise(ls, ln)
    np.random.seed(9)
    all_draws = [np.random.uniform(0, 2) for _ in range(218)]
    assert start == 0 and len(gains) == 8 and np.array_equal(gains, all_draws[:8])
    for snr in (0, 10, -5):
        ref = cf.mix(speech, noise, snr, 0, gains)
        mix = mix_snr_batch(dev(speech)[None], dev(noise)[None], snr, gains=[gains]).cpu().numpy()[0]
        worst = (np.abs(mix - ref) / np.maximum(mix_bar(speech, ref), 1e-300)).max()
        # the normalisation by p_back: the measured SNR of the result is the configured one within the fp32 store's rounding
        m64, s64 = mix.astype(np.float64), speech.astype(np.float64)
        measured = 10 * np.log10(np.sum(s64 ** 2) / np.sum((m64 - s64) ** 2))
        snr_bar = 2 * DB * 2.0 ** -23 * np.linalg.norm(m64) / np.linalg.norm(m64 - s64)
        print("snr %3d: worst |mix - ref| / bar = %.3f; measured SNR %.9f dB (off %.2e, bar %.2e)"
              % (snr, worst, measured, abs(measured - snr), snr_bar))
        assert worst <= 1
        assert abs(measured - snr) <= snr_bar
    with pytest.raises(Exception) as ei:                                 # too few gains: refused on the host side
        mix_snr_batch(dev(speech)[None], dev(noise)[None], 0, gains=[gains[:7]])
    assert getattr(ei.value, "code", None) == 1                          # RCED_ERR_ARG


def test_tiny_noise_multiplies_gains_out_from_the_bits():
    """ln so small that a slice spans more tiles than the LDS table holds (the other branch of the gain lookup)."""
    from fullycnnspeechenhancement_amd.audio import gains_needed, mix_snr_batch
    rng = np.random.default_rng(5)
    for ls, ln in ((5000, 3), (4099, 1), (6000, 13)):
        speech, noise = (0.2 * rng.standard_normal(ls)).astype(np.float32), (0.05 + 0.05 * rng.random(ln)).astype(np.float32)
        gains = 0.9 + 0.2 * rng.random(gains_needed(ls, ln))             # near 1: the products stay in range
        ref = cf.mix(speech, noise, 3, 0, gains)
        mix = mix_snr_batch(dev(speech)[None], dev(noise)[None], 3, gains=[gains]).cpu().numpy()[0]
        assert (np.abs(mix - ref) <= mix_bar(speech, ref)).all(), (ls, ln)


# ---- invariance ---------------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_the_batch_around_them(gold):
    """Utterance i's mix and SDR, bit for bit: alone, at row 0 and at row 200 of a 256-row batch, with other row widths
    (so other alignments: dword instead of dwordx4 loads), and twice in a row."""
    import torch
    from fullycnnspeechenhancement_amd.audio import mix_snr_batch, sdr_batch
    b = fixture_batch(gold)
    rng = np.random.default_rng(3)
    n = len(b["sl"])
    for i in (0, 2, 3, 4):                                                       # tile, crop, 7 doublings, short
        ls = b["sl"][i]
        alone = mix_snr_batch(dev(b["speech"][i])[None], dev(b["noise"][i])[None], 5, starts=[b["starts"][i]], gains=[b["gains"][i]])
        again = mix_snr_batch(dev(b["speech"][i])[None], dev(b["noise"][i])[None], 5, starts=[b["starts"][i]], gains=[b["gains"][i]])
        assert torch.equal(alone, again)
        est_alone = dev(cf.rebuilt(gold, i, 512, 1.0))[None]
        s_alone = sdr_batch(dev(b["speech"][i])[None], est_alone)
        assert torch.equal(s_alone, sdr_batch(dev(b["speech"][i])[None], est_alone))
        for Ls, Ln, Le in ((8192 + 64, 5000 + 4, 8192 + 128), (8192 + 1, 5000 + 3, 8192 + 2)):
            rows = [int(rng.integers(n)) for _ in range(256)]
            rows[0] = rows[200] = i
            speech = dev(padded([b["speech"][r] for r in rows], Ls))
            noise = dev(padded([b["noise"][r] for r in rows], Ln))
            mix = mix_snr_batch(speech, noise, 5, [b["sl"][r] for r in rows], [b["nl"][r] for r in rows],
                                [b["starts"][r] for r in rows], [b["gains"][r] for r in rows])
            assert torch.equal(mix[0, :ls], alone[0]) and torch.equal(mix[200, :ls], alone[0]), (i, Ls)
            est = dev(padded([cf.rebuilt(gold, r, 512, 1.0) for r in rows], Le))
            s = sdr_batch(speech, est, [b["sl"][r] for r in rows])
            assert s[0] == s_alone[0] and s[200] == s_alone[0], (i, Ls)


# ---- the chain ----------------------------------------------------------------------------------------------------

def test_chain_pinned_to_the_reference(gold, K):
    """evaluate_pcm with the stand-in model pred = gain * mag against the reference's STFT -> gain -> rebuild -> SDR.
    Audio: the bound the suite already holds the STFT -> ISTFT chain to (tests/test_audio_gpu.py:106,109): eps = 5e-5 of
    the scale for nfft = 512, 2e-4 for 256.  SDR: the first-order propagation of that eps through the score,
    2 * (20 / ln 10) * eps * max|rebuilt| * sqrt(L) / ||rebuilt - clean||  dB (factor 2 for the second-order term)."""
    from fullycnnspeechenhancement_amd import FullyCNNTester
    from oracle import rced_np
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=rced_np.make_weights("FullyCNNV3", seed=42))   # not run: model= replaces it
    n = len(gold["cases"])
    mixes = [gold["mix_%d" % i].astype(np.float32) for i in range(n)]
    cleans = [gold["speech_%d" % i] for i in range(n)]
    for nfft, eps in ((512, 5e-5), (256, 2e-4)):
        for gain in cf.GAINS:
            den, sdr = eng.evaluate_pcm(mixes, cleans, nfft, model=lambda m: gain * m, kernels=K)
            assert sdr.dtype == np.float64 and len(den) == n
            for i in range(n):
                ref = cf.rebuilt(gold, i, nfft, gain).astype(np.float64)
                stored = float(gold["sdr_%d_%d_%d" % (i, nfft, int(gain * 10))])
                L = len(ref)
                err = np.abs(den[i] - ref).max() / np.abs(ref).max()
                sdr_bar = 2 * 2 * DB * eps * np.abs(ref).max() * np.sqrt(L) / np.linalg.norm(ref - cleans[i])
                print("%s nfft %d gain %.1f case %d (L %d): audio %.2e of the scale (bar %.0e); sdr %+.6f vs %+.6f: off %.2e dB (bar %.2e)"
                      % (K, nfft, gain, i, L, err, eps, sdr[i], stored, abs(sdr[i] - stored), sdr_bar))
                assert den[i].dtype == np.float32 and den[i].shape == (L,)
                assert err <= eps
                assert abs(sdr[i] - stored) <= sdr_bar


def ragged_batches(seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for lens in ((3000, 1800, 4096), (2500, 5000)):
        clean = [(0.2 * rng.standard_normal(L)).astype(np.float32) for L in lens]
        mix = [c + (0.1 * rng.standard_normal(len(c))).astype(np.float32) for c in clean]
        out.append((None, None, mix, clean))                  # the reference's 4-tuple; the spectrograms are not read
    return out


def test_chain_with_the_real_net(built, capsys):
    import torch
    from fullycnnspeechenhancement_amd import FullyCNNTester
    from fullycnnspeechenhancement_amd.audio import istft_batch, stft_batch
    from oracle import rced_np
    eng = FullyCNNTester(net_work="FullyCNNV3", weights=rced_np.make_weights("FullyCNNV3", seed=42))
    batches = ragged_batches()
    scores = []
    for _, _, mix, clean in batches:
        den, sdr = eng.evaluate_pcm(mix, clean)
        lens = [len(c) for c in clean]
        mag, ph = stft_batch(dev(padded(mix, max(lens), fill=0.0)), lens)          # the same chain composed by hand
        by_hand = istft_batch(eng.model(mag), ph, 512).cpu().numpy()
        for i, L in enumerate(lens):
            assert np.array_equal(den[i], by_hand[i, :L])
            assert abs(sdr[i] - cf.sdr(clean[i], den[i])) <= 1e-9
        # a padded device tensor with lengths is the same call
        den2, sdr2 = eng.evaluate_pcm(dev(padded(mix, max(lens), fill=0.0)), dev(padded(clean, max(lens), fill=0.0)), lengths=lens)
        assert all(np.array_equal(a, b) for a, b in zip(den, den2)) and np.array_equal(sdr, sdr2)
        scores.extend(sdr.tolist())
    avg = eng.test(batches)
    assert eng.sdr_score.count == len(scores) == 5
    assert abs(avg - np.mean(scores)) <= 1e-12 and avg == eng.sdr_score.avg
    assert "Average sd_score: %.4f." % avg in capsys.readouterr().out
    assert torch.cuda.is_available()


def test_trainer_valid_scores_with_batch_statistics(built, capsys):
    """FullyCNNTrainer.valid: the same core over valid_step (BatchNorm with the batch's own statistics)."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    from fullycnnspeechenhancement_amd.audio import istft_batch, stft_batch
    from oracle import rced_np
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=3, weights=rced_np.make_weights("FullyCNNV3", seed=42))
    batches = ragged_batches()
    scores = []
    for _, _, mix, clean in batches:
        lens = [len(c) for c in clean]
        mag, ph = stft_batch(dev(padded(mix, max(lens), fill=0.0)), lens)
        audio = istft_batch(tr.valid_step(mag), ph, 512).cpu().numpy()
        scores.extend(cf.sdr(clean[i], audio[i, :L]) for i, L in enumerate(lens))

    class Log(object):
        lines = []

        def info(self, msg):
            self.lines.append(msg)

    avg = tr.valid(batches, 4, Log())
    assert tr.sdr_score.count == 5 and abs(avg - np.mean(scores)) <= 1e-9
    line = "Epoch: 4, Average sd_score: %.4f." % avg
    assert line in capsys.readouterr().out and line in Log.lines[0]
    tr.close()


def test_entries_replay_from_a_captured_graph(gold):
    """After one call of a shape the two entries allocate nothing (the slice workspace is kept per device and stream), so
    they can be captured: a replayed graph gives the bits of the eager calls, also after the inputs changed in place."""
    import torch
    from fullycnnspeechenhancement_amd.audio import mix_snr_batch, sdr_batch
    rng = np.random.default_rng(8)
    speech = dev((0.2 * rng.standard_normal((3, 5000))).astype(np.float32))
    noise = dev((0.1 * rng.standard_normal((3, 1200))).astype(np.float32))
    gains = dev(2 * rng.random((3, 3)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on the capture stream: sizes its workspace
        mix_snr_batch(speech, noise, 5, gains=gains)
        sdr_batch(speech, speech)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mix = mix_snr_batch(speech, noise, 5, gains=gains)
        sdr = sdr_batch(speech, mix)
    for scale in (1.0, 0.5):
        speech.mul_(scale)
        graph.replay()
        torch.cuda.synchronize()
        eager = mix_snr_batch(speech, noise, 5, gains=gains)
        assert torch.equal(mix, eager) and torch.equal(sdr, sdr_batch(speech, eager))
        assert abs(float(sdr[0]) - 5.0) < 1e-5         # the mix is at 5 dB, so is its SDR against the speech
