"""GPU parity of the STFT / ISTFT kernels where test_audio_gpu.py does not reach: every regime of the frame-range split
(audio_api.hip: range_split), the block seams of the persistent kernels, odd and very short lengths, and spectra that are not the
STFT of a real signal (nonzero imaginary parts at bins 0 and 128).  The reference is always oracle/audio_np.py in float64 -- pinned
to the reference's own code at these edges by tests/test_audio_oracle.py -- never one kernel family against the other, except where
a test says so.  Each test prints the worst error it measured before it asserts (pytest -s shows them)."""

import functools

import numpy as np
import pytest

from oracle import audio_np

pytestmark = pytest.mark.gpu

BLOCK = 64            # kFramesPerWg: frames per block of the kernels
MAG_BOUND = 2e-6      # of max(ref): test_audio_gpu.py's figure against real reference outputs
PHASE_BOUND = 2e-3    # where ref_mag > 1e-3 * scale
ISTFT_BOUND = 5e-5    # of max|ref|: test_stft_then_matching_inverse_round_trip's figure against the same restatement
PATHS_BOUND = 2e-6    # fused against split: test_rebuild_fused_and_split_paths_agree's figure


@pytest.fixture(params=["x6", "f32"], ids=["x6", "fp32-mfma"])
def K(request, built):
    """Both kernel families, as in test_audio_gpu.py."""
    return request.param


# ---- 0. the case table ----------------------------------------------------------------------------------------------------------

def range_split(N, T):
    """Mirrors range_split() of csrc/audio_api.hip and the kernels' `per`: (blocks, workgroups per utterance, blocks per workgroup)."""
    nblk = -(-T // BLOCK)
    s = 1
    while s < nblk and N * s < 256:
        s *= 2
    split = min(s, nblk)
    return nblk, split, -(-nblk // split)


# (N, T): (nblk, split, per), regime
CASES = {
    (2, 1): ((1, 1, 1), "single block"),
    (1, 2): ((1, 1, 1), "single block"),
    (3, 63): ((1, 1, 1), "single block"),
    (2, 64): ((1, 1, 1), "single block"),
    (3, 65): ((2, 2, 1), "split, per 1"),            # the second range has one live frame
    (255, 65): ((2, 2, 1), "split, per 1"),          # just under the 256 threshold
    (256, 65): ((2, 1, 2), "one workgroup walks"),   # STFT prefetch loop, fused ISTFT carry across the seam
    (257, 128): ((2, 1, 2), "one workgroup walks"),
    (256, 129): ((3, 1, 3), "one workgroup walks"),  # the last block has one live frame
    (100, 257): ((5, 4, 2), "split, per 2"),         # fourth range empty: blk0 = 6 >= blk1 = 5
    (64, 321): ((6, 4, 2), "split, per 2"),          # fourth range empty: 6 >= 6
}
CASE_IDS = ["%dx%d" % c for c in CASES]


def test_case_table_lands_in_the_regimes_named():
    """If the heuristic moves, pick new shapes: the tests below must not silently lose a regime."""
    for (N, T), (want, _) in CASES.items():
        assert range_split(N, T) == want, ((N, T), range_split(N, T), want)
    for N, T in ((100, 257), (64, 321)):
        nblk, split, per = range_split(N, T)
        assert 1 < split < nblk and (split - 1) * per >= nblk        # the trailing workgroup's range is empty
    assert range_split(3, 156) == (3, 3, 1) and range_split(300, 156)[1] == 1   # the two points test_audio_gpu.py visits


def row_width(T):
    return 256 + 128 * (T - 1)                       # exactly T frames


def special_lengths(T):
    L = row_width(T)
    sp = [L, L - 77, 1, 2, 131, 255, 257]            # L - 77: odd, num_frames = T (inside the last block)
    if T > BLOCK:
        sp += [8319, 8320, 8321]                     # 64 / 64 / 65 frames: either side of a block
    return sp


TINY_LENGTHS = {(2, 1): [256, 1], (1, 2): [2], (3, 63): [row_width(63), 131, 255], (2, 64): [257, row_width(64) - 77],
                (3, 65): [8321, 8319, row_width(65)]}


def stft_batch_inputs(N, T):
    """Distinct seeded rows of 0.2 * randn [N, L] on the device, ragged lengths holding the special ones, junk past each length.
    Returns (pcm, lens, rows to check: first, last, every special length, two seeded picks)."""
    import torch
    L = row_width(T)
    rng = np.random.default_rng(1000 * N + T)
    if (N, T) in TINY_LENGTHS:
        lens, rows = list(TINY_LENGTHS[(N, T)]), list(range(N))
    else:
        sp = special_lengths(T)
        assert N >= len(sp) + 2 and max(sp) == L and audio_np.num_frames(L - 77) == T and (L - 77) % 2 == 1
        lens = [int(v) for v in rng.integers(1, L + 1, N)]
        at = [0, N - 1] + [int(v) for v in 1 + rng.choice(N - 2, len(sp) - 2, replace=False)]
        for r, v in zip(at, sp):                     # the first row is full, the last ends at an odd length inside the last block
            lens[r] = v
        rows = sorted(set(at + [int(v) for v in rng.integers(0, N, 2)]))
    assert len(lens) == N and all(1 <= v <= L for v in lens)
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 * N + T)
    pcm = 0.2 * torch.randn((N, L), generator=g, device="cuda")
    past = torch.arange(L, device="cuda")[None, :] >= torch.tensor(lens, device="cuda")[:, None]
    pcm.masked_fill_(past, 7.0)                      # junk past the utterance must not leak in
    return pcm, lens, rows


def check_stft_rows(pcm, lens, rows, mag, ph, T):
    """Rows `rows` of a stft_batch result against the float64 restatement; returns the worst (magnitude, phase) errors."""
    import torch
    assert tuple(mag.shape) == (pcm.shape[0], T, 129, 1) and tuple(ph.shape) == (pcm.shape[0], T, 129)
    idx = torch.tensor(rows, device="cuda")
    sig, m, p = pcm[idx].cpu().numpy(), mag[idx].cpu().numpy()[..., 0], ph[idx].cpu().numpy()
    worst_m = worst_p = 0.0
    for j, r in enumerate(rows):
        ref_m, ref_p = audio_np.stft(sig[j, :lens[r]])
        t = min(ref_m.shape[0], T)
        ref_m, ref_p = ref_m[:t], ref_p[:t]
        scale = ref_m.max()
        em = np.abs(m[j, :t] - ref_m).max() / scale
        strong = ref_m > 1e-3 * scale
        ep = np.abs(p[j, :t] - ref_p)[strong].max()
        worst_m, worst_p = max(worst_m, em), max(worst_p, ep)
        assert em <= MAG_BOUND, "row %d (length %d): magnitude off by %.3e of the scale" % (r, lens[r], em)
        assert ep <= PHASE_BOUND, "row %d (length %d): phase off by %.3e" % (r, lens[r], ep)
        assert not m[j, t:].any(), "row %d (length %d): a frame past the utterance is not zero" % (r, lens[r])
        assert np.all(p[j, t:] == 1.0 + 0.0j), "row %d (length %d): phase of a dead frame is not 1 + 0j" % (r, lens[r])
    return worst_m, worst_p


# ---- 1. STFT over the table -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(CASES), ids=CASE_IDS)
def test_stft_over_the_split_regimes(case, K):
    """Ragged batches in every regime of the split: odd lengths (the half-filled sample pair), lengths 1 and 2, lengths on either
    side of a block, rows whose later blocks are wholly dead."""
    from fullycnnspeechenhancement_amd.audio import stft_batch
    N, T = case
    pcm, lens, rows = stft_batch_inputs(N, T)
    mag, ph = stft_batch(pcm, lens, frames=T, kernels=K)
    em, ep = check_stft_rows(pcm, lens, rows, mag, ph, T)
    print("[edges] stft %s %dx%d (%s, %d rows): magnitude %.2e (bound %.0e), phase %.2e (bound %.0e)"
          % (K, N, T, CASES[case][1], len(rows), em, MAG_BOUND, ep, PHASE_BOUND))


@pytest.mark.parametrize("frames", [65, 130], ids=["fewer", "more"])
def test_stft_frames_argument_truncates_and_pads(frames, K):
    """frames= below the batch's own maximum (70: the kernel drops frames at or past T inside a block) and above it (a third,
    wholly dead block)."""
    import torch
    from fullycnnspeechenhancement_amd.audio import stft_batch
    L = row_width(70)
    lens = [L, 8321, 131]
    g = torch.Generator(device="cuda")
    g.manual_seed(70)
    pcm = 0.2 * torch.randn((3, L), generator=g, device="cuda")
    pcm[1, 8321:] = 7.0
    pcm[2, 131:] = 7.0
    mag, ph = stft_batch(pcm, lens, frames=frames, kernels=K)
    em, ep = check_stft_rows(pcm, lens, [0, 1, 2], mag, ph, frames)
    print("[edges] stft %s frames=%d of 70: magnitude %.2e, phase %.2e" % (K, frames, em, ep))


# ---- 2. STFT: a row does not depend on the batch around it ----------------------------------------------------------------------

@pytest.mark.parametrize("case", [(256, 129), (100, 257)], ids=["256x129", "100x257"])
def test_stft_row_is_bit_equal_alone_and_in_a_batch(case, K):
    """A frame's arithmetic is the same wherever it runs (one rounded multiply and subtract for the pre-emphasis, a deterministic
    split into parts, the same N-tile slot), so a row transformed alone (N = 1: one block per workgroup, nothing prefetched) equals
    the same row inside a batch whose workgroups walk several blocks with the next block's samples fetched ahead: bit for bit."""
    import torch
    from fullycnnspeechenhancement_amd.audio import stft_batch
    N, T = case
    assert range_split(N, T)[2] >= 2 and range_split(1, T)[2] == 1
    pcm, lens, rows = stft_batch_inputs(N, T)
    mag, ph = stft_batch(pcm, lens, frames=T, kernels=K)
    for r in rows:
        m1, p1 = stft_batch(pcm[r:r + 1], [lens[r]], frames=T, kernels=K)
        assert torch.equal(m1[0], mag[r]), "row %d (length %d): magnitude differs from the row alone" % (r, lens[r])
        assert torch.equal(torch.view_as_real(p1[0]), torch.view_as_real(ph[r])), "row %d (length %d): phase differs" % (r, lens[r])


# ---- 3. ISTFT of arbitrary spectra over the table -------------------------------------------------------------------------------

def arbitrary_spectra(N, T, seed):
    """|randn| magnitudes and a uniform unit phase at EVERY bin, bins 0 and 128 included: float32 / complex64 on the device."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mag = torch.randn((N, T, 129), generator=g, device="cuda").abs()
    ang = (torch.rand((N, T, 129), generator=g, device="cuda") * 2 - 1) * np.pi
    return mag, torch.polar(torch.ones_like(ang), ang)


def sample_rows(N, seed, count=8):
    """First, last and seeded picks: the restatement has a Python loop per sample."""
    if N <= count:
        return list(range(N))
    rng = np.random.default_rng(seed)
    return sorted([0, N - 1] + [int(v) for v in 1 + rng.choice(N - 2, count - 2, replace=False)])


def check_istft_rows(mag, ph, out, rows, nfft):
    """Whole output rows -- head, every seam, the last frame -- against the restatement run on the same rounded inputs."""
    import torch
    idx = torch.tensor(rows, device="cuda")
    m, p, o = mag[idx].cpu().numpy(), ph[idx].cpu().numpy(), out[idx].cpu().numpy()
    worst = 0.0
    for j, r in enumerate(rows):
        ref = audio_np.rebuild(m[j], p[j], nfft=nfft)
        assert o[j].shape == ref.shape == ((mag.shape[1] + 1) * 128,)
        err = np.abs(o[j] - ref).max() / np.abs(ref).max()
        worst = max(worst, err)
        assert err <= ISTFT_BOUND, "row %d: off by %.3e of the maximum at sample %d" % (r, err, int(np.abs(o[j] - ref).argmax()))
    return worst


@pytest.mark.parametrize("nfft", [512, 256])
@pytest.mark.parametrize("case", list(CASES), ids=CASE_IDS)
def test_istft_of_arbitrary_spectra_over_the_split_regimes(case, nfft, K):
    """The STFT of a real signal has im(bin 0) = im(bin 128) = 0, so it never multiplies the rank-1 term of im(bin 128) at
    nfft = 512, slots 256 / 257 of the head table, or the rule that bin 0 (and bin 128 at nfft = 256) lose their imaginary part,
    by anything but zero.  Arbitrary spectra do."""
    from fullycnnspeechenhancement_amd.audio import istft_batch
    N, T = case
    mag, ph = arbitrary_spectra(N, T, 7000 * N + T)
    out = istft_batch(mag, ph, nfft=nfft, kernels=K)
    assert tuple(out.shape) == (N, (T + 1) * 128)
    rows = sample_rows(N, 31 * N + T)
    assert len(rows) >= min(N, 8) and rows[0] == 0 and rows[-1] == N - 1
    err = check_istft_rows(mag, ph, out, rows, nfft)
    print("[edges] istft %s nfft=%d %dx%d (%s%s, %d rows): %.2e of max|ref| (bound %.0e)"
          % (K, nfft, N, T, CASES[case][1], ", fused" if range_split(N, T)[1] == 1 else "", len(rows), err, ISTFT_BOUND))


# ---- 4. known answers, one spectrum term at a time ------------------------------------------------------------------------------

TERM_FRAMES = (0, 63, 64)                  # the head path; either side of the seam; 64 is also T - 1
TERM_BINS = (0, 1, 127, 128)
TERMS = [(f, b, c) for f in TERM_FRAMES for b in TERM_BINS for c in (0, 1)]     # c: 0 re, 1 im


@functools.lru_cache(maxsize=None)
def term_response(f, b, c, nfft, T=65):
    mag = np.zeros((T, 129))
    ph = np.ones((T, 129), np.complex128)
    mag[f, b] = 1.5
    ph[f, b] = 1j if c else 1.0
    return audio_np.rebuild(mag, ph, nfft=nfft)


@pytest.mark.parametrize("nfft", [512, 256])
@pytest.mark.parametrize("N", [2, 256], ids=["split", "fused"])
def test_istft_single_term_responses(N, nfft, K):
    """The spectrum is zero but for one entry per row: re or im of bin 0, 1, 127 or 128, at frame 0, 63 or 64 of T = 65.  The response
    is one windowed sinusoid through the de-emphasis, so a wrong slot or row mapping is an O(1) error.  The coefficients of
    im(bin 0), and of im(bin 128) at nfft = 256, are exact zeros (istft_coef / pack_istft): those rows come out EXACTLY zero.
    im(bin 128) at nfft = 512 is an ordinary term: nonzero."""
    import torch
    from fullycnnspeechenhancement_amd.audio import istft_batch
    T = 65
    assert range_split(N, T)[1] == (1 if N == 256 else 2)
    rng = np.random.default_rng(N)
    if N >= len(TERMS) + 2:                # one call: a term per row, first and last row included, all-zero rows between
        at = [0, N - 1] + [int(v) for v in 1 + rng.choice(N - 2, len(TERMS) - 2, replace=False)]
        calls = [dict(zip(at, TERMS))]
    else:
        calls = [dict(enumerate(TERMS[i:i + N])) for i in range(0, len(TERMS), N)]
    worst = 0.0
    for call in calls:
        mag = torch.zeros((N, T, 129), device="cuda")
        ph = torch.ones((N, T, 129), dtype=torch.complex64, device="cuda")
        for r, (f, b, c) in call.items():
            mag[r, f, b] = 1.5
            ph[r, f, b] = 1j if c else 1.0
        out = istft_batch(mag, ph, nfft=nfft, kernels=K).cpu().numpy()
        for r in range(N):
            if r not in call:
                assert not out[r].any(), "row %d: a zero spectrum gives a nonzero signal" % r
                continue
            f, b, c = call[r]
            what = "%s of bin %d at frame %d (row %d)" % ("im" if c else "re", b, f, r)
            ref = term_response(f, b, c, nfft)
            if c and (b == 0 or (b == 128 and nfft == 256)):
                assert not ref.any()
                assert not out[r].any(), "%s must have no effect at all: max %.3e" % (what, np.abs(out[r]).max())
                continue
            assert np.abs(ref).max() > 1e-3, what
            err = np.abs(out[r] - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert err <= ISTFT_BOUND, "%s: off by %.3e of the maximum at sample %d" % (what, err, int(np.abs(out[r] - ref).argmax()))
            assert out[r].any()
    print("[edges] istft %s nfft=%d single terms, N=%d: %.2e of max|ref| (bound %.0e)" % (K, nfft, N, worst, ISTFT_BOUND))


# ---- 5. fused against split, widened --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nfft", [512, 256])
@pytest.mark.parametrize("T", [65, 129])
def test_rebuild_fused_and_split_paths_agree_on_arbitrary_spectra(T, nfft, K):
    """test_rebuild_fused_and_split_paths_agree at T = 65 and 129 (a seam with one live frame behind it), both nfft, on arbitrary
    spectra: 3 utterances are cut into frame ranges, 300 copies of them are walked by one workgroup each.  Here the two paths ARE
    compared with each other (to fp32 scan noise), and both with the restatement; copies inside the big batch are bit-equal."""
    import torch
    from fullycnnspeechenhancement_amd.audio import istft_batch
    assert range_split(3, T)[1] > 1 and range_split(300, T)[1] == 1
    mag, ph = arbitrary_spectra(3, T, 50 + T)
    small = istft_batch(mag, ph, nfft=nfft, kernels=K)
    big = istft_batch(mag.repeat(100, 1, 1), ph.repeat(100, 1, 1), nfft=nfft, kernels=K)
    assert torch.equal(big[:3], big[297:]) and torch.equal(big[:3], big[150:153])
    scale = float(small.abs().max())
    diff = float((big[:3] - small).abs().max()) / scale
    e_small = check_istft_rows(mag, ph, small, [0, 1, 2], nfft)
    e_big = check_istft_rows(mag, ph, big, [0, 1, 2], nfft)
    print("[edges] istft %s nfft=%d T=%d: fused - split %.2e of the scale (bound %.0e); split %.2e, fused %.2e of max|ref| (bound %.0e)"
          % (K, nfft, T, diff, PATHS_BOUND, e_small, e_big, ISTFT_BOUND))
    assert diff <= PATHS_BOUND


# ---- 6. the chain at odd and short lengths --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain(built):
    from fullycnnspeechenhancement_amd import InferenceEngine
    from oracle import rced_np
    w = rced_np.make_weights("FullyCNNV3", seed=42)
    return w, InferenceEngine(net_work="FullyCNNV3", weights=w)


@pytest.mark.parametrize("length", [1, 255, 257, 1235, 8321])
def test_pipeline_denoise_pcm_at_odd_and_short_lengths(length, chain):
    """test_pipeline_denoise_pcm_matches_oracle_chain (one length, 4000) at odd lengths: one sample, either side of one frame, an
    odd length of a few frames, and the first length with a second block."""
    from oracle import rced_c
    w, eng = chain
    sig = (0.2 * np.random.default_rng(length).standard_normal(length)).astype(np.float32)
    out = eng.denoise_pcm(sig)
    mag, phase = audio_np.stft(sig)
    pred = rced_c.forward("FullyCNNV3", w, mag.astype(np.float32)[None, :, :, None], np.float64)[0, :, :, 0]
    ref = audio_np.rebuild(pred, phase, len(sig))
    assert out.shape == sig.shape
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print("[edges] denoise_pcm length %d: %.2e of max|ref| (bound 1e-4)" % (length, err))
    assert err <= 1e-4


# ---- 7. refusals launch nothing -------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(K):
    """Every argument the host code rejects (audio_api.hip: each case below returns before the launch) leaves the outputs untouched;
    N = 0 or T = 0 succeeds and touches nothing either."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    from fullycnnspeechenhancement_amd.audio import KERNELS, stft_batch
    lib, k = _lib.load(), KERNELS[K]
    ARG = _lib.RCED_ERR_ARG
    N, L, T = 2, 2048, 15
    pcm = torch.randn(N, L, device="cuda")
    lens = torch.tensor([L, 100], dtype=torch.int32, device="cuda")
    mag = torch.full((N, T, 129), -7.0, device="cuda")
    ph = torch.full((N, T, 129, 2), -7.0, device="cuda")
    audio = torch.full((N, (T + 1) * 128), -7.0, device="cuda")
    smag = torch.rand(N, T, 129, device="cuda")
    sph = torch.randn(N, T, 129, 2, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P, Ln, M, Ph, A, SM, SP = (t.data_ptr() for t in (pcm, lens, mag, ph, audio, smag, sph))

    def stft(p=P, ln=Ln, n=N, l=L, t=T, m=M, q=Ph, kernels=k):
        return lib.rced_stft_ex(p, ln, n, l, t, m, q, 0, st, kernels)

    def istft(m=SM, q=SP, n=N, t=T, nfft=512, a=A, kernels=k):
        return lib.rced_istft_ex(m, q, n, t, nfft, a, 0, st, kernels)

    for kw in (dict(n=-1), dict(l=-1), dict(t=-1), dict(l=0), dict(p=None), dict(m=None), dict(n=65536), dict(kernels=7)):
        assert stft(**kw) == ARG, kw
    for kw in (dict(nfft=300), dict(nfft=300, n=0), dict(n=-1), dict(t=-1), dict(m=None), dict(q=None), dict(a=None), dict(n=65536),
               dict(kernels=7)):
        assert istft(**kw) == ARG, kw
    for kw in (dict(n=0), dict(t=0), dict(n=0, l=0), dict(n=0, p=None, m=None)):
        assert stft(**kw) == 0, kw
    for kw in (dict(n=0), dict(t=0), dict(n=0, m=None, a=None)):
        assert istft(**kw) == 0, kw
    if K == "x6":                                             # the plain entries are the x6 family: same refusals
        assert lib.rced_stft(P, Ln, N, L, -1, M, Ph, 0, st) == ARG and lib.rced_stft(P, Ln, 0, L, T, M, Ph, 0, st) == 0
        assert lib.rced_istft(SM, SP, N, T, 300, A, 0, st) == ARG and lib.rced_istft(SM, SP, N, 0, 512, A, 0, st) == 0
    for bad in ([L, 0], [L + 1, 5]):
        with pytest.raises(ValueError):
            stft_batch(pcm, bad, kernels=K)
    torch.cuda.synchronize()
    for buf in (mag, ph, audio):
        assert bool((buf == -7.0).all())
    assert stft() == 0 and istft() == 0                       # the same buffers, valid arguments: now they are written
    torch.cuda.synchronize()
    for buf in (mag, ph, audio):
        assert not bool((buf == -7.0).any())
