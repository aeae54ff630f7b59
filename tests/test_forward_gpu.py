"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the C ABI,
against the fp64 oracle and the committed golden vectors.  Tolerance: BASELINE.json north_star,
"masks within 1e-4 rel fp32" -> max|y - ref| <= 1e-4 * max|ref|  (conftest.RTOL)."""

import ctypes
import os

import numpy as np
import pytest

from conftest import NETS, ROOT as ROOT_DIR, RTOL, check_parity, load_golden, rel_err
from oracle import layers as L, rced_c, rced_np

pytestmark = pytest.mark.gpu

PATHS = ["layerwise", "auto"]
# bf16 (opt-in, BASELINE config 2): bounds at about twice the measured error, relative to the largest output.  Against the emulation the
# LARGEST element error is one bf16 ulp of a mid-size activation that a differently ordered fp32 sum rounds the other way (measured
# 1.1e-3 .. 4.3e-3 over the nets and shapes below: single elements); the ROOT-MEAN-SQUARE error is what a systematic fault moves first
# (measured 1e-4 .. 2.3e-4; round 6's stale-accumulator hazard: 6e-2 largest, 1.1e-2 rms), so both are bounded.
BF16_VS_EMULATION, BF16_RMS_VS_EMULATION, BF16_VS_FP32 = 1e-2, 1e-3, 1.5e-2


def rms_err(y, ref):
    return float(np.sqrt(np.mean((np.asarray(y, np.float64) - np.asarray(ref, np.float64)) ** 2)) / np.abs(ref).max())


def make_model(variant, w, path="auto"):
    from fullycnnspeechenhancement_amd import model as M
    cls = {1: M.FullyCNNSEModel, 2: M.FullyCNNSEModelV2, 3: M.FullyCNNSEModelV3}[variant]
    m = cls(False, weights=w, device=0)
    m.set_path(path)
    return m


def test_extension_is_loaded_and_is_the_hip_one(built):
    import torch
    from fullycnnspeechenhancement_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    maps = open("/proc/self/maps").read()
    assert "librced_hip.so" in maps


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_golden_vectors(net_work, tag, variant, path, built):
    w, g = load_golden(tag)
    m = make_model(variant, w, path)
    for key in ("small", "long", "c1"):      # c1 = BASELINE configs[0]'s shape, [1,256,129,1] (SURVEY 8 c4 iii)
        y = m(g["x_" + key])
        assert y.shape == g["y_" + key].shape and y.dtype == np.float32
        check_parity(y, g["y_" + key])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("net_work,tag,variant", NETS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (1, 3), (1, 7), (3, 8), (2, 9), (5, 33), (1, 256), (7, 64)])
def test_parity_vs_oracle_shapes(net_work, tag, variant, path, shape, built):
    """Includes T < 8 (fewer frames than the first kernel is tall) and T not a multiple of any tile."""
    n, t = shape
    w = rced_np.make_weights(net_work, seed=100 + variant)
    x = rced_np.make_input(n, t, seed=n * 1000 + t)
    ref = rced_c.forward(net_work, w, x, np.float64)
    y = make_model(variant, w, path)(x)
    check_parity(y, ref)


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_parity_vs_oracle_random_shapes_weights_and_inputs(net_work, tag, variant, built):
    """Fuzz: 8 seeded draws per net of batch, frames (1..40: below / across / far past the tile sizes 3 and 4),
    weight seed, input scale and sparsity (zero frames, zero utterances), fused path vs the plain-C oracle in fp64."""
    rng = np.random.default_rng(9000 + variant)
    for _ in range(8):
        n, t = int(rng.integers(1, 5)), int(rng.integers(1, 41))
        w = rced_np.make_weights(net_work, seed=int(rng.integers(1, 1 << 30)))
        x = rced_np.make_input(n, t, seed=int(rng.integers(1, 1 << 30))) * np.float32(rng.choice([1e-3, 1.0, 30.0]))
        if rng.random() < 0.5:
            x[:, rng.integers(0, t)] = 0.0           # a silent frame
        if n > 1 and rng.random() < 0.3:
            x[rng.integers(0, n)] = 0.0              # a silent utterance (zero padding of the loader, data_loader.py:198-209)
        ref = rced_c.forward(net_work, w, x, np.float64)
        y = make_model(variant, w, "auto")(x)
        assert np.isfinite(y).all()
        check_parity(y, ref)


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_device_resident_path_equals_host_path(net_work, tag, variant, built):
    import torch
    w, g = load_golden(tag)
    m = make_model(variant, w)
    x = g["x_small"]
    y_host = m(x)
    xd = torch.from_numpy(x).cuda()
    yd = m(xd)
    assert yd.is_cuda and yd.shape == xd.shape
    assert np.array_equal(yd.cpu().numpy(), y_host)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y2 = m(xd)
    s.synchronize()
    assert np.array_equal(y2.cpu().numpy(), y_host)


@pytest.mark.parametrize("chunks", [0, 1, 3, 64])
def test_pipelined_host_path_equals_resident_path(chunks, built):
    """rced_forward_host splits batches >= 8 MB into utterance chunks and overlaps upload / compute / download;
    the result must not depend on the split (13 utterances: ragged chunks; 64 chunks > N clamps to N)."""
    import torch
    w, _ = load_golden("v3")
    m = make_model(3, w)
    x = np.abs(np.random.default_rng(7).standard_normal((13, 1300, 129, 1))).astype(np.float32)   # 8.7 MB
    ref = m(torch.from_numpy(x).cuda()).cpu().numpy()
    m.set_option("host_chunks", chunks)
    assert m.get_option("host_chunks") == chunks
    for _ in range(2):
        assert np.array_equal(m(x), ref)
    with pytest.raises(Exception):
        m.set_option("host_chunks", 65)


@pytest.mark.parametrize("net_work,tag,variant", [n for n in NETS if n[2] in (1, 2)])
def test_bf16_variant_matches_its_emulation(net_work, tag, variant, built, capsys):
    """BASELINE config 2 names bf16 for R-CED V2: kernels_frame16.h keeps the input, every activation and every kernel
    in bf16 (fp32 accumulation), all layers in one launch.  Checked against oracle.rced_np.forward_bf16, which rounds at the
    same places.  Bounds = 2x what is measured (printed), relative to the largest output: against the emulation -- fp32
    accumulation order differs, and a sum that lands on the other side of a bf16 rounding boundary moves that
    activation by one bf16 ulp (2^-8) -- largest element 1e-2 (measured 1.1e-3 / 4.3e-3), rms 1e-3 (measured 9.5e-5 / 2.3e-4);
    and 1.5e-2 against the fp32 oracle, which is what 16 layers of 8-bit mantissas cost (measured 6.5e-3 / 9.1e-3).  NOT
    within the 1e-4 bar of the fp32 path, which remains the default."""
    from fullycnnspeechenhancement_amd import build_model
    w, g = load_golden(tag)
    x = rced_np.make_input(3, 20, seed=5)            # 20 frames: full tiles + a ragged one (3 frames per tile)
    m = build_model(net_work, False, weights=w, dtype="bfloat16")
    assert m.get_option("bf16") == 1
    y = m(x)
    ref16 = rced_np.forward_bf16(net_work, w, x)
    ref32 = rced_np.forward(net_work, w, x)
    e16, r16, e32 = rel_err(y, ref16), rms_err(y, ref16), rel_err(y, ref32)
    with capsys.disabled():
        print("\n[bf16 %s] vs bf16 emulation %.2e (rms %.2e), vs fp32 oracle %.2e (of the largest output)" % (net_work, e16, r16, e32))
    assert e16 < BF16_VS_EMULATION and r16 < BF16_RMS_VS_EMULATION
    assert e32 < BF16_VS_FP32
    assert np.array_equal(m(x), y)                   # deterministic
    m.restore(w)                                     # restore() keeps the options set before it (bf16 stays on)
    assert m.get_option("bf16") == 1 and np.array_equal(m(x), y)
    m.set_option("bf16", 0)                          # and back: the fp32 kernel is untouched
    check_parity(m(x), ref32)


@pytest.mark.parametrize("net_work,tag,variant", [n for n in NETS if n[2] in (1, 2)])
def test_bf16_ragged_batches_and_tile_maps(net_work, tag, variant, built, capsys):
    """The bf16 kernel gives a wave a frame and a workgroup four consecutive frames of one utterance: utterances whose length is no
    multiple of four (the last tile's idle waves), shorter than the first kernel is tall, and workgroups that walk SEVERAL tiles
    (option fused_grid: the state a tile leaves in LDS -- the output layer's image lies over two activation planes' zero rows --
    and in the weight ring) against the emulation, and bit-identical whatever the grid."""
    from fullycnnspeechenhancement_amd import build_model
    w = rced_np.make_weights(net_work, seed=77 + variant)
    m = build_model(net_work, False, weights=w, dtype="bfloat16")
    worst = 0.0
    for n, t in ((1, 1), (1, 3), (2, 5), (3, 37), (1, 64), (2, 9)):
        x = rced_np.make_input(n, t, seed=31 * n + t)
        ref16 = rced_np.forward_bf16(net_work, w, x)
        m.set_option("fused_grid", 0)
        y = m(x)
        assert np.isfinite(y).all()
        e16, r16 = rel_err(y, ref16), rms_err(y, ref16)
        worst = max(worst, e16)
        assert e16 < BF16_VS_EMULATION and r16 < BF16_RMS_VS_EMULATION, (n, t, e16, r16)
        for grid in (1, 2, 5):
            m.set_option("fused_grid", grid)
            assert np.array_equal(m(x), y), (n, t, grid)
        # four or eight frames per workgroup (option bf16_frames; 0 = chosen per call): a frame's arithmetic does not depend on it
        for frames, grid in ((4, 0), (8, 0), (8, 1), (8, 3), (4, 3)):
            m.set_option("bf16_frames", frames)
            m.set_option("fused_grid", grid)
            assert np.array_equal(m(x), y), (n, t, frames, grid)
        m.set_option("bf16_frames", 0)
    with pytest.raises(Exception, match="bf16_frames takes"):
        m.set_option("bf16_frames", 2)
    with capsys.disabled():
        print("\n[bf16 %s ragged] worst vs bf16 emulation %.2e" % (net_work, worst))


def test_full_size_config2_bf16_sampled_against_its_emulation(built, capsys):
    """BASELINE configs[1] at its full size: R-CED V2 (model.py:32-61), batch 64, 129x512, bf16.  A frame's output
    depends on frames t-3..t+4 only, so sampled output frames are checked against the bf16 emulation (and the fp32
    oracle) run on each frame's 8-frame receptive field."""
    import torch
    from fullycnnspeechenhancement_amd import build_model
    w = rced_np.make_weights("FullyCNNV2", seed=42)
    m = build_model("FullyCNNV2", False, weights=w, dtype="bfloat16")
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn((64, 512, 129, 1), generator=g, device="cuda").abs_()
    y = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    scale = float(y.abs().max())
    rng = np.random.default_rng(2)
    picks = [(0, 0), (0, 2), (63, 511), (63, 509), (31, 255)] + \
            [(int(rng.integers(64)), int(rng.integers(512))) for _ in range(19)]
    w16 = w32 = 0.0
    for n, t in picks:
        lo, hi = max(t - 3, 0), min(t + 5, 512)
        win = x[n:n + 1, lo:hi].cpu().numpy()
        got = y[n, t].cpu().numpy()
        w16 = max(w16, np.abs(got - rced_np.forward_bf16("FullyCNNV2", w, win)[0, t - lo]).max() / scale)
        w32 = max(w32, np.abs(got - rced_c.forward("FullyCNNV2", w, win, np.float64)[0, t - lo]).max() / scale)
    with capsys.disabled():
        print("\n[config 2 full size] %d sampled frames: vs bf16 emulation %.2e, vs fp32 oracle %.2e" % (len(picks), w16, w32))
    assert w16 < BF16_VS_EMULATION and w32 < BF16_VS_FP32
    assert torch.equal(m(x[10:12].contiguous()), y[10:12])      # utterances are independent, launches deterministic
    m.set_option("bf16_frames", 4)                              # this size runs eight frames per workgroup by default
    assert torch.equal(m(x), y)
    m.set_option("bf16_frames", 0)


@pytest.mark.parametrize("net_work,dtype,batch", [("FullyCNN", "bfloat16", 64), ("FullyCNNV2", "bfloat16", 64),
                                                  ("FullyCNNV2", "float32", 128), ("FullyCNNV3", "float32", 128)])
def test_full_batch_and_random_slices_bit_for_bit(net_work, dtype, batch, built):
    """Race screen at full occupancy (the bf16 kernels run two workgroups per CU): rerunning the batch, and rerunning
    random slices of it (other tile -> workgroup maps, other neighbours in LDS), reproduces every mask bit for bit.
    (An experimental restructuring of the bf16 epilogue that was semantically the same code failed exactly this on V2.)"""
    import torch
    from fullycnnspeechenhancement_amd import build_model
    m = build_model(net_work, False, weights=rced_np.make_weights(net_work, seed=42), dtype=dtype)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((batch, 512, 129, 1), generator=g, device="cuda").abs_()
    y = m(x).clone()
    rng = np.random.default_rng(0)
    for _ in range(8):
        assert torch.equal(m(x), y)
        a = int(rng.integers(0, batch - 1))
        b = int(rng.integers(a + 1, min(batch, a + 9) + 1))
        assert torch.equal(m(x[a:b].contiguous()), y[a:b]), (a, b)


def test_bf16_is_refused_for_cr_ced(built):
    from fullycnnspeechenhancement_amd import build_model
    w, _ = load_golden("v3")
    with pytest.raises(Exception, match="bf16"):
        build_model("FullyCNNV3", False, weights=w, dtype="bfloat16")


def test_empty_and_degenerate_batches(built):
    w, _ = load_golden("v3")
    m = make_model(3, w)
    assert m(np.zeros((0, 5, 129, 1), np.float32)).shape == (0, 5, 129, 1)
    assert m(np.zeros((2, 0, 129, 1), np.float32)).shape == (2, 0, 129, 1)
    with pytest.raises(ValueError):
        m(np.zeros((2, 5, 128, 1), np.float32))
    y0 = m(np.zeros((1, 4, 129, 1), np.float32))       # all-zero input: output is the bias path only
    ref = rced_c.forward("FullyCNNV3", w, np.zeros((1, 4, 129, 1), np.float32))
    check_parity(y0, ref)


def test_ragged_batch_zero_padding_matches_reference_loader(built):
    """data_loader.py:198-209 zero-pads short utterances to the longest T; the net then runs on the
    padded tensor.  The frames of a short utterance at least 4 frames before its end are unaffected."""
    w, _ = load_golden("v2")
    m = make_model(2, w)
    lens = [40, 17, 29]
    xs = [rced_np.make_input(1, t, seed=50 + t)[0] for t in lens]
    batch = np.zeros((3, 40, 129, 1), np.float32)
    for i, x in enumerate(xs):
        batch[i, :lens[i]] = x
    y = m(batch)
    check_parity(y, rced_c.forward("FullyCNNV2", w, batch))
    for i, x in enumerate(xs):
        alone = m(x[None])
        keep = lens[i] - 4 if lens[i] < 40 else lens[i]
        assert np.abs(alone[0, :keep] - y[i, :keep]).max() <= 1e-5 * np.abs(alone).max()


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_batch_and_time_shard_invariance(net_work, tag, variant, built):
    """Size-independent properties: utterances are independent; frame t needs frames t-3..t+4 only."""
    w = rced_np.make_weights(net_work, seed=9)
    m = make_model(variant, w)
    x = rced_np.make_input(6, 48, seed=10)
    y = m(x)
    for i in (0, 3, 5):
        assert np.array_equal(m(x[i:i + 1])[0], y[i])
    a = m(x[:, :28])          # frames 0..27 -> valid 0..23
    b = m(x[:, 21:])          # frames 21..47 -> valid 24..47
    # a frame lands on a different pixel slot of its tile when the time origin moves, which changes
    # the fp32 summation order inside the MFMA passes: equal to rounding, not bit for bit
    scale = np.abs(y).max()
    assert np.abs(a[:, :24] - y[:, :24]).max() <= 1e-5 * scale
    assert np.abs(b[:, 3:] - y[:, 24:]).max() <= 1e-5 * scale


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_full_size_config3_sampled_against_oracle(net_work, tag, variant, built):
    """BASELINE config 3 (CR-CED, batch 256, 129x512) on the device path -- and the two R-CED nets at the same size
    (every persistent workgroup walks 128-171 tiles); a random sample of output frames is checked against the oracle
    run on each frame's 8-frame receptive field."""
    import torch
    w = rced_np.make_weights(net_work, seed=42)
    m = make_model(variant, w)
    import bench
    x = torch.from_numpy(bench.synthetic_magnitudes((256, 512, 129, 1), 1234)).cuda()   # bench.py's own input
    y = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    rng = np.random.default_rng(0)
    picks = [(0, 0), (0, 1), (255, 511), (255, 508), (17, 3), (200, 510)] + \
            [(int(rng.integers(256)), int(rng.integers(512))) for _ in range(26)]
    scale = float(y.abs().max())
    for n, t in picks:
        lo, hi = max(t - 3, 0), min(t + 5, 512)
        win = x[n:n + 1, lo:hi].cpu().numpy()
        ref = rced_c.forward(net_work, w, win, np.float64)[0, t - lo]
        got = y[n, t].cpu().numpy()
        assert np.abs(got - ref).max() <= RTOL * scale, (net_work, n, t)
    # utterances are independent: rerunning a slice of the batch reproduces it bit for bit
    assert torch.equal(m(x[100:104].contiguous()), y[100:104])
    # ... and so does rerunning all of it (race screen with every CU busy: hand-offs, LDS-DMA packets, skip scratch)
    for _ in range(3):
        assert torch.equal(m(x), y)


# the two forms of the CR-CED kernel in the product library (kernels_fused_v3.h): the product (every layer as three-part bf16 products) and
# the comparator (every layer on the fp32 MFMA, bit-for-bit an fp32 fmaf chain) agree to fp32 summation noise.  (Rounds 3 / 4's forms 1
# and 2 are history: RCED_V3_LEGACY_FORMS builds only.)
V3_FORMS_AGREE = 5e-6
V3_FORMS = (3, 0)
V3_FORM_NAMES = ("all x6", "fp32-MFMA")


def v3_forms(w):
    """Models running the product form and the fp32-MFMA comparator -- option v3_l2x6 = 3, 0."""
    ms = []
    for form in V3_FORMS:
        m = make_model(3, w)
        if form == 3:
            assert m.get_option("v3_l2x6") == 3   # the default
        else:
            m.set_option("v3_l2x6", form)
            assert m.get_option("v3_l2x6") == form
        ms.append(m)
    return ms


def v3_check_forms(ms, x, ref, what=""):
    """Every form against the oracle (RTOL) and against the fp32-MFMA form (V3_FORMS_AGREE); -> (errors vs the oracle, vs fp32)"""
    ys = [m(x) for m in ms]
    ys = [y.cpu().numpy() if hasattr(y, "cpu") else y for y in ys]
    eo = [check_parity(y, ref, what="%s %s form" % (what, n)) for y, n in zip(ys, V3_FORM_NAMES)]
    ef = [rel_err(y, ys[-1]) for y in ys[:-1]]
    return ys, eo, ef


def test_v3_kernel_forms_agree_with_the_oracle_and_each_other(built, capsys):
    """rced_set_option(m, "v3_l2x6", 3 | 0): same inputs through the product form and the comparator -- the golden vectors and a
    fuzz set (shapes across the tile size, input scales 1e-3 .. 30, silent frames) -- each held to the oracle (1e-4) and the
    product to the fp32-MFMA form (5e-6 of the scale: fp32 summation noise; measured errors printed)."""
    w, g = load_golden("v3")
    ms = v3_forms(w)
    worst = [0.0] * 3
    cases = [(w, g["x_small"], g["y_small"]), (w, g["x_long"], g["y_long"]), (w, g["x_c1"], g["y_c1"])]
    rng = np.random.default_rng(4242)
    for _ in range(8):
        n, t = int(rng.integers(1, 5)), int(rng.integers(1, 41))
        wf = rced_np.make_weights("FullyCNNV3", seed=int(rng.integers(1, 1 << 30)))
        x = rced_np.make_input(n, t, seed=int(rng.integers(1, 1 << 30))) * np.float32(rng.choice([1e-3, 1.0, 30.0]))
        if rng.random() < 0.5:
            x[:, rng.integers(0, t)] = 0.0
        cases.append((wf, x, rced_c.forward("FullyCNNV3", wf, x, np.float64)))
    for wf, x, ref in cases:
        if wf is not w:
            ms = v3_forms(wf)
        _, eo, ef = v3_check_forms(ms, x, ref)
        worst = [max(a, b) for a, b in zip(worst, eo + ef)]
        assert max(ef) <= V3_FORMS_AGREE, ef
    with capsys.disabled():
        print("\n[v3 forms] worst error of the scale vs the oracle: all x6 %.2e, fp32-MFMA %.2e; the product vs the fp32-MFMA form: %.2e" % tuple(worst))


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_whole_output_config3_against_the_fp64_restatement(net_work, tag, variant, built, capsys):
    """BASELINE config 3 (batch 256, 129x512), EVERY one of the 131,072 output frames (the reference boundary returns all of
    them: tester.py:85-90) against oracle/infer_ref.py run in float64 on the same GPU -- all three nets, and for CR-CED both
    forms of the kernel, which must also agree with each other."""
    import torch
    import bench
    from oracle import infer_ref
    w = rced_np.make_weights(net_work, seed=42)
    x = torch.from_numpy(bench.synthetic_magnitudes((256, 512, 129, 1), 1234)).cuda()
    ref = infer_ref.forward(net_work, w, x, device="cuda", dtype=torch.float64).cpu().numpy()
    torch.cuda.empty_cache()
    if variant == 3:
        _, eo, ef = v3_check_forms(v3_forms(w), x, ref)
        assert max(ef) <= V3_FORMS_AGREE, ef
        msg = "all x6 %.2e, fp32-MFMA %.2e; the product vs the fp32-MFMA form %.2e" % tuple(eo + ef)
    else:
        msg = "%.2e" % check_parity(make_model(variant, w)(x).cpu().numpy(), ref)
    with capsys.disabled():
        print("\n[config 3, all 131072 frames, %s] max error of the scale vs fp64: %s" % (net_work, msg))


def test_results_do_not_depend_on_the_tile_to_workgroup_map(built):
    """A persistent workgroup owns a contiguous range of tiles (balanced over the grid).  Whatever the grid -- every CU, 77,
    3 or one workgroup -- a tile's arithmetic is the same, so the masks are bit-identical; and frames on both sides of every
    range boundary of the 77-workgroup map are checked against the oracle."""
    w = rced_np.make_weights("FullyCNNV3", seed=12)
    n, t = 37, 200                       # 37 utterances x 50 tiles = 1850 tiles
    x = rced_np.make_input(n, t, seed=99)
    m = make_model(3, w)
    y = m(x)
    for grid in (77, 3, 1):
        m.set_option("fused_grid", grid)
        assert np.array_equal(m(x), y), grid
    m.set_option("fused_grid", 0)
    total, grid = n * 50, 77
    base, rem = divmod(total, grid)
    scale = np.abs(y).max()
    for b in range(1, grid):
        first = b * base + min(b, rem)                      # first tile of workgroup b
        for tile in (first - 1, first):
            u, t0 = divmod(tile, 50)
            for fr in (4 * t0, 4 * t0 + 3):                 # first and last frame of the tile
                lo, hi = max(fr - 3, 0), min(fr + 5, t)
                ref = rced_c.forward("FullyCNNV3", w, x[u:u + 1, lo:hi], np.float64)[0, fr - lo]
                assert np.abs(y[u, fr] - ref).max() <= RTOL * scale, (b, tile, fr)


@pytest.mark.parametrize("net_work,tag,variant", [n for n in NETS if n[2] != 3])
def test_latency_form_is_bit_identical_to_the_throughput_form(net_work, tag, variant, built):
    """R-CED V1 / V2: a call with fewer 3-frame tiles than the part has CUs runs on one-frame tiles (option `latency_form`, on by
    default; BASELINE configs[0] = one utterance of 256 frames is such a call).  Same packets, same arithmetic per pixel -- the
    remainder pass's columns of pixels are frame-aligned, so a bin's taps meet in the same K-steps wherever its frame sits in a
    tile -- hence bit-identical masks (an utterance's result does not depend on the batch it came in), for ragged T and T < 8 too."""
    w, g = load_golden(tag)
    m = make_model(variant, w)
    assert m.get_option("latency_form") == 1
    cases = [g["x_c1"], rced_np.make_input(1, 1, seed=5), rced_np.make_input(2, 7, seed=6), rced_np.make_input(3, 100, seed=7),
             rced_np.make_input(5, 151, seed=8)]          # 5 x 151: 255 three-frame tiles, one under the CU count of the part
    fast = [m(x) for x in cases]
    m.set_option("latency_form", 0)
    assert m.get_option("latency_form") == 0
    for x, y in zip(cases, fast):
        assert np.array_equal(m(x), y), x.shape
    check_parity(fast[0], g["y_c1"])
    check_parity(fast[4], rced_c.forward(net_work, w, cases[4], np.float64))
    m.set_option("latency_form", 1)
    m.set_option("fused_grid", 3)            # the rule counts the workgroups the call may use
    assert np.array_equal(m(cases[3]), fast[3])
    m.set_option("fused_grid", 0)
    with pytest.raises(Exception, match="0 or 1"):
        m.set_option("latency_form", 2)
    w3 = rced_np.make_weights("FullyCNNV3", seed=3)
    with pytest.raises(Exception, match="one form of tile"):
        make_model(3, w3).set_option("latency_form", 1)


def _scaled_inner_channels(w, rng, lo=-4.0, hi=4.0):
    """CR-CED weights in which every channel of the 18- and 30-channel tensors (one consumer each, no skip) carries its own
    scale 10^U(lo, hi): BatchNorm gamma / beta of the producer are multiplied by it and the consumer's kernel slice divided,
    so the net computes the same function (ReLU is positively homogeneous) while the values that meet in one K = 32 chunk of
    the three-part products differ by up to eight orders of magnitude."""
    w = {k: np.array(v, dtype=np.float64) for k, v in w.items()}
    for blk in ("CE1", "CE2", "CE3", "CD1", "CD2"):
        for prod, cons in (("%s_encode_1" % blk, "%s_encode_2" % blk), ("%s_encode_2" % blk, "%s_decode" % blk)):
            s = 10.0 ** rng.uniform(lo, hi, w[prod + "/batch_norm/gamma"].shape[0])
            w[prod + "/batch_norm/gamma"] *= s
            w[prod + "/batch_norm/beta"] *= s
            w[cons + "/kernel"] /= s[None, None, :, None]
    return {k: v.astype(np.float32) for k, v in w.items()}


def test_three_part_products_on_adversarial_magnitudes(built, capsys):
    """The split x = h + m + l (bf16 parts) of the CR-CED kernel's 18-channel tensor under magnitudes the synthetic inputs never
    produce: per-channel scales spanning 1e-4 .. 1e4 inside one K = 32 chunk, inputs x 1e-6 and x 1e4, a frame of exact zeros
    next to a frame of 1e4.  Both forms of the kernel against the oracle (1e-4) and each other; measured errors printed."""
    rng = np.random.default_rng(2024)
    base = rced_np.make_weights("FullyCNNV3", seed=5)
    rows = []
    for name, w, x in (
            ("channel scales 1e-4..1e4", _scaled_inner_channels(base, rng), rced_np.make_input(3, 21, seed=1)),
            ("channel scales 1e-2..1e2, input x 30", _scaled_inner_channels(base, rng, -2, 2), rced_np.make_input(2, 9, seed=2) * np.float32(30)),
            ("input x 1e-6", base, rced_np.make_input(2, 13, seed=3) * np.float32(1e-6)),
            ("input x 1e4", base, rced_np.make_input(2, 13, seed=4) * np.float32(1e4)),
            ("zero frame beside a 1e4 frame", base, None)):
        if x is None:
            x = rced_np.make_input(2, 16, seed=5)
            x[:, 7] = 0.0
            x[:, 8] *= np.float32(1e4)
        ref = rced_c.forward("FullyCNNV3", w, x, np.float64)
        ys, eo, ef = v3_check_forms(v3_forms(w), x, ref, what=name)
        assert all(np.isfinite(y).all() for y in ys)
        rows.append((name,) + tuple(eo + ef))
        assert max(ef) <= 4 * V3_FORMS_AGREE, rows[-1]
    with capsys.disabled():
        print()
        for r in rows:
            print("[adversarial] %-40s all x6 %.2e  fp32-MFMA %.2e  product vs fp32-MFMA %.2e" % r)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("form", [3, 0])
def test_non_finite_input_stays_inside_its_tiles(bad, form, built):
    """One Inf / NaN magnitude at (utterance 1, frame 21, bin 40).  Frame t of the output needs frames t-3 .. t+4 of the input
    (only the first layer looks along time), so frames 17..24 of utterance 1 are the ones the oracle changes.  The kernel
    works on tiles of 4 frames whose frames sit side by side in one pixel row, and its zero-weight padding slots (K rounded
    up to the MFMA's K, SAME padding as rows of zeros) turn Inf x 0 into NaN: a non-finite value can reach the edge bins of
    the other frames of its TILE (here tiles 16..19, 20..23, 24..27), never another tile.
    What the values INSIDE the field are is not compared: ReLU is an integer max(bits, 0) here -- a NaN with the sign bit
    clear stays NaN, one with the sign bit set becomes 0, which is also what IEEE maxNum(NaN, 0), CUDA's fmaxf and the plain-C
    oracle give, while numpy's maximum (the other oracle) keeps every NaN; the reference's own answer (TF 1.14 `tf.nn.relu` on
    a NaN) is not defined by anything in its source.  Checked: every frame outside those tiles is BIT-IDENTICAL to the run on
    the clean input; the bad value does change its field; the call returns, rced_check is clean, and the next call on the
    clean input gives the clean result."""
    from fullycnnspeechenhancement_amd import _lib
    w = rced_np.make_weights("FullyCNNV3", seed=8)
    x = rced_np.make_input(3, 40, seed=6)
    m = make_model(3, w)
    m.set_option("v3_l2x6", form)
    clean = m(x)
    xb = x.copy()
    xb[1, 21, 40, 0] = bad
    y = m(xb)
    assert _lib.load().rced_check(m._infer_handle()) == 0
    with np.errstate(all="ignore"):
        ref = rced_np.forward("FullyCNNV3", w, xb, np.float64)
    field = np.zeros((3, 40), bool)
    field[1, 17:25] = True                      # the oracle's receptive field
    tiles = np.zeros((3, 40), bool)
    tiles[1, 16:28] = True                      # the tiles that contain it
    assert np.isfinite(ref[~field]).all() and not np.isfinite(ref[field]).all()
    assert np.array_equal(y[~tiles], clean[~tiles])
    assert not np.array_equal(y[field], clean[field])
    assert np.array_equal(m(x), clean)


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_repeated_launches_are_bit_identical(net_work, tag, variant, built):
    """Race screen: the fused kernels hand tiles between waves (K-split hand-off, LDS-DMA packets,
    hand-placed pipelines); a hazard shows up as run-to-run differences long before it shows up as a
    tolerance failure.  Many small launches (1 tile per workgroup) and a few large ones."""
    w = rced_np.make_weights(net_work, seed=21)
    m = make_model(variant, w)
    for shape, reps in (((1, 40), 12), ((3, 7), 6), ((64, 128), 3)):
        x = rced_np.make_input(*shape, seed=sum(shape))
        ref = rced_c.forward(net_work, w, x, np.float64) if shape[0] * shape[1] <= 64 else None
        y0 = m(x)
        if ref is not None:
            check_parity(y0, ref)
        for _ in range(reps):
            assert np.array_equal(m(x), y0)


def test_out_argument_for_host_and_device_buffers(built):
    """model(x, out=buf): the caller's buffer is written and returned, for ndarray and for cuda tensors; a buffer of the
    wrong kind, shape or dtype is refused."""
    import torch
    w = rced_np.make_weights("FullyCNNV3", seed=3)
    m = make_model(3, w)
    x = rced_np.make_input(3, 10, seed=4)
    y = m(x)
    buf = np.full_like(x, -7.0)
    assert m(x, out=buf) is buf and np.array_equal(buf, y)
    xt = torch.from_numpy(x).cuda()
    bt = torch.full_like(xt, -7.0)
    assert m(xt, out=bt) is bt and np.array_equal(bt.cpu().numpy(), y)
    for bad in (np.zeros((3, 10, 129), np.float32), np.zeros(x.shape, np.float64), bt, np.zeros(x.shape, np.float32)[:, ::-1]):
        with pytest.raises(ValueError):
            m(x, out=bad)
    with pytest.raises(ValueError):
        m(xt, out=buf)


def test_single_op_conv_bn_relu_known_answers(built):
    """rced_conv_bn_relu against the analytic cases of test_oracle.py, and against the oracle op."""
    import torch
    from fullycnnspeechenhancement_amd import conv_bn_relu
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    # kh = 8 asymmetry: 3 past / 4 future
    x = torch.ones((1, 12, 129, 1), device=dev)
    p = {"c/kernel": np.ones((8, 1, 1, 1), np.float32), "c/bias": np.zeros(1, np.float32)}
    y = conv_bn_relu(x, 1, (8, 1), (1, 1), False, use_norm=False, use_act=False, scope="c", params=p).cpu().numpy()
    assert y[0, 0, 0, 0] == 5 and y[0, 11, 0, 0] == 4 and y[0, 5, 0, 0] == 8
    # random layers of every shape class the three nets use, with BN, skip and ReLU
    for (kh, kw, cin, cout) in ((8, 13, 1, 12), (1, 11, 12, 16), (1, 5, 15, 19), (1, 9, 30, 8), (1, 129, 8, 1), (1, 7, 25, 23)):
        xin = rng.standard_normal((2, 9, 129, cin)).astype(np.float32)
        k = (rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * cin)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
        bn = (rng.uniform(0.5, 1.5, cout), rng.uniform(-0.1, 0.1, cout), rng.normal(0, 0.1, cout), rng.uniform(0.5, 1.5, cout))
        bn = tuple(a.astype(np.float32) for a in bn)
        skip = rng.standard_normal((2, 9, 129, cout)).astype(np.float32)
        p = {"s/kernel": k, "s/bias": b, "s/batch_norm/gamma": bn[0], "s/batch_norm/beta": bn[1],
             "s/batch_norm/moving_mean": bn[2], "s/batch_norm/moving_variance": bn[3]}
        ref = rced_np.conv_bn_relu(xin, k, b, bn, skip, True)
        y = conv_bn_relu(torch.from_numpy(xin).to(dev), cout, (kh, kw), (1, 1), False, scope="s",
                         skip_input=torch.from_numpy(skip).to(dev), params=p).cpu().numpy()
        check_parity(y, ref)
        ref = rced_np.conv_bn_relu(xin, k, b, None, None, False)
        y = conv_bn_relu(torch.from_numpy(xin).to(dev), cout, (kh, kw), (1, 1), False, use_norm=False,
                         use_act=False, scope="s", params=p).cpu().numpy()
        check_parity(y, ref)


def test_engine_test_step_surface(built):
    """tester.py:85-90 surface: ndarray [N,T,129,1] -> ndarray [N,T,129,1]."""
    import configparser
    from fullycnnspeechenhancement_amd import FullyCNNTester
    w, g = load_golden("v3")
    cfg = configparser.ConfigParser()
    cfg.read_dict({"model": {"net_arch": "FullyCNN", "net_work": "FullyCNNV3"}, "data": {"feature_dim": "129"},
                   "inference": {"checkpoint_filepath": ""}})
    eng = FullyCNNTester(cfg, weights=w)
    assert eng.param_count() == 32653
    out = eng.test_step(g["x_small"])
    assert isinstance(out, np.ndarray) and rel_err(out, g["y_small"]) < RTOL
    again = eng.test_step(g["x_small"])
    assert again is not out and np.array_equal(again, out)            # a fresh array per call, as sess.run returns one
    mine = np.empty_like(out)
    assert eng.test_step(g["x_small"], out=mine) is mine and np.array_equal(mine, out)     # a caller-owned output array
    pooled = FullyCNNTester(cfg, weights=w, reuse_output=True)        # opt-in: two pooled arrays per shape, alternating
    a = pooled.test_step(g["x_small"])
    b = pooled.test_step(g["x_small"])
    c = pooled.test_step(g["x_small"])
    assert a is not b and c is a and np.array_equal(a, out) and np.array_equal(b, out)


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_forward_is_capturable_into_a_hip_graph(net_work, tag, variant, built):
    """rced.h: after rced_reserve, rced_forward allocates nothing and can be stream-captured."""
    import torch
    w, g = load_golden(tag)
    m = make_model(variant, w)
    x = torch.from_numpy(g["x_long"]).cuda()
    m.reserve(x.shape[0], x.shape[1])
    y_eager = m(x).clone()
    static_x = x.clone()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(static_x)                      # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(graph):
        static_y = m(static_x)
    for scale in (1.0, 0.5):
        static_x.copy_(x * scale)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, m(static_x))
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, y_eager)


def test_restore_swaps_weights(built):
    w1 = rced_np.make_weights("FullyCNN", seed=1)
    w2 = rced_np.make_weights("FullyCNN", seed=2)
    x = rced_np.make_input(1, 10, seed=3)
    m = make_model(1, w1)
    y1 = m(x)
    m.restore(w2)
    y2 = m(x)
    check_parity(y1, rced_c.forward("FullyCNN", w1, x))
    check_parity(y2, rced_c.forward("FullyCNN", w2, x))
    assert np.abs(y1 - y2).max() > 1e-3


def test_c_abi_status_codes_on_device(built):
    from fullycnnspeechenhancement_amd import _lib, weights
    lib = _lib.load()
    blob = weights.pack_blob(3, rced_np.make_weights("FullyCNNV3", seed=1))
    h = ctypes.c_void_p()
    assert lib.rced_create(3, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), blob.size, 99, ctypes.byref(h)) == _lib.RCED_ERR_ARG
    bad = blob.copy()
    bad[5] = np.inf
    assert lib.rced_create(3, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), bad.size, 0, ctypes.byref(h)) == _lib.RCED_ERR_ARG
    assert lib.rced_create(3, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), blob.size, 0, ctypes.byref(h)) == 0
    assert lib.rced_forward(h, None, None, 1, 1, None) == _lib.RCED_ERR_ARG
    assert lib.rced_forward(h, None, None, 0, 7, None) == 0            # empty batch is fine
    assert lib.rced_forward(h, None, None, -1, 7, None) == _lib.RCED_ERR_ARG
    assert lib.rced_set_option(h, b"nonsense", 1) == _lib.RCED_ERR_ARG
    v = ctypes.c_int(-1)
    assert lib.rced_get_option(h, b"v3_l2x6", ctypes.byref(v)) == 0 and v.value == 3        # the product form is the default
    assert lib.rced_set_option(h, b"v3_l2x6", 4) == _lib.RCED_ERR_ARG                       # 3 and 0 are the forms in the library
    assert b"v3_l2x6 takes 3" in lib.rced_last_error()                                      # the specific refusal, not "unknown option"
    assert lib.rced_set_option(h, b"v3_l2x6", 2) == _lib.RCED_ERR_ARG                       # round 4's product: a legacy build's
    assert lib.rced_set_option(h, b"final_x6", 1) == _lib.RCED_ERR_ARG and b"R-CED V1 / V2 output-layer" in lib.rced_last_error()
    assert lib.rced_set_option(h, b"nonsense", 1) == _lib.RCED_ERR_ARG and b"unknown option" in lib.rced_last_error()
    assert lib.rced_set_option(h, b"v3_l2x6", -1) == _lib.RCED_ERR_ARG
    assert lib.rced_get_option(h, b"v3_l2x6", ctypes.byref(v)) == 0 and v.value == 3        # a refused value changes nothing
    lib.rced_destroy(h)


def test_from_root_on_rccl_world_size_1(built):
    """dist.BatchShardedForward over the "nccl" backend (= RCCL) with a single rank: the process-group plumbing, the
    in-place root forward and the no-peer path on the real backend (world_size > 1 is covered on gloo, tests/test_dist_cpu.py;
    a second rank cannot share this one GPU under RCCL)."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from fullycnnspeechenhancement_amd.dist import BatchShardedForward
    w, g = load_golden("v3")
    m = make_model(3, w)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(s.getsockname()[1])
    s.close()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        one = torch.ones(1, device="cuda")
        dist.all_reduce(one)                               # RCCL itself runs
        assert int(one.item()) == 1
        eng = BatchShardedForward(m, device="cuda:0", forward_into=lambda a, out: m(a, out=out))
        x = torch.from_numpy(rced_np.make_input(5, 12, seed=8)).cuda()
        y = eng.forward_from_root(x, root=0, chunks=3)
        torch.cuda.synchronize()
        assert torch.equal(y, m(x))
        assert torch.equal(eng.forward_resident(x), y)
        # the CU reservation bench.py's from_root leg sweeps: inside the block the forwards run on num_cus - r workgroups
        # (CUs left to RCCL's kernels), the masks are the same bits, and the option is restored afterwards
        from fullycnnspeechenhancement_amd.dist import reserved_cus
        cus = m.get_option("num_cus")
        xb = torch.from_numpy(rced_np.make_input(64, 40, seed=9)).cuda()     # 640 tiles: every workgroup of either grid has work
        yb = m(xb)
        for r in (4, 16):
            with reserved_cus(m, r):
                assert m.get_option("fused_grid") == cus - r
                assert torch.equal(eng.forward_from_root(xb, root=0, chunks=2), yb)
            assert m.get_option("fused_grid") == 0
        # BASELINE configs[3]'s WORKLOAD on the real backend, as far as one rank goes: the whole global batch [2048, 512, 129, 1]
        # (541 MB in, 541 MB out: indices past 2^27 floats, the default chunking of bench.py's from_root leg) through the no-peer path
        g = torch.Generator(device="cuda").manual_seed(4)
        xg = torch.randn((2048, 512, 129, 1), generator=g, device="cuda").abs_()
        yg = eng.forward_from_root(xg, root=0, chunks=8)
        torch.cuda.synchronize()
        assert yg.shape == xg.shape and bool(torch.isfinite(yg).all())
        for a, b in ((0, 3), (1023, 1026), (2045, 2048)):
            assert torch.equal(yg[a:b], m(xg[a:b].contiguous())), (a, b)
        del xg, yg
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_integration_md_binding_runs_verbatim(net_work, tag, variant, built):
    """INTEGRATION.md section 1 shows the ctypes binding a maintainer of the reference would add (`RcedSession`).  The code
    block is extracted from the markdown AS PRINTED -- only the library's file name is made absolute -- executed, and its
    `run()` held to the committed golden vectors: the document cannot drift from the ABI."""
    import re
    from conftest import ROOT
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = md[md.index("## 1."):md.index("## 2.")]
    code = re.search(r"```python\n(.*?)```", section, re.S).group(1)
    assert "class RcedSession" in code and 'ctypes.CDLL("librced_hip.so")' in code
    code = code.replace('"librced_hip.so"', repr(os.path.join(ROOT, "fullycnnspeechenhancement_amd", "librced_hip.so")))
    ns = {}
    exec(compile(code, "INTEGRATION.md#1", "exec"), ns)
    w, g = load_golden(tag)
    sess = ns["RcedSession"](net_work, w)
    try:
        for key in ("small", "long"):
            y = sess.run(g["x_" + key])
            assert y.shape == g["y_" + key].shape and y.dtype == np.float32
            check_parity(y, g["y_" + key])
    finally:
        sess.close()


def test_rced_check_reports_the_sticky_handoff_error(built):
    """include/rced.h rced_check: a caller that enqueues one device-resident forward and synchronises its own stream
    asks the model whether that launch was valid.  The error word is forced through the documented test hook."""
    import torch
    from fullycnnspeechenhancement_amd import _lib
    w = rced_np.make_weights("FullyCNNV3", seed=7)
    m = make_model(3, w)
    x = torch.from_numpy(rced_np.make_input(2, 16, seed=3)).cuda()
    y = m(x)
    torch.cuda.synchronize()
    assert m.check() is True and _lib.load().rced_check(m._handle) == _lib.RCED_OK
    m.set_option("inject_handoff_error", 2)
    del m._options["inject_handoff_error"]          # a test hook, not a setting to replay on restore()
    assert _lib.load().rced_check(m._handle) == _lib.RCED_ERR_STATE
    with pytest.raises(_lib.RcedError) as ei:
        m.check()
    assert ei.value.code == _lib.RCED_ERR_STATE and "hand-off" in str(ei.value)
    with pytest.raises(_lib.RcedError):             # ... and the model refuses further launches
        m(x)
    m.set_option("inject_handoff_error", 0)
    del m._options["inject_handoff_error"]
    assert m.check() is True
    assert torch.equal(m(x), y)
    assert _lib.load().rced_check(None) == _lib.RCED_ERR_ARG


@pytest.mark.parametrize("shape", [(2, 9, 129, 1, 18, 8, 9), (3, 5, 129, 8, 30, 1, 5), (1, 4, 129, 6, 7, 1, 3)])
@pytest.mark.parametrize("use_act,with_skip", [(True, False), (True, True), (False, True)])
def test_single_op_conv_bn_relu_training_mode(shape, use_act, with_skip, built):
    """module.py:11-34 with is_training=True: BatchNorm with the statistics of the batch (biased variance, eps 1e-3),
    then + skip, then ReLU -- against the numpy fp64 restatement of the same op (oracle/rced_np.conv_bn_relu with the
    batch's own mean / variance as the 'moving' statistics)."""
    import torch
    from fullycnnspeechenhancement_amd.model import conv_bn_relu
    n, t, f, cin, cout, kh, kw = shape
    rng = np.random.default_rng(hash(shape) % 1000)
    x = rng.standard_normal((n, t, f, cin)).astype(np.float32)
    k = (rng.standard_normal((kh, kw, cin, cout)) * 0.2).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    beta = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
    skip = rng.standard_normal((n, t, f, cout)).astype(np.float32) if with_skip else None
    z = rced_np.conv_bn_relu(x, k, b, None, None, use_act=False)                 # conv + bias, fp64
    mean, var = z.mean(axis=(0, 1, 2)), z.var(axis=(0, 1, 2))                    # biased variance
    ref = rced_np.conv_bn_relu(x, k, b, (gamma, beta, mean, var), skip, use_act=use_act)
    params = {"c/kernel": k, "c/bias": b, "c/batch_norm/gamma": gamma, "c/batch_norm/beta": beta,
              "c/batch_norm/moving_mean": np.full(cout, 7.0, np.float32),        # must be ignored in training mode
              "c/batch_norm/moving_variance": np.full(cout, 9.0, np.float32)}
    y = conv_bn_relu(torch.from_numpy(x).cuda(), cout, (kh, kw), is_training=True, use_act=use_act, scope="c",
                     skip_input=torch.from_numpy(skip).cuda() if with_skip else None, params=params)
    check_parity(y.cpu().numpy(), ref, what="conv_bn_relu(is_training=True) %s" % (shape,))


def _run_bench_rehearsal(extra_env, timeout_s, *args):
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update({"RCED_BENCH_REHEARSE": "1"}, **extra_env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
                        "--cpu-seconds", "0", "--no-secondary", "--batch", "8", "--frames", "64"] + list(args),
                       env=env, capture_output=True, text=True, timeout=timeout_s)
    lines = [l for l in r.stdout.splitlines() if l.lstrip().startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


@pytest.mark.gpu
def test_bench_two_ranks_control_flow_rehearsal():
    """bench.py's N > 1 branch (self-launch through torch.distributed.run, barriers around the timed region, the max over
    ranks, one JSON line from rank 0) with two ranks sharing this box's GPU and gloo as the control plane: RCCL itself
    cannot be rehearsed on one GPU, everything around it can."""
    r, d = _run_bench_rehearsal({}, 600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert d is not None and d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 16 and d["config"]["rccl_world_size"] == 2 and "rehearsal" in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 2 * 8 * 64 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    assert d["roofline"]["kernel"] == "rced_fused" and d["roofline"]["launches"] == 3
    fr = d["from_root"]          # the copy transport (IPC handles, device-to-device copies) runs for real between two processes on one GPU
    assert fr["transport"] == "copy" and fr["value"] > 0 and fr["global_batch"] == 16 and "error" not in fr["transports"]["copy"], fr
    assert "of WORLD_SIZE=2 started" in r.stderr


@pytest.mark.gpu
def test_bench_line_survives_a_from_root_that_never_returns():
    """The first exchange of utterances between GPUs must not be able to take the headline line down, and must not read as
    success either: with a from_root that hangs, rank 0 prints the line (from_root.error = the timeout), `launch_ranks` relays
    it, and every rank exits non-zero by default (--from-root-fail-status 0 for callers that read the line only)."""
    r, d = _run_bench_rehearsal({"RCED_BENCH_REHEARSE_HANG": "1"}, 600, "--from-root-timeout", "5")
    assert r.returncode != 0, r.stderr[-3000:]          # (torch.distributed.run turns the ranks' status 3 into its own failure code)
    assert d is not None and d["n_gpus"] == 2 and d["value"] > 0 and d["roofline"] is not None
    assert "timeout" in d["from_root"]["error"]
    r, d = _run_bench_rehearsal({"RCED_BENCH_REHEARSE_HANG": "1"}, 600, "--from-root-timeout", "5", "--from-root-fail-status", "0")
    assert r.returncode == 0, r.stderr[-3000:]
    assert d is not None and "timeout" in d["from_root"]["error"]


def test_plain_bench_line_and_dumped_masks(built, tmp_path):
    """A plain `bench.py --gpus 1` run prints the headline and nothing measured beside it (that is --full's), times exactly
    --steps steps, and --dump-outputs writes the masks of the timed path: those of the oracle on bench.py's own seeded inputs,
    and the same on a second run."""
    import json
    import subprocess
    import sys
    import bench
    from fullycnnspeechenhancement_amd import weights
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    B, T, steps = 3, 40, 4
    masks = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT_DIR, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--batch", str(B), "--frames", str(T), "--dump-outputs", str(tmp_path / run)],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout[-3000:]
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["warmup"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
        assert d["unit"] == "frames/s" and d["ms_per_step"] > 0
        assert abs(d["value"] - B * T * steps / (d["ms_per_step"] * steps * 1e-3)) < 1e-6 * d["value"]
        assert not {"roofline", "cpu_baseline", "host_buffers", "secondary", "from_root"} & set(d), sorted(d)
        y = np.load(str(tmp_path / run / "mask.npy"))
        assert y.dtype == np.float32 and y.shape == (B, T, 129, 1)
        masks.append(y)
    x = bench.synthetic_magnitudes((B, T, 129, 1), 1234)
    check_parity(masks[0], rced_c.forward("FullyCNNV3", weights.synthetic_weights(3, seed=42), x, np.float64), what="bench dump")
    assert np.array_equal(masks[0], masks[1])


def _copy_gpu_worker(rank, world, port, out_path):
    import sys
    sys.path.insert(0, ROOT_DIR)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)      # control plane only: RCCL refuses two ranks on one device
    try:
        from fullycnnspeechenhancement_amd import build_model
        from fullycnnspeechenhancement_amd.dist import BatchShardedForward
        torch.cuda.set_device(0)
        w = rced_np.make_weights("FullyCNNV3", seed=42)
        model = build_model("FullyCNNV3", False, weights=w, device=0)
        eng = BatchShardedForward(model, device="cuda:0", forward_into=lambda a, out: model(a, out=out), transport="copy")
        x = torch.from_numpy(rced_np.make_input(7, 24, seed=31)).cuda() if rank == 0 else None
        for chunks in (1, 3):
            y = eng.forward_from_root(x, root=0, chunks=chunks)
            if rank == 0:
                ref = model(x)
                assert torch.equal(y, ref), chunks        # the peers' slices came back through the root's IPC-shared output, bit for bit
        if rank == 0:
            check_parity(y.cpu().numpy(), rced_c.forward("FullyCNNV3", w, x.cpu().numpy(), np.float64))
            open(out_path, "w").write("ok")
        dist.barrier()
        eng.close()
        model.close()
    finally:
        dist.destroy_process_group()


def _config4_worker(rank, world, port, out_path):
    import sys
    sys.path.insert(0, ROOT_DIR)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from fullycnnspeechenhancement_amd import build_model
        from fullycnnspeechenhancement_amd.dist import BatchShardedForward, shard_bounds
        torch.cuda.set_device(0)
        w = rced_np.make_weights("FullyCNNV3", seed=42)
        model = build_model("FullyCNNV3", False, weights=w, device=0)
        eng = BatchShardedForward(model, device="cuda:0", forward_into=lambda a, out: model(a, out=out), transport="copy")
        x = None
        if rank == 0:
            g = torch.Generator(device="cuda").manual_seed(1234)
            x = torch.randn((2048, 512, 129, 1), generator=g, device="cuda").abs_()
        ys = [eng.forward_from_root(x, root=0, chunks=8) for _ in range(2)]      # twice: the handle caches, the second output buffer
        if rank == 0:
            torch.cuda.synchronize()
            y = ys[1]
            assert ys[0].data_ptr() != ys[1].data_ptr() and torch.equal(ys[0], ys[1])
            assert bool(torch.isfinite(y).all())
            (lo0, hi0), (lo1, hi1) = shard_bounds(2048, 2)
            assert (lo1, hi1) == (1024, 2048)
            # sampled pieces of both shards, chunk seams and the ends included, against the root computing them itself: bit for bit
            for a, b in ((0, 2), (127, 130), (1022, 1024), (1024, 1027), (1151, 1154), (1535, 1538), (2046, 2048)):
                assert torch.equal(y[a:b], model(x[a:b].contiguous())), (a, b)
            # ... and sampled frames against the oracle on their receptive fields (frames t - 3 .. t + 4)
            rng = np.random.default_rng(5)
            picks = [(0, 0), (2047, 511), (1024, 0), (1023, 511)] + [(int(rng.integers(2048)), int(rng.integers(512))) for _ in range(8)]
            scale = float(y.abs().max())
            worst = 0.0
            for n, t in picks:
                lo, hi = max(t - 3, 0), min(t + 5, 512)
                ref = rced_c.forward("FullyCNNV3", w, x[n:n + 1, lo:hi].cpu().numpy(), np.float64)[0, t - lo]
                worst = max(worst, float(np.abs(y[n, t].cpu().numpy() - ref).max()) / scale)
            assert worst < RTOL, worst
            open(out_path, "w").write("ok %.3e" % worst)
        dist.barrier()
        eng.close()
        model.close()
    finally:
        dist.destroy_process_group()


def test_config4_workload_through_the_copy_transport(built, tmp_path, capsys):
    """BASELINE configs[3]'s workload -- the global batch [2048, 512, 129, 1] of one host process (tester.py:85-90; layout
    data_loader.py:198-209) -- through BatchShardedForward.forward_from_root with transport="copy", bench.py's default chunking,
    between two processes that share this box's GPU: 541 MB in and out through IPC handles, shards of 1,024 utterances in 8
    chunks, indices past 2^27 floats, the handle caches and both output buffers.  Sampled pieces of both shards are bit-equal to
    the root computing them itself; twelve sampled frames meet the oracle on their receptive fields.  (What one GPU cannot
    show is the scaling: no byte crosses xGMI here.)"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "ok")
    mp.spawn(_config4_worker, args=(2, port, out), nprocs=2, join=True)
    res = open(out).read()
    assert res.startswith("ok")
    with capsys.disabled():
        print("\n[config 4 workload, copy transport, two processes on one GPU] worst sampled frame vs oracle %s" % res[3:])


def test_from_root_copy_transport_through_ipc_handles(built, tmp_path):
    """dist.py's transport="copy" on device tensors: two processes share this box's GPU; the root exports CUDA IPC memory handles of
    its input and output, the peer pulls its utterances and pushes its masks with device-to-device copies on side streams.  The
    gathered result is bit-equal to the root computing the whole batch itself.  (Between two GPUs the same copies run over xGMI;
    that leg has no box in the build pool.)"""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "ok")
    mp.spawn(_copy_gpu_worker, args=(2, port, out), nprocs=2, join=True)
    assert open(out).read() == "ok"
