"""The guard on the bars of tests/forward_bars.py, on the CPU, over the very cases test_forward_tight_gpu.py runs on the device:
the bars are neither inside the spread of their own yardsticks, nor so wide that a forward which is subtly wrong in one bin,
one tile slot or at a time edge would pass them -- as it passes conftest.check_parity, which is asserted here too: that is the
gap the tight tests close.  Figures in the docstrings: this suite's seeds, printed by every test."""

import numpy as np
import pytest

import forward_bars as fb
from conftest import check_parity
from oracle import layers as L, rced_np, torch_ref

NETS = list(fb.VARIANT)
R16 = 2.0 ** -16                 # one dropped cross term of a three-part bf16 split; a part truncated where it should be rounded


def cases_of(net_work):
    return [fb.case(net_work, regime, shape) for regime in fb.regimes_of(net_work) for shape in fb.SHAPES]


def with_defect(case, fn):
    """The case's fp32 chain (yardstick A's outputs) with `fn(y)` applied in place to a float64 copy, back in float32."""
    ys = []
    for y in case.chain:
        y = np.array(y, np.float64)
        fn(y)
        ys.append(y.astype(np.float32))
    return ys


def passes_check_parity(case, ys):
    for y, ref in zip(ys, case.refs):
        check_parity(y, ref, what=case.name)
    return True


@pytest.mark.parametrize("net_work", NETS)
def test_groups_hold_enough_values_and_cover_the_tensor(net_work, built):
    for case in cases_of(net_work):
        size = sum(r.size for r in case.refs)
        for kind, (labels, names) in case.groups.items():
            counts = np.bincount(labels[labels >= 0], minlength=len(names))
            assert labels.size == size and counts.min() >= fb.MIN_GROUP, (case.name, kind, counts.min())
            if kind in ("bin", "slot", "end"):
                assert counts.sum() == size, (case.name, kind)          # a partition of the tensor
        assert len(case.groups["bin"][1]) == 129


@pytest.mark.parametrize("net_work", NETS)
def test_the_two_yardstick_chains_agree_within_the_margin(net_work, built, capsys):
    """Otherwise MARGIN would sit inside the yardstick's own spread.  Measured: at most 3.2x (largest element; the rms groups,
    floored as the yardstick is, at most 2.6x)."""
    worst = {}
    for case in cases_of(net_work):
        for kind, r in case.spread().items():
            worst[kind] = max(worst.get(kind, (0.0, ""))[0:2], (r, case.name))
            assert r <= fb.MARGIN, "%s: the yardstick chains are %.2fx apart in group kind `%s`" % (case.name, r, kind)
    with capsys.disabled():
        print("\n[bars, host] %s: yardstick chains apart by at most %s" % (net_work, "  ".join("%s %.2f" % (k, v[0]) for k, v in worst.items())))


@pytest.mark.parametrize("net_work", NETS)
def test_a_third_fp32_chain_needs_at_most_half_of_every_bar(net_work, built, capsys):
    """oracle/torch_ref.TorchRef(float32) -- oneDNN convolutions, another order of summation again -- as a stand-in for the device:
    a stand-in that needed the whole margin would leave none for the device.  Measured: at most 0.37 of a bar."""
    worst = {}
    for regime in fb.regimes_of(net_work):
        stand_in = torch_ref.TorchRef(net_work, fb.weights_of(net_work, regime))
        for shape in fb.SHAPES:
            case = fb.case(net_work, regime, shape)
            for kind, (f, group) in case.fractions([stand_in(x).numpy() for x in case.xs]).items():
                worst[kind] = max(worst.get(kind, 0.0), f)
                assert f <= 0.5, "%s: the stand-in is at %.2f of the bar of `%s` (%s)" % (case.name, f, kind, group)
    with capsys.disabled():
        print("\n[bars, host] %s: torch fp32 stand-in, worst fraction of the bar: %s" % (net_work, "  ".join("%s %.2f" % kv for kv in worst.items())))


@pytest.mark.parametrize("net_work", NETS)
def test_relative_defects_of_2_to_the_minus_16_miss_the_bar_of_their_group(net_work, built, capsys):
    """An fp32 chain's output with a relative error of 2^-16 on bin 128 only / on every output / on the frames of one tile slot
    (each slot in turn), and of 2^-15 on each utterance's last frame: every one misses the bar of its named group (`bin`, `bin`,
    `slot`, `edge` -- the short set has no slot group, and its last frame is group `end`) on EVERY case, and every one passes
    check_parity.  Measured, the smallest factor by which a defect misses its bar over all cases: bin 128 1.4x, every output 2.9x,
    one slot 1.6x, last frame 1.8x (all four on CR-CED's loud-edge-bin cases, whose yardsticks are the largest; elsewhere
    2.4x / 7.2x / 4.7x / 5.4x and more)."""
    tile, least = fb.TILE[net_work], {}

    def hold(case, name, kind, fn):
        ys = with_defect(case, fn)
        assert passes_check_parity(case, ys)                       # the gap: the present bar lets every one of them through
        f, group = case.fractions(ys)[kind]
        least[name] = min(least.get(name, np.inf), f)
        assert f > 1.0, "%s: the bar of `%s` does not see %s (%.2f of the bar, %s)" % (case.name, kind, name, f, group)
        return group

    def bin128(y):
        y[:, :, 128] *= 1 + R16

    def every(y):
        y *= 1 + R16

    def last_frame(y):
        y[:, -1] *= 1 + 2 * R16

    for case in cases_of(net_work):
        short = len(case.refs) > 1
        assert hold(case, "2^-16 on bin 128", "bin", bin128) == "bin 128"
        hold(case, "2^-16 on every output", "bin", every)
        assert hold(case, "2^-15 on the last frame", "end" if short else "edge", last_frame) == "frame T-1"
        for s in range(0 if short else tile):
            def slot(y, s=s):
                y[:, s::tile] *= 1 + R16
            assert hold(case, "2^-16 on one tile slot", "slot", slot) == "slot %d of %d" % (s, tile)
    with capsys.disabled():
        print("\n[bars, host] %s: a defect misses its group's bar by at least: %s" % (net_work, "  ".join("%s %.2fx" % kv for kv in least.items())))


def _truncate_bf16(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).reshape(np.shape(a))


def _three_parts(a, to_bf16):
    a = np.asarray(a, np.float32)
    h = to_bf16(a)
    m = to_bf16(a - h)
    return [p.astype(np.float64) for p in (h, m, to_bf16(a - h - m))]


def output_layer_in_three_part_products(net_work, w, a, to_bf16=rced_np.bf16_round):
    """The output layer (1 x 129) on the fp32 activations `a` as the device's three-part bf16 products: both operands split
    x = h + m + l, the six products h.h, h.m, m.h, h.l, l.h, m.m, each summed exactly (float64).
    -> f(drop=()) giving the layer's float32 output [N, T, 129, 1] without the products named in `drop`."""
    layer = L.layers_for(net_work)[-1]
    a, k = _three_parts(a, to_bf16), _three_parts(w[layer.scope + "/kernel"], to_bf16)
    prod = {(i, j): rced_np.conv2d_same(a[i], k[j], np.zeros(1), np.float64) for i in range(3) for j in range(3 - i)}
    bias = np.asarray(w[layer.scope + "/bias"], np.float64).reshape(1, 1, 1, 1)
    return lambda drop=(): (bias + sum(v for ij, v in prod.items() if ij not in drop)).astype(np.float32)


@pytest.mark.parametrize("net_work", NETS)
def test_real_faults_of_the_three_part_split_in_the_output_layer(net_work, built, capsys):
    """Arithmetic faults instead of painted-on errors, in the one layer rced_np's per-layer functions let one rebuild alone:
      * the split as it should be (six products, parts rounded) needs 0.05 .. 0.27 of the bars: the form itself is not the error;
      * the m.m product dropped (about 2^-16 of a product, signs random, so it does not add up over K = 129 cin): misses a
        bar (group `bin` on all cases but one, where `edge`) by 1.08x .. 3.7x on every case -- but NOT on CR-CED with loud
        edge bins and raised right-hand taps, where the yardstick chains' own error is 2 .. 3 times the usual and the fault
        reaches only 0.62 .. 0.73 of the bar: short by 1.4x .. 1.6x, stated here and not asserted;
      * parts built by truncation instead of rounding, all six products kept: NOT seen, 0.05 .. 0.27 of the bars, within 10 % of
        the rounded split.  Three truncated parts still hold 24 bits, and what the six products leave out (m.l, l.m, l.l) grows
        from about 2^-24 to about 2^-22 of a product: under an fp32 chain's summation error.  The bars fall short of this one by
        3.7x or more; it is a change of the size fp32 restatements differ by, not a defect they could tell apart;
      * and, as a control, the h.m product dropped (2^-8 of a product): 200x a bar and more, and over check_parity's bar too.
    Every form but the control passes check_parity."""
    seen, blind, clean = [], [], []
    for regime in fb.regimes_of(net_work):
        w = fb.weights_of(net_work, regime)
        for shape in fb.SHAPES:
            case = fb.case(net_work, regime, shape)

            acts = [rced_np.forward(net_work, w, x, np.float32, return_all=True)[-2] for x in case.xs]   # the output layer's input
            rounded = [output_layer_in_three_part_products(net_work, w, a) for a in acts]
            truncated = [output_layer_in_three_part_products(net_work, w, a, _truncate_bf16) for a in acts]

            def worst(forms, drop=()):
                ys = [f(drop) for f in forms]
                return max(f for f, _ in case.fractions(ys).values()), ys

            for forms in (rounded, truncated):
                f, ys = worst(forms)
                assert f <= 0.5 and passes_check_parity(case, ys), (case.name, f)
                clean.append(f)
            f, ys = worst(rounded, ((1, 1),))
            assert passes_check_parity(case, ys)
            if (net_work, regime) == ("FullyCNNV3", "edge_bins"):
                blind.append(f)
            else:
                assert f > 1.0, "%s: no bar sees the dropped m.m product (%.2f)" % (case.name, f)
                seen.append(f)
            f, ys = worst(rounded, ((0, 1),))
            assert f > 100.0, (case.name, f)
            with pytest.raises(AssertionError):
                passes_check_parity(case, ys)
    with capsys.disabled():
        print("\n[bars, host] %s: output layer in three-part products: as it should be / truncated parts %.2f .. %.2f of a bar; m.m dropped "
              "%.2f .. %.2f%s" % (net_work, min(clean), max(clean), min(seen), max(seen),
                                  "; not seen on loud edge bins: %.2f .. %.2f" % (min(blind), max(blind)) if blind else ""))


@pytest.mark.parametrize("full", [True, False], ids=["bn_skip_relu", "bare"])
@pytest.mark.parametrize("cls", range(len(fb.LAYER_CLASSES)), ids=["%dx%d_%dto%d" % c for c in fb.LAYER_CLASSES])
def test_single_layer_bars(cls, full, built):
    """The single-op cases: groups of at least MIN_GROUP values (one output channel: bins pooled in pairs), the two tap-wise
    chains within the margin of each other, the one-product-at-a-time chain above them by what forward_bars.layer_case
    derives, and a 2^-16 error on every output, on one channel or on the last bin group far over the bars while
    check_parity passes it."""
    case = fb.layer_case(cls, full)[0]
    cin, cout = fb.LAYER_CLASSES[cls][2:]
    for kind, (labels, names) in case.groups.items():
        assert np.bincount(labels, minlength=len(names)).min() >= fb.MIN_GROUP
    assert len(case.groups["bin"][1]) == (129 if cout > 1 else 64) and len(case.groups["chan"][1]) == cout
    assert max(case.spread().values()) <= fb.MARGIN
    taps, _, products = (case.measures(e)["all"][0] for e in case.yard)
    assert (products == pytest.approx(taps, rel=0.05)) if cin == 1 else (1.3 * taps < products < 2 * np.sqrt(cin) * taps)
    shape = case.refs[0].shape

    def every(y):
        y *= 1 + R16

    def channel(y):
        y[..., cout - 1] *= 1 + R16

    def last_bins(y):
        y[:, :, 126:] *= 1 + R16

    for fn, kind in ((every, "bin"), (every, "chan"), (channel, "chan"), (last_bins, "bin")):
        ys = with_defect(case, fn)
        assert ys[0].shape == shape and passes_check_parity(case, ys)
        f, group = case.fractions(ys)[kind]
        assert f > 1.0, (case.name, fn.__name__, kind, f, group)
