"""Bars for the fp32 forward that come from fp32 restatements of it, per bin, tile slot and time edge.
Test infrastructure (oracle only), shared by test_forward_bars_host.py (the guard on the bars themselves) and
test_forward_tight_gpu.py (the device held to them).  conftest.check_parity stays the bar of every other test; these are held
in addition.

A case is (net, weights, x), or several of them pooled (the short set: B = 1, T = 1 .. 9).  Per part of a case:

    ref         = rced_c.forward(net, w, x, float64)
    yardstick A = rced_c.forward(net, w, x, float32) - ref        plain C, one product at a time
    yardstick B = rced_np.forward(net, w, x, float32) - ref       numpy, tap-wise matmuls: another order of summation

Every error is divided by max |ref| of its part, and looked at in groups:

    all    root mean square over the tensor
    max    the largest element
    bin    rms per frequency bin 0 .. 128 over utterances and frames
    slot   rms per t mod S, S = 4 for CR-CED and 3 for R-CED: a frame's place in the tile of the fused kernels
    edge   rms per frame 0, 1, 2 and T-4 .. T-1 over utterances and bins: the frames whose first-layer taps reach into SAME padding
    last   rms over the frames of each utterance's last tile (T mod S frames; a full tile when that is 0)
    end    (short set only) rms per frame index counted from the utterance's end
    chan   (single layers only) rms per output channel

A group's yardstick is the larger of A's and B's value; for the rms groups it is floored at the case's `all` yardstick, so that
a bin that happens to come out exact in both chains does not demand exactness.  The bar of a group is MARGIN x its yardstick.
Every rms group holds at least MIN_GROUP values: a group with fewer is pooled with its neighbours (single layers with one
output channel: 18 values per bin, pooled in pairs), never dropped.

MARGIN = 4.  From below: the two yardstick chains are themselves up to 3.2x apart (largest element; 2.6x in the rms groups
after the floor), and test_forward_bars_host.py holds them within MARGIN of each other -- a margin inside that spread would be
a bar on which chain one happened to pick.  A third fp32 chain, oracle/torch_ref.TorchRef(float32), needs at most 0.37 of any
bar (held at 0.5).  The device is a fourth order of summation, and what its three-part bf16 products drop (m.l, l.m, l.l:
about 3 x 2^-24 of a product) is the size of an fp32 rounding, so it earns no term of its own: the output layer rebuilt
on the host in that form, summed exactly, needs 0.05 .. 0.27 of the bars.  From above: MARGIN may rise only as far as the
host test still sees every emulated defect in its named group on every case.  At 4 a relative error of 2^-16 on bin 128
misses `bin` by 1.4x at the least, on every output by 2.9x, on one tile slot `slot` by 1.6x, and 2^-15 on the last frame
`edge` by 1.8x; a dropped m.m product in the output layer misses a bar by as little as 1.08x -- there is no room above 4.

What the bars do not see, measured in test_forward_bars_host.py and stated there: the dropped m.m product on CR-CED with loud
edge bins and raised right-hand taps (0.62 .. 0.73 of the bar: the yardsticks' own error is two to three times the usual
there); three-part splits whose parts are truncated instead of rounded, all six products kept (0.27 of a bar at most: the
parts still hold 24 bits, the result is an fp32-quality form like another).

The one derived term -- single layers only.  The yardsticks the single op was first given, rced_np.conv_bn_relu in float32 and
the same with K reversed, both add kh.kw tap-wise [pixels, cin] x [cin, cout] products: kh.kw roundings of a growing sum per
output.  The kernel the single op runs, csrc/kernels_generic.h conv_layer_generic, is ONE fmaf chain per output over all
K = kh.kw.cin products (read from its source: loops i, ci, j around acc = fmaf(x, w, acc)) -- the plainest fp32 form there
is, and it rounds the growing sum K times.  With products of independent sign the partial sum after k of K terms has variance
k/K of the result's, every rounding adds about (0.4 U)^2 of the partial sum squared, U = 2^-24, so the chain's error is about
0.4 U sqrt(sum_k k / K) = 0.29 U sqrt(K) of the result's rms, against 0.29 U sqrt(kh.kw) for the tap-wise sum: sqrt(cin) times
more where summation dominates (1 x 129, cin = 8: 0.29 U sqrt(1032) = 9.3 U of the output's rms, tap-wise 3.3 U).  Measured on
the device before this term: the 1 x 129 class at 0.65 of `all` and 1.12 of one `bin` bar, every other class within.  The term
is not taken from that closed form, which ignores zero padding, BatchNorm, the skip and the final rounding, but from a third
chain that does exactly this arithmetic on the host -- conv_bn_relu_f32(order="products"): one product at a time, float32 --
whose error joins the two tap-wise ones in the maximum: bar = MARGIN x max(taps, reversed, products).  It measures 1.0x (cin =
1) to 2.6x (rms) the tap-wise chains' error, below sqrt(cin) as derived, and test_single_layer_bars holds it there.  The whole
forward needs no such term: its yardstick A, the plain-C oracle in float32, already is a one-product-at-a-time chain.

If the device comes out over a bar, that is a finding, not a reason to widen: note the group, net, path and form; see whether
the comparator (CR-CED: v3_l2x6 = 0; R-CED output layer: final_x6 = 0) shares it; see whether the single-layer cases show it
for that layer class.  A bug is fixed; a consequence of the kernel's arithmetic is derived and added to the bar HERE, in writing,
as above and as test_train_adam_gpu.py does.  Widening MARGIN is not the remedy."""

import functools

import numpy as np

from oracle import rced_c, rced_np

MARGIN = 4
MIN_GROUP = 32
TILE = {"FullyCNN": 3, "FullyCNNV2": 3, "FullyCNNV3": 4}      # frames per tile of the fused kernels
VARIANT = {"FullyCNN": 1, "FullyCNNV2": 2, "FullyCNNV3": 3}
GROUP_SHAPES = [(3, 21), (2, 37), (5, 33), (1, 64)]            # ragged against tiles of 3 and of 4 frames
SHORT = "short"                                                 # B = 1, T = 1 .. 9, pooled into one case
SHORT_T = tuple(range(1, 10))
SHAPES = GROUP_SHAPES + [SHORT]
LOUD = 1e4
REGIMES = ("x1e-3", "x1", "x30", "zero_loud", "edge_bins", "channel_scales")
RMS_KINDS = ("bin", "slot", "edge", "last", "end", "chan")


def regimes_of(net_work):
    """channel_scales rescales CR-CED's 18- and 30-channel tensors (test_forward_gpu._scaled_inner_channels): CR-CED only."""
    return REGIMES if net_work == "FullyCNNV3" else REGIMES[:-1]


# ---------------------------------------------------------------------------------------------------------------- groups

def _pool(labels, names):
    """Merge neighbouring labels until every group holds MIN_GROUP values; -> (labels, names)."""
    counts = np.bincount(labels[labels >= 0], minlength=len(names))
    if counts.min() >= MIN_GROUP:
        return labels, list(names)
    new, out, first, acc = np.zeros(len(names), np.int64), [], 0, 0
    for i, c in enumerate(counts):
        acc += int(c)
        new[i] = len(out)
        if acc >= MIN_GROUP:
            out.append(names[i] if first == i else "%s..%s" % (names[first], names[i]))
            first, acc = i + 1, 0
    if acc:                                       # a remainder joins the last complete group
        assert out, "fewer than %d values in all: %s" % (MIN_GROUP, names)
        new[first:] = len(out) - 1
        out[-1] = "%s..%s" % (out[-1].split("..")[0], names[-1])
    return np.where(labels >= 0, new[np.maximum(labels, 0)], -1), out


def _flat(a, shape):
    return np.broadcast_to(a, shape).reshape(-1).astype(np.int64)


def forward_groups(n, t, tile, short=False):
    """kind -> (label of every element of an [n, t, 129, 1] tensor, -1 = in no group; names of the labels), unpooled."""
    shape, fr = (n, t, 129, 1), np.arange(t)
    g = {"bin": (_flat(np.arange(129)[None, None, :, None], shape), ["bin %d" % b for b in range(129)])}
    if short:
        g["end"] = (_flat((t - 1 - fr)[None, :, None, None], shape), ["frame T-%d" % (k + 1) for k in range(max(SHORT_T))])
        return g
    assert t >= 7, "the edge groups take 3 + 4 distinct frames"
    edge = np.full(t, -1)
    edge[:3] = (0, 1, 2)
    edge[t - 4:] = (3, 4, 5, 6)
    g["slot"] = (_flat((fr % tile)[None, :, None, None], shape), ["slot %d of %d" % (s, tile) for s in range(tile)])
    g["edge"] = (_flat(edge[None, :, None, None], shape), ["frame 0", "frame 1", "frame 2", "frame T-4", "frame T-3", "frame T-2", "frame T-1"])
    g["last"] = (_flat(np.where(fr >= tile * ((t - 1) // tile), 0, -1)[None, :, None, None], shape), ["last tile"])
    return g


def layer_groups(n, t, cout):
    shape = (n, t, 129, cout)
    return {"bin": (_flat(np.arange(129)[None, None, :, None], shape), ["bin %d" % b for b in range(129)]),
            "chan": (_flat(np.arange(cout)[None, None, None, :], shape), ["channel %d" % c for c in range(cout)])}


# ----------------------------------------------------------------------------------------------------------------- cases

class Case:
    """Parts (x, ref, scale), the two yardstick errors and the groups, all flat and concatenated over the parts."""

    def __init__(self, name, parts, groups):
        self.name = name
        self.xs = [p[0] for p in parts]
        self.refs = [p[1] for p in parts]
        self.chain = [p[2] for p in parts]        # yardstick A's outputs: what the host test puts its emulated defects on
        self.scales = [max(float(np.abs(p[1]).max()), 1e-30) for p in parts]
        self.groups = {}
        for kind in groups[0]:
            labels = np.concatenate([g[kind][0] for g in groups])
            self.groups[kind] = _pool(labels, groups[0][kind][1])
        self.yard = [self.errors([p[2 + i] for p in parts]) for i in range(len(parts[0]) - 2)]
        self.bars = self._bars()

    def errors(self, ys):
        """Outputs, one per part -> the flat error as a fraction of each part's max |ref|."""
        assert len(ys) == len(self.refs)
        out = []
        for y, ref, s in zip(ys, self.refs, self.scales):
            y = np.asarray(y, np.float64)
            assert y.shape == ref.shape, (y.shape, ref.shape)
            assert np.isfinite(y).all(), "%s: non-finite output" % self.name
            out.append(((y - ref) / s).reshape(-1))
        return np.concatenate(out)

    def measures(self, e):
        """kind -> one value per group."""
        m = {"all": np.array([np.sqrt(np.mean(e * e))]), "max": np.array([np.abs(e).max()])}
        for kind, (labels, names) in self.groups.items():
            inside = labels >= 0
            s = np.bincount(labels[inside], weights=(e * e)[inside], minlength=len(names))
            m[kind] = np.sqrt(s / np.bincount(labels[inside], minlength=len(names)))
        return m

    def yardsticks(self):
        ms = [self.measures(e) for e in self.yard]
        y = {k: np.maximum.reduce([m[k] for m in ms]) for k in ms[0]}
        return {k: np.maximum(v, y["all"][0]) if k in RMS_KINDS else v for k, v in y.items()}

    def spread(self):
        """kind -> the largest ratio, over the kind's groups, between the first two chains (rms groups floored as the yardstick is)."""
        a, b = (self.measures(e) for e in self.yard[:2])
        floor, out = max(a["all"][0], b["all"][0]), {}
        for k in a:
            u, v = (np.maximum(m[k], floor) if k in RMS_KINDS else m[k] for m in (a, b))
            out[k] = float(np.maximum(u / v, v / u).max())
        return out

    def _bars(self):
        return {k: MARGIN * v for k, v in self.yardsticks().items()}

    def fractions(self, ys=None, e=None):
        """kind -> (the worst fraction of the bar over the kind's groups, the name of that group)."""
        m = self.measures(self.errors(ys) if e is None else e)
        out = {}
        for kind, v in m.items():
            f = v / np.maximum(self.bars[kind], 1e-300)
            i = int(np.argmax(f))
            out[kind] = (float(f[i]), self.groups[kind][1][i] if kind in self.groups else kind)
        return out


def chains(net_work, w, x):
    """(ref fp64, C fp32, numpy fp32) of one input."""
    return (rced_c.forward(net_work, w, x, np.float64), rced_c.forward(net_work, w, x, np.float32),
            rced_np.forward(net_work, w, x, np.float32))


@functools.lru_cache(maxsize=None)
def weights_of(net_work, regime):
    """One set of weights per net and regime (so a device model is made once per test), another seed in each."""
    seed = 300 + 10 * VARIANT[net_work] + REGIMES.index(regime)
    if regime == "channel_scales":
        from test_forward_gpu import _scaled_inner_channels
        return _scaled_inner_channels(rced_np.make_weights(net_work, seed=seed), np.random.default_rng(seed))
    if regime == "edge_bins" and net_work == "FullyCNNV3":
        from test_v3_bin128 import _edge_weights
        return _edge_weights(seed)
    return rced_np.make_weights(net_work, seed=seed)


def input_of(regime, n, t, seed):
    if regime == "edge_bins":
        from test_v3_bin128 import _edge_input
        return _edge_input(n, t, seed, 30.0)
    x = rced_np.make_input(n, t, seed=seed)
    if regime == "zero_loud":
        # a frame of exact zeros beside a frame LOUD times the rest, every eighth frame, so that every group keeps MIN_GROUP values
        # that carry weight; utterance 0 ends on such a pair (its last, ragged tile), the others are shifted by three frames each
        for i in range(n):
            for z in range((t - 2 + 3 * i) % 8 if t > 9 else (t - 1) // 2, t, 8):
                if t > 1:
                    x[i, z] = 0.0
                x[i, min(z + 1, t - 1)] *= np.float32(LOUD)
    elif regime.startswith("x"):
        x *= np.float32(float(regime[1:]))
    return x


@functools.lru_cache(maxsize=None)
def case(net_work, regime, shape):
    """Once per (net, regime, shape), shared by every path and form that runs it, and left unchanged."""
    w, tile = weights_of(net_work, regime), TILE[net_work]
    seed = 7000 + 1000 * VARIANT[net_work] + 100 * REGIMES.index(regime)
    dims = [(1, t) for t in SHORT_T] if shape == SHORT else [shape]
    parts, groups = [], []
    for n, t in dims:
        x = input_of(regime, n, t, seed + 10 * n + t)
        parts.append((x,) + chains(net_work, w, x))
        groups.append(forward_groups(n, t, tile, short=shape == SHORT))
    return Case("%s %s %s" % (net_work, regime, shape), parts, groups)


# --------------------------------------------------------------------------------------------------------- single layers

LAYER_CLASSES = ((8, 13, 1, 12), (1, 11, 12, 16), (1, 5, 15, 19), (1, 9, 30, 8), (1, 129, 8, 1), (1, 7, 25, 23))   # kh, kw, cin, cout
LAYER_NT = (2, 9)


def conv_bn_relu_f32(x, k, b, bn, skip, act, order="taps"):
    """rced_np.conv_bn_relu in float32.  order: "taps" = as it stands (one [pixels, cin] x [cin, cout] product per tap, added
    tap by tap); "reversed" = the same with K -- the taps, and the input channels inside a tap -- walked last term first;
    "products" = one product at a time over all K = kh kw cin of them (see layer_case)."""
    if order == "taps":
        return rced_np.conv_bn_relu(x, k, b, bn, skip, act, np.float32)
    x, k = np.asarray(x, np.float32), np.asarray(k, np.float32)
    (n, t, f, _), (kh, kw, _, cout) = x.shape, k.shape
    xp = np.zeros((n, t + kh - 1, f + kw - 1, x.shape[3]), np.float32)
    xp[:, rced_np.same_pad(kh)[0]:rced_np.same_pad(kh)[0] + t, rced_np.same_pad(kw)[0]:rced_np.same_pad(kw)[0] + f] = x
    y = np.zeros((n, t, f, cout), np.float32)
    for i in reversed(range(kh)):
        for j in reversed(range(kw)):
            if order == "reversed":
                y += np.ascontiguousarray(xp[:, i:i + t, j:j + f, ::-1]) @ np.ascontiguousarray(k[i, j, ::-1])
            else:
                for c in range(x.shape[3]):
                    y += xp[:, i:i + t, j:j + f, c:c + 1] * k[i, j, c]
    y += np.asarray(b, np.float32)
    if bn is not None:
        y = rced_np.batch_norm_inference(y, *bn, dtype=np.float32)
    if skip is not None:
        y = y + np.asarray(skip, np.float32)
    return np.maximum(y, 0) if act else y


@functools.lru_cache(maxsize=None)
def layer_case(cls, full):
    """One conv_bn_relu of shape class `cls`, with BatchNorm, skip and ReLU (`full`) or the bare convolution;
    -> (Case, kernel, bias, the four BatchNorm vectors)."""
    kh, kw, cin, cout = LAYER_CLASSES[cls]
    n, t = LAYER_NT
    rng = np.random.default_rng(50 + cls)
    x = rng.standard_normal((n, t, 129, cin)).astype(np.float32)
    k = (rng.standard_normal((kh, kw, cin, cout)) / np.sqrt(kh * kw * cin)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, cout).astype(np.float32)
    bn = tuple(a.astype(np.float32) for a in (rng.uniform(0.5, 1.5, cout), rng.uniform(-0.1, 0.1, cout), rng.normal(0, 0.1, cout),
                                              rng.uniform(0.5, 1.5, cout)))
    skip = rng.standard_normal((n, t, 129, cout)).astype(np.float32)
    args = (k, b, bn, skip, True) if full else (k, b, None, None, False)
    ref = rced_np.conv_bn_relu(x, *args)
    part = ((x, skip if full else None), ref) + tuple(conv_bn_relu_f32(x, *args, order=o) for o in ("taps", "reversed", "products"))
    return Case("conv_bn_relu %s %s" % (LAYER_CLASSES[cls], "BN+skip+ReLU" if full else "bare"), [part], [layer_groups(n, t, cout)]), k, b, bn
