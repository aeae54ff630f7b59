"""The optimizer step pinned through the public API: train::adam_step and the host's bias-corrected lr_t
(train_api.hip: optimizer_step) against TF's form of Adam with float32 constants, evaluated in float64.

Per net, on an unscreened 2 x 3 batch: seeded Adam slots are loaded (m of both signs over six decades, v over 1e-16 .. 1,
a tenth of the entries m = v = 0), the step count is set to t, the learning rate explicitly, and ONE train_step runs.  The
device's own gradient g is the input of the expected values, which isolates the optimizer from gradient error -- and
covers the eps regime for free: the biases in front of BatchNorm have g at rounding-noise scale.

    m' = B1 m + (1 - B1) g        v' = B2 v + (1 - B2) g^2        lr_t = float32(lr sqrt(1 - B2^(t+1)) / (1 - B1^(t+1)))
    p' = p - lr_t m' / (sqrt(v') + EPS)          B1, B2, EPS = float32(0.9), float32(0.999), float32(1e-8); 1 - B in float32

The bars are derived, not measured.  Every fp32 operation rounds by at most U = 2^-24 of its result; HIP's default fp32
sqrtf is good to 1 ulp and its division to 2.5 ulp.
  * m' and v': two (three) roundings per term and one for the sum, each at most U of a partial result that is at most the
    sum of the terms' magnitudes: within 4 U of that sum.
  * the update p - p': sqrtf, + EPS, the division and the product with lr_t are about 5 U of the update; lr_t itself
    may sit one float32 off the test's (two libms' pow); v' as held above adds 2 U (the root halves its 4 U).  Within 16 U of
    the update's own magnitude, plus U |p'| for the final subtraction.  "Of its own magnitude" holds for the update as
    the device formed it, from ITS m' and v' -- which the first bar has already pinned to float64 -- so the expected update
    is evaluated at the device's m' and v'.  (From the float64 m' instead, an entry where B1 m and (1 - B1) g nearly
    cancel carries m's 4 U of the TERMS into an update that is far smaller than the terms: no multiple of the update's
    own magnitude bounds that.)  The whole chain from the loaded slots is held as well, with exactly that term added:
    16 U |update| + U |p'| + lr_t 4 U (|B1 m| + |(1 - B1) g|) / (sqrt(v') + EPS).
test_the_bars_pass_fp32_adam_and_see_each_wrong_form shows on the CPU that float32 arithmetic passes these bars with
room and that a wrong beta2, an eps inside the root, and a wrong bias correction miss them.

TF r1's AdamOptimizer keeps beta^t as float32 powers and epsilon outside the root; the device's double pow of the
float32 constants differs from float32 powers by less than the bars see.  oracle/train_ref.py's train_step uses the
double constants 0.9 / 0.999: test_lr_t_of_the_float32_constants_is_the_restatements_to_1e_5 documents that known
difference (at most 4e-6 relative, at t = 999), so nobody "fixes" either side later."""

import ctypes
import functools

import numpy as np
import pytest

from conftest import NETS
from oracle import layers as L, rced_np, train_ref

gpu = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -140                           # room for a result in the subnormal range, where a rounding is absolute (2^-150)
F32 = lambda c: np.float64(np.float32(c))   # noqa: E731
B1, B2, EPS = F32(0.9), F32(0.999), F32(1e-8)
OMB1, OMB2 = np.float64(np.float32(1) - np.float32(0.9)), np.float64(np.float32(1) - np.float32(0.999))
MOMENTUM = F32(0.99)                         # kBnMomentum
STEPS = [0, 1, 9, 999, 10 ** 6]
LR = 3.7e-4


def lr_t_of(lr, t):
    """After t earlier steps: the step's bias-corrected rate, as a float32."""
    n = float(t + 1)
    return np.float64(np.float32(F32(lr) * np.sqrt(1.0 - B2 ** n) / (1.0 - B1 ** n)))


def expected(p, g, m, v, t, lr):
    """float64 (m', v', terms of m', terms of v', lr_t) from float32 inputs."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    return B1 * m + OMB1 * g, B2 * v + OMB2 * g * g, np.abs(B1 * m) + np.abs(OMB1 * g), B2 * v + OMB2 * g * g, lr_t_of(lr, t)


def bar_fractions(p, g, m, v, t, lr, p1, m1, v1):
    """The worst observed fraction of each bar: (m', v', update at the device's m' and v', update from the loaded slots)."""
    m_exp, v_exp, m_terms, v_terms, lr_t = expected(p, g, m, v, t, lr)
    p, p1, m1, v1 = (np.asarray(a, np.float64) for a in (p, p1, m1, v1))
    assert np.isfinite(p1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
    f_m = np.abs(m1 - m_exp) / (4 * U * m_terms + TINY)
    f_v = np.abs(v1 - v_exp) / (4 * U * v_terms + TINY)
    upd = p - p1                                            # exact in float64
    at_dev = lr_t * m1 / (np.sqrt(v1) + EPS)
    f_u = np.abs(upd - at_dev) / (16 * U * np.abs(at_dev) + U * np.abs(p1) + TINY)
    chain = lr_t * m_exp / (np.sqrt(v_exp) + EPS)
    f_c = np.abs(upd - chain) / (16 * U * np.abs(chain) + U * np.abs(p1) + lr_t * 4 * U * m_terms / (np.sqrt(v_exp) + EPS) + TINY)
    return float(f_m.max()), float(f_v.max()), float(f_u.max()), float(f_c.max())


def seeded_slots(shapes, seed):
    """m: both signs, |m| over 1e-6 .. 1; v: 1e-16 .. 1; a tenth of the entries m = v = 0."""
    rng = np.random.default_rng(seed)
    m, v = {}, {}
    for name, shape in shapes:
        mm = rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 0, shape)
        vv = 10.0 ** rng.uniform(-16, 0, shape)
        zero = rng.random(shape) < 0.1
        m[name], v[name] = np.where(zero, 0, mm).astype(np.float32), np.where(zero, 0, vv).astype(np.float32)
    return m, v


# ---- on the CPU: the bars and the known difference of the constants ------------------------------------------------

def adam_fp32(p, g, m, v, lr_t, b1=np.float32(0.9), b2=np.float32(0.999), eps=np.float32(1e-8), eps_inside=False):
    """train::adam_step's expressions in numpy float32 (no contraction)."""
    one = np.float32(1)
    m1 = b1 * m + (one - b1) * g
    v1 = b2 * v + (one - b2) * g * g
    den = np.sqrt(v1 + eps) if eps_inside else np.sqrt(v1) + eps
    return p - np.float32(lr_t) * m1 / den, m1, v1


def test_the_bars_pass_fp32_adam_and_see_each_wrong_form():
    rng = np.random.default_rng(5)
    shapes = [("a", (40000,))]
    m, v = (d["a"] for d in seeded_slots(shapes, 6))
    p = rng.standard_normal(40000).astype(np.float32)
    g = (rng.standard_normal(40000) * 10.0 ** rng.uniform(-9, 1, 40000)).astype(np.float32)
    g[:4000] *= np.float32(1e-8)             # rounding-noise gradients: the eps regime
    g[:40] = 0
    for t in STEPS:
        good = bar_fractions(p, g, m, v, t, LR, *adam_fp32(p, g, m, v, lr_t_of(LR, t)))
        print("\n[adam bars] t = %d, float32 arithmetic: worst fraction of the bars m' %.2f v' %.2f update %.2f chain %.2f" % ((t,) + good))
        assert max(good) < 1.0, (t, good)
        wrong_b2 = bar_fractions(p, g, m, v, t, LR, *adam_fp32(p, g, m, v, lr_t_of(LR, t), b2=np.float32(0.99)))
        assert wrong_b2[1] > 1.0, t
        inside = bar_fractions(p, g, m, v, t, LR, *adam_fp32(p, g, m, v, lr_t_of(LR, t), eps_inside=True))
        assert inside[2] > 1.0 and inside[3] > 1.0, t
        if 0 < t < 10 ** 6:                  # (at t = 0 an uncorrected beta2 power is the right one; at 1e6 both powers are 0)
            late = bar_fractions(p, g, m, v, t, LR, *adam_fp32(p, g, m, v, lr_t_of(LR, t - 1)))     # beta^t for beta^(t+1)
            assert late[2] > 1.0 and late[3] > 1.0, t
        if t < 10 ** 6:
            none = bar_fractions(p, g, m, v, t, LR, *adam_fp32(p, g, m, v, np.float32(LR)))          # no bias correction
            assert none[2] > 1.0, t


def test_lr_t_of_the_float32_constants_is_the_restatements_to_1e_5():
    for t in STEPS:
        n = t + 1
        double_constants = LR * np.sqrt(1 - train_ref.BETA2 ** n) / (1 - train_ref.BETA1 ** n)     # train_ref.train_step
        assert abs(lr_t_of(LR, t) - double_constants) <= 1e-5 * double_constants, t


# ---- on the device ----------------------------------------------------------------------------------------------------

def batch():
    return rced_np.make_input(2, 3, seed=301), rced_np.make_input(2, 3, seed=302)


def raw_slots(tr):
    """The whole m and v blobs as they cross the ABI (optimizer_state hides the entries of the moving statistics)."""
    from fullycnnspeechenhancement_amd import _lib, spec
    n = tr._blob_n
    mb, vb = np.empty(n, np.float32), np.empty(n, np.float32)
    step = ctypes.c_longlong()
    fp = ctypes.POINTER(ctypes.c_float)
    _lib.check(_lib.load().rced_train_get_state(tr._h, mb.ctypes.data_as(fp), vb.ctypes.data_as(fp), n, ctypes.byref(step)))
    moving, o = np.zeros(n, bool), 0
    for name, shape in spec.variable_shapes(tr.variant):
        k = int(np.prod(shape))
        moving[o:o + k] = "moving_" in name
        o += k
    return mb, vb, moving


@functools.lru_cache(maxsize=None)
def device_sums(net_work):
    """Once per net: the device's own fp64 (sum z, sum z^2) per BatchNorm channel and the pixel count of the batch's forward,
    from the exchange buffer of a gradient-only pass on a second trainer (the same kernels on the same data: the same bits
    the step stashes for its epilogue)."""
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    x, y = batch()
    tr = FullyCNNTrainer(net_work, batch_size=4, lr=1e-3, weights=rced_np.make_weights(net_work, seed=13))
    try:
        tr.grad_step(x, y)
        s = tr.exchange_tensors()[1].cpu().numpy()
    finally:
        tr.close()
    out, o = {}, 0
    for l in L.layers_for(net_work):
        if l.use_norm:
            out[l.scope] = (s[o:o + 2 * l.cout:2].copy(), s[o + 1:o + 2 * l.cout:2].copy(), float(s[o + 2 * l.cout]))
            o += 2 * l.cout + 1
    return out


@gpu
@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("net_work,tag,variant", NETS)
def test_one_adam_step_from_loaded_slots(net_work, tag, variant, t, built, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer
    w = rced_np.make_weights(net_work, seed=13)
    x, y = batch()
    shapes = [(k, w[k].shape) for k in train_ref.trainable_names(net_work)]
    m0, v0 = seeded_slots(shapes, 100 + variant)
    tr = FullyCNNTrainer(net_work, batch_size=4, lr=1e-3, weights=w)
    try:
        tr.load_optimizer_state(m0, v0, t)
        tr.lr = LR                                          # load_optimizer_state set it from the Noam schedule
        p0 = tr.variables()
        _, _, step = tr.train_step(x, y)
        g, p1 = tr.gradients(), tr.variables()
        m1, v1, step_state = tr.optimizer_state()
        mb, vb, moving = raw_slots(tr)
    finally:
        tr.close()
    assert step == step_state == t + 1
    # what crosses the ABI has the reference's own (unpadded) shapes: R-CED V2 trains odd channel counts even-padded inside
    for d in (p0, p1, g):
        assert {k: a.shape for k, a in d.items()} == {k: a.shape for k, a in w.items()}
    for d in (m1, v1):
        assert {k: a.shape for k, a in d.items()} == dict(shapes)
    for k in w:
        assert np.array_equal(p0[k], w[k]), k
    worst, still = np.zeros(4), 0
    for name, _ in shapes:
        worst = np.maximum(worst, bar_fractions(p0[name], g[name], m0[name], v0[name], t, LR, p1[name], m1[name], v1[name]))
        # 0 / (0 + eps): an entry with nothing in its slots and no gradient stays where it is
        idle = (m0[name] == 0) & (v0[name] == 0) & (g[name] == 0)
        still += int(idle.sum())
        assert np.array_equal(p1[name][idle], p0[name][idle]) and not m1[name][idle].any() and not v1[name][idle].any(), name
    with capsys.disabled():
        print("\n[adam] %s t = %d: worst fraction of the bars m' %.3f v' %.3f update %.3f chain %.3f; %d idle entries stayed put"
              % ((net_work, t) + tuple(worst) + (still,)))
    assert worst.max() < 1.0, worst
    # Adam touches no moving statistic, in the variables or in the slots: the moving statistics are exactly step_epilogue's
    # update (train::moving_update, fp64 rounded once to float32) of the device's own sums
    assert not mb[moving].any() and not vb[moving].any()
    for scope, (s1, s2, px) in device_sums(net_work).items():
        mean = s1 / px
        var = np.maximum(s2 / px - mean * mean, 0.0)
        unbiased = var * px / (px - 1.0)
        for name, batch_stat in (("moving_mean", mean), ("moving_variance", unbiased)):
            key = scope + "/batch_norm/" + name
            want = MOMENTUM * np.asarray(w[key], np.float64) + (1.0 - MOMENTUM) * batch_stat
            assert np.all(np.abs(p1[key] - want) <= 2.0 ** -23 * np.abs(want)), key
