"""The fp32 forward held to the bars of tests/forward_bars.py: MARGIN x the error of two fp32 restatements against the fp64
oracle, per group -- the whole tensor (rms and largest element), every frequency bin, every slot of the fused kernels' tile,
every frame at the time edges, each utterance's last (ragged) tile; for the short set (B = 1, T = 1 .. 9, pooled) every
frame index counted from the end.  All three nets; paths "layerwise" and "auto" (R-CED's fused kernel on its three-frame
tiles: the one-frame latency form is held bit-identical to it in test_forward_gpu.py); CR-CED's fused kernel in both forms,
v3_l2x6 = 3 (the product) and 0 (the fp32-MFMA comparator).  Input regimes: synthetic magnitudes x 1e-3, x 1, x 30; exact zero
frames beside frames x 1e4; bins 120 .. 128 loud (CR-CED: with the raised right-hand taps of test_v3_bin128.py); CR-CED's
per-channel scales 1e-4 .. 1e4 of test_three_part_products_on_adversarial_magnitudes.  The yardsticks are computed per case, so
no regime has a bar of its own.  conftest.check_parity is held as well.

The single op is held the same way (groups: tensor, largest element, bin, output channel; yardsticks: the numpy op in
float32 and the same with K walked backwards) over the six layer classes of test_single_op_conv_bn_relu_known_answers, with
BatchNorm + skip + ReLU and bare: the one place where a layer class is seen alone.

Measured, one run on one MI355X: the table in DESIGN.md next to "The bar, as the tests state it"."""

import numpy as np
import pytest

import forward_bars as fb
from conftest import check_parity

pytestmark = pytest.mark.gpu

# (net, path, v3_l2x6 or None)
RUNS = [(net, path, None) for net in ("FullyCNN", "FullyCNNV2") for path in ("layerwise", "auto")] + \
       [("FullyCNNV3", "layerwise", None), ("FullyCNNV3", "auto", 3), ("FullyCNNV3", "auto", 0)]
CASES = [run + (regime,) for run in RUNS for regime in fb.regimes_of(run[0])]
WORST = {}          # (net, path, form) -> kind -> (fraction, group, case)


def _model(net_work, regime, path, form):
    from fullycnnspeechenhancement_amd import model as M
    cls = {1: M.FullyCNNSEModel, 2: M.FullyCNNSEModelV2, 3: M.FullyCNNSEModelV3}[fb.VARIANT[net_work]]
    m = cls(False, weights=fb.weights_of(net_work, regime), device=0)
    m.set_path(path)
    if path == "auto":
        assert m.get_option("has_fused") == 1
        if form is not None:
            m.set_option("v3_l2x6", form)
            assert m.get_option("v3_l2x6") == form
        else:
            m.set_option("latency_form", 0)     # the three-frame tiles the slot and last-tile groups are cut for
    return m


def _run_name(net_work, path, form):
    return "%s %s%s" % (net_work, path, "" if form is None else " v3_l2x6=%d" % form)


def _hold(case, ys, worst, what):
    """Every group of the case against its bar; -> the failures, each naming its group."""
    failed = []
    for kind, (frac, group) in case.fractions(ys).items():
        if frac > worst.get(kind, (0.0,))[0]:
            worst[kind] = (frac, group, case.name)
        if not frac <= 1.0:
            failed.append("%s | %s: group `%s` (%s) at %.2f of its bar (%.3e of the scale)" % (what, case.name, kind, group, frac, case.bars[kind].max()))
    return failed


def _line(worst):
    return "  ".join("%s %.2f" % (k, v[0]) for k, v in worst.items())


@pytest.mark.parametrize("net_work,path,form,regime", CASES, ids=["%s-%s" % (_run_name(*c[:3]).replace(" ", "-"), c[3]) for c in CASES])
def test_forward_within_the_bars_of_the_fp32_restatements(net_work, path, form, regime, built, capsys):
    m = _model(net_work, regime, path, form)
    what, worst, failed = _run_name(net_work, path, form), {}, []
    for shape in fb.SHAPES:
        case = fb.case(net_work, regime, shape)
        ys = [np.asarray(m(x)) for x in case.xs]
        for y, ref in zip(ys, case.refs):
            assert y.dtype == np.float32
            check_parity(y, ref, what="%s %s" % (what, case.name))
        failed += _hold(case, ys, worst, what)
    total = WORST.setdefault((net_work, path, form), {})
    for kind, v in worst.items():
        if v[0] > total.get(kind, (0.0,))[0]:
            total[kind] = v
    with capsys.disabled():
        print("\n[forward bars] %-32s %-14s worst fraction of the bar: %s" % (what, regime, _line(worst)))
    assert not failed, "\n".join(failed)


def test_worst_fractions_per_net_path_and_form(capsys):
    """Prints what the cases above measured (those that ran in this session), per net, path and form, with the case and group."""
    with capsys.disabled():
        print()
        for (net_work, path, form), worst in WORST.items():
            print("[forward bars, worst] %-32s %s" % (_run_name(net_work, path, form), _line(worst)))
            for kind, (frac, group, name) in worst.items():
                print("[forward bars, worst]     %-5s %.2f  %s, %s" % (kind, frac, group, name))
    for run, worst in WORST.items():
        assert all(v[0] <= 1.0 for v in worst.values()), (run, worst)


@pytest.mark.parametrize("full", [True, False], ids=["bn_skip_relu", "bare"])
@pytest.mark.parametrize("cls", range(len(fb.LAYER_CLASSES)), ids=["%dx%d_%dto%d" % c for c in fb.LAYER_CLASSES])
def test_single_op_within_the_bars_of_the_fp32_restatements(cls, full, built, capsys):
    import torch
    from fullycnnspeechenhancement_amd import conv_bn_relu
    kh, kw, cin, cout = fb.LAYER_CLASSES[cls]
    case, k, b, bn = fb.layer_case(cls, full)
    x, skip = case.xs[0]
    p = {"s/kernel": k, "s/bias": b, "s/batch_norm/gamma": bn[0], "s/batch_norm/beta": bn[1],
         "s/batch_norm/moving_mean": bn[2], "s/batch_norm/moving_variance": bn[3]}
    dev = torch.device("cuda:0")
    if full:
        y = conv_bn_relu(torch.from_numpy(x).to(dev), cout, (kh, kw), (1, 1), False, scope="s",
                         skip_input=torch.from_numpy(skip).to(dev), params=p)
    else:
        y = conv_bn_relu(torch.from_numpy(x).to(dev), cout, (kh, kw), (1, 1), False, use_norm=False, use_act=False, scope="s", params=p)
    y = y.cpu().numpy()
    check_parity(y, case.refs[0], what=case.name)
    worst = {}
    failed = _hold(case, [y], worst, "single op")
    with capsys.disabled():
        print("\n[forward bars] %-60s worst fraction of the bar: %s" % (case.name, _line(worst)))
    assert not failed, "\n".join(failed)
