"""GPU tests of the training step with a wave objective (rced_train_step_wave / rced_train_grad_wave, FullyCNNTrainer(objective=)):
loss and every gradient of every layer against oracle/train_ref.TrainRef in float64 composed with the torch restatement of the
wave terms (tests/wave_loss_np.torch_terms), on an input screened as test_train_gpu.screened_input does, held to the bar
test_all_gradients_tight_on_inputs_without_relu_ties holds the spectral step to (1e-4 of a tensor's largest entry, the loss to
1e-5); the plain objective bit for bit; accumulation; a short descent; the refusals; reproducibility.
N = 2, T = 5, lengths (700, 640): F = (5, 4), one padded frame, a range that ends inside a hop.
Measured: loss within 9.3e-8, the worst gradient tensor 8.1e-6 (CR-CED, CE3_decode/batch_norm/gamma) and 1.5e-6 (R-CED V1) of its
largest entry -- under a tenth of the bar."""

import numpy as np
import pytest

import wave_loss_np as wl
from oracle import rced_np, train_ref
from test_train_gpu import TIGHT, screened_input

pytestmark = pytest.mark.gpu

N, T, BATCH = 2, 5, 4
LENGTHS = (700, 640)
FRAMES = tuple(wl.num_frames(v) for v in LENGTHS)
WEIGHTS = (1.0, 0.5, 1.0)                       # spectral, wave_sse, si_sdr: every term in one step
CASES = {}


def case(net_work):
    """Weights, the screened input, the target, the phase, the clean rows and the float64 loss and gradients: once per net."""
    if net_work in CASES:
        return CASES[net_work]
    import torch
    variant = {"FullyCNN": 1, "FullyCNNV2": 2, "FullyCNNV3": 3}[net_work]
    w = rced_np.make_weights(net_work, seed=11)
    ref = train_ref.TrainRef(net_work, w, batch_size=BATCH)
    x, seed = screened_input(ref, N, T, 6000 + 100 * variant)
    y = rced_np.make_input(N, T, seed=79 + variant)
    rng = np.random.default_rng(40 + variant)
    phase = np.exp(2j * np.pi * rng.random((N, T, 129))).astype(np.complex64)
    for k in ref.m:
        ref.vars[k].grad = None
    pred, _ = ref.forward_train(x)
    clean = np.zeros((N, max(LENGTHS)), np.float32)
    for n in range(N):                           # 0.7 of what the untrained net rebuilds, plus noise at half its rms
        yy = wl.rebuild(pred[n, :, :, 0].detach().numpy(), phase[n], FRAMES[n])[:LENGTHS[n]]
        clean[n, :LENGTHS[n]] = 0.7 * yy + 0.5 * np.sqrt(np.mean(yy * yy)) * rng.standard_normal(LENGTHS[n])
    spectral = ((torch.as_tensor(y).to(pred.dtype) - pred) ** 2).sum()
    sse, si = 0.0, 0.0
    for n in range(N):
        a, b, valid = wl.torch_terms(pred[n, :, :, 0], phase[n], clean[n], LENGTHS[n], FRAMES[n], True)
        assert valid == 1.0
        sse, si = sse + a, si + b
    loss = (WEIGHTS[0] * spectral + WEIGHTS[1] * sse - WEIGHTS[2] * si) / BATCH
    loss.backward()
    grads = {k: ref.vars[k].grad.clone().numpy() for k in ref.m}
    CASES[net_work] = (w, x, y, phase, clean, loss.item(), (spectral.item(), sse.item(), si.item()), grads)
    return CASES[net_work]


def on_device(phase, clean):
    import torch
    return torch.tensor(phase, device="cuda"), torch.tensor(clean, device="cuda"), list(LENGTHS)


def trainer(net_work, w, objective="default", **kw):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, audio
    if objective == "default":
        objective = audio.WaveObjective(*WEIGHTS)
    return FullyCNNTrainer(net_work, batch_size=BATCH, lr=1e-4, weights=w, objective=objective, **kw)


@pytest.mark.parametrize("net_work", ["FullyCNNV3", "FullyCNN"])
def test_loss_and_every_gradient_against_the_float64_composition(net_work, built, capsys):
    w, x, y, phase, clean, loss_ref, parts_ref, grads_ref = case(net_work)
    tr = trainer(net_work, w)
    loss, _, step = tr.train_step(x, y, wave=on_device(phase, clean))
    assert step == 1
    g = tr.gradients()
    worst = {}
    for name, gr in grads_ref.items():
        if name.endswith("/bias") and (name[:-5] + "/batch_norm/gamma") in grads_ref:
            assert np.abs(g[name]).max() <= 1e-4 * max(np.abs(g[name[:-5] + "/kernel"]).max(), 1e-30), name
            continue
        worst[name] = np.abs(g[name].astype(np.float64) - gr).max() / np.abs(gr).max()
    k = max(worst, key=worst.get)
    with capsys.disabled():
        print("\n[train wave parity] %s: loss %.8e (ref %.8e, rel err %.2e), parts %s (ref %s), worst gradient %s %.2e of its max (%d tensors)"
              % (net_work, loss, loss_ref, abs(loss - loss_ref) / abs(loss_ref), tr.loss_parts, parts_ref, k, worst[k], len(worst)))
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref)
    for got, want in zip(tr.loss_parts, parts_ref):
        assert abs(got - want) <= 1e-5 * abs(want)
    assert worst[k] < TIGHT, (k, worst[k])
    tr.close()


def test_the_plain_objective_is_train_step_bit_for_bit(built):
    from fullycnnspeechenhancement_amd import audio
    w, x, y = case("FullyCNNV3")[:3]
    outs = []
    for objective in (None, audio.WaveObjective(1, 0, 0), audio.WaveObjective()):
        tr = trainer("FullyCNNV3", w, objective)
        loss = tr.train_step(x, y)[0]
        outs.append((loss, tr.gradients(), tr.variables()))
        tr.close()
    for loss, g, v in outs[1:]:
        assert loss == outs[0][0]
        assert all(np.array_equal(g[k], outs[0][1][k]) for k in g) and all(np.array_equal(v[k], outs[0][2][k]) for k in v)


def test_a_spectral_weight_alone_scales_the_plain_loss(built):
    from fullycnnspeechenhancement_amd import audio
    w, x, y = case("FullyCNNV3")[:3]
    a, b = trainer("FullyCNNV3", w, None), trainer("FullyCNNV3", w, audio.WaveObjective(2, 0, 0))
    la, lb = a.train_step(x, y)[0], b.train_step(x, y)[0]
    assert lb == 2 * la and b.loss_parts == (la * BATCH, 0.0, 0.0)
    ga, gb = a.gradients(), b.gradients()
    assert all(np.array_equal(2 * ga[k], gb[k]) for k in ga)              # a power of two: the same bits, one exponent up
    a.close()
    b.close()


def test_accumulation_is_the_ordered_sum_of_its_shards(built):
    import torch
    w, x, y, phase, clean = case("FullyCNNV3")[:5]
    wave = on_device(phase, clean)
    acc, one = trainer("FullyCNNV3", w, accumulate=2), trainer("FullyCNNV3", w)
    loss = acc.train_step(x, y, wave=wave)[0]
    summed = acc.exchange_tensors()[0].clone()
    parts, losses, gs = [], [], []
    for a, b in ((0, 1), (1, 2)):
        losses.append(one.grad_step(x[a:b], y[a:b], wave=(wave[0][a:b], wave[1][a:b], wave[2][a:b])))
        parts.append(one.loss_parts)
        gs.append(one.exchange_tensors()[0].clone())
    assert loss == losses[0] + losses[1]
    assert acc.loss_parts == tuple(p + q for p, q in zip(*parts))
    assert torch.equal(summed, gs[0] + gs[1])
    # the sharded form with the shards named is the same step
    two = trainer("FullyCNNV3", w)
    assert two.train_step_sharded([(x[a:b], y[a:b], (wave[0][a:b], wave[1][a:b], wave[2][a:b])) for a, b in ((0, 1), (1, 2))])[0] == loss
    assert torch.equal(two.exchange_tensors()[0], summed)
    for tr in (acc, one, two):
        tr.close()


def test_thirty_steps_of_spectral_plus_si_sdr_descend(built, capsys):
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, audio
    w, x, y, phase, clean = case("FullyCNNV3")[:5]
    tr = FullyCNNTrainer("FullyCNNV3", batch_size=BATCH, lr=1e-3, weights=w, objective=audio.WaveObjective(1.0, 0.0, 1.0))
    wave = on_device(phase, clean)
    losses = [tr.train_step(x, y, wave=wave)[0] for _ in range(30)]
    with capsys.disabled():
        print("\n[train wave descent] loss %.5f -> %.5f over 30 steps; si_sdr sum %.3f dB at the end" % (losses[0], losses[-1], tr.loss_parts[2]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0] and tr.global_step == 30
    tr.close()


def test_train_takes_the_phase_and_the_clean_rows_from_the_loader(built):
    """An epoch over a paired corpus is the steps by hand with wave_of_batch's tuple; its phase comes from an STFT of the
    mixture's rows whose magnitudes are the loader's batch, bit for bit."""
    import torch
    from fullycnnspeechenhancement_amd import FullyCNNTrainer, audio, loader
    from fullycnnspeechenhancement_amd.trainer import wave_of_batch
    rng = np.random.default_rng(5)
    clean = [(3000 * rng.standard_normal(n)).astype(np.int16) for n in (1500, 1300, 1100, 900)]
    mixes = [np.clip(s.astype(np.int32) + rng.integers(-1000, 1000, len(s)), -32768, 32767).astype(np.int16) for s in clean]
    w = rced_np.make_weights("FullyCNNV3", seed=42)
    objective = audio.WaveObjective(1.0, 0.5, 0.1)

    def make_loader():
        np.random.seed(3)
        ds = loader.DataSet(loader.Corpus.from_arrays(clean), mix=loader.Corpus.from_arrays(mixes))
        return loader.DataLoader(ds, 2, sampler=loader.Sampler(ds, 2))

    class Recording(FullyCNNTrainer):
        def fit_step(self, x, y, wave=None):
            out = FullyCNNTrainer.fit_step(self, x, y, wave=wave)
            self.seen.append((out[0], self.loss_parts))
            return out

    a = Recording("FullyCNNV3", batch_size=2, lr=1e-3, weights=w, objective=objective)
    a.seen = []
    steps = len(make_loader())                                            # (the sampler fills its last batch: three of them)
    assert a.train(make_loader(), None, 1) == steps == len(a.seen)
    b = FullyCNNTrainer("FullyCNNV3", batch_size=2, lr=1e-3, weights=w, objective=objective)
    dl, by_hand = make_loader(), []
    dl.shuffle()
    for batch_mix, batch_clean, mix_sig, clean_sig in dl:
        wave = wave_of_batch(dl, batch_mix, mix_sig, clean_sig)
        mag, phase = audio.stft_batch(mix_sig.rows, mix_sig.lengths, frames=int(batch_mix.shape[1]))
        assert torch.equal(mag, batch_mix) and torch.equal(phase, wave[0]) and wave[2] == list(clean_sig.lengths)
        by_hand.append((b.fit_step(batch_mix, batch_clean, wave=wave)[0], b.loss_parts))
    assert by_hand == a.seen and all(np.isfinite(v[0]) and v[1][1] > 0 for v in by_hand)
    va, vb = a.variables(), b.variables()
    assert all(np.array_equal(va[k], vb[k]) for k in va)
    a.close()
    b.close()


def test_steps_are_bit_reproducible(built):
    w, x, y, phase, clean = case("FullyCNNV3")[:5]
    outs = []
    for _ in range(2):
        tr = trainer("FullyCNNV3", w)
        loss = tr.train_step(x, y, wave=on_device(phase, clean))[0]
        outs.append((loss, tr.loss_parts, tr.gradients()))
        tr.close()
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert all(np.array_equal(outs[0][2][k], outs[1][2][k]) for k in outs[0][2])


def test_the_four_refusals_name_the_combination(built):
    from fullycnnspeechenhancement_amd import audio, dist
    from fullycnnspeechenhancement_amd.trainer import wave_of_batch
    w, x, y, phase, clean = case("FullyCNNV3")[:5]
    wave = on_device(phase, clean)
    tr = trainer("FullyCNNV3", w)
    before = tr.variables()
    with pytest.raises(ValueError, match="sync_bn=True cannot be combined with an objective that has a wave term"):
        tr.train_step_sharded([(x[:1], y[:1], None), (x[1:], y[1:], None)], sync_bn=True)
    with pytest.raises(ValueError, match="DataParallelTrainer cannot be combined with an objective that has a wave term"):
        dist.DataParallelTrainer(tr)
    with pytest.raises(ValueError, match="wave=None"):
        tr.train_step(x, y)
    with pytest.raises(ValueError, match="wave=None"):
        tr.grad_step(x, y)

    class Loader(object):
        class dataset(object):
            framing = audio.Framing(200, 100, "hanning")

    with pytest.raises(ValueError, match="loader whose framing"):
        wave_of_batch(Loader, x, None, None)
    plain = trainer("FullyCNNV3", w, None)
    with pytest.raises(ValueError, match="has no wave term"):
        trainer("FullyCNNV3", w, audio.WaveObjective(2, 0, 0)).train_step(x, y, wave=wave)
    with pytest.raises(ValueError):
        trainer("FullyCNNV3", w, objective="si_sdr")
    with pytest.raises(ValueError, match="phase"):
        tr.train_step(x, y, wave=(wave[0][:, :3], wave[1], wave[2]))
    with pytest.raises(ValueError, match="lengths"):
        tr.train_step(x, y, wave=(wave[0], wave[1], [701, 640]))
    after = tr.variables()
    assert tr.global_step == 0 and all(np.array_equal(before[k], after[k]) for k in before)      # a refused step changes nothing
    tr.close()
    plain.close()
