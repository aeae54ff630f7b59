"""numpy float64 restatement of the device loader's batch build (not a test module), in the style of tests/stream_np.py:
gather (arena[b : b + c] / 32768), the closed-form mix of tests/eval_closed_form.py, the STFT of oracle/audio_np.py, zero
padding.  Checked against the reference's own loader output (tests/golden/loader_ref.npz) by tests/test_loader_host.py."""

import os

import numpy as np

import eval_closed_form as cf
from oracle import audio_np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "loader_ref.npz"))
    return {k: z[k] for k in z.files}


def signals(gold, what):
    """The fixture's int16 signals, in id order: what = "clean" or "noise"."""
    out = []
    while "%s_%d" % (what, len(out)) in gold:
        out.append(gold["%s_%d" % (what, len(out))])
    return out


def arena_of(items):
    """(arena, offsets, lengths): the items back to back."""
    lengths = np.asarray([len(a) for a in items], np.int64)
    return np.concatenate(items), np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64), lengths


def gather(arena, begin, count):
    """float64 rows of the gather: int16 / 32768 (exact), float copied."""
    row = np.asarray(arena[begin:begin + count], np.float64)
    return row / 32768.0 if arena.dtype == np.int16 else row


def magnitudes(sig):
    """|STFT| [T, 129] float64 of a signal given as exactly representable float64 (oracle/audio_np.py casts to float32)."""
    return audio_np.stft(sig)[0]


def pad_batch(mags):
    t = max(m.shape[0] for m in mags)
    out = np.zeros((len(mags), t, audio_np.BINS, 1))
    for i, m in enumerate(mags):
        out[i, :m.shape[0], :, 0] = m
    return out


def build_batch(clean_arena, clean_index, noise_arena, noise_index, plan, snr):
    """plan: (clean id, noise id, start, gains) per row, as loader.DataSet.plan gives them.  *_index = (offsets, lengths).
    Returns (batch_mix, batch_clean [N, T, 129, 1] float64, mixes, speeches: lists of float64 signals).  The mixture is
    rounded to float32 before the STFT, as the device stores it."""
    mix_mag, clean_mag, mixes, speeches = [], [], [], []
    for cid, nid, start, gains in plan:
        speech = gather(clean_arena, int(clean_index[0][cid]), int(clean_index[1][cid]))
        ls, ln = len(speech), int(noise_index[1][nid])
        if ln > ls:         # only the samples add_noise keeps are gathered
            noise = gather(noise_arena, int(noise_index[0][nid]) + start, ls)
            mixed = cf.mix(speech, noise, snr, 0, [])
        else:
            noise = gather(noise_arena, int(noise_index[0][nid]), ln)
            mixed = cf.mix(speech, noise, snr, 0, gains)
        mixed = mixed.astype(np.float32).astype(np.float64)
        mixes.append(mixed)
        speeches.append(speech)
        mix_mag.append(magnitudes(mixed))
        clean_mag.append(magnitudes(speech))
    return pad_batch(mix_mag), pad_batch(clean_mag), mixes, speeches
