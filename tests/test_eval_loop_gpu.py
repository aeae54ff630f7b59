"""GPU test of the evaluation loop's score table (evaluation._EXTRA): denoise_and_score with every score switched on gives,
column by column, the bits of the direct *_batch call on the audio it returns, over utterances that take every branch."""

import numpy as np
import pytest

from test_stoi_gpu import dev, padded

pytestmark = pytest.mark.gpu


def test_the_loop_equals_the_direct_calls(built):
    """Three utterances at 8 kHz: 4000 samples (38 STOI frames at 10 kHz, every one kept: nine 30-frame segments), 2500 (23 STOI
    frames: no segment, but 38 frames of 240 samples for the frame-based scores) and 200 (shorter than one 240-sample frame).
    White noise, so that the silent-frame removal keeps every frame."""
    import torch
    from fullycnnspeechenhancement_amd import audio, evaluation
    from fullycnnspeechenhancement_amd._args import SAMPLE_RATE
    lens = [4000, 2500, 200]
    rng = np.random.default_rng(2024)
    clean = [(0.1 * rng.standard_normal(L)).astype(np.float32) for L in lens]
    mix = [(c + 0.03 * rng.standard_normal(len(c))).astype(np.float32) for c in clean]
    names = ("wss", "bss_sdr", "estoi", "llr", "si_sdr", "seg_snr")          # all six, not in the table's order
    assert sorted(names) == sorted(evaluation.ALL_EXTRA) and names != evaluation.ALL_EXTRA
    c, m = dev(padded(clean, max(lens), fill=0.0)), dev(padded(mix, max(lens), fill=0.0))
    out, sdr, stoi, more = audio.denoise_and_score(lambda mag: mag, m, c, lens, stoi=True, extra=names, rebuild="reference")
    assert list(more) == list(names)                                        # the caller's order
    direct = {"sdr": audio.sdr_batch(c, out, lens),
              "stoi": audio.stoi_batch(c, out, lens, SAMPLE_RATE),
              "estoi": audio.stoi_batch(c, out, lens, SAMPLE_RATE, extended=True),
              "si_sdr": audio.si_sdr_batch(c, out, lens),
              "seg_snr": audio.seg_snr_batch(c, out, lens, SAMPLE_RATE),
              "llr": audio.llr_batch(c, out, lens, SAMPLE_RATE, limit=2.0),
              "wss": audio.wss_batch(c, out, lens, SAMPLE_RATE),
              "bss_sdr": audio.bss_sdr_batch(c, out, lens, filter_length=512)}
    got = dict(more, sdr=sdr, stoi=stoi)
    assert sorted(got) == sorted(direct)
    for name, want in direct.items():
        assert got[name].dtype == torch.float64 and got[name].shape == (3,)
        assert np.array_equal(got[name].cpu().numpy(), want.cpu().numpy(), equal_nan=True), name
    col = {name: v.cpu().numpy() for name, v in got.items()}
    assert np.isfinite([v[0] for v in col.values()]).all() and col["stoi"][0] != 1e-5 and col["estoi"][0] != 1e-5
    for row in (1, 2):                                                      # no 30-frame segment
        assert col["stoi"][row] == 1e-5 and col["estoi"][row] == 1e-5
        assert np.isfinite([col[name][row] for name in ("sdr", "si_sdr")]).all()
    for name in ("seg_snr", "llr", "wss"):                                  # frames at 2500 samples, none at 200
        assert np.isfinite(col[name][1]) and np.isnan(col[name][2])
