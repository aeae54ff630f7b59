"""Host-side mirror of the reference's AudioParser and batch padding (data_utils/data_loader.py:16-61, 198-209).

`add_noise` mixes on the device (rced_mix_snr) from the random draws `plan_noise` makes on the host exactly as the
reference consumes np.random, so that after np.random.seed(s) both give the same mixture.  `load_audio` (librosa),
manifests, Sampler and the joblib DataLoader are not built.
"""

import numpy as np

from . import audio


def plan_noise(len_speech, len_noise):
    """The random draws of AudioParser.add_noise (data_loader.py:36-45), taken from np.random in the reference's order:
    speech at least as long as the noise -> ceil((ls - ln) / ln) calls of np.random.uniform(0, 2), one per doubling of
    the noise buffer; otherwise one np.random.randint(0, ln - ls).  Returns (start, gains): the crop offset (0 when the
    noise is tiled) and, as float64, the draws that can reach the first ls samples (audio.gains_needed) -- every draw is
    made, to leave np.random where the reference leaves it, but a doubling past the speech's end changes nothing."""
    ls, ln = int(len_speech), int(len_noise)
    if ln < 1:
        raise ValueError("empty noise")
    if ls >= ln:
        draws = [np.random.uniform(0, 2) for _ in range(int(np.ceil((ls - ln) / ln)))]
        return 0, np.asarray(draws[:audio.gains_needed(ls, ln)], np.float64)
    return int(np.random.randint(0, ln - ls)), np.zeros(0, np.float64)


def padding_batch(batch_list):
    """DataLoader.padding_batch (data_loader.py:198-209): [F, T_i] spectrograms -> [N, Tmax, F, 1], zero-padded in time,
    with the dtype of the longest one."""
    longest = max(batch_list, key=lambda x: x.shape[1])
    out = np.zeros((len(batch_list),) + longest.shape, longest.dtype)
    for i, arr in enumerate(batch_list):
        out[i, :arr.shape[0], :arr.shape[1]] = arr
    return np.transpose(out[:, None], (0, 3, 2, 1))


class AudioParser(object):
    """data_loader.py:16-61 with the mixing and the STFT on the GPU (numpy in, numpy out, like the reference)."""

    def __init__(self, sample_rate=8000, window_ms=32, stride_ms=16, snr=0, windows_name=None, use_complex=False, device=0):
        self.snr = snr
        self.sample_rate = sample_rate
        self.window_s = window_ms / 1000
        self.stride_s = stride_ms / 1000
        self.extractor = audio.AudioFeature(windows_name, device=device)
        self.complex = use_complex
        self.device = device

    def add_noise(self, speech, noise):
        """Mix at self.snr dB; consumes np.random as the reference does.  Returns float32 [len(speech)]."""
        import torch
        speech, noise = np.asarray(speech, np.float32).reshape(-1), np.asarray(noise, np.float32).reshape(-1)
        start, gains = plan_noise(len(speech), len(noise))
        dev = "cuda:%d" % self.device
        mix = audio.mix_snr_batch(torch.as_tensor(speech, device=dev)[None], torch.as_tensor(noise, device=dev)[None],
                                  self.snr, starts=[start], gains=[gains])
        return mix[0].cpu().numpy()

    def parse_audio(self, sig):
        return self.extractor.compute_spectrogram(sig, self.sample_rate, window_s=self.window_s, stride_s=self.stride_s,
                                                  nfft=256, use_complex=self.complex)
