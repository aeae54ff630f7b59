"""Host-side mirror of the reference's STFT front-end and ISTFT rebuild, over the C ABI.

Reference surface kept:
    AudioFeature(windows_name).compute_spectrogram(signal, sample_rate, window_s, stride_s, nfft, use_complex)
        data_utils/audio_feature.py:12-44  (+ power_spectrum :102-110, divide_phase :113-115)
    AudioReBuild(windows_name, nfft).rebuild_audio(sig_length_list, spec, phase, sample_rate, windows_ms, stride_ms)
        model_utils/utils.py:93-183
The framing is a parameter (`Framing`: window <= 256 samples, stride <= window, hamming / hanning / blackman / bartlett) under
rfft(256); the default, 256 / 128 / hamming, is what the reference's cfgs use and runs kernels specialised for it.  The reference
rebuild exists for hamming only (the other windows end in zero, and it divides by them).  The batch functions `stft_batch` / `istft_batch` keep everything on the device
(torch.cuda tensors in and out) so that STFT -> CNN -> ISTFT runs without leaving HBM.
"""

import numpy as np

from . import _args, _lib
from ._args import BINS, FRAME, SAMPLE_RATE, STEP  # noqa: F401
# what lived here before the file was split by concern: every public name is still handed out as audio.<name>
from .evaluation import (EXTRA_METRICS, PROJECTION_METRICS, SEPM_METRICS, SPECTRAL_METRICS, SPECTRAL_RATES, STOI_RATES, bss_sdr_batch,  # noqa: F401
                         CONV_MAX_TAPS, cep_dist_batch, convolve_batch, fw_seg_snr_batch,
                         denoise_and_score, gains_needed, llr_batch, mix_snr_batch, sdr_batch, seg_snr_batch, seg_snr_window, si_sdr_batch, stoi_batch, wss_batch)
from .arena import PCM_DTYPES, gather_pcm, resample_arena, resample_batch, resample_length, resample_taps  # noqa: F401
from .streaming import (STREAM_DELAY, STREAM_FINISH_MAX, STREAM_MAX_HOPS, StreamingDenoiser, StreamingResampler,  # noqa: F401
                        resampler_delay, stream_delay, stream_delay_fr)
from .freerun import BlockDenoiser, FreeResampler, block_delay, free_available  # noqa: F401
from .objective import WaveObjective, mr_stft_batch, wave_loss_batch  # noqa: F401


WINDOWS = {"hamming": 0, "hanning": 1, "blackman": 2, "bartlett": 3}     # rced.h: RCED_WINDOW_*; numpy's windows of those names


def _refused(rc):
    """A framing the library refuses is the caller's mistake: ValueError with the library's reason."""
    if rc != _lib.RCED_OK:
        raise ValueError(_lib.load().rced_last_error().decode())


class Framing(object):
    """How a signal is cut into frames: `window` samples per frame (2 .. 256, under rfft(256)), `stride` samples from one frame
    to the next (1 .. window), and the window's name (numpy's hamming / hanning / blackman / bartlett at that length).  An
    immutable value; Framing() is what every reference cfg runs with and what the specialised kernels are built for."""

    __slots__ = ("window", "stride", "windows_name")

    def __init__(self, window=FRAME, stride=STEP, windows_name="hamming"):
        if windows_name not in WINDOWS:
            raise ValueError("windows_name must be one of %s, got %r" % (", ".join(sorted(WINDOWS, key=WINDOWS.get)), windows_name))
        if int(window) != window or int(stride) != stride:
            raise ValueError("window and stride are whole numbers of samples, got %r and %r" % (window, stride))
        _refused(_lib.load().rced_framing_check(int(window), int(stride), WINDOWS[windows_name]))
        object.__setattr__(self, "window", int(window))
        object.__setattr__(self, "stride", int(stride))
        object.__setattr__(self, "windows_name", windows_name)

    @classmethod
    def from_seconds(cls, sample_rate, window_s, stride_s, windows_name="hamming"):
        """The framing compute_spectrogram cuts: int(round(s * sample_rate)), as en_frame (audio_feature.py:67-68)."""
        return cls(int(round(window_s * sample_rate)), int(round(stride_s * sample_rate)), windows_name)

    @classmethod
    def from_ms(cls, sample_rate, windows_ms, stride_ms, windows_name="hamming"):
        """The framing rebuild_audio cuts: int(ms * sample_rate / 1000) (utils.py:172-173)."""
        return cls(int((windows_ms * sample_rate) / 1000), int((stride_ms * sample_rate) / 1000), windows_name)

    def __setattr__(self, name, value):
        raise AttributeError("a Framing is immutable")

    __delattr__ = __setattr__

    def _key(self):
        return (self.window, self.stride, self.windows_name)

    def __eq__(self, other):
        return isinstance(other, Framing) and self._key() == other._key()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Framing(window=%d, stride=%d, windows_name=%r)" % self._key()

    @property
    def is_default(self):
        return self._key() == (FRAME, STEP, "hamming")

    @property
    def code(self):
        return WINDOWS[self.windows_name]

    def width(self, frames):
        """Columns of a rebuild of `frames` frames: (W - S) + T * S."""
        return (self.window - self.stride) + int(frames) * self.stride


def __getattr__(name):
    """MR_STFT_8K, the default resolutions of the multi-resolution STFT term at 8 kHz, made on first use (a Framing asks the library)."""
    if name == "MR_STFT_8K":
        value = (Framing(256, 64, "hanning"), Framing(128, 32, "hanning"), Framing(64, 16, "hanning"))
        globals()[name] = value
        return value
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def _general(framing):
    """None or the default framing -> None (the specialised entries); anything else -> the Framing (the _fr entries)."""
    if framing is None:
        return None
    if not isinstance(framing, Framing):
        raise ValueError("framing must be an audio.Framing or None, got %r" % (framing,))
    return None if framing.is_default else framing


def check_reference_rebuild(framing):
    """The reference rebuild divides by the window: ValueError, with the reason, for the windows that end in zero."""
    if framing is not None:
        _refused(_lib.load().rced_istft_fr_check(framing.window, framing.stride, framing.code))


def num_frames(length, framing=None):
    fr = _general(framing)
    if fr is None:
        return int(_lib.load().rced_stft_num_frames(int(length)))
    return int(_lib.load().rced_stft_num_frames_fr(int(length), fr.window, fr.stride))


KERNELS = {"x6": 1, "f32": 0}     # rced.h: RCED_AUDIO_X6 (the product: three-part bf16 products), RCED_AUDIO_F32 (the fp32-MFMA comparators)


def _kernels(name):
    if name not in KERNELS:
        raise ValueError("kernels must be 'x6' (the product) or 'f32' (the fp32-MFMA comparator), got %r" % (name,))
    return KERNELS[name]


def _check_nfft(nfft):
    if nfft is not None and nfft != 256:
        raise ValueError("only rfft(256) -> 129 bins is built (data_loader.py:59 hard-codes it)")


def _windows_name(windows_name):
    """The `windows_name` of AudioFeature / AudioReBuild: None is hamming (audio_feature.py:20).  The reference takes an unknown
    name for hamming as well; here it is refused."""
    name = "hamming" if windows_name is None else windows_name
    if name not in WINDOWS:
        raise ValueError("windows_name must be one of %s (or None: hamming), got %r" % (", ".join(sorted(WINDOWS, key=WINDOWS.get)), windows_name))
    return name


def _general_x6(framing, kernels):
    fr = _general(framing)
    if fr is not None and _kernels(kernels) != KERNELS["x6"]:
        raise ValueError("kernels='f32' (the fp32-MFMA comparators) exists for the default framing only, got %r" % (fr,))
    return fr


def stft_batch(pcm, lengths=None, frames=None, with_phase=True, kernels="x6", framing=None):
    """pcm: torch.cuda float32 [N, L]; lengths: per-utterance sample counts (list / tensor) or None.
    Returns (mag [N, T, 129, 1], phase [N, T, 129] complex64 or None); T = frames or the batch maximum
    (zero-padded like DataLoader.padding_batch, data_loader.py:198-209).  framing: a Framing, or None for Framing()."""
    import torch
    fr = _general_x6(framing, kernels)
    if not (pcm.is_cuda and pcm.dim() == 2):
        raise ValueError("pcm must be a CUDA/HIP tensor [N, L]")
    pcm = pcm.float().contiguous()
    n, L = int(pcm.shape[0]), int(pcm.shape[1])
    dev = pcm.device
    if lengths is None:
        lens = [L] * n
        ldev = None
    else:
        lens = _args.host_ints(lengths, n, "lengths")
        if any(v < 1 or v > L for v in lens):
            raise ValueError("lengths must lie in [1, %d]" % L)
        ldev = torch.tensor(lens, dtype=torch.int32, device=dev)
    t = int(frames) if frames is not None else (max(num_frames(v, fr) for v in lens) if n else 0)
    mag = torch.empty((n, t, BINS, 1), dtype=torch.float32, device=dev)
    ph = torch.empty((n, t, BINS, 2), dtype=torch.float32, device=dev) if with_phase else None
    if n and t and fr is not None:
        _lib.check(_lib.load().rced_stft_fr(pcm.data_ptr(), ldev.data_ptr() if ldev is not None else None, n, L, t, fr.window, fr.stride,
                                            fr.code, mag.data_ptr(), ph.data_ptr() if ph is not None else None, dev.index,
                                            _args.current_stream(dev)))
    elif n and t:
        _lib.check(_lib.load().rced_stft_ex(pcm.data_ptr(), ldev.data_ptr() if ldev is not None else None, n, L, t, mag.data_ptr(),
                                            ph.data_ptr() if ph is not None else None, dev.index, _args.current_stream(dev), _kernels(kernels)))
    return mag, (torch.view_as_complex(ph) if ph is not None else None)


def istft_batch(mag, phase, nfft=512, kernels="x6", rebuild="reference", frames=None, framing=None):
    """mag [N, T, 129(,1)] float32, phase [N, T, 129] complex64 (torch.cuda) -> audio [N, (T+1)*128], at a framing (a Framing, or
    None for Framing()) [N, (W - S) + T * S]; the reference rebuild exists for hamming windows only (check_reference_rebuild).
    rebuild: "reference" (AudioReBuild.rebuild_audio as shipped: divide by the window, keep half of every frame; nfft as there)
    or "ola" (least-squares weighted overlap-add, rced_istft_ola: both halves of every frame, nfft plays no part).
    frames (rebuild="ola" only): per-utterance frame counts (list / tensor, clamped into [0, T]) or None (= T each); frames at or
    past an utterance's count are never read, and its columns from 128 (frames + 1) -- (frames - 1) S + W -- on are zero."""
    import torch
    _args.check_rebuild(rebuild, kernels)
    fr = _general_x6(framing, kernels)
    if rebuild == "reference":
        check_reference_rebuild(fr)
    if frames is not None and rebuild != "ola":
        raise ValueError("frames belongs to rebuild='ola' (the reference rebuild keeps every frame apart: the caller trims)")
    if mag.dim() == 4:
        mag = mag.squeeze(-1)
    mag = mag.float().contiguous()
    ph = torch.view_as_real(phase.to(torch.complex64).contiguous()).contiguous()
    n, t = int(mag.shape[0]), int(mag.shape[1])
    if tuple(mag.shape) != (n, t, BINS) or tuple(ph.shape) != (n, t, BINS, 2):
        raise ValueError("mag must be [N, T, 129], phase [N, T, 129] complex")
    out = torch.empty((n, (fr or Framing()).width(t)), dtype=torch.float32, device=mag.device)
    if rebuild == "ola":
        fdev = None
        if frames is not None:
            if hasattr(frames, "is_cuda") and frames.is_cuda:
                fdev = frames.to(device=mag.device, dtype=torch.int32).reshape(-1).contiguous()
                if int(fdev.shape[0]) != n:
                    raise ValueError("frames must hold N = %d values, got %d" % (n, int(fdev.shape[0])))
            else:
                fdev = torch.tensor(_args.host_ints(frames, n, "frames"), dtype=torch.int32, device=mag.device)
        if n and fr is not None:
            _lib.check(_lib.load().rced_istft_ola_fr(mag.data_ptr() if t else None, ph.data_ptr() if t else None,
                                                     fdev.data_ptr() if fdev is not None else None, n, t, fr.window, fr.stride, fr.code,
                                                     out.data_ptr(), mag.device.index, _args.current_stream(mag.device)))
        elif n:
            _lib.check(_lib.load().rced_istft_ola(mag.data_ptr() if t else None, ph.data_ptr() if t else None,
                                                  fdev.data_ptr() if fdev is not None else None, n, t, out.data_ptr(), mag.device.index,
                                                  _args.current_stream(mag.device)))
        return out
    if n and t and fr is not None:
        _lib.check(_lib.load().rced_istft_fr(mag.data_ptr(), ph.data_ptr(), n, t, int(nfft), fr.window, fr.stride, out.data_ptr(),
                                             mag.device.index, _args.current_stream(mag.device)))
    elif n and t:
        _lib.check(_lib.load().rced_istft_ex(mag.data_ptr(), ph.data_ptr(), n, t, int(nfft), out.data_ptr(), mag.device.index,
                                             _args.current_stream(mag.device), _kernels(kernels)))
    return out


class AudioFeature(object):
    """data_utils/audio_feature.py:12-115 on the GPU (numpy in, numpy out, like the reference)."""

    def __init__(self, windows_name=None, device=0, kernels="x6"):
        self.windows_name = _windows_name(windows_name)
        self.device, self.kernels = device, kernels
        _kernels(kernels)

    def compute_spectrogram(self, signal, sample_rate, window_s=0.02, stride_s=0.01, nfft=512, use_complex=False):
        import torch
        if stride_s > window_s:
            raise ValueError("Stride size must not be greater than window size.")   # audio_feature.py:29-30
        _check_nfft(nfft)
        framing = Framing.from_seconds(sample_rate, window_s, stride_s, self.windows_name)
        sig = torch.as_tensor(np.asarray(signal, dtype=np.float32), device="cuda:%d" % self.device)[None]
        mag, ph = stft_batch(sig, with_phase=use_complex, kernels=self.kernels, framing=framing)
        if use_complex:   # [129, T] complex, like np.transpose(fft_frames)
            return (mag[0, :, :, 0] * ph[0]).cpu().numpy().T
        return mag[0, :, :, 0].cpu().numpy().T

    @staticmethod
    def power_spectrum(frames):
        return np.absolute(frames)

    @staticmethod
    def divide_phase(fft_frames):
        return np.exp(1.j * np.angle(fft_frames))


class AudioReBuild(object):
    """model_utils/utils.py:93-183 on the GPU.  nfft defaults to 512 exactly as the reference's does."""

    def __init__(self, windows_name=None, nfft=512, device=0, kernels="x6", rebuild="reference"):
        self.windows_name = _windows_name(windows_name)
        if nfft not in (256, 512):
            raise ValueError("nfft must be 512 (reference default) or 256")
        self.nfft, self.device, self.kernels = nfft, device, kernels
        _kernels(kernels)
        self.rebuild = _args.check_rebuild(rebuild, kernels)      # "ola": weighted overlap-add over num_frames(length) frames each
        if self.rebuild == "reference":
            check_reference_rebuild(Framing(windows_name=self.windows_name))

    def rebuild_audio(self, sig_length_list, spec, phase, sample_rate, windows_ms, stride_ms):
        import torch
        framing = Framing.from_ms(sample_rate, windows_ms, stride_ms, self.windows_name)
        dev = "cuda:%d" % self.device
        mag = torch.as_tensor(np.asarray(spec, dtype=np.float32), device=dev)
        ph = torch.as_tensor(np.asarray(phase).astype(np.complex64), device=dev)
        frames = [num_frames(v, framing) for v in sig_length_list] if self.rebuild == "ola" else None
        audio = istft_batch(mag, ph, self.nfft, kernels=self.kernels, rebuild=self.rebuild, frames=frames, framing=framing).cpu().numpy()
        return [audio[i][:sig_length_list[i]] for i in range(len(audio))]
