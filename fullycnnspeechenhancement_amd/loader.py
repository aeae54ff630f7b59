"""Host-side mirror of the reference's data loader (data_utils/data_loader.py), with the batches built on the device.

One utterance at a time, numpy in and numpy out (data_loader.py:16-61, 198-209): `AudioParser.add_noise` mixes on the
device (rced_mix_snr) from the random draws `plan_noise` makes on the host exactly as the reference consumes np.random, so
that after np.random.seed(s) both give the same mixture; `padding_batch` pads as the reference does.

Training from audio (data_loader.py:64-262): a `Corpus` is uploaded once -- one int16 (or float32) arena
on the device plus a host index --, `DataSet` / `Sampler` / `DataLoader` keep the reference's order of items and of
np.random draws (as its loader runs with num_works=1), and every batch is cut out of the arenas (rced_gather_pcm), mixed
(rced_mix_snr) and transformed (one rced_stft over the clean and the mixed rows) on the device; per batch the host sends
the plan only: which items, which crop offsets, which gains.  Manifests are the reference's json lines; wav files are read
with the standard library: PCM16, mono, at the corpus rate -- or, with resample=True, PCM16 of any rate and channel count,
downmixed and resampled on the device while the corpus is uploaded (rced_resample, DESIGN.md 3.4f: what librosa's
`load_audio` does on the host).  Beyond the reference: `DataSet(rir=RirCorpus)` convolves the speech with room impulse
responses on the device (rced_convolve) before the noise is mixed in.  Not built: other sample formats (8 / 24 / 32 bit, flac), drop_last=True, worker
processes, prefetch.
"""

import codecs
import json
import wave

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


# ---- the corpus: a host index, wav / manifest reading (no GPU needed), and the arena on the device ------------------

def read_manifest(manifest_path, min_duration=0.4, max_duration=float("inf")):
    """DataSet.read_manifest (data_loader.py:93-107): the json lines whose "duration" lies in [min, max]."""
    manifest = []
    for json_line in codecs.open(manifest_path, "r", "utf-8"):
        try:
            json_data = json.loads(json_line)
        except Exception as e:
            raise IOError("Error reading manifest: %s" % str(e))
        if max_duration >= json_data["duration"] >= min_duration:
            manifest.append(json_data)
    return manifest


def _open_wav(path, sample_rate, resample=False):
    try:
        w = wave.open(path, "rb")
    except (wave.Error, EOFError) as e:
        raise ValueError("%s: not a PCM wav file (%s)" % (path, e))
    got = (w.getnchannels(), 8 * w.getsampwidth(), w.getframerate())
    if resample:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE" or got[0] < 1 or got[2] < 1:
            w.close()
            raise ValueError("%s: %d channel(s), %d bit, %d Hz; only PCM16 is read" % ((path,) + got))
    elif got[0] != 1 or w.getsampwidth() != 2 or w.getcomptype() != "NONE" or got[2] != int(sample_rate):
        w.close()
        raise ValueError("%s: %d channel(s), %d bit, %d Hz; only mono PCM16 at %d Hz is read (resample=True converts PCM16 of "
                         "any rate and channel count on the device)" % ((path,) + got + (int(sample_rate),)))
    return w


def wav_info(path):
    """(rate, channels, frames) of a PCM16 wav file, from its header."""
    w = _open_wav(path, None, resample=True)
    try:
        return int(w.getframerate()), int(w.getnchannels()), int(w.getnframes())
    finally:
        w.close()


def read_wav_frames(path):
    """A PCM16 wav file as it is stored: (int16 [frames, channels], rate)."""
    w = _open_wav(path, None, resample=True)
    try:
        sig = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
        return sig.reshape(-1, w.getnchannels()), int(w.getframerate())
    finally:
        w.close()


def wav_length(path, sample_rate, resample=False):
    """Samples in a wav file at sample_rate, from its header; ValueError unless it is mono PCM16 at sample_rate.  With
    resample=True any PCM16 file: the samples it has once resampled (audio.resample_length)."""
    if resample:
        rate, _, frames = wav_info(path)
        return audio.resample_length(frames, rate, sample_rate)
    w = _open_wav(path, sample_rate)
    try:
        return int(w.getnframes())
    finally:
        w.close()


def read_wav(path, sample_rate, resample=False, device=0):
    """The samples of a mono PCM16 wav file at sample_rate, int16 [n].  With resample=True any PCM16 file, downmixed and
    resampled to sample_rate on the device (needs a GPU), int16 [n] by the rule of rced_resample."""
    if resample:
        frames, rate = read_wav_frames(path)
        rows, lens = audio.resample_batch(frames[None], rate, sample_rate, dtype="int16", device=device)
        return rows[0, :lens[0]].cpu().numpy()
    w = _open_wav(path, sample_rate)
    try:
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
    finally:
        w.close()


STAGING_BYTES = 256 << 20      # raw PCM16 per upload of Corpus.from_manifest(resample=True)


def staged_uploads(paths, device):
    """PCM16 wav files of any rate and channel count, uploaded as they are stored, at most STAGING_BYTES at a time (a larger
    file goes alone).  Yields (raw, groups) per upload: raw, an int16 device tensor, and groups[(rate, channels)] = [(i, first
    frame, frames)] -- where file i lies in raw, in frames of its own channel count.  Host memory holds one staging buffer."""
    import torch
    infos = [wav_info(p) for p in paths]
    sizes = [frames * channels for _, channels, frames in infos]
    chans = [channels for _, channels, _ in infos]
    stage = np.empty((min(max([STAGING_BYTES // 2] + sizes), sum(sizes) + sum(chans)),), np.int16)
    first = 0
    while first < len(paths):
        # the files of one upload: each starts on a whole frame of its own channel count; always at least one file
        last, used, starts = first, 0, []
        while last < len(paths):
            at = -(-used // chans[last]) * chans[last]
            if last > first and at + sizes[last] > stage.size:
                break
            starts.append(at)
            used = at + sizes[last]
            last += 1
        groups = {}
        for i, at in zip(range(first, last), starts):
            rate, channels, frames = infos[i]
            sig, _ = read_wav_frames(paths[i])
            if sig.shape[0] != frames:
                raise ValueError("%s: header says %d frames, the data holds %d" % (paths[i], frames, sig.shape[0]))
            stage[at:at + sizes[i]] = sig.reshape(-1)
            groups.setdefault((rate, channels), []).append((i, at // channels, frames))
        yield torch.from_numpy(stage[:used]).to(device), groups
        first = last


class CorpusIndex(object):
    """Where every item lies in the arena: offsets[i] (first sample, absolute) and lengths[i], items packed back to back in
    the order given.  Host only."""

    def __init__(self, lengths, paths=None):
        self.lengths = np.asarray(list(lengths), np.int64).reshape(-1)
        if (self.lengths < 1).any():
            raise ValueError("empty item %d" % int(np.argmax(self.lengths < 1)))
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64) if self.lengths.size else \
            np.zeros(0, np.int64)
        self.total = int(self.lengths.sum())
        self.paths = list(paths) if paths is not None else None

    def __len__(self):
        return int(self.lengths.size)

    @classmethod
    def from_manifest(cls, path, sample_rate, min_duration=0.4, max_duration=float("inf"), key="audio_filepath", resample=False):
        """The index of a manifest's wav files, from their headers alone (nothing but the headers is read).  resample=True:
        PCM16 files of any rate and channel count; the lengths are those they have at sample_rate."""
        paths = [item[key] for item in read_manifest(path, min_duration, max_duration)]
        return cls([wav_length(p, sample_rate, resample) for p in paths], paths)


class Corpus(object):
    """Every utterance of a corpus in one device tensor (`arena`, int16 or float32 [total]) plus the host `index`
    (CorpusIndex).  AISHELL-1 at 8 kHz int16 is about 10 GB: it is uploaded once and stays."""

    def __init__(self, index, arena):
        if int(arena.shape[0]) != index.total:
            raise ValueError("the arena holds %d samples, the index %d" % (int(arena.shape[0]), index.total))
        self.index, self.arena = index, arena
        self.device = arena.device.index

    def __len__(self):
        return len(self.index)

    @property
    def lengths(self):
        return self.index.lengths

    @property
    def offsets(self):
        return self.index.offsets

    @staticmethod
    def _dtype(arrays):
        """int16 in -> int16 arena; float in -> float32 arena."""
        kinds = set("i" if a.dtype == np.int16 else ("f" if a.dtype.kind == "f" else "?") for a in arrays)
        if kinds == {"i"}:
            return np.int16
        if kinds == {"f"}:
            return np.float32
        raise ValueError("items must all be int16 or all be float arrays")

    @classmethod
    def from_arrays(cls, arrays, device=0):
        import torch
        arrays = [np.asarray(a) for a in arrays]
        if any(a.ndim != 1 for a in arrays):
            raise ValueError("items must be 1-D arrays")
        index = CorpusIndex([a.size for a in arrays])
        dtype = cls._dtype(arrays) if arrays else np.int16
        host = np.concatenate([a.astype(dtype, copy=False) for a in arrays]) if arrays else np.zeros(0, dtype)
        return cls(index, torch.as_tensor(host, device="cuda:%d" % device))

    @classmethod
    def from_manifest(cls, path, sample_rate, min_duration=0.4, max_duration=float("inf"), key="audio_filepath", device=0,
                      resample=False, arena_dtype=None):
        """The wav files a reference manifest names (json lines, filtered by duration as data_loader.py:93-107 does; `key`
        picks the field: "audio_filepath", or "clean_audio_filepath" / "mix_audio_filepath" of a paired manifest).  The
        arena is sized from the headers, then filled file by file: host memory holds one file at a time.
        resample=True: PCM16 files of any rate and channel count.  They are uploaded as stored, at most STAGING_BYTES at a
        time, and downmixed and resampled to sample_rate on the device straight into the arena (audio.resample_arena in
        packed mode, one call per (rate, channels) of an upload); the arena is float32, or int16 with arena_dtype="int16".
        Host memory holds one staging buffer, never the corpus."""
        import torch
        if not resample:
            if arena_dtype not in (None, "int16"):
                raise ValueError("without resample=True the arena holds the files' int16 samples")
            index = CorpusIndex.from_manifest(path, sample_rate, min_duration, max_duration, key)
            arena = torch.empty((index.total,), dtype=torch.int16, device="cuda:%d" % device)
            for p, off, n in zip(index.paths, index.offsets, index.lengths):
                sig = read_wav(p, sample_rate)
                if sig.size != n:
                    raise ValueError("%s: header says %d samples, the data holds %d" % (p, n, sig.size))
                arena[int(off):int(off) + int(n)].copy_(torch.from_numpy(sig))
            return cls(index, arena)
        arena_dtype = arena_dtype or "float32"
        if arena_dtype not in audio.PCM_DTYPES:
            raise ValueError("arena_dtype must be 'float32' or 'int16', got %r" % (arena_dtype,))
        index = CorpusIndex.from_manifest(path, sample_rate, min_duration, max_duration, key, resample=True)
        arena = torch.empty((index.total,), dtype=torch.float32 if arena_dtype == "float32" else torch.int16,
                            device="cuda:%d" % device)
        for raw, groups in staged_uploads(index.paths, arena.device):
            for (rate, channels), rows in groups.items():
                audio.resample_arena(raw, [a for _, a, _ in rows], [f for _, _, f in rows], channels, rate, sample_rate,
                                     out=arena, out_begins=[int(index.offsets[i]) for i, _, _ in rows], dtype=arena_dtype)
        return cls(index, arena)

    def gather(self, items, starts=None, counts=None, L=None, out=None):
        """Rows cut from the arena: row n = item items[n] from its sample starts[n] (None = 0) over counts[n] samples (None =
        to its end); audio.gather_pcm with the absolute positions."""
        items = [int(i) for i in items]
        starts = [0] * len(items) if starts is None else [int(s) for s in starts]
        lens = [int(self.index.lengths[i]) for i in items]
        counts = [n - s for n, s in zip(lens, starts)] if counts is None else [int(c) for c in counts]
        for i, s, c, n in zip(items, starts, counts, lens):
            if s < 0 or c < 0 or s + c > n:
                raise ValueError("item %d has %d samples: [%d, %d) leaves it" % (i, n, s, s + c))
        return audio.gather_pcm(self.arena, [int(self.index.offsets[i]) + s for i, s in zip(items, starts)], counts, L, out)


class RirCorpus(Corpus):
    """Room impulse responses for DataSet(rir=...) (DESIGN.md 3.4e "Reverberation"): a Corpus of float32 responses at
    `sample_rate` plus `direct`, a host int64 index per item: the first position of max |h|, the direct path, found once
    at build.  normalize=True (default) divides each response by h[direct], so the direct path is exactly +1 and a
    reverberant utterance keeps its dry level and polarity.  A response longer than audio.CONV_MAX_TAPS (8192 taps, 1.02 s
    at 8 kHz) is cut there, with one warning that names how many were; a direct path behind the cut is found in what is
    left.  One sample past the indexed items the arena holds 1.0: the one-tap identity the rows that stay dry are
    convolved with.  index_only=True builds everything but the arena (no GPU needed): enough for DataSet.plan."""

    def __init__(self, index, arena, direct, sample_rate=8000):
        if arena is not None and int(arena.shape[0]) != index.total + 1:
            raise ValueError("the arena holds %d samples, the index %d and the identity tap" % (int(arena.shape[0]), index.total))
        self.index, self.arena = index, arena
        self.device = arena.device.index if arena is not None else None
        self.direct = np.asarray(direct, np.int64).reshape(-1)
        self.sample_rate = int(sample_rate)
        if self.direct.size != len(index) or ((self.direct < 0) | (self.direct >= index.lengths)).any():
            raise ValueError("direct must hold one position inside each response")

    @staticmethod
    def prepare(arrays, normalize=True):
        """Host only: (responses as float32 arrays, cut and normalised as the class says; direct int64 [count])."""
        import warnings
        out, direct, cut = [], [], 0
        for i, a in enumerate(arrays):
            h = np.asarray(a)
            if h.ndim != 1 or h.size < 1:
                raise ValueError("response %d must be a 1-D array with at least one tap" % i)
            h = (h.astype(np.float32) / np.float32(32768)) if h.dtype == np.int16 else h.astype(np.float32)
            if h.size > audio.CONV_MAX_TAPS:
                h, cut = h[:audio.CONV_MAX_TAPS], cut + 1
            d = int(np.argmax(np.abs(h)))
            if not np.isfinite(h).all() or h[d] == 0:
                raise ValueError("response %d is silent or not finite" % i)
            if normalize:
                h = (h.astype(np.float64) / np.float64(h[d])).astype(np.float32)
            out.append(h)
            direct.append(d)
        if cut:
            warnings.warn("%d of %d impulse responses are longer than %d taps and were truncated" % (cut, len(out), audio.CONV_MAX_TAPS))
        return out, np.asarray(direct, np.int64)

    @classmethod
    def from_arrays(cls, arrays, device=0, normalize=True, sample_rate=8000, index_only=False):
        """int16 arrays are read as value / 32768, float arrays as they are."""
        import torch
        rows, direct = cls.prepare(arrays, normalize)
        index = CorpusIndex([h.size for h in rows])
        if index_only:
            return cls(index, None, direct, sample_rate)
        host = np.concatenate(rows + [np.ones(1, np.float32)])
        return cls(index, torch.as_tensor(host, device="cuda:%d" % device), direct, sample_rate)

    @classmethod
    def from_manifest(cls, path, sample_rate, min_duration=0.0, max_duration=float("inf"), key="audio_filepath", device=0,
                      resample=False, normalize=True, index_only=False):
        """The wav files a manifest names, read as Corpus.from_manifest reads them (mono PCM16 at sample_rate; with
        resample=True PCM16 of any rate and channel count, downmixed and resampled on the device to float32).  Responses
        are short: min_duration defaults to 0."""
        rows = []
        for item in read_manifest(path, min_duration, max_duration):
            if resample:
                frames, rate = read_wav_frames(item[key])
                out, lens = audio.resample_batch(frames[None], rate, sample_rate, dtype="float32", device=device)
                rows.append(out[0, :lens[0]].cpu().numpy())
            else:
                rows.append(read_wav(item[key], sample_rate))
        return cls.from_arrays(rows, device, normalize, sample_rate, index_only)

    def early_taps(self, rid, early_ms):
        """Taps of the direct path plus early reflections: min(K, direct + round(early_ms * sample_rate / 1000) + 1)."""
        return min(int(self.lengths[rid]), int(self.direct[rid]) + int(round(early_ms * self.sample_rate / 1000.0)) + 1)

    def filters(self, rids):
        """The filter rows of a batch: (rows [N, Kmax] float32 on the device, taps [N], shifts [N]); a rid of None is the
        one-tap identity [1.0] at shift 0."""
        if self.arena is None:
            raise ValueError("an index-only RirCorpus builds no batches")
        begins = [int(self.index.offsets[r]) if r is not None else self.index.total for r in rids]
        taps = [int(self.index.lengths[r]) if r is not None else 1 for r in rids]
        return audio.gather_pcm(self.arena, begins, taps), taps, [int(self.direct[r]) if r is not None else 0 for r in rids]


def synthetic_rirs(count, sample_rate=8000, rt60=(0.2, 0.8), seed=0):
    """`count` made-up impulse responses as float32 arrays, for tests, benchmarks and users without recordings -- NOT a room
    simulator: no geometry, no early-reflection pattern, no frequency-dependent absorption.  Each is zeros over a pre-delay
    drawn from 0 .. 4 ms, a direct path of exactly 1, then Gaussian noise (sigma 0.3, clipped to +-0.9) under an exponential
    decay that reaches -60 dB at an RT60 drawn uniformly from `rt60` seconds, where it ends (at most audio.CONV_MAX_TAPS taps).
    Draws come from np.random.RandomState(seed): reproducible, and the global np.random is not touched."""
    rs = np.random.RandomState(seed)
    lo, hi = float(rt60[0]), float(rt60[1])
    if count < 0 or sample_rate < 1 or not 0 < lo <= hi:
        raise ValueError("need count >= 0, sample_rate >= 1 and 0 < rt60[0] <= rt60[1]")
    out = []
    for _ in range(int(count)):
        t60 = rs.uniform(lo, hi) * sample_rate                       # samples to -60 dB
        pre = int(rs.randint(0, int(0.004 * sample_rate) + 1))
        tail = min(max(int(t60), 1), audio.CONV_MAX_TAPS - pre - 1)
        h = np.zeros(pre + 1 + tail, np.float64)
        h[pre] = 1.0
        h[pre + 1:] = np.clip(0.3 * rs.standard_normal(tail), -0.9, 0.9) * 10.0 ** (-3.0 * np.arange(1, tail + 1) / t60)
        out.append(h.astype(np.float32))
    return out


class PcmRows(object):
    """The `mix_sig` / `clean_sig` slot of a batch: zero-padded device rows [N, L] and their lengths.  len() and indexing
    give what the reference's lists give, as trimmed device views; engine.evaluate_pcm takes the object as it is."""

    def __init__(self, rows, lengths):
        self.rows, self.lengths = rows, [int(v) for v in lengths]

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(i)
        return self.rows[i, :self.lengths[i]]


# ---- data_loader.py:64-262 -------------------------------------------------------------------------------------------

class DataSet(object):
    """data_loader.py:64-134 over corpora instead of manifests.  clean, noise, mix: Corpus objects (a CorpusIndex does
    for everything but building batches).  `item_list` holds item ids of `clean`; with `noise`, `noise_list` holds its
    ids, replicated ceil(len(items) / len(noise)) times where it is shorter (data_loader.py:87-91), and item k of a
    batch is mixed with noise_list[k] at `snr` dB.  `mix=` is the paired mode (the reference's clean_audio_filepath /
    mix_audio_filepath manifests): item i of `mix` is the mixture of item i of `clean`, nothing is mixed.
    use_complex=True (the validation set of train.py): the reference then yields complex spectrograms that test() /
    valid() never read (they recompute them from the PCM, engine.py); here the two spectrogram slots are None.
    framing: the audio.Framing the batches' spectrograms are cut with (None: the default); kept as `.framing`, where
    FullyCNNTester.test and FullyCNNTrainer.valid read it, as the reference reads window_s from the dataset.
    rir: a RirCorpus (the reference has no reverberation; DESIGN.md 3.4e "Reverberation").  An item is then convolved, with
    probability rir_prob, with a response drawn uniformly, aligned on its direct path, before the noise is mixed in at
    `snr` against the reverberant speech.  target: what the clean half of a batch holds -- "reverberant" (the task stays
    denoising), "early" (the same speech under the direct path and the reflections of the first early_ms milliseconds:
    dereverberation) or "dry" (the speech as gathered).  With rir=None nothing changes: the same plans, draws and bits."""

    TARGETS = ("reverberant", "early", "dry")

    def __init__(self, clean, noise=None, mix=None, snr=0, use_complex=False, framing=None, rir=None, rir_prob=1.0,
                 target="reverberant", early_ms=50.0):
        if target not in self.TARGETS:
            raise ValueError("target must be one of %r, got %r" % (self.TARGETS, target))
        if not 0.0 <= float(rir_prob) <= 1.0:
            raise ValueError("rir_prob must lie in [0, 1], got %r" % (rir_prob,))
        if not float(early_ms) >= 0.0:
            raise ValueError("early_ms must not be negative, got %r" % (early_ms,))
        if rir is not None and mix is not None:
            raise ValueError("rir= needs noise=: a paired corpus (mix=) holds finished mixtures, nothing is convolved or mixed")
        if rir is not None and len(rir) < 1:
            raise ValueError("empty rir corpus")
        self.rir, self.rir_prob, self.target, self.early_ms = rir, float(rir_prob), target, float(early_ms)
        if framing is not None and not isinstance(framing, audio.Framing):
            raise ValueError("framing must be an audio.Framing or None, got %r" % (framing,))
        self.framing = framing
        if (noise is None) == (mix is None):
            raise ValueError("give either noise= (mixed at snr on the device) or mix= (a paired corpus)")
        if mix is not None and len(mix) != len(clean):
            raise ValueError("a paired corpus holds one mixture per clean item: %d != %d" % (len(mix), len(clean)))
        self.clean, self.noise, self.mix = clean, noise, mix
        self.snr, self.complex = snr, bool(use_complex)
        self.item_list = list(range(len(clean)))
        if noise is not None:
            if len(noise) < 1:
                raise ValueError("empty noise corpus")
            self.noise_list = list(range(len(noise)))
            if len(self.noise_list) < len(self.item_list):
                self.noise_list = self.noise_list * int(np.ceil(len(self.item_list) / len(self.noise_list)))
            assert len(self.noise_list) >= len(self.item_list)

    def plan(self, index):
        """The host half of DataSet.__getitem__ (data_loader.py:109-125): (clean id, noise id, start, gains) with the draws
        add_noise makes -- or (clean id, None, 0, no gains) in the paired mode.  IndexError where the reference raises it.
        With rir= a fifth element, the response's id or None for an item that stays dry: np.random.uniform(0, 1) and
        np.random.randint(0, len(rir)) are drawn first, always both and in that order, then add_noise's draws (they depend
        on lengths only, which reverberation does not change); the item stays dry when the uniform draw is >= rir_prob."""
        if self.noise is not None:
            cid, nid = self.item_list[index], self.noise_list[index]
            if self.rir is not None:
                u, rid = np.random.uniform(0, 1), int(np.random.randint(0, len(self.rir)))
                start, gains = plan_noise(self.clean.lengths[cid], self.noise.lengths[nid])
                return cid, nid, start, gains, (rid if u < self.rir_prob else None)
            start, gains = plan_noise(self.clean.lengths[cid], self.noise.lengths[nid])
            return cid, nid, start, gains
        return self.item_list[index], None, 0, np.zeros(0, np.float64)

    def __len__(self):
        return len(self.item_list)

    def __call__(self, *args, **kwargs):
        return self

    def shuffle(self):
        np.random.shuffle(self.item_list)


class Sampler(object):
    """data_loader.py:137-168 as train.py uses it (drop_last=False), quirks included: the item list is extended by its own
    tail to the next multiple of batch_size -- by a whole batch when it already is one --, and the bins are shuffled in
    place, so they stay shuffled across epochs."""

    def __init__(self, dataset, batch_size, start_index=0, drop_last=False):
        if drop_last:
            raise NotImplementedError("drop_last=True is not built (train.py does not use it)")
        self.dataset = dataset
        self.batch_size = batch_size
        self.start_index = start_index
        last_size = (int(len(self.dataset) / batch_size) + 1) * batch_size - len(self.dataset)
        self.dataset.item_list.extend(self.dataset.item_list[-last_size:])
        ids = list(range(len(self.dataset)))
        self.bins = [ids[i:i + self.batch_size] for i in range(0, len(ids), self.batch_size)]
        self.indices = (np.random.permutation(len(self.bins) - self.start_index) + self.start_index).tolist()

    def __iter__(self):
        for x in self.indices:
            batch_ids = self.bins[x]
            np.random.shuffle(batch_ids)
            yield batch_ids

    def __len__(self):
        return len(self.bins) - self.start_index

    def reset_start_index(self, start_index):
        self.start_index = start_index

    def __call__(self, *args, **kwargs):
        return self

    def iter_num(self):
        return len(self.indices)


class DataLoader(object):
    """data_loader.py:171-262 with the batch built on the device.  Iterating yields the reference's 4-tuple
    (batch_mix, batch_clean, mix_sig, clean_sig): two [N, T, 129, 1] float32 device tensors, zero past each utterance's
    frames as padding_batch leaves them (None with use_complex=True, see DataSet), and two PcmRows.  np.random is
    consumed in the order of the reference's loader with num_works=1: the sampler's shuffle of a bin, then add_noise's
    draws item by item (with more workers the reference draws in forked processes and repeats nothing)."""

    def __init__(self, dataset, batch_size, sampler=None):
        self.dataset = dataset
        self.batch_size = batch_size
        self.sampler = sampler
        if self.sampler is None:
            self.bins = []
            for i in range(0, len(self.dataset), self.batch_size):
                self.bins.append(list(range(i, min(i + self.batch_size, len(self.dataset)))))

    def plans(self):
        """The host half of an epoch: per batch the list of DataSet.plan tuples, drawn lazily, batch by batch."""
        if self.sampler is not None:
            if self.sampler.batch_size != self.batch_size:
                self.batch_size = self.sampler.batch_size
                print("Warrning: sampler.batch_size != batch_size. batch_size changed!")
            source = self.sampler
        else:
            source = self.bins
        for index_list in source:
            yield [self.dataset.plan(index) for index in index_list]

    def build(self, plan):
        """One batch on the device from its plan: gather the speech into rows 0..N of a [2N, Ls] buffer, the noise -- only the
        ls samples add_noise keeps where it is longer than the speech, whole where it is shorter -- into [N, <= Ls], mix
        into rows N..2N, one STFT over the 2N rows.  Paired mode: both halves are gathered.
        With DataSet(rir=...): the gathered speech is convolved with its rows' responses at shift = direct in one launch (the
        rows that stay dry take the one-tap identity, which returns them bit for bit), the noise is mixed into the
        result, and rows 0..N hold what `target` names."""
        import torch
        ds = self.dataset
        n = len(plan)
        cids = [p[0] for p in plan]
        ls = [int(ds.clean.lengths[c]) for c in cids]
        if ds.mix is not None:
            lm = [int(ds.mix.lengths[c]) for c in cids]
            width = (max(ls + lm) + 3) // 4 * 4
            both = torch.empty((2 * n, width), dtype=torch.float32, device=ds.clean.arena.device)
            ds.clean.gather(cids, L=width, out=both[:n])
            ds.mix.gather(cids, L=width, out=both[n:])
        else:
            lm = ls
            width = (max(ls) + 3) // 4 * 4           # every row starts 16-byte aligned
            both = torch.empty((2 * n, width), dtype=torch.float32, device=ds.clean.arena.device)
            if ds.rir is None:
                speech = ds.clean.gather(cids, L=width, out=both[:n])
            else:
                rids = [p[4] for p in plan]
                filt, taps, shifts = ds.rir.filters(rids)
                dry = ds.clean.gather(cids, L=width, out=both[:n] if ds.target == "dry" else None)
                speech = audio.convolve_batch(dry, filt, ls, taps, shifts, out=both[:n] if ds.target == "reverberant" else None)
                if ds.target == "early":
                    early = [ds.rir.early_taps(r, ds.early_ms) if r is not None else 1 for r in rids]
                    audio.convolve_batch(dry, filt, ls, early, shifts, out=both[:n])
            nids, starts, counts, gains = [], [], [], []
            for (_, nid, start, g), s in zip([p[:4] for p in plan], ls):
                ln = int(ds.noise.lengths[nid])
                nids.append(nid)
                starts.append(start if ln > s else 0)
                counts.append(s if ln > s else ln)         # cropped to the speech: it mixes as ln == ls, start 0, no gains
                gains.append(g)
            noise = ds.noise.gather(nids, starts, counts)
            audio.mix_snr_batch(speech, noise, ds.snr, speech_lengths=ls, noise_lengths=counts, gains=gains, out=both[n:])
        clean_sig, mix_sig = PcmRows(both[:n], ls), PcmRows(both[n:], lm)
        if ds.complex:
            return None, None, mix_sig, clean_sig
        mag, _ = audio.stft_batch(both, ls + lm, with_phase=False, framing=ds.framing)
        return mag[n:], mag[:n], mix_sig, clean_sig

    def __iter__(self):
        for plan in self.plans():
            yield self.build(plan)

    def __len__(self):
        if self.sampler is not None:
            return len(self.sampler)
        return len(self.bins)

    def shuffle(self):
        self.dataset.shuffle()
