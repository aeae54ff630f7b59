"""Host-side mirror of the reference's evaluation engines for the forward hot path.

Reference: BaseTester / FullyCNNTester (model_utils/tester.py:18-90) and InferenceEngine
(infer.py:19-52): read cfg -> creat_graph() -> _init_session() -> _load_checkpoint() ->
test_step(ndarray[N,T,129,1]) -> ndarray[N,T,129,1], and the evaluation loop over it (tester.py:92-167):
`evaluate_pcm` / `test` take ragged PCM through STFT -> net -> ISTFT rebuild -> SDR (and STOI, ESTOI, SI-SDR, segmental SNR, LLR, WSS, fwSNRseg, CD, the SDR of BSS Eval on request) on the device.
PESQ scoring and the evaluation loop's wav files are not mirrored; the manifest-driven DataLoader is loader.DataLoader (batches built on the device).
"""

import numpy as np

from . import model as _model, spec, weights as _weights
from ._args import check_rebuild
from .evaluation import EVERY_EXTRA, check_extra
from .metrics import AverageMeter


class FullyCNNTester(object):
    """test_config: a configparser-like object (config.py:9-12) or None with keyword overrides.

    Keys read, as the reference does: [model] net_work (tester.py:21-22), [testing]
    checkpoint_filepath (tester.py:20) -- a TF V2 checkpoint prefix, a frozen .pb or a .npz of TF variables --, [data] feature_dim
    (tester.py:54).  The shipped infer cfgs name the section [inference]: both are accepted.
    """

    def __init__(self, test_config=None, net_work=None, checkpoint_file=None, weights=None, device=0, reuse_output=False):
        self.device = device
        # test_step's default already avoids the page faults of a fresh 67 MB ndarray per call (model.HostOutputPool: a new ndarray object
        # over recycled warm pages, never one the caller still holds).  reuse_output is the blunt form: one of TWO pooled arrays per shape,
        # alternating, whatever the caller holds -- the result of call k is overwritten by call k + 2.
        self.reuse_output = bool(reuse_output)
        self._out_pool = {}
        self.net_work = net_work
        self.checkpoint_file = checkpoint_file
        self.feature_dim = spec.FEATURE_DIM
        if test_config is not None:
            self.net_work = test_config.get("model", "net_work")
            for section in ("testing", "inference"):
                if test_config.has_section(section) and test_config.has_option(section, "checkpoint_filepath"):
                    self.checkpoint_file = test_config.get(section, "checkpoint_filepath")
                    break
            if test_config.has_option("data", "feature_dim"):
                self.feature_dim = int(test_config.get("data", "feature_dim"))
        if self.feature_dim != spec.FEATURE_DIM:
            raise ValueError("feature_dim must be %d (nfft 256), got %d" % (spec.FEATURE_DIM, self.feature_dim))
        self._weights = weights
        self.sdr_score = AverageMeter()     # tester.py:63; test() adds to it and never resets it, as there
        self.stoi_score = AverageMeter()    # tester.py:62; filled by test(..., stoi=True)
        self.extra_scores = {name: AverageMeter() for name in EVERY_EXTRA}    # filled by test(..., extra=(names))
        self.creat_graph()
        self._load_checkpoint()

    def creat_graph(self):
        """tester.py:69-83: pick the model by net_work and build pred = model(input_x)."""
        if self.net_work not in ("FullyCNNV2", "FullyCNNV3"):
            print("net_work set default or not wright. Use FullyCNN")
        self.model = _model.build_model(self.net_work, is_training=False, device=self.device)

    def _load_checkpoint(self):
        """tester.py:36-39."""
        if self._weights is not None:
            self.model.restore(self._weights)
        elif self.checkpoint_file:
            self.model.restore(_weights.load(self.checkpoint_file, self.model.variant))
            print("recover from checkpoint_file: {}".format(self.checkpoint_file))

    def param_count(self):
        """tester.py:41-47."""
        n = self.model.param_count()
        print("\nTotal number of Parameters: {}\n".format(n))
        return n

    def test_step(self, input_x, out=None):
        """tester.py:85-90: output = sess.run(self.pred, {self.input_x: input_x}).
        `out`: a caller-owned C-contiguous float32 ndarray of the input's shape to write into; with reuse_output=True (and no
        `out`) the result lands in one of two pooled arrays of this shape, alternating."""
        if out is None and self.reuse_output and isinstance(input_x, np.ndarray):
            key = tuple(input_x.shape)
            pool = self._out_pool.get(key)
            if pool is None:
                pool = self._out_pool[key] = [np.empty(key, np.float32), np.empty(key, np.float32), 0]
                if len(self._out_pool) > 4:                       # a few shapes at most: drop the oldest
                    self._out_pool.pop(next(iter(self._out_pool)))
            out = pool[pool[2]]
            pool[2] ^= 1
        return self.model(input_x, out=out) if out is not None else self.model(input_x)

    def evaluate_pcm(self, mix_sig, clean_sig, nfft=512, model=None, lengths=None, kernels="x6", stoi=False, extra=(), rebuild="reference",
                     framing=None):
        """One batch of the evaluation loop (tester.py:100-146) from PCM, on the device: the module's evaluate_pcm with
        this engine's network, or with `model` (a callable, device [N, T, 129, 1] -> same) in its place."""
        return evaluate_pcm(model if model is not None else self.model, mix_sig, clean_sig, nfft, self.device, lengths, kernels,
                            stoi=stoi, extra=extra, rebuild=rebuild, framing=framing)

    def test(self, valid_loader, stoi=False, extra=(), rebuild="reference"):
        """tester.py:92-167 over anything that yields the reference's 4-tuple (batch_mix, batch_clean, mix_sig,
        clean_sig): every batch goes through evaluate_pcm(mix_sig, clean_sig), every utterance's SDR into
        self.sdr_score (an AverageMeter); prints the reference's summary line with its SDR field and returns the
        average.  The spectrogram is recomputed on the device from mix_sig (equal to batch_mix within the STFT's
        pinned 2e-6 of the scale), so batch_mix / batch_clean are not read.  With stoi=True every utterance's STOI goes
        into self.stoi_score as well and the line gains the reference's st_score field, in the reference's order.
        extra: names from evaluation.EXTRA_METRICS ("estoi", "si_sdr", "seg_snr") and evaluation.SPECTRAL_METRICS ("llr", limited
        at 2, and "wss"), evaluation.PROJECTION_METRICS ("bss_sdr", BSS Eval's SDR with 512 taps) and evaluation.SEPM_METRICS
        ("fw_seg_snr", the frequency-weighted segmental SNR, and "cd", the cepstral distance at LLR's order); every utterance's score goes into self.extra_scores[name], and one further line with their averages follows the reference's.
        rebuild: "reference" (the rebuild the reference's scores are made with) or "ola" (weighted overlap-add: evaluate_pcm).
        The framing is valid_loader.dataset.framing where the loader has one (loader.DataSet(framing=...)), as the reference
        reads window_s from the dataset; else the default.
        PESQ and the wav files the reference writes next to the scores are not built; everything else the composite measures
        need is (metrics.composite)."""
        extra = check_extra(extra)
        check_rebuild(rebuild)
        framing = loader_framing(valid_loader)
        for _batch_mix, _batch_clean, mix_sig, clean_sig in valid_loader:
            scores = self.evaluate_pcm(mix_sig, clean_sig, stoi=stoi, extra=extra, rebuild=rebuild, framing=framing)
            feed_meters(self, scores, stoi, extra)
        if stoi:
            print("Average st_score: {:.4f}; Average sd_score: {:.4f}.\n".format(self.stoi_score.avg, self.sdr_score.avg))
        else:
            print("Average sd_score: {:.4f}.\n".format(self.sdr_score.avg))
        if extra:
            print(extra_line(extra, self.extra_scores))
        return self.sdr_score.avg


def feed_meters(owner, scores, stoi, extra):
    """One batch's scores, as evaluate_pcm returns them, into the owner's sdr_score, stoi_score and extra_scores meters, utterance by
    utterance: what test() and valid() do alike."""
    for score in scores[1]:
        owner.sdr_score.update(float(score))
    if stoi:
        for score in scores[2]:
            owner.stoi_score.update(float(score))
    for name in extra:
        for score in scores[-1][name]:
            owner.extra_scores[name].update(float(score))


def extra_line(extra, meters):
    """The line test() and valid() add under the reference's when extra scores were asked for."""
    return "; ".join("Average {}: {:.4f}".format(name, meters[name].avg) for name in extra) + ".\n"


def loader_framing(loader):
    """The framing a loader's batches were cut with: loader.dataset.framing, or None (the default) where there is none."""
    return getattr(getattr(loader, "dataset", None), "framing", None)


def evaluate_pcm(forward, mix_sig, clean_sig, nfft=512, device=0, lengths=None, kernels="x6", stoi=False, extra=(), rebuild="reference",
                 framing=None):
    """What FullyCNNTester.test and FullyCNNTrainer.valid do with one batch (tester.py:104-146, trainer.py:264-307), each
    with its own forward (device [N, T, 129, 1] -> same): one upload, STFT with the lengths -> forward -> ISTFT rebuild
    (AudioReBuild(nfft), 512 as the reference ships it) -> SDR against the clean rows; the audio and N scores come back.
    mix_sig, clean_sig: lists of 1-D float arrays of ragged lengths (utterance i is scored over len(clean_sig[i]), the
    reference's sig_length_list), or two zero-padded device tensors [N, L] with `lengths`, or two loader.PcmRows (padded
    device rows that carry their lengths: the device loader's batches, scored where they lie).  kernels: the STFT / ISTFT
    kernel family, as in audio.stft_batch.
    Returns (denoise: list of numpy float32, row i trimmed to its length; sdr: numpy float64 [N]); with stoi=True a third
    element, STOI per utterance (numpy float64 [N], audio.stoi_batch of the rebuilt audio against the clean rows).
    extra: names from evaluation.EXTRA_METRICS + evaluation.SPECTRAL_METRICS + evaluation.PROJECTION_METRICS +
    evaluation.SEPM_METRICS ("estoi", "si_sdr", "seg_snr", "llr", "wss", "bss_sdr", "fw_seg_snr", "cd"; anything else is a ValueError
    before any device work).  With extra non-empty the tuple gains one last element, a dict
    name -> numpy float64 [N] (audio.stoi_batch(extended=True), audio.si_sdr_batch, audio.seg_snr_batch, audio.llr_batch
    with its limit of 2, audio.wss_batch, audio.bss_sdr_batch with 512 taps, audio.fw_seg_snr_batch, audio.cep_dist_batch at
    LLR's order, of the same pairs).
    rebuild: "reference" (AudioReBuild as shipped, the default) or "ola" (weighted overlap-add, audio.istft_batch: utterance i is
    rebuilt from its own num_frames(length) frames, nfft plays no part); anything else, or "ola" with kernels="f32", is a
    ValueError before any device work.
    framing: an audio.Framing (STFT and rebuild are cut by it; the reference rebuild exists for hamming windows only), or None
    for the default, 256 / 128 / hamming."""
    extra = check_extra(extra)
    check_rebuild(rebuild, kernels)
    import torch
    from . import _args, audio
    if rebuild == "reference":
        audio.check_reference_rebuild(framing)
    empty = ([], np.zeros(0, np.float64)) + ((np.zeros(0, np.float64),) if stoi else ())
    if extra:
        empty += ({name: np.zeros(0, np.float64) for name in extra},)
    if hasattr(mix_sig, "rows") and hasattr(clean_sig, "rows"):      # loader.PcmRows: what the device loader yields
        if len(mix_sig) != len(clean_sig) or list(mix_sig.lengths) != list(clean_sig.lengths):
            raise ValueError("mix_sig and clean_sig must pair up, utterance by utterance and sample by sample")
        lens = [int(v) for v in clean_sig.lengths]
        if not lens:
            return empty
        mix, clean = mix_sig.rows, clean_sig.rows
    elif hasattr(mix_sig, "is_cuda"):
        if lengths is None:
            raise ValueError("padded device tensors need lengths")
        lens = _args.host_ints(lengths)
        mix, clean = mix_sig, clean_sig
    else:
        lens = [len(c) for c in clean_sig]
        if len(mix_sig) != len(lens) or any(len(m) != n for m, n in zip(mix_sig, lens)):
            raise ValueError("mix_sig and clean_sig must pair up, utterance by utterance and sample by sample")
        if not lens:
            return empty
        both = np.zeros((2, len(lens), max(lens)), np.float32)
        for i, n in enumerate(lens):
            both[0, i, :n] = mix_sig[i]
            both[1, i, :n] = clean_sig[i]
        both = torch.as_tensor(both, device="cuda:%d" % device)
        mix, clean = both[0], both[1]
    scored = audio.denoise_and_score(forward, mix, clean, lens, nfft, kernels, stoi=stoi, extra=extra, rebuild=rebuild, framing=framing)
    audio_host = scored[0].cpu().numpy()
    host = lambda s: {k: v.cpu().numpy() for k, v in s.items()} if isinstance(s, dict) else s.cpu().numpy()      # noqa: E731
    return ([audio_host[i, :lens[i]].copy() for i in range(len(lens))],) + tuple(host(s) for s in scored[1:])


class InferenceEngine(FullyCNNTester):
    """infer.py:19-52, the forward slice: `denoise_magnitude` is infer.py:62-65 without the
    STFT/ISTFT around it."""

    def denoise_pcm(self, sig, nfft=512, sample_rate=8000, rebuild="reference", framing=None):
        """infer.py:54-71 end to end on the device: STFT (audio_feature.py) -> model -> rebuild (utils.py:171-183).
        The magnitude is laid out [1, T, 129, 1] by TRANSPOSE, as the batch loader does
        (data_loader.py:206-208); infer.py:59 itself reshapes without transposing.
        sig: 1-D float PCM at 8 kHz.  Returns the denoised signal, same length, numpy float32.
        sample_rate other than 8000: sig is at that rate and is resampled to 8 kHz on the device first (audio.resample_batch:
        what infer.py's librosa.load(sr=8000) does to a file); the result is at 8 kHz, audio.resample_length samples.
        rebuild: "reference" (utils.py:171-183 as shipped) or "ola" (weighted overlap-add, audio.istft_batch; nfft plays no part).
        framing: an audio.Framing, the framing the network was trained with, or None for the default (the cfg key `windows` is
        not read, as in the reference: a checkpoint is never fed another window silently)."""
        import torch
        from . import audio
        check_rebuild(rebuild)
        if rebuild == "reference":
            audio.check_reference_rebuild(framing)
        dev = "cuda:%d" % self.device
        if int(sample_rate) != audio.SAMPLE_RATE:
            rows, lens = audio.resample_batch(np.asarray(sig, dtype=np.float32).reshape(1, -1), sample_rate, audio.SAMPLE_RATE,
                                              device=self.device)
            pcm, n = rows[:, :lens[0]], lens[0]
        else:
            pcm, n = torch.as_tensor(np.asarray(sig, dtype=np.float32), device=dev)[None], len(sig)
        mag, phase = audio.stft_batch(pcm, framing=framing)
        pred = self.model(mag)
        out = audio.istft_batch(pred, phase, nfft, rebuild=rebuild, framing=framing)
        return out[0, :n].cpu().numpy()

    def denoise_file(self, path, save_dir=None, nfft=512, rebuild="reference", framing=None):
        """infer.py:54-76 for one wav file: PCM16 of any rate and channel count is downmixed and resampled to 8 kHz on the
        device (loader.read_wav_frames + audio.resample_batch, in place of librosa.load(sr=8000)), denoised as denoise_pcm
        does, and -- with save_dir -- written as PCM16 at 8 kHz to save_dir/<basename with .wav -> _de.wav> (infer.py:72-76's
        name; int16 by clip(rint(y * 32768))).  Returns the denoised float32 signal.  rebuild, framing: as in denoise_pcm."""
        import os
        import wave
        from . import audio, loader
        check_rebuild(rebuild)
        if rebuild == "reference":
            audio.check_reference_rebuild(framing)
        frames, rate = loader.read_wav_frames(path)
        rows, lens = audio.resample_batch(frames[None], rate, audio.SAMPLE_RATE, device=self.device)
        n = lens[0]
        mag, phase = audio.stft_batch(rows[:, :n], framing=framing)
        out = audio.istft_batch(self.model(mag), phase, nfft, rebuild=rebuild, framing=framing)[0, :n].cpu().numpy()
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
            pcm16 = np.clip(np.rint(out.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2")
            w = wave.open(os.path.join(save_dir, os.path.basename(path).replace(".wav", "_de.wav")), "wb")
            try:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(audio.SAMPLE_RATE)
                w.writeframes(pcm16.tobytes())
            finally:
                w.close()
        return out

    def denoise_stream(self, chunks, hops=8, nfft=512, sample_rate=8000, output_rate=None, rebuild="reference", block=None, framing=None):
        """denoise_pcm for audio that arrives in pieces: a generator over an iterable of 1-D PCM pieces of any size.  The
        pieces are re-blocked to whole hops (128 samples) and pushed, at most `hops` hops at a time, through a one-lane
        audio.StreamingDenoiser; every push's output is yielded as it comes (numpy float32, the result delayed by 640
        samples, zeros first), then what the stream still owed.  All pieces joined, with the leading zeros dropped, equal
        denoise_pcm of the joined input.
        sample_rate / output_rate: the pieces are mono float at sample_rate and re-blocked to that rate's hop; the lane is
        StreamingDenoiser(sample_rate=..., output_rate=...), which see for the delay and the rates it refuses.
        rebuild: "reference" or "ola", as in denoise_pcm; the delay is the same.
        block: None, or a number of frames: the pieces are cut to blocks of that size and go through a one-lane
        audio.BlockDenoiser(block=..., sample_rate=..., output_rate=...), which serves every rate (44.1 kHz too) and yields block *
        output_rate / sample_rate samples a block, the result delayed by audio.block_delay(block, sample_rate, output_rate);
        `hops` plays no part.
        framing: an audio.Framing (None: the default): the pieces are re-blocked to hops of its stride, through
        StreamingDenoiser(framing=...); the result is denoise_pcm(..., framing=framing) delayed by audio.stream_delay_fr(framing).
        8 kHz only, and without `block`: anything else with a framing is a ValueError."""
        from . import audio
        check_rebuild(rebuild)
        if block is not None:
            lane = audio.BlockDenoiser(self.model, 1, int(block), sample_rate=sample_rate, output_rate=output_rate, nfft=nfft, rebuild=rebuild,
                                       framing=framing)
            try:
                held = np.zeros(0, np.float32)
                for piece in chunks:
                    held = np.concatenate([held, np.asarray(piece, np.float32).reshape(-1)])
                    while held.size >= lane.block:
                        yield lane.process(held[None, :lane.block])[0]
                        held = held[lane.block:]
                yield lane.finish([0], [held])[0]
            finally:
                lane.close()
            return
        stream = audio.StreamingDenoiser(self.model, 1, max_hops=int(hops), nfft=nfft, sample_rate=sample_rate, output_rate=output_rate,
                                         rebuild=rebuild, framing=framing)
        hop = stream.hop_in
        try:
            held = np.zeros(0, np.float32)
            for piece in chunks:
                held = np.concatenate([held, np.asarray(piece, np.float32).reshape(-1)])
                while held.size >= hop:
                    k = min(held.size // hop, stream.max_hops)
                    yield stream.push(held[None, :k * hop])[0]
                    held = held[k * hop:]
            yield stream.finish([0], [held])[0]
        finally:
            stream.close()

    def denoise_magnitude(self, mag):
        mag = np.asarray(mag, dtype=np.float32)
        if mag.ndim == 2:  # [T, 129] -> [1, T, 129, 1]  (a transpose-correct version of infer.py:59)
            mag = mag[None, :, :, None]
        return self.test_step(mag)
