"""Host-side mirror of the reference's training step, over the C ABI (rced_train_*).

Reference: FullyCNNTrainer (model_utils/trainer.py:121-192) -- creat_graph builds
`pred = Model(is_training=True)(input_x)`, `loss = sum((target - pred)^2) / batch_size`, Adam under the
BatchNorm UPDATE_OPS; train_step runs `[loss, summaries, global_step, train_op]`; the training loop feeds the
learning rate: `init_lr` for the first step, then the Noam schedule of the returned global step
(trainer.py:27,68-76,215).  `train` is the epoch loop (trainer.py:194-243) over a loader that yields the reference's 4-tuple
-- loader.DataLoader builds the batches on the device --, with a checkpoint per epoch under the reference's name.  TF
summaries are not built.

The step in shards: `grad_step` runs forward, loss and backward of one shard into the trainer's exchange
tensors and changes nothing else, `apply_step` updates the moving statistics and runs Adam once from them;
`train_step_sharded` is one optimizer step over a list of shards, and `accumulate=k` makes train_step / fit_step / train
cut every batch into k of them.  BatchNorm normalises every shard by its own statistics.  dist.DataParallelTrainer runs
the same step with the shards on ranks.  Opt-in, `sync_bn=True` (train_step_sharded, DataParallelTrainer): BatchNorm over the
union of the shards -- `grad_step_sync` is a shard's pass as a generator that stops at every BatchNorm layer, forward and
backward, for the caller to add up the shards' sums; the step is then the unsharded one.
"""

import ctypes
import os
import time

import numpy as np

from . import _args, _lib, model as _model, spec, weights as _weights
from .evaluation import EVERY_EXTRA, check_extra
from .objective import WaveObjective
from .metrics import AverageMeter


def checkpoint_path(checkpoints_path, net_arch, net_work, epoch, global_step):
    """trainer.py:232-238: {checkpoints_path}/{arch}_{net}/{arch}_{net}_{epoch}_{global_step-1}.ckpt."""
    return os.path.join(checkpoints_path + "/{}_{}".format(net_arch, net_work),
                        "{}_{}_{}_{}.ckpt".format(net_arch, net_work, epoch, global_step - 1))


def accumulation_slices(n, k):
    """The k contiguous row ranges `accumulate=k` cuts a batch of n rows into (dist.shard_bounds: balanced, the first
    n % k one row longer).  k > n would leave a shard without rows: ValueError."""
    from .dist import shard_bounds
    n, k = int(n), int(k)
    if k < 1:
        raise ValueError("accumulate must be a positive integer, got %d" % k)
    if k > n:
        raise ValueError("cannot cut a batch of %d rows into %d shards: every shard needs at least one row" % (n, k))
    return shard_bounds(n, k)


def start_epoch(continue_from):
    """trainer.py:198-201: the epoch after the one a checkpoint's name carries; 0 without a checkpoint."""
    return int(continue_from.split("_")[-2]) + 1 if continue_from is not None else 0


def run_epochs(tr, fit_step, train_loader, valid_loader, epochs, logger, checkpoints_path, net_arch, num_iter_print, root):
    """The epoch loop of trainer.py:194-243 over `fit_step` (FullyCNNTrainer.train, dist.DataParallelTrainer.train); tr: the
    FullyCNNTrainer whose meters, checkpoints and valid() it uses.  root=False (a data-parallel rank other than 0): the same
    steps and validations without the progress lines, the log and the checkpoints."""
    global_step = 0
    for epoch in range(start_epoch(tr.continue_from), epochs):
        train_batch_id = 0
        train_loader.shuffle()
        start_time = time.time()
        for batch_mix, batch_clean, mix_sig, clean_sig in train_loader:
            train_batch_id += 1
            tr.data_time.update(time.time() - start_time)
            start_time = time.time()
            if tr.has_wave_term:
                from .engine import loader_framing
                fr = loader_framing(train_loader)
                wave = wave_of_batch(train_loader, batch_mix, mix_sig, clean_sig)
                if fr is None or fr.is_default:     # today's call, for a fit_step that knows no framing
                    batch_loss, _, global_step = fit_step(batch_mix, batch_clean, wave=wave)
                else:
                    batch_loss, _, global_step = fit_step(batch_mix, batch_clean, wave=wave, framing=fr)
            else:
                batch_loss, _, global_step = fit_step(batch_mix, batch_clean)
            tr.train_loss.update(batch_loss, n=1)
            tr.batch_time.update(time.time() - start_time)
            if root and train_batch_id % num_iter_print == 0:
                print("epoch: {}, batch: {}/{}, "
                      "TrainLoss: {train_loss.val:.4f}({train_loss.avg:.4f}), "
                      "DataTime: {data_time.val:.3f}({data_time.avg:.3f}), "
                      "BatchTime: {batch_time.val:.3f}({batch_time.avg:.3f})".format(
                          epoch, train_batch_id, len(train_loader), train_loss=tr.train_loss,
                          data_time=tr.data_time, batch_time=tr.batch_time))
            start_time = time.time()
        if root and checkpoints_path is not None:
            path = checkpoint_path(checkpoints_path, net_arch, tr.net_work, epoch, global_step)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            tr.save_checkpoint(path)
        if (epoch + 1) % 5 == 0:
            if root:
                tr.valid(valid_loader, epoch, logger)
            else:
                tr.valid(valid_loader, epoch, None, verbose=False)
    return global_step


def wave_of_batch(loader, batch_mix, mix_sig, clean_sig):
    """The `wave` argument of a step from a loader's 4-tuple: (the mixture's unit phase [N, T, 129] complex64, the clean rows, the
    samples scored per utterance: min(len(mix), len(clean))).  The phase is audio.stft_batch's of the mixture's rows at the loader's
    framing (engine.loader_framing), whose magnitudes are the loader's batch_mix bit for bit.  mix_sig, clean_sig: loader.PcmRows
    (the device loader's batches)."""
    from . import audio
    from .engine import loader_framing
    fr = loader_framing(loader)
    if not (hasattr(mix_sig, "rows") and hasattr(clean_sig, "rows")) or len(mix_sig) != len(clean_sig):
        at = "" if fr is None or fr.is_default else " (a loader whose framing is %r)" % (fr,)
        raise ValueError("an objective with a wave term needs the loader's mix_sig and clean_sig as device rows (loader.PcmRows), one pair "
                         "per utterance%s" % at)
    _, phase = audio.stft_batch(mix_sig.rows, mix_sig.lengths, frames=int(batch_mix.shape[1]), with_phase=True, framing=fr)
    return phase, clean_sig.rows, [min(a, b) for a, b in zip(mix_sig.lengths, clean_sig.lengths)]


class FullyCNNTrainer(object):
    model = None

    def __init__(self, net_work="FullyCNNV3", batch_size=1, lr=1e-3, warmup_steps=4000.0, weights=None, device=0,
                 seed=None, accumulate=1, objective=None):
        if objective is not None and not isinstance(objective, WaveObjective):
            raise ValueError("objective must be an audio.WaveObjective or None (the spectral loss), got %r" % (objective,))
        self.objective = objective                 # None: sum((target - pred)^2) / batch_size, the reference's loss
        self.loss_parts = None                     # the last step's unweighted (spectral, wave_sse, si_sdr[, mr_stft]) sums, with an objective
        if isinstance(accumulate, bool) or int(accumulate) != accumulate or int(accumulate) < 1:
            raise ValueError("accumulate must be a positive integer (1: the whole batch in one piece), got %r" % (accumulate,))
        self.accumulate = int(accumulate)          # train_step cuts its batch into this many shards (gradient accumulation)
        self._exch = None                          # (gradient fp32, statistics sums fp64): the sharded step's exchange tensors
        self._sync_xs = None                       # the synchronised step's exchange tensor (grad_step_sync yields it)
        self._replicas = []                        # train_step_sharded(sync_bn=True): one more trainer per further shard
        self.net_work = net_work
        self.variant = spec.variant_of(net_work)
        self.batch_size = int(batch_size)          # [training] batch_size: what the loss divides by
        self.init_lr = float(lr)                   # [training] lr
        self.lr = float(lr)                        # fed for the next step (trainer.py:27)
        self.warmup_steps = float(warmup_steps)    # [training] warmup_steps
        self.device = int(device)
        self.sdr_score = AverageMeter()            # trainer.py:34; valid() adds to it and never resets it, as there
        self.stoi_score = AverageMeter()           # trainer.py:33; filled by valid(..., stoi=True)
        self.extra_scores = {name: AverageMeter() for name in EVERY_EXTRA}    # filled by valid(..., extra=(names))
        self.train_loss = AverageMeter()           # trainer.py:29-31; train() updates the three
        self.data_time = AverageMeter()
        self.batch_time = AverageMeter()
        self.continue_from = None                  # trainer.py:24; from_checkpoint records the path, train() resumes after its epoch
        w = weights if weights is not None else _weights.initial_weights(self.variant, seed)
        self._blob_n = spec.num_weights(self.variant)
        # creat_graph (trainer.py:165-172): self.model = Model(is_training=True); self.pred = self.model(self.input_x).
        # The model object owns the library's training handle; train_step runs on the same one.
        self.model = _model.build_model(net_work, True, weights=w, device=self.device, batch_size=self.batch_size)

    @property
    def _h(self):
        """The library's training handle, looked up on every call: the model object owns it, and
        `trainer.model.restore(w)` / `trainer.model.close()` replace / free it (a cached pointer would dangle)."""
        h = self.model._train if self.model is not None else None
        if h is None:
            raise RuntimeError("the trainer's model is closed")
        return h

    def noam_scheme(self, global_step, warmup_steps=None):
        """trainer.py:68-76."""
        w = self.warmup_steps if warmup_steps is None else warmup_steps
        step = global_step + 1
        return self.init_lr * w ** 0.5 * min(step * w ** -1.5, step ** -0.5)

    def _on_device(self, input_x, target_y):
        import torch
        dev = "cuda:%d" % self.device
        x = torch.as_tensor(np.asarray(input_x, dtype=np.float32) if not hasattr(input_x, "is_cuda") else input_x,
                            device=dev).float().contiguous()
        y = torch.as_tensor(np.asarray(target_y, dtype=np.float32) if not hasattr(target_y, "is_cuda") else target_y,
                            device=dev).float().contiguous()
        if x.dim() != 4 or x.shape[2] != spec.FEATURE_DIM or x.shape[3] != 1 or x.shape != y.shape:
            raise ValueError("input and target must both be [N, T, 129, 1]")
        return x, y

    # -- the objective ----------------------------------------------------------------
    @property
    def has_wave_term(self):
        return self.objective is not None and self.objective.has_wave_term

    @property
    def _plain(self):
        """The reference's loss, through the entries that have always computed it: no objective, or the spectral term alone at weight 1."""
        o = self.objective
        return o is None or (not o.has_wave_term and o.spectral == 1.0)

    def _wave_args(self, wave, x):
        """rced_wave_args for a step over x [N, T, 129, 1] from wave = (phase [N, T, 129] complex, clean rows [N, >= max length],
        N lengths), and the tensors it points into."""
        import torch
        o = self.objective
        if o is None or not o.has_wave_term:
            if wave is not None:
                raise ValueError("wave=... was given, but the trainer's objective %r has no wave term" % (o,))
        a = _lib.WaveArgs(o.spectral, o.wave_sse, o.si_sdr, int(o.skip_edges), None, None, 0, None, None)
        if not o.has_wave_term:
            return a, ()
        if wave is None:
            raise ValueError("the trainer's objective %r has a wave term (wave_sse or si_sdr) and the step was given wave=None: it needs "
                             "wave=(phase, clean_rows, lengths)" % (o,))
        phase, clean, lengths = wave
        n, t = int(x.shape[0]), int(x.shape[1])
        if not (hasattr(phase, "is_cuda") and phase.is_cuda and phase.device == x.device and tuple(phase.shape) == (n, t, spec.FEATURE_DIM)):
            raise ValueError("wave[0], the phase, must be a complex [N = %d, T = %d, 129] tensor on %s" % (n, t, x.device))
        ph = torch.view_as_real(phase.to(torch.complex64).contiguous()).contiguous()
        clean = _args.rows(clean, "wave[1], the clean rows,")
        if int(clean.shape[0]) != n or clean.device != x.device:
            raise ValueError("wave[1], the clean rows, must hold N = %d rows on %s" % (n, x.device))
        lens = _args.host_ints(lengths, n, "wave[2], the lengths,")
        if any(v < 0 or v > int(clean.shape[1]) for v in lens):
            raise ValueError("wave[2], the lengths, must lie in [0, %d]" % int(clean.shape[1]))
        ldev = torch.tensor(lens, dtype=torch.int32, device=x.device)
        a.phase_dev, a.clean_dev, a.clean_stride, a.lengths_dev = ph.data_ptr(), clean.data_ptr(), _args.row_stride(clean), ldev.data_ptr()
        return a, (ph, clean, ldev)

    @staticmethod
    def _wave_rows(wave, a, b):
        return None if wave is None else (wave[0][a:b], wave[1][a:b], list(_args.host_ints(wave[2]))[a:b])

    @staticmethod
    def _wave_framing(framing):
        """None for framing=None and Framing() (the specialised entries), else the Framing (the _fr entries)."""
        from .audio import _general
        return _general(framing)

    def _mr_args(self):
        """rced_mr_args of an objective with mr_stft > 0 (the _mr entries, loss_parts of 4), else None."""
        o = self.objective
        return o.mr_args() if o is not None and o.mr_stft > 0.0 else None

    @staticmethod
    def _mr_framing(fr):
        """The framing the _mr entries rebuild at: they take one always, the default included."""
        from .audio import Framing
        return fr if fr is not None else Framing()

    def train_step(self, input_x, target_y, wave=None, framing=None):
        """trainer.py:181-192: returns (batch_loss, summary (None here), global_step).  With accumulate=k > 1 the batch is
        cut into k contiguous row ranges (accumulation_slices) and the step is train_step_sharded over them.
        With an objective that has a wave term, wave = (phase, clean_rows, lengths): the mixture's unit phase [N, T, 129] complex,
        the clean signals as device rows and the samples scored per utterance (audio.wave_loss_batch); accumulate=k cuts it by
        the same rows.  self.loss_parts then holds the step's unweighted (spectral, wave_sse, si_sdr) sums, and a fourth, mr_stft,
        with an objective whose mr_stft > 0.
        framing: the audio.Framing the wave terms are rebuilt at (the one `wave`'s phase was taken at); None is Framing()."""
        import torch
        fr = self._wave_framing(framing)
        x, y = self._on_device(input_x, target_y)
        if self.accumulate > 1:
            return self.train_step_sharded([(x[a:b], y[a:b], self._wave_rows(wave, a, b))
                                            for a, b in accumulation_slices(x.shape[0], self.accumulate)], framing=fr)
        loss = ctypes.c_double()
        st = torch.cuda.current_stream(x.device).cuda_stream
        if self._plain and wave is None:
            _lib.check(_lib.load().rced_train_step(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]),
                                                   ctypes.c_float(self.lr), ctypes.byref(loss), st))
            return loss.value, None, self.global_step
        args, keep = self._wave_args(wave, x)
        mr = self._mr_args()
        parts = (ctypes.c_double * (4 if mr is not None else 3))()
        if mr is not None:
            at = self._mr_framing(fr)
            _lib.check(_lib.load().rced_train_step_wave_mr(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]),
                                                           ctypes.c_float(self.lr), ctypes.byref(args), at.window, at.stride, at.code,
                                                           ctypes.byref(mr), ctypes.byref(loss), parts, st))
        elif fr is not None:
            _lib.check(_lib.load().rced_train_step_wave_fr(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]),
                                                           ctypes.c_float(self.lr), ctypes.byref(args), fr.window, fr.stride, fr.code,
                                                           ctypes.byref(loss), parts, st))
        else:
            _lib.check(_lib.load().rced_train_step_wave(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]),
                                                        ctypes.c_float(self.lr), ctypes.byref(args), ctypes.byref(loss), parts, st))
        self.loss_parts = tuple(parts)
        del keep
        return loss.value, None, self.global_step

    # -- the step in shards ----------------------------------------------------------
    def exchange_tensors(self):
        """(g, s): the trainer's exchange tensors on its device -- float32 gradient in blob order, float64 (sum z, sum z^2)
        per BatchNorm channel and the pixel count per layer.  Adding two trainers' tensors elementwise is the sum of their
        shards.  Their sizes depend on the net alone; they are made on first use."""
        import torch
        if self._exch is None:
            nf, nd = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(_lib.load().rced_train_exchange_size(self._h, ctypes.byref(nf), ctypes.byref(nd)))
            dev = "cuda:%d" % self.device
            self._exch = (torch.zeros(nf.value, dtype=torch.float32, device=dev), torch.zeros(nd.value, dtype=torch.float64, device=dev))
        return self._exch

    def grad_step(self, input_x, target_y, accumulate=False, wave=None, framing=None):
        """One shard: forward (BatchNorm with THIS shard's statistics), loss = sum((y - pred)^2) / batch_size, backward.
        The gradient and the statistics sums overwrite the exchange tensors, or (accumulate) are added to them; variables,
        Adam slots, moving statistics and global_step stay as they are.  Returns the shard's loss.  wave: as in train_step;
        self.loss_parts then holds this shard's sums (every term is a sum over utterances, divided by batch_size: shards add up).
        framing: as in train_step."""
        import torch
        fr = self._wave_framing(framing)
        x, y = self._on_device(input_x, target_y)
        g, s = self.exchange_tensors()
        loss = ctypes.c_double()
        st = torch.cuda.current_stream(x.device).cuda_stream
        if self._plain and wave is None:
            _lib.check(_lib.load().rced_train_grad(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]), g.data_ptr(),
                                                   s.data_ptr(), 1 if accumulate else 0, ctypes.byref(loss), st))
            return loss.value
        args, keep = self._wave_args(wave, x)
        mr = self._mr_args()
        parts = (ctypes.c_double * (4 if mr is not None else 3))()
        if mr is not None:
            at = self._mr_framing(fr)
            _lib.check(_lib.load().rced_train_grad_wave_mr(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]), g.data_ptr(),
                                                           s.data_ptr(), 1 if accumulate else 0, ctypes.byref(args), at.window, at.stride,
                                                           at.code, ctypes.byref(mr), ctypes.byref(loss), parts, st))
        elif fr is not None:
            _lib.check(_lib.load().rced_train_grad_wave_fr(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]), g.data_ptr(),
                                                           s.data_ptr(), 1 if accumulate else 0, ctypes.byref(args), fr.window, fr.stride,
                                                           fr.code, ctypes.byref(loss), parts, st))
        else:
            _lib.check(_lib.load().rced_train_grad_wave(self._h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]), g.data_ptr(),
                                                        s.data_ptr(), 1 if accumulate else 0, ctypes.byref(args), ctypes.byref(loss), parts, st))
        self.loss_parts = tuple(parts)
        del keep
        return loss.value

    def apply_step(self):
        """The optimizer step from the exchange tensors: moving statistics from the summed statistics (they follow the union
        of the shards), Adam once with self.lr.  Returns the global step.  gradients() then returns the summed gradient."""
        import torch
        g, s = self.exchange_tensors()
        st = torch.cuda.current_stream(g.device).cuda_stream
        _lib.check(_lib.load().rced_train_apply(self._h, g.data_ptr(), s.data_ptr(), ctypes.c_float(self.lr), st))
        return self.global_step

    def train_step_sharded(self, shards, sync_bn=False, framing=None):
        """One optimizer step over a list of (x, y) shards, each [N_s, T_s, 129, 1] (shapes may differ): the gradient is the
        fp32 sum of the shards' gradients in list order, the reported loss the sum of their losses, BatchNorm per shard.
        One shard is train_step, bit for bit.  Returns (loss, None, global_step).  Nothing is applied if a shard fails.
        framing: the audio.Framing of every shard's wave terms, as in train_step.

        sync_bn=True: BatchNorm over the UNION of the shards (the synchronised step) -- the step is then the
        unsharded train_step over all the shards' rows up to the rounding of a few fp64 additions, and it is what
        dist.DataParallelTrainer(sync_bn=True) computes with the shards on ranks, bit for bit.  The shards' passes run in
        lockstep, one trainer per shard (this one and cached replicas that are handed this one's variables before the step),
        and stop together at every BatchNorm layer, forward and backward, to add up their sums in list order.  EVERY SHARD'S
        ACTIVATIONS ARE LIVE AT ONCE: this form saves no memory over the whole batch in one piece; it states on one device
        what a world of ranks computes.  Not with accumulate=k > 1 (ValueError): accumulation runs its shards one after the
        other, and whole-batch statistics would need every layer's forward of every shard again."""
        if sync_bn and self.accumulate > 1:
            raise ValueError("sync_bn=True cannot be combined with accumulate=%d: accumulation runs its shards one after the other, "
                             "synchronised BatchNorm needs them all at every layer" % self.accumulate)
        if sync_bn and self.has_wave_term:
            raise ValueError("sync_bn=True cannot be combined with an objective that has a wave term (%r): the synchronised pass has no "
                             "wave form" % (self.objective,))
        fr = self._wave_framing(framing)
        waves = [sh[2] if len(sh) > 2 else None for sh in shards]     # a shard: (x, y) or (x, y, wave)
        shards = [self._on_device(sh[0], sh[1]) for sh in shards]
        if not shards:
            raise ValueError("train_step_sharded needs at least one shard")
        if sync_bn:
            return self._train_step_sharded_sync(shards)
        loss, parts = 0.0, None
        for i, ((x, y), w) in enumerate(zip(shards, waves)):
            loss += self.grad_step(x, y, accumulate=i > 0, wave=w, framing=fr)
            if self.loss_parts is not None and not (self._plain and w is None):
                parts = self.loss_parts if parts is None else tuple(p + q for p, q in zip(parts, self.loss_parts))
        if parts is not None:
            self.loss_parts = parts
        return loss, None, self.apply_step()

    # -- the synchronised step ----------------------------------------------------------
    def sync_points(self):
        """(exchange points of one synchronised pass, doubles in the buffer that grad_step_sync yields)."""
        n, nd = ctypes.c_int(), ctypes.c_size_t()
        _lib.check(_lib.load().rced_train_sync_points(self._h, ctypes.byref(n), ctypes.byref(nd)))
        return n.value, nd.value

    def grad_step_sync(self, input_x, target_y, pixels_total):
        """grad_step with BatchNorm over more than this shard, as a generator.  At every exchange point (sync_points()[0] of
        them: each BatchNorm layer once forward, once backward) it yields ONE float64 device tensor, always the same, that
        holds this shard's raw sums of the layer; the caller overwrites it in place with the ordered sum over all shards, on
        the current stream, and resumes.  pixels_total: the pixels of all shards, sum N_s * T_s * 129.  The generator's
        return value (StopIteration.value) is the shard's loss; the exchange tensors then hold the shard's gradient and
        statistics sums as after grad_step.  Closing the generator early aborts the pass; until it has ended one way or
        the other, every other call on this trainer raises.  With the yielded tensor left as it is and pixels_total this
        shard's own count, the pass is grad_step bit for bit."""
        import torch
        x, y = self._on_device(input_x, target_y)
        g, s = self.exchange_tensors()
        if self._sync_xs is None:
            self._sync_xs = torch.zeros(self.sync_points()[1], dtype=torch.float64, device="cuda:%d" % self.device)
        xs, lib, h = self._sync_xs, _lib.load(), self._h
        st = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(lib.rced_train_sync_begin(h, x.data_ptr(), y.data_ptr(), int(x.shape[0]), int(x.shape[1]),
                                             ctypes.c_double(float(pixels_total)), xs.data_ptr(), st))
        ended = False
        try:
            more = ctypes.c_int(1)
            while more.value:
                yield xs
                _lib.check(lib.rced_train_sync_next(h, ctypes.byref(more)))
            loss = ctypes.c_double()
            _lib.check(lib.rced_train_sync_end(h, g.data_ptr(), s.data_ptr(), ctypes.byref(loss), 0))
            ended = True
            return loss.value
        finally:
            if not ended:
                lib.rced_train_sync_abort(h)

    def sync_reduce(self, rows, xs, stride=None):
        """xs[i] = ((rows[0][i] + rows[1][i]) + ...): the ordered sum of an exchange point in one launch.  rows: float64
        device tensor [shards, >= len(xs)], contiguous; a row's first len(xs) entries are added."""
        import torch
        st = torch.cuda.current_stream(xs.device).cuda_stream
        _lib.check(_lib.load().rced_train_sync_reduce(self._h, rows.data_ptr(), int(rows.shape[0]),
                                                      int(rows.stride(0) if stride is None else stride), xs.data_ptr(), st))

    def _train_step_sharded_sync(self, shards):
        import torch
        while len(self._replicas) < len(shards) - 1:      # made once, from this trainer's variables; refreshed below
            self._replicas.append(FullyCNNTrainer(self.net_work, batch_size=self.batch_size, weights=self.variables(),
                                                  device=self.device))
        trainers = [self] + self._replicas[:len(shards) - 1]
        st = torch.cuda.current_stream(shards[0][0].device).cuda_stream
        for r in trainers[1:]:
            _lib.check(_lib.load().rced_train_copy_variables(r._h, self._h, st))
        pixels_total = float(sum(int(x.shape[0]) * int(x.shape[1]) * spec.FEATURE_DIM for x, _ in shards))
        passes = [tr.grad_step_sync(x, y, pixels_total) for tr, (x, y) in zip(trainers, shards)]
        losses = [None] * len(shards)
        try:
            bufs = [next(p) for p in passes]
            rows = torch.empty((len(shards), bufs[0].numel()), dtype=torch.float64, device=bufs[0].device)
            while bufs:
                for i, b in enumerate(bufs):
                    rows[i].copy_(b)
                for tr, b in zip(trainers, bufs):
                    tr.sync_reduce(rows, b)
                bufs = []
                for i, p in enumerate(passes):
                    try:
                        bufs.append(next(p))
                    except StopIteration as e:
                        losses[i] = e.value
                if bufs and len(bufs) != len(passes):
                    raise RuntimeError("the shards' passes did not stop at the same exchange points")
        finally:
            for p in passes:
                p.close()
        g, s = self.exchange_tensors()
        loss = 0.0
        for tr, l in zip(trainers, losses):              # the ordered sum, as dist.DataParallelTrainer forms it
            if tr is not self:
                gr, sr = tr.exchange_tensors()
                g.add_(gr)
                s.add_(sr)
            loss += l
        return loss, None, self.apply_step()

    def valid_step(self, input_x):
        """trainer.py:245-250: `sess.run(self.pred)` on the training graph.  That graph was built with
        is_training=True (trainer.py:165-172), so BatchNorm uses the statistics of the batch it is given; fetching
        only `pred` runs no UPDATE_OPS and no optimizer step, so nothing changes.  ndarray in -> ndarray out, cuda
        tensor in -> cuda tensor out.  (The inference graph of tester.py / infer.py, which normalises with the moving
        statistics, is `build_model(net_work, False, weights=trainer.variables())`.)"""
        return self.model(input_x)

    def valid(self, valid_loader, epoch, logger=None, nfft=512, stoi=False, extra=(), rebuild="reference", verbose=True):
        """trainer.py:252-338 over anything that yields the reference's 4-tuple (batch_mix, batch_clean, mix_sig,
        clean_sig): engine.evaluate_pcm with valid_step as the forward (BatchNorm with each batch's own statistics),
        every utterance's SDR into self.sdr_score; prints -- and logs, given a logger -- the reference's line with its
        SDR field and returns the average.  With stoi=True every utterance's STOI goes into self.stoi_score as well and
        the line gains the reference's st_score field, in the reference's order.  extra: names from
        evaluation.EXTRA_METRICS + evaluation.SPECTRAL_METRICS + evaluation.PROJECTION_METRICS + evaluation.SEPM_METRICS; every utterance's score goes into self.extra_scores[name], and one further line with their
        averages is printed and logged after the reference's.  rebuild: "reference" or "ola" (engine.evaluate_pcm).
        The framing is valid_loader.dataset.framing where there is one, else the default.
        verbose=False computes and returns the same without printing (the ranks of dist.DataParallelTrainer other than 0).
        PESQ and the wav files are not built."""
        from .engine import check_rebuild, evaluate_pcm, extra_line, feed_meters, loader_framing
        extra = check_extra(extra)
        check_rebuild(rebuild)
        framing = loader_framing(valid_loader)
        for _batch_mix, _batch_clean, mix_sig, clean_sig in valid_loader:
            scores = evaluate_pcm(self.valid_step, mix_sig, clean_sig, nfft, self.device, stoi=stoi, extra=extra, rebuild=rebuild,
                                  framing=framing)
            feed_meters(self, scores, stoi, extra)
        if stoi:
            line = "Epoch: {}, Average st_score: {:.4f}; Average sd_score: {:.4f}.\n".format(epoch, self.stoi_score.avg,
                                                                                             self.sdr_score.avg)
        else:
            line = "Epoch: {}, Average sd_score: {:.4f}.\n".format(epoch, self.sdr_score.avg)
        if verbose:
            print(line)
        if logger is not None:
            logger.info(line)
        if extra:
            more = "Epoch: {}, ".format(epoch) + extra_line(extra, self.extra_scores)
            if verbose:
                print(more)
            if logger is not None:
                logger.info(more)
        return self.sdr_score.avg

    def fit_step(self, input_x, target_y, wave=None, framing=None):
        """One iteration of the loop body of trainer.py:212-215: step, then set lr for the next step.  wave, framing: as in train_step."""
        if framing is not None:
            out = self.train_step(input_x, target_y, wave=wave, framing=framing)
        else:
            out = self.train_step(input_x, target_y, wave=wave) if wave is not None else self.train_step(input_x, target_y)
        self.lr = self.noam_scheme(out[2], self.warmup_steps)
        return out

    def train(self, train_loader, valid_loader, epochs, logger=None, checkpoints_path=None, net_arch="FullyCNN",
              num_iter_print=100):
        """trainer.py:194-243: per epoch shuffle, one fit_step per batch of train_loader (anything that yields the reference's
        4-tuple and has shuffle(), batch_size and len(): loader.DataLoader), the reference's progress line every
        num_iter_print batches, a checkpoint (save_checkpoint) under the reference's name when checkpoints_path is given,
        valid(valid_loader, epoch, logger) after every fifth epoch.  A trainer made by from_checkpoint starts at the epoch
        after the one its checkpoint's name carries.  Returns the last global step.  TF summaries are not built."""
        return run_epochs(self, self.fit_step, train_loader, valid_loader, epochs, logger, checkpoints_path, net_arch,
                          num_iter_print, True)

    @property
    def global_step(self):
        return int(_lib.load().rced_train_global_step(self._h))

    def grid_stats(self):
        """(largest grid, largest tiles per workgroup) over the tile-walking launchers of the last pass on the handle
        (rced_train_grid_stats): what RCED_TRAIN_MAX_GRID made of it.  (0, 0) before the first pass and under RCED_TRAIN_MFMA=0."""
        grid, walk = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().rced_train_grid_stats(self._h, ctypes.byref(grid), ctypes.byref(walk)))
        return grid.value, walk.value

    def _blob(self, fn):
        buf = np.empty(self._blob_n, np.float32)
        _lib.check(fn(self._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), buf.size))
        out, o = {}, 0
        for name, shape in spec.variable_shapes(self.variant):
            n = int(np.prod(shape))
            out[name] = buf[o:o + n].reshape(shape).copy()
            o += n
        return out

    def variables(self):
        """Current TF variables (incl. moving statistics), keyed by name -- what Saver.save would write."""
        return self._blob(_lib.load().rced_train_get_variables)

    def gradients(self):
        return self._blob(_lib.load().rced_train_get_gradients)

    # -- optimizer state / checkpoints (trainer.py:50-65, 232-239) ------------------------------------
    def optimizer_state(self):
        """(adam_m, adam_v, global_step): dicts keyed by TRAINABLE variable name (TF slots `<var>/Adam`, `<var>/Adam_1`)."""
        n = self._blob_n
        mb, vb = np.empty(n, np.float32), np.empty(n, np.float32)
        step = ctypes.c_longlong()
        fp = ctypes.POINTER(ctypes.c_float)
        _lib.check(_lib.load().rced_train_get_state(self._h, mb.ctypes.data_as(fp), vb.ctypes.data_as(fp), n, ctypes.byref(step)))
        m, v, o = {}, {}, 0
        for name, shape in spec.variable_shapes(self.variant):
            k = int(np.prod(shape))
            if "moving_" not in name:
                m[name], v[name] = mb[o:o + k].reshape(shape).copy(), vb[o:o + k].reshape(shape).copy()
            o += k
        return m, v, int(step.value)

    def load_optimizer_state(self, adam_m, adam_v, global_step):
        """Resume: set the Adam moments (dicts as returned by optimizer_state; missing names start at zero, as a
        variable without slots would in TF) and the step counter; the next learning rate follows the Noam schedule."""
        n = self._blob_n
        mb, vb, o = np.zeros(n, np.float32), np.zeros(n, np.float32), 0
        for name, shape in spec.variable_shapes(self.variant):
            k = int(np.prod(shape))
            for blob, src in ((mb, adam_m), (vb, adam_v)):
                if src is not None and name in src:
                    a = np.asarray(src[name], np.float32)
                    if a.shape != tuple(shape):
                        raise ValueError("optimizer slot of %r has shape %s, expected %s" % (name, a.shape, tuple(shape)))
                    blob[o:o + k] = a.reshape(-1)
            o += k
        fp = ctypes.POINTER(ctypes.c_float)
        _lib.check(_lib.load().rced_train_set_state(self._h, mb.ctypes.data_as(fp), vb.ctypes.data_as(fp), n, int(global_step)))
        if global_step > 0:
            self.lr = self.noam_scheme(int(global_step), self.warmup_steps)     # what the loop would have set (trainer.py:215)

    def save_checkpoint(self, prefix, with_optimizer=True):
        """Write a TF V2 checkpoint holding what `tf.train.Saver(tf.global_variables())` stores for the reference's
        training graph (trainer.py:50-51): the model variables, `global_step`, and -- with_optimizer -- the Adam
        slots `<var>/Adam`, `<var>/Adam_1` and the `beta1_power` / `beta2_power` accumulators (beta^(t+1) after t
        steps, as tf.train.AdamOptimizer keeps them).  The reference's test / infer / freeze graphs restore the model
        variables from it (tester.py:36-39); `FullyCNNTrainer.from_checkpoint` resumes from it.  Also written: the
        `checkpoint` state file `tf.train.latest_checkpoint` needs.  NOT written: `<prefix>.meta` (a serialized
        MetaGraphDef of the TF graph, which only TensorFlow can produce) -- the reference's own `continue_train`
        restores only when `continue_from + '.meta'` exists (trainer.py:59-65), so resuming THERE additionally needs
        a .meta from any checkpoint of the same graph (or `touch`, since only its existence is tested)."""
        from . import tf_checkpoint
        tensors = dict(self.variables())
        m, v, step = self.optimizer_state()
        tensors["global_step"] = np.asarray(step, np.int64)
        if with_optimizer:
            for name in m:
                tensors[name + "/Adam"] = m[name]
                tensors[name + "/Adam_1"] = v[name]
            tensors["beta1_power"] = np.asarray(0.9 ** (step + 1), np.float32)
            tensors["beta2_power"] = np.asarray(0.999 ** (step + 1), np.float32)
        tf_checkpoint.write_checkpoint(prefix, tensors)
        tf_checkpoint.write_checkpoint_state(prefix)
        return prefix

    @classmethod
    def from_checkpoint(cls, path, net_work="FullyCNNV3", **kw):
        """trainer.py:52-65 `continue_train`: variables, Adam slots (if the checkpoint has them) and global_step."""
        from . import tf_checkpoint
        variant = spec.variant_of(net_work)
        weights, adam_m, adam_v, step = tf_checkpoint.load_training_state(path, variant)
        tr = cls(net_work, weights=weights, **kw)
        tr.load_optimizer_state(adam_m, adam_v, step)
        tr.continue_from = path
        return tr

    def restore(self, weights, keep_optimizer=True):
        """Saver.restore of model variables into a running trainer (trainer.py:59-65).  keep_optimizer: the Adam slots and
        global_step survive (a TF restore of a checkpoint that holds only model variables leaves them as they are);
        False resets them, which is what `trainer.model.restore(weights)` alone does."""
        state = self.optimizer_state() if keep_optimizer else None
        self.model.restore(weights)
        if state is not None:
            self.load_optimizer_state(*state)
        return self

    def close(self):
        replicas, self._replicas = getattr(self, "_replicas", []), []
        for r in replicas:
            r.close()
        if self.model is not None:
            self.model.close()     # the model owns the handle

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
