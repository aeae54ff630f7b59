"""Float64 restatement of the SYNCHRONISED sharded training step on top of oracle.train_ref.TrainRef --
test infrastructure, not product code.

Shards s = 0 .. S-1 of (x_s, y_s), [N_s, T_s, 129, 1] each (the shapes may differ), through ONE graph:
  1. per layer: every shard is convolved on its own; a BatchNorm layer forms mean and BIASED variance of the pre-activations
     over the pixels of ALL shards (P = sum N_s T_s 129) and normalises every shard with them; skips and ReLU per shard;
  2. loss = sum_s sum((y_s - pred_s)^2) / batch_size; autograd does the backward, through the shared statistics;
  3. moving_mean = 0.99 moving_mean + 0.01 mean, moving_variance = 0.99 moving_variance + 0.01 var P / (P - 1), once, and
     Adam once in TF's form, as tests/train_shard_np.py applies them; global_step += 1.
With the shards the row ranges of one batch this is TrainRef.train_step over the whole batch, up to float64 rounding.
"""

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import layers as L
from oracle.train_ref import ADAM_EPS, BETA1, BETA2


def forward_sync(ref, xs, pre=None):
    """The train-mode forward of the TrainRef `ref` over a list of inputs with shared BatchNorm statistics.  Returns
    (list of predictions [N_s, T_s, 129, 1], list of (scope, mean, biased variance, pixels of all shards)).  pre: a list
    that receives the smallest |value entering a ReLU| of every layer and shard."""
    tens = [[torch.as_tensor(x).to(ref.dtype).permute(0, 3, 1, 2)] for x in xs]
    stats = []
    for l in ref.layers:
        k = ref.vars[l.scope + "/kernel"].permute(3, 2, 0, 1).contiguous()   # HWIO -> OIHW
        pt, pb = (l.kh - 1) // 2, (l.kh - 1) - (l.kh - 1) // 2
        pl, pr = (l.kw - 1) // 2, (l.kw - 1) - (l.kw - 1) // 2
        ys = [Fn.conv2d(Fn.pad(t[l.src], (pl, pr, pt, pb)), k, ref.vars[l.scope + "/bias"]) for t in tens]
        if l.use_norm:
            p = l.scope + "/batch_norm/"
            n = sum(y.numel() // y.shape[1] for y in ys)
            mean = (sum(y.sum(dim=(0, 2, 3)) for y in ys) / n).view(1, -1, 1, 1)
            var = (sum(((y - mean) ** 2).sum(dim=(0, 2, 3)) for y in ys) / n).view(1, -1, 1, 1)
            ys = [(y - mean) / torch.sqrt(var + L.BN_EPS) * ref.vars[p + "gamma"].view(1, -1, 1, 1) +
                  ref.vars[p + "beta"].view(1, -1, 1, 1) for y in ys]
            stats.append((l.scope, mean.detach().flatten(), var.detach().flatten(), n))
        for t, y in zip(tens, ys):
            if l.skip_pre >= 0:
                y = y + t[l.skip_pre]
            if l.use_act:
                if pre is not None:
                    pre.append(float(y.detach().abs().min()))
                y = torch.relu(y)
            if l.skip_post >= 0:
                y = y + t[l.skip_post]
            t.append(y)
    return [t[-1].permute(0, 2, 3, 1) for t in tens], stats


def min_abs_preactivation(ref, xs):
    """TrainRef.min_abs_preactivation for the synchronised forward: the smallest |value entering a ReLU| over the net and
    the shards.  A ReLU whose input is within fp32 rounding of zero may take the other branch on the device, which changes
    gradients by whole terms; tests screen their inputs with it."""
    pre = []
    with torch.no_grad():
        forward_sync(ref, xs, pre)
    return min(pre)


def loss_and_grads(ref, shards):
    """(loss, gradients keyed by trainable variable name, statistics) of the synchronised step over `shards`."""
    for k in ref.m:
        ref.vars[k].grad = None
    preds, stats = forward_sync(ref, [x for x, _ in shards])
    loss = sum(((torch.as_tensor(y).to(ref.dtype) - p) ** 2).sum() for (_, y), p in zip(shards, preds)) / ref.batch_size
    loss.backward()
    return loss.item(), {k: ref.vars[k].grad.clone() for k in ref.m}, stats


def synced_step(ref, shards, lr):
    """One synchronised step on the TrainRef `ref` (variables, Adam slots and global_step are updated in place).
    Returns (loss, G, global_step)."""
    loss, G, stats = loss_and_grads(ref, shards)
    ref.global_step += 1
    t = ref.global_step
    lr_t = lr * np.sqrt(1 - BETA2 ** t) / (1 - BETA1 ** t)
    with torch.no_grad():
        for k, g in G.items():
            ref.m[k].mul_(BETA1).add_(g, alpha=1 - BETA1)
            ref.v[k].mul_(BETA2).addcmul_(g, g, value=1 - BETA2)
            ref.vars[k].sub_(lr_t * ref.m[k] / (ref.v[k].sqrt() + ADAM_EPS))
        for scope, mean, var, n in stats:
            p = float(n)
            unbiased = var * p / (p - 1.0) if p > 1.0 else var
            name = scope + "/batch_norm/"
            ref.vars[name + "moving_mean"].mul_(L.BN_MOMENTUM).add_(mean, alpha=1 - L.BN_MOMENTUM)
            ref.vars[name + "moving_variance"].mul_(L.BN_MOMENTUM).add_(unbiased, alpha=1 - L.BN_MOMENTUM)
    return loss, G, ref.global_step
