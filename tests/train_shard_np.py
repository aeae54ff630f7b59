"""Float64 restatement of the sharded training step on top of oracle.train_ref.TrainRef -- test
infrastructure, not product code.

Shards s = 0 .. S-1 of (x_s, y_s):
  1. per shard: TrainRef.loss_and_grads -- the forward with BatchNorm normalising by THAT shard's statistics,
     loss_s = sum((y_s - pred_s)^2) / batch_size, and g_s = d loss_s / d variables;
  2. G = ((g_0 + g_1) + g_2) + ..., in shard order;
  3. per BatchNorm channel S1 = sum z, S2 = sum z^2 and the pixel count P are added over the shards (S1, S2 from the
     shard's mean and biased variance of the pre-activations: S1 = P_s mean_s, S2 = P_s (var_s + mean_s^2)); then ONCE
     m = S1 / P, var = max(S2 / P - m^2, 0), moving_mean = 0.99 moving_mean + 0.01 m,
     moving_variance = 0.99 moving_variance + 0.01 var P / (P - 1)   (the union batch's statistics);
  4. Adam once, from G and lr, in TF's form; global_step += 1;
  5. the loss reported is sum_s loss_s.
"""

import numpy as np
import torch

from oracle import layers as L
from oracle.train_ref import ADAM_EPS, BETA1, BETA2


def sharded_step(ref, shards, lr):
    """One sharded step on the TrainRef `ref` (its variables, Adam slots and global_step are updated in place).
    Returns (loss, G, global_step): G a dict of float64 tensors keyed by trainable variable name."""
    loss, G, sums = 0.0, None, {}
    for x, y in shards:
        loss_s, g_s, stats = ref.loss_and_grads(x, y)
        loss += loss_s
        G = g_s if G is None else {k: G[k] + g_s[k] for k in G}
        for scope, mean, var, n in stats:
            s1, s2 = mean * n, (var + mean * mean) * n
            if scope in sums:
                a = sums[scope]
                sums[scope] = (a[0] + s1, a[1] + s2, a[2] + float(n))
            else:
                sums[scope] = (s1, s2, float(n))
    ref.global_step += 1
    t = ref.global_step
    lr_t = lr * np.sqrt(1 - BETA2 ** t) / (1 - BETA1 ** t)
    with torch.no_grad():
        for k, g in G.items():
            ref.m[k].mul_(BETA1).add_(g, alpha=1 - BETA1)
            ref.v[k].mul_(BETA2).addcmul_(g, g, value=1 - BETA2)
            ref.vars[k].sub_(lr_t * ref.m[k] / (ref.v[k].sqrt() + ADAM_EPS))
        for scope, (s1, s2, p) in sums.items():
            m = s1 / p
            var = torch.clamp(s2 / p - m * m, min=0.0)
            unbiased = var * p / (p - 1.0) if p > 1.0 else var
            name = scope + "/batch_norm/"
            ref.vars[name + "moving_mean"].mul_(L.BN_MOMENTUM).add_(m, alpha=1 - L.BN_MOMENTUM)
            ref.vars[name + "moving_variance"].mul_(L.BN_MOMENTUM).add_(unbiased, alpha=1 - L.BN_MOMENTUM)
    return loss, G, ref.global_step
