#!/usr/bin/env python3
"""Time the importance-weighted bound (csrc/iwae.hip through ops.iw_bound) on one MI355X, at the batch of the flagship workload
(oracle.cases.full_config(2): N = 512, K = 64, the training L of that configuration) and, beside it, at L = 8 and L = 64 draws:

  (a) forward + backward of the fused pair (one forward launch; backward: the per-sample launch, the class fold, the sigma sum)
      against the SAME bound written as a torch expression under autograd on the device, from the same wmse_s, z, log_var, eps,
      class means and sigma, with the same upstream gradient - interleaved call by call, the largest difference of every
      gradient reported;
  (b) train_step() of that configuration under TRAIN_OBJECTIVE 'elbo' and 'iwae' on two models in the same state and on the same
      batch, alternating step by step.

    python tools/iwae_bench.py [--calls 30] [--reps 200] [--warmup 5] [--out profiles/iwae_bench.json]

What is timed is a CALL, host side included: HIP events around a window of `reps` back-to-back calls (20 training steps) on the
launch stream, ended by the event's synchronise, divided by the number of calls; medians and min-max over `calls` windows after
the warm-up, the two sides alternating window by window.  At these sizes a call is a handful of launches of a few microseconds
each: the figure is the rate at which the host can issue them (launches and Python), not the kernels' arithmetic - it says what a
training step pays for the tail, which is what the two sides are compared on.  No kernel trace is taken here.  Needs the GPU
(there is no other path).  Prints one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

LOG2PI = math.log(2 * math.pi)


def event_ms(fn, reps=1):
    """Milliseconds per call over a window of `reps` back-to-back calls."""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_max_ms': [float(np.min(ms)), float(np.max(ms))]}


def torch_bound(wmse_s, z, lv, eps, y, means, T, log_sigma, D, beta):
    """The bound as a torch expression (scalar prior variance, one learned log sigma: the flagship's kinds)."""
    t = T[y].unsqueeze(-1)
    dist = (t * (z[1:] - means[y])).pow(2).sum(-1)
    slog = z.shape[-1] * T[y].log()
    q = (eps.pow(2) + lv).sum(-1)
    lw = -0.5 * D * (wmse_s + 2 * log_sigma + LOG2PI) + beta * (0.5 * (q - dist) + slog)
    return torch.logsumexp(lw, 0) - math.log(lw.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=200, help='calls per timed window')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import det_inputs, load_det_state
    assert torch.cuda.is_available(), 'iwae_bench needs the MI355X'
    dev = 'cuda:0'
    case = full_config(2, 512)
    kw = case['net']
    N, K, C, D = case['N'], kw['latent_dim'], kw['num_labels'], int(np.prod(kw['input_shape']))
    L_train = kw['latent_sampling']
    out = {'metric': 'iwae_call_ms', 'windows': a.calls, 'calls_per_window': a.reps, 'warmup_windows': a.warmup, 'N': N, 'K': K,
           'C': C, 'D': D,
           'timing': 'host-bound call time: HIP events around a window of back-to-back calls on the launch stream, per call; the '
                     'two sides alternate window by window; medians, min-max over the windows; launches and Python included, no '
                     'kernel trace', 'fused_vs_torch': []}
    g = torch.Generator().manual_seed(0)
    for L in sorted({L_train, 8, 64}):
        mu, lv0, eps = torch.randn(N, K, generator=g), -2 + 3 * torch.rand(N, K, generator=g), torch.randn(L, N, K, generator=g)
        z0 = torch.cat([mu.unsqueeze(0), mu + (0.5 * lv0).exp() * eps])
        y = torch.randint(0, C, (N,), generator=g).to(dev)
        eps = eps.to(dev)
        gb = (torch.rand(N, generator=g) / N).to(dev)
        leaves = [t.to(dev).requires_grad_(True) for t in (0.5 + torch.rand(L, N, generator=g), z0, lv0, torch.randn(C, K, generator=g),
                                                           torch.tensor([math.log(0.7)]))]
        T = (0.8 + 0.4 * torch.rand(C, generator=g)).to(dev)

        def fused():
            wm, z, lv, means, sg = leaves
            bound, _ = ops.iw_bound(wm, z, lv, eps, y, means, T, sg, ops.SIGMA_LOG, D)
            return torch.autograd.grad(bound, leaves, gb)

        def by_torch():
            wm, z, lv, means, sg = leaves
            return torch.autograd.grad(torch_bound(wm, z, lv, eps, y, means, T, sg, D, 1.), leaves, gb)
        diff = [float((p - q).abs().max() / q.abs().max().clamp(min=1e-30)) for p, q in zip(fused(), by_torch())]
        ms = {'fused': [], 'torch': []}
        for i in range(a.warmup + a.calls):
            for name, fn in (('fused', fused), ('torch', by_torch)):
                t = event_ms(fn, a.reps)
                if i >= a.warmup:
                    ms[name].append(t)
        f, t = float(np.median(ms['fused'])), float(np.median(ms['torch']))
        out['fused_vs_torch'].append({'L': L, 'fused_fwd_bwd': stats(ms['fused']), 'torch_fwd_bwd': stats(ms['torch']),
                                      'torch_over_fused': t / f,
                                      'largest_relative_difference': dict(zip(('wmse_s', 'z', 'lv', 'means', 'sigma'), diff))})

    # (b) the training step under both objectives: two models in one state, one batch, alternating
    x, yb, e = det_inputs(N, kw['input_shape'], C, L_train, K, seed=42)
    x, yb, e = x.to(dev), yb.to(dev), e.to(dev)
    nets = {}
    for objective in ('elbo', 'iwae'):
        net = Net(**kw)
        load_det_state(net, seed=0)
        net.to(dev).train()
        net.TRAIN_OBJECTIVE = objective
        nets[objective] = net
    ms = {k: [] for k in nets}
    for i in range(a.warmup + a.calls):
        for name, net in nets.items():
            t = event_ms(lambda: net.train_step(x, yb, epsilon=e), 20)
            if i >= a.warmup:
                ms[name].append(t)
    el, iw = float(np.median(ms['elbo'])), float(np.median(ms['iwae']))
    out['train_step'] = {'model': 'cvae conv32/deconv32 K=64 C=10 batch_norm (BASELINE config 2), eager train_step()', 'N': N,
                         'L': L_train, 'elbo': stats(ms['elbo']), 'iwae': stats(ms['iwae']), 'iwae_over_elbo': iw / el}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
