#!/usr/bin/env python3
"""Time the MMD objective (csrc/mmd.hip through ops.mmd_objective) on one MI355X, at the batch of the flagship workload
(oracle.cases.full_config(2): N = 512, K = 64, C = 10) with L = 1 and L = 8 draws:

  (a) forward + backward of the fused op (forward, three launches: prepare, pair sums, finish; backward, five: prepare, pair
      gradients, finish and the two class folds) against the SAME objective written as a torch fp32 expression under autograd on
      the device, from the same z, noise and class means, with the same upstream gradient - interleaved window by window, the
      largest difference of every gradient reported;
  (b) train_step() of that configuration under TRAIN_OBJECTIVE 'elbo' and 'mmd' on two models in the same state and on the same
      batch, alternating window by window.

    python tools/mmd_bench.py [--calls 30] [--reps 50] [--warmup 5] [--out profiles/mmd_bench.json]

What is timed is a CALL, host side included: HIP events around a window of `reps` back-to-back calls (20 training steps) on the
launch stream, ended by the event's synchronise, divided by the number of calls; medians and min-max over `calls` windows after
the warm-up, the two sides alternating window by window.  No kernel trace is taken here (run the tool under a kernel trace on its
own for the launches' names and times).  Needs the GPU (there is no other path).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

WAE_SCALES = (.1, .2, .5, 1., 2., 5., 10.)


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


def torch_rows(z, eps_p, y, means, T):
    """The rows as a torch expression (scalar prior variance, the inverse multiquadric kernel at the default scales, pairs inside
    a class: the flagship's kinds), squared distances in the direct form."""
    N, K = z.shape[1:]
    p = means[y] + eps_p / T[y].unsqueeze(-1)
    mask = (y.view(-1, 1) == y.view(1, -1)).to(z.dtype)
    off = mask * (1 - torch.eye(N, device=z.device, dtype=z.dtype))

    def gram(a, b):
        d2 = ((a.unsqueeze(2) - b.unsqueeze(1)) ** 2).sum(-1)                        # (L, N, N)
        return sum(2. * K * s / (2. * K * s + d2) for s in WAE_SCALES)
    zq = z[1:]
    return ((gram(zq, zq) * off).sum(2) / (N - 1) + (gram(p, p) * off).sum(2) / (N - 1) - 2. / N * (gram(zq, p) * mask).sum(2)).mean(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=50, help='calls per timed window')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import det_inputs, load_det_state
    assert torch.cuda.is_available(), 'mmd_bench needs the MI355X'
    dev = 'cuda:0'
    case = full_config(2, 512)
    kw = case['net']
    N, K, C = case['N'], kw['latent_dim'], kw['num_labels']
    L_train = kw['latent_sampling']
    out = {'metric': 'mmd_call_ms', 'windows': a.calls, 'calls_per_window': a.reps, 'warmup_windows': a.warmup, 'N': N, 'K': K, 'C': C,
           'kernel': ['imq', None], 'joint': True,
           'timing': 'call time: HIP events around a window of back-to-back calls on the launch stream, per call, host side '
                     'included; the two sides alternate window by window; medians, min-max over the windows; no kernel trace',
           'fused_vs_torch': []}
    g = torch.Generator().manual_seed(0)
    for L in (1, 8):
        means0 = torch.randn(C, K, generator=g)
        y = torch.randint(0, C, (N,), generator=g)
        mu = means0[y] + 0.5 * torch.randn(N, K, generator=g)
        z0 = torch.cat([mu.unsqueeze(0), mu + 0.8 * torch.randn(L, N, K, generator=g)])
        eps_p = torch.randn(L, N, K, generator=g).to(dev)
        y = y.to(dev)
        gb = (torch.rand(N, generator=g) / N).to(dev)
        leaves = [t.to(dev).requires_grad_(True) for t in (z0, means0)]
        T = (0.8 + 0.4 * torch.rand(C, generator=g)).to(dev)

        def fused():
            z, means = leaves
            return torch.autograd.grad(ops.mmd_objective(z, eps_p, y, means, T), leaves, gb)

        def by_torch():
            z, means = leaves
            return torch.autograd.grad(torch_rows(z, eps_p, y, means, T), leaves, gb)
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
                                      'largest_relative_difference': dict(zip(('z', 'means'), diff))})

    # (b) the training step under both objectives: two models in one state, one batch, alternating
    x, yb, e = det_inputs(N, kw['input_shape'], C, L_train, K, seed=42)
    x, yb, e = x.to(dev), yb.to(dev), e.to(dev)
    nets = {}
    for objective in ('elbo', 'mmd'):
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
    el, mm = float(np.median(ms['elbo'])), float(np.median(ms['mmd']))
    out['train_step'] = {'model': 'cvae conv32/deconv32 K=64 C=10 batch_norm (BASELINE config 2), eager train_step()', 'N': N,
                         'L': L_train, 'elbo': stats(ms['elbo']), 'mmd': stats(ms['mmd']), 'mmd_over_elbo': mm / el}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
