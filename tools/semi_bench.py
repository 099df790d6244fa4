#!/usr/bin/env python3
"""Time the class-marginal KL of semi-supervised training (csrc/semisup.hip through ops.class_marginal_kl) on one MI355X, at the
batch of the flagship workload (N = 512, K = 64) with C = 10 and C = 100 classes and every second row unlabelled:

  (a) forward + backward of the fused op (one launch forward; two backward: the row pass and the class pass) against the SAME
      objective written as a torch fp32 expression under autograd on the device (the (N, C, K) tensor exists there), from the same
      mu, log_var, class means and upstream gradient - interleaved window by window, the largest difference of every gradient
      reported;
  (b) train_step() of configuration 2 (oracle.cases.full_config(2)) with SEMI_SUPERVISED off - the step of the parent commit: the
      switch left off changes nothing - and on with every second label hidden, on two models in the same state and on the same
      batch, alternating window by window.

    python tools/semi_bench.py [--calls 30] [--reps 50] [--warmup 5] [--out profiles/semi_bench.json]

What is timed is a CALL, host side included: HIP events around a window of `reps` back-to-back calls (20 training steps) on the
launch stream, ended by the event's synchronise, divided by the number of calls; medians and min-max over `calls` windows after
the warm-up, the two sides alternating window by window.  No kernel trace is taken here.  Needs the GPU (there is no other path).
Prints one JSON line."""
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


def torch_kl(mu, lv, y, means, T, kl_in):
    """The merged KL rows as a torch expression (scalar prior variance, uniform class weights: the flagship's kinds)."""
    K, C = mu.shape[1], means.shape[0]
    t2 = (T * T).view(1, C, 1)
    dist = (t2 * (mu.unsqueeze(1) - means.unsqueeze(0)) ** 2).sum(-1)               # (N, C, K) -> (N, C)
    var = (lv.exp().unsqueeze(1) * t2).sum(-1) - lv.sum(-1, keepdim=True) - K * (T * T).log().view(1, C) - K
    U = -torch.logsumexp(-0.5 * (dist + var) - math.log(C), 1)
    return torch.where(y < 0, U, kl_in)


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
    assert torch.cuda.is_available(), 'semi_bench needs the MI355X'
    dev = 'cuda:0'
    N, K = 512, 64
    out = {'metric': 'semi_call_ms', 'device': torch.cuda.get_device_name(0), 'windows': a.calls, 'calls_per_window': a.reps,
           'warmup_windows': a.warmup, 'N': N, 'K': K, 'unlabelled': 'every second row',
           'timing': 'call time: HIP events around a window of back-to-back calls on the launch stream, per call, host side '
                     'included; the two sides alternate window by window; medians, min-max over the windows; no kernel trace',
           'fused_vs_torch': []}
    g = torch.Generator().manual_seed(0)
    for C in (10, 100):
        mu, lv0 = torch.randn(N, K, generator=g), -2 + 2 * torch.rand(N, K, generator=g)
        y = torch.randint(0, C, (N,), generator=g)
        y[::2] = -1
        y = y.to(dev)
        gb = (torch.rand(N, generator=g) / N).to(dev)
        kl_in, zd_in, vkl_in = (torch.rand(N, generator=g).to(dev) for _ in range(3))
        leaves = [t.to(dev).requires_grad_(True) for t in (mu, lv0, torch.randn(C, K, generator=g))]
        T = (0.8 + 0.4 * torch.rand(C, generator=g)).to(dev)

        def fused():
            m, lv, means = leaves
            kl = ops.class_marginal_kl(m, lv, y, means, T, kl_in, zd_in, vkl_in)[0]
            return torch.autograd.grad(kl, leaves, gb)

        def by_torch():
            m, lv, means = leaves
            return torch.autograd.grad(torch_kl(m, lv, y, means, T, kl_in), leaves, gb)
        diff = [float((p - q).abs().max() / q.abs().max().clamp(min=1e-30)) for p, q in zip(fused(), by_torch())]
        ms = {'fused': [], 'torch': []}
        for i in range(a.warmup + a.calls):
            for name, fn in (('fused', fused), ('torch', by_torch)):
                t = event_ms(fn, a.reps)
                if i >= a.warmup:
                    ms[name].append(t)
        f, t = float(np.median(ms['fused'])), float(np.median(ms['torch']))
        out['fused_vs_torch'].append({'C': C, 'fused_fwd_bwd': stats(ms['fused']), 'torch_fwd_bwd': stats(ms['torch']),
                                      'torch_over_fused': t / f,
                                      'largest_relative_difference': dict(zip(('mu', 'lv', 'means'), diff))})

    # (b) the training step with the switch off (the parent's step) and on: two models in one state, one batch, alternating
    case = full_config(2, N)
    kw = case['net']
    x, yb, e = det_inputs(N, kw['input_shape'], kw['num_labels'], kw['latent_sampling'], kw['latent_dim'], seed=42)
    x, yb, e = x.to(dev), yb.to(dev), e.to(dev)
    yh = yb.clone()
    yh[::2] = -1
    nets = {}
    for name in ('elbo', 'semi'):
        net = Net(**kw)
        load_det_state(net, seed=0)
        net.to(dev).train()
        net.SEMI_SUPERVISED = name == 'semi'
        nets[name] = net
    ms = {k: [] for k in nets}
    for i in range(a.warmup + a.calls):
        for name, net in nets.items():
            labels = yh if name == 'semi' else yb
            t = event_ms(lambda: net.train_step(x, labels, epsilon=e), 20)
            if i >= a.warmup:
                ms[name].append(t)
    el, se = float(np.median(ms['elbo'])), float(np.median(ms['semi']))
    out['train_step'] = {'model': 'cvae conv32/deconv32 K=64 C=10 batch_norm (BASELINE config 2), eager train_step()', 'N': N,
                         'L': kw['latent_sampling'], 'elbo_switch_off': stats(ms['elbo']), 'semi_half_unlabelled': stats(ms['semi']),
                         'semi_over_elbo': se / el}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
