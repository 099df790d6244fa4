#!/usr/bin/env python3
"""Time the two things jvae_compat/wim.py adds, each against what it replaces, on config 2 at N = 512 with the L = 128 latent
draws of `bench.py --workload eval`:

  both_priors   one `evaluate_on_both_priors()` evaluation with the shared pass (WIM_SHARED_PASS = True) against two full
                evaluate(x) calls with the prior swapped in between (WIM_SHARED_PASS = False: what the reference does, and what
                a base model can be driven to do by hand);
  score_rows    the 12 OOD rows {kl, zdist, iws, elbo} x {~, @, ~@} of one batch from ONE `ops.wim_scores` launch against the
                torch expressions of ft/wim.py:145-192 (`Row.torch_row` of module/score_rows.py), on the losses of that evaluation.

    python tools/wim_bench.py [--calls 20] [--warmup 5] [--n 512] [--L 128] [--out profiles/wim_bench.json]

HIP events around each call on the current stream, after a warm-up, every call with its own epsilon draw; the median of the calls
is reported, minimum and maximum beside it.  Prints one JSON line."""
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


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--L', type=int, default=128)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from jvae_compat.wim import WIMJob
    from module import score_rows
    from oracle.cases import WIM_CASES, full_config
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    kw = dict(full_config(2, a.n)['net'], test_latent_sampling=a.L)
    job = WIMJob(**kw, alternate_prior=dict(WIM_CASES['w2_n8']['alternate_prior'], num_priors=1, dim=kw['latent_dim']))
    load_det_state(job, seed=0)
    job.to(dev)
    job.eval()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((a.n, *kw['input_shape']), device=dev, generator=g)
    y_est = torch.randint(0, kw['num_labels'], (a.n,), device=dev, generator=g)
    kept = {}

    def both(shared):
        def call():
            job.WIM_SHARED_PASS = shared
            with torch.no_grad(), job.evaluate_on_both_priors():
                kept['out'] = job.evaluate((x, y_est))
        return call
    out = {'metric': 'wim_bench', 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'hip': torch.version.hip,
           'config': f'config 2 (conv32 / deconv32, K = 64, C = 10), N = {a.n}, L = {a.L}, eval mode, fp32',
           'calls': a.calls, 'warmup': a.warmup, 'timing': 'HIP events around each call, median of the calls'}
    one, two = timed(both(True), a.calls, a.warmup), timed(both(False), a.calls, a.warmup)
    out['both_priors'] = {'shared_pass': one, 'two_passes': two, 'two_over_shared': two['ms_median'] / one['ms_median']}
    losses = kept['out'][2]
    methods = [k + s for k in ('kl', 'zdist', 'iws', 'elbo') for s in ('~', '@', '~@')]
    records = [score_rows.parse(m, score_rows.traits_of(job)) for m in methods]
    buf = torch.empty((len(methods), a.n), dtype=torch.float32, device=dev)
    fused = timed(lambda: job.batch_dist_measures(None, losses, methods, out=buf), a.calls, a.warmup)
    by_torch = timed(lambda: [r.torch_row(losses) for r in records], a.calls, a.warmup)
    ref = [r.torch_row(losses) for r in records]
    worst = max(float((row - want).abs().max() / want.abs().max().clamp_min(1e-30)) for row, want in zip(buf, ref))
    out['score_rows'] = {'rows': len(methods), 'wim_scores_one_launch': fused, 'torch_expressions': by_torch,
                         'torch_over_fused': by_torch['ms_median'] / fused['ms_median'], 'max_relative_difference': worst}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
