#!/usr/bin/env python3
"""Time WIMJob.finetune_step() in its two forms on config 2: the fused step (`WIM_FUSED_STEP = True`: one pass over the
concatenated batch, two-prior latent kernel) against the two-pass step (`False`: finetune_batch(), two evaluations), at
64 + 64 and 512 + 512 images (labelled + mixture).

  forward   finetune_step() alone: the pass(es) through the network and the loss;
  step      what the loop runs per batch: zero_grad, finetune_step(), backward, optimizer.step(), optimizer.clip().

    python tools/wim_finetune_bench.py [--calls 20] [--warmup 5] [--sizes 64 512] [--out profiles/wim_finetune_bench.json]

HIP events around each call on the current stream, after the warm-up calls; median, minimum and maximum of the calls.  Prints
one JSON line and writes it to --out."""
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
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 512])
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'wim_finetune_bench.json'))
    a = ap.parse_args()
    from jvae_compat.wim import WIMJob
    from oracle.cases import WIM_CASES, full_config
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    kw = full_config(2, max(a.sizes))['net']
    job = WIMJob(**kw, alternate_prior=dict(WIM_CASES['w2_n8']['alternate_prior'], num_priors=1, dim=kw['latent_dim']))
    load_det_state(job, seed=0)
    job.to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    out = {'metric': 'wim_finetune_bench', 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__,
           'hip': torch.version.hip, 'config': 'config 2 (conv32 / deconv32, K = 64, C = 10), L = 1, BatchNorm in eval mode, fp32',
           'calls': a.calls, 'warmup': a.warmup, 'timing': 'HIP events around each call, median / min / max of the calls',
           'sizes': {}}
    for n in a.sizes:
        x_in = torch.rand((n, *kw['input_shape']), device=dev, generator=g)
        y_in = torch.randint(0, kw['num_labels'], (n,), device=dev, generator=g)
        x_mix = torch.rand((n, *kw['input_shape']), device=dev, generator=g)
        routes = {}

        def forward():
            with torch.no_grad():
                job.finetune_step(0, 0, x_in, y_in, x_mix, alpha=0.1)
            routes[job.WIM_FUSED_STEP] = job.last_finetune_route

        def step():
            job.optimizer.zero_grad()
            L, _, _ = job.finetune_step(0, 0, x_in, y_in, x_mix, alpha=0.1)
            L.backward()
            job.optimizer.step()
            job.optimizer.clip(job.parameters())

        res = {}
        for name, fn in (('forward', forward), ('step', step)):
            for fused in (True, False):
                job.WIM_FUSED_STEP = fused
                res.setdefault(name, {})['fused' if fused else 'two_pass'] = timed(fn, a.calls, a.warmup)
            res[name]['two_pass_over_fused'] = res[name]['two_pass']['ms_median'] / res[name]['fused']['ms_median']
        assert routes == {True: 'fused', False: 'two_pass'}, routes
        out['sizes'][f'{n}+{n}'] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
