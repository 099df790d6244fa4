#!/usr/bin/env python3
"""Time the two things the latent-space inspection changes, on config 2 at N = 512, batches of a device-resident synthetic set:

  zsample   the statistics of `module.sample.zsample` per batch through `net.latent_posterior` + `ops.latent_moments` (what
            zsample() runs), against the same statistics through `net.evaluate(x, z_output=True)` + the torch sums - the only
            route to mu and log_var before latent_posterior existed, and what the reference's zsample does.
  moments   `ops.latent_moments(mu, log_var, group = y)` - one launch pair into device accumulators - against the 2 C boolean
            mask selections of torch per batch (per class: mu[y == c] and var[y == c], then their sums), each a host
            synchronisation.

    python tools/inspection_bench.py [--batches 4] [--calls 10] [--warmup 3] [--out profiles/inspection_bench.txt]

HIP events around each call (a call = all batches) on the current stream, after a warm-up; the median of the calls, minimum and
maximum beside it.  Prints one JSON line.  No ratio is promised: the figures are whatever was measured."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd'), os.path.join(REPO, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from aggregation_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('inspection_bench needs the GPU: nothing is measured without one')
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import load_det_state
    dev, N = 'cuda:0', 512
    kw = full_config(2, N)['net']
    torch.manual_seed(0)
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(dev).eval()
    C, K = kw['num_labels'], kw['latent_dim']
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.rand((N, *kw['input_shape']), device=dev, generator=g) for _ in range(a.batches)]
    ys = [torch.randint(0, C, (N,), device=dev, generator=g) for _ in range(a.batches)]
    groups = [y.to(torch.int32) for y in ys]

    def accumulators():
        return torch.zeros((C, 4, K), dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.int64, device=dev)

    def encode_only():
        sums, counts = accumulators()
        for x, grp in zip(xs, groups):
            mu, lv = net.latent_posterior(x)
            ops.latent_moments(mu, lv, grp, sums, counts)
        return sums.cpu(), counts.cpu()

    def masked_sums(mu, var, y, sums, counts):
        for c in range(C):
            i = y == c
            m, v = mu[i], var[i]                     # the two mask selections of a class: each one synchronises
            sums[c, 0] += m.sum(0)
            sums[c, 1] += m.pow(2).sum(0)
            sums[c, 2] += v.sum(0)
            sums[c, 3] += v.pow(2).sum(0)
            counts[c] += len(m)

    def through_evaluate():
        sums, counts = accumulators()
        with torch.no_grad():
            for x, y in zip(xs, ys):
                out = net.evaluate(x, z_output=True)
                masked_sums(out[4], out[5].exp(), y, sums, counts)
        return sums.cpu(), counts.cpu()

    with torch.no_grad():
        posts = [net.latent_posterior(x) for x in xs]

    def kernel():
        sums, counts = accumulators()
        for (mu, lv), grp in zip(posts, groups):
            ops.latent_moments(mu, lv, grp, sums, counts)
        return sums, counts

    def by_torch():
        sums, counts = accumulators()
        for (mu, lv), y in zip(posts, ys):
            masked_sums(mu, lv.exp(), y, sums, counts)
        return sums, counts

    out = {'metric': 'inspection_bench', 'device': torch.cuda.get_device_name(0),
           'arch': getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''), 'torch': torch.__version__, 'hip': torch.version.hip,
           'calls': a.calls, 'warmup': a.warmup, 'timing': 'HIP events around each call (all batches), median of the calls',
           'shape': dict(config=2, N=N, batches=a.batches, C=C, K=K, L=net.latent_sampling)}
    out['zsample_latent_posterior'] = timed(encode_only, a.calls, a.warmup)
    out['zsample_evaluate'] = timed(through_evaluate, a.calls, a.warmup)
    out['moments_kernel'] = timed(kernel, a.calls, a.warmup)
    out['moments_torch_masks'] = timed(by_torch, a.calls, a.warmup)
    out['evaluate_over_latent_posterior'] = out['zsample_evaluate']['ms_median'] / out['zsample_latent_posterior']['ms_median']
    out['torch_masks_over_kernel'] = out['moments_torch_masks']['ms_median'] / out['moments_kernel']['ms_median']
    k, t = kernel()[0], by_torch()[0]
    out['max_relative_difference'] = float((k - t).abs().max() / t.abs().max())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
