#!/usr/bin/env python3
"""Time ops.aggpost_logdensity (csrc/aggpost.hip: the log-density of the aggregate posterior of a bank of N diagonal Gaussians at
M codes) at N = 50 000 bank rows (the CIFAR-10 training set), M = 10 000 queries and K = 64 (the latent size of BASELINE
configs[1]), with and without the per-coordinate marginals, and beside it, interleaved call by call, the CHUNKED torch expression
a user could run today: per chunk of queries the materialised (chunk, N, K) block of exponents, its sum over k and
torch.logsumexp over the bank (chunks of `--chunk-mb` of fp32 exponents); with the marginals, torch.logsumexp over the block itself.

    python tools/aggpost_bench.py [--calls 20] [--warmup 3] [--out profiles/aggpost_bench.json]

HIP events around one call on the launch stream; medians and min-max over `calls` calls after the warm-up.  The pair-coordinate
products the definition needs - N M K - and, with the marginals, as many exponentials over the kernel path's time are reported as
rates.  Prints one JSON line."""
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


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_max_ms': [float(np.min(ms)), float(np.max(ms))]}


def torch_logdensity(z, mu, lv, dims, chunk):
    """log q(z) (and the per-coordinate marginals) from torch ops: materialised (chunk, N, K) blocks and torch.logsumexp."""
    N, K = mu.shape
    w, half_c = (-lv).exp(), 0.5 * lv.sum(1)
    logq = torch.empty(z.shape[0], dtype=torch.float32, device=z.device)
    logq_dims = torch.empty_like(z) if dims else None
    for i in range(0, z.shape[0], chunk):
        E = (z[i:i + chunk, None, :] - mu[None]).square_().mul_(w[None])                # (chunk, N, K)
        logq[i:i + chunk] = torch.logsumexp(E.sum(2).mul_(-0.5).sub_(half_c[None]), 1)
        if dims:
            logq_dims[i:i + chunk] = torch.logsumexp(E.add_(lv[None]).mul_(-0.5), 1)
    logq -= math.log(N) + 0.5 * K * math.log(2 * math.pi)
    if dims:
        logq_dims -= math.log(N) + 0.5 * math.log(2 * math.pi)
    return logq, logq_dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=1024)
    ap.add_argument('--N', type=int, default=50000)
    ap.add_argument('--M', type=int, default=10000)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from jvae_hip import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    N, M, K = a.N, a.M, a.K
    # posteriors as a trained encoder leaves them: means of unit scale, variances log-uniform in [1e-4, 1]; a query is a draw of a row
    mu = torch.randn(N, K, device=dev, generator=g)
    lv = -math.log(1e4) * torch.rand(N, K, device=dev, generator=g)
    src = torch.randint(0, N, (M,), device=dev, generator=g)
    z = (mu[src] + (0.5 * lv[src]).exp() * torch.randn(M, K, device=dev, generator=g)).contiguous()
    out = {'metric': 'aggpost_logdensity_ms', 'N': N, 'M': M, 'K': K, 'calls': a.calls, 'warmup': a.warmup,
           'partition': ops.aggpost_partition(),
           'timing': 'HIP events around one call on the launch stream; kernel and torch calls interleaved; medians, min-max',
           'torch': f'per chunk of queries ({a.chunk_mb} MB of fp32 exponents) the materialised (chunk, N, K) block, its sum over k '
                    'and torch.logsumexp over the bank; with dims torch.logsumexp over the block as well'}
    bank = ops.aggpost_bank(mu, lv)
    out['prepare'] = stats([event_ms(lambda: ops.aggpost_bank(mu, lv)) for _ in range(a.warmup + a.calls)][a.warmup:])
    chunk = max(1, (a.chunk_mb << 20) // (4 * N * K))
    pieces = math.ceil(N / ops.aggpost_partition())
    for dims in (False, True):
        got, ref = ops.aggpost_logdensity(z, bank, dims=dims), torch_logdensity(z, mu, lv, dims, chunk)
        ms = {'kernel': [], 'torch': []}
        for i in range(a.warmup + a.calls):
            for name, fn in (('kernel', lambda: ops.aggpost_logdensity(z, bank, dims=dims)),
                             ('torch', lambda: torch_logdensity(z, mu, lv, dims, chunk))):
                t = event_ms(fn)
                if i >= a.warmup:
                    ms[name].append(t)
        k = float(np.median(ms['kernel']))
        row = {'kernel': stats(ms['kernel']), 'torch': stats(ms['torch']), 'torch_over_kernel': float(np.median(ms['torch'])) / k,
               'pair_coordinates': N * M * K, 'pair_coordinates_per_s': N * M * K * (2 if dims else 1) / (k * 1e-3),
               'workspace_mb': pieces * M * (12 + (8 * K if dims else 0)) / 2 ** 20,
               'max_difference_over_1_plus_abs': float(((got[0] - ref[0]).abs() / (1 + ref[0].abs())).max())}
        if dims:
            row['exponentials_per_s'] = N * M * K / (k * 1e-3)
            row['max_difference_over_1_plus_abs_dims'] = float(((got[1] - ref[1]).abs() / (1 + ref[1].abs())).max())
        out['dims' if dims else 'logq'] = row
    ops.aggpost_check_status()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
