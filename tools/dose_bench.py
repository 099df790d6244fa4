#!/usr/bin/env python3
"""Time ops.kde_logdensity (csrc/dose.hip: the Gaussian kernel density estimate of S statistics over a score bank, one scoring
launch and one merge launch) at S = 5 statistics and M = 50 000 bank samples, for N = 100 queries (one batch) and N = 26 032 (one
OOD set), and beside it, interleaved call by call, a CHUNKED torch logsumexp of the same values on the same device: per
statistic and chunk of queries the (chunk, M) matrix of exponents, torch.logsumexp over it, the joint row from their scaled sum
(chunks of `--chunk-mb` of fp32 exponents).  Also ops.kde_fit over the bank.

    python tools/dose_bench.py [--calls 20] [--warmup 3] [--out profiles/dose_bench.json]

HIP events around one call on the launch stream; medians and min-max over `calls` calls after the warm-up.  The exponentials
the definitions need - N M (S + 1) - over the kernel's time are reported as a rate.  Prints one JSON line."""
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


def torch_logdensity(raw, fit, chunk):
    """The marginal rows, `dose` and `dose-joint` from torch ops on the standardised fp32 values the kernel uses."""
    S, M = fit['S'], fit['M']
    t = ((raw.double() - fit['centre'][:, None]) / fit['h1'][:, None]).float()
    ratio2 = float((fit['h1'][0] / fit['hS'][0]) ** 2)
    out = torch.empty((S + 2, raw.shape[1]), dtype=torch.float32, device=raw.device)
    for i in range(0, raw.shape[1], chunk):
        joint = None
        for s in range(S):
            E = (t[s, i:i + chunk, None] - fit['z'][s][None]).square().mul_(-0.5)
            out[s, i:i + chunk] = torch.logsumexp(E, 1) - fit['lognorm'][s].float()
            joint = E if joint is None else joint.add_(E)
        out[S + 1, i:i + chunk] = torch.logsumexp(joint.mul_(ratio2), 1) - fit['lognorm'][S].float()
    out[S] = out[:S].sum(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chunk-mb', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from jvae_hip import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    S, M = 5, 50000
    off = torch.tensor([-3000., 30., 25., 0.01, -2990.], device=dev)[:, None]
    scale = torch.tensor([40., 3., 2., 1e-3, 40.], device=dev)[:, None]
    bank = off + scale * torch.randn(S, M, device=dev, generator=g)
    out = {'metric': 'kde_logdensity_ms', 'S': S, 'M': M, 'calls': a.calls, 'warmup': a.warmup, 'partition': ops.kde_partition(),
           'timing': 'HIP events around one call on the launch stream; kernel and torch calls interleaved; medians, min-max',
           'torch': f'per statistic and chunk of queries ({a.chunk_mb} MB of fp32 exponents) the (chunk, M) exponents and '
                    'torch.logsumexp, the joint row from their sum'}
    fit = ops.kde_fit(bank)
    out['fit'] = dict(stats([event_ms(lambda: ops.kde_fit(bank)) for _ in range(a.warmup + a.calls)][a.warmup:]), launches=5,
                      note='with the read of its status word')
    chunk = max(1, (a.chunk_mb << 20) // (4 * M))
    for N in (100, 26032):
        far = torch.where(torch.arange(N, device=dev) % 5 == 4, 8., 1.)
        raw = (off + scale * far * torch.randn(S, N, device=dev, generator=g)).contiguous()
        got, ref = ops.kde_logdensity(raw, fit), torch_logdensity(raw, fit, chunk)
        ms = {'kernel': [], 'torch': []}
        for i in range(a.warmup + a.calls):
            for name, fn in (('kernel', lambda: ops.kde_logdensity(raw, fit)), ('torch', lambda: torch_logdensity(raw, fit, chunk))):
                t = event_ms(fn)
                if i >= a.warmup:
                    ms[name].append(t)
        k = float(np.median(ms['kernel']))
        out[f'N={N}'] = {'kernel': stats(ms['kernel']), 'torch': stats(ms['torch']),
                         'torch_over_kernel': float(np.median(ms['torch'])) / k,
                         'exponentials': N * M * (S + 1), 'exponentials_per_s': N * M * (S + 1) / (k * 1e-3),
                         'workspace_mb': math.ceil(M / ops.kde_partition()) * (S + 1) * N * 8 / 2 ** 20,
                         'max_difference_over_1_plus_abs': float(((got[:S + 2] - ref).abs() / (1 + ref.abs())).max())}
    ops.kde_check_status()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
