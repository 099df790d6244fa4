#!/usr/bin/env python3
"""Time what module/aggregation.py adds, each against the same formulas written with the torch ops and the library ops the project
had before it, on the same device:

  latent_mi   given the two models' draws z (L, N, K): the kernel chain of `latent_mutual_info` (two `ops.class_posterior`, the
              argmax of the mean log-density, `ops.latent_mutual_info`) against `GaussianPrior.log_density` on the expanded z,
              (logp / T).softmax(0), the broadcast product of the two posteriors, sum over the classes, log, mean - the
              reference's arithmetic.  Shapes: C = 10, L0 = L1 = 128, N = 256, K = 64 and C = 100, L = 32, N = 256, K = 64, T = 1.
              Also the peak memory each side adds while it runs, and the largest difference of their Im.
  ensemble    `ensemble()` at E = 3, C = 10, N = 26 032 (the SVHN test set), the ten temperatures of results/aggregation.py:279,
              for 'mean', 'joint' and 'mean~', against the torch expressions of module/aggregation.py written out.

    python tools/aggregation_bench.py [--calls 20] [--warmup 5] [--out profiles/aggregation_bench.json]

HIP events around each call on the current stream, after a warm-up; the median of the calls, minimum and maximum beside it.
Prints one JSON line.  No ratio is promised: the figures are whatever was measured."""
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

RESULT_TEMPS = [-1, 1, 2, 5, 10, 20, 50, 100, 200, 500]


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


def peak_rise(fn):
    """Bytes the call adds at its peak to what is allocated when it starts (after a call that has warmed every cache)."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return int(rise)


def latent_mi_case(C, L0, L1, N, K, calls, warmup, dev):
    from jvae_hip import ops
    from module import aggregation as A
    from module.priors import GaussianPrior
    g = torch.Generator(device=dev).manual_seed(0)
    priors = []
    for _ in range(2):
        pr = GaussianPrior(K, var_dim='scalar', num_priors=C, init_mean=1., learned_means=True).to(dev)
        with torch.no_grad():
            pr.mean.copy_(torch.randn(C, K, device=dev, generator=g))
            pr._var_parameter.copy_(.8 + .4 * torch.rand(C, device=dev, generator=g))
        priors.append(pr)
    z = [torch.randn(L, N, K, device=dev, generator=g) * 1.2 for L in (L0, L1)]
    kept = {}

    def kernels():
        with torch.no_grad():
            logp, P0 = A.class_posteriors(priors[0], z[0], [1])
            _, P1 = A.class_posteriors(priors[1], z[1], [1], logp=False)
            _, _, _, y_ = ops.aggregate_scores([logp.mean(1)], 'joint', factors=1., post=False, argmax=True)
            kept['kernels'] = (ops.latent_mutual_info(P0, P1)[0], y_)
        return kept['kernels']

    def by_torch():
        with torch.no_grad():
            pyz = []
            for pr, zi in zip(priors, z):
                L = zi.shape[0]
                y = torch.arange(C, device=dev).view(C, 1, 1).expand(C, L, N)
                logp = pr.log_density(zi.unsqueeze(0).expand(C, L, N, K), y)
                pyz.append((logp / 1).softmax(0))
                if len(pyz) == 1:
                    y_ = logp.mean(1).argmax(0)
            Im = (pyz[0].unsqueeze(1) * pyz[1].unsqueeze(2)).sum(0).log().mean((0, 1))
            kept['torch'] = (Im, y_)
        return kept['torch']
    out = {'shape': dict(C=C, L0=L0, L1=L1, N=N, K=K, temps=[1])}
    out['kernel_chain'], out['torch_ops'] = timed(kernels, calls, warmup), timed(by_torch, calls, warmup)
    out['torch_over_kernels'] = out['torch_ops']['ms_median'] / out['kernel_chain']['ms_median']
    out['peak_bytes'] = {'kernel_chain': peak_rise(kernels), 'torch_ops': peak_rise(by_torch), 'z': int(sum(t.numel() for t in z) * 4),
                         'one_expanded_z': C * max(L0, L1) * N * K * 4}
    a, b = kept['kernels'], kept['torch']
    out['max_abs_difference_of_Im'] = float((a[0] - b[0]).abs().max())
    out['max_abs_Im'] = float(b[0].abs().max())
    out['predictions_that_differ'] = int((a[1] != b[1]).sum())
    return out


def ensemble_case(E, C, N, calls, warmup, dev):
    from module import aggregation as A
    g = torch.Generator(device=dev).manual_seed(1)
    scores = {'iws': [-1000. + 30. * torch.randn(C, N, device=dev, generator=g) for _ in range(E)],
              'zdist': [(30. + 8. * torch.randn(C, N, device=dev, generator=g)).abs() for _ in range(E)],
              'kl': [(20. + 5. * torch.randn(C, N, device=dev, generator=g)).abs() for _ in range(E)]}
    temps = RESULT_TEMPS

    def posterior(logits):
        return {t: logits.clone() if t in (None, -1, 0) else (logits / t).softmax(0) for t in temps}

    def lme(ts):
        t = torch.stack(ts)
        ref = t.max(0)[0]
        return (t - ref).exp().mean(0).log() + ref

    def by_torch(agg):
        def call():
            if agg == 'mean':
                p = posterior(lme(scores['iws']))
                extra = lme(scores['iws']).max(0)[0]
            elif agg == 'joint':
                p, extra = posterior(-torch.stack(scores['zdist']).sum(0) / 2), None
            else:
                each = [posterior(-k) for k in scores['kl']]
                p, extra = {t: torch.stack([e[t] for e in each]).mean(0) for t in temps}, None
            return p, p[temps[0]].argmax(0), p[temps[0]].max(0)[0], extra
        return call
    out = {'shape': dict(E=E, C=C, N=N, temps=temps)}
    for agg in ('mean', 'joint', 'mean~'):
        k, t = timed(lambda: A.ensemble(scores, agg, temps), calls, warmup), timed(by_torch(agg), calls, warmup)
        mine, ref = A.ensemble(scores, agg, temps), by_torch(agg)()
        worst = max(float((mine['p_y_x'][tp] - ref[0][tp]).abs().max() / ref[0][tp].abs().max()) for tp in temps)
        out[agg] = {'ensemble': k, 'torch_ops': t, 'torch_over_ensemble': t['ms_median'] / k['ms_median'],
                    'max_relative_difference': worst, 'predictions_that_differ': int((mine['y'] != ref[1]).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('aggregation_bench needs the GPU: nothing is measured without one')
    dev = 'cuda:0'
    out = {'metric': 'aggregation_bench', 'device': torch.cuda.get_device_name(0),
           'arch': getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''), 'torch': torch.__version__, 'hip': torch.version.hip,
           'calls': a.calls, 'warmup': a.warmup, 'timing': 'HIP events around each call, median of the calls',
           'latent_mi': [latent_mi_case(10, 128, 128, 256, 64, a.calls, a.warmup, dev),
                         latent_mi_case(100, 32, 32, 256, 64, a.calls, a.warmup, dev)],
           'ensemble': ensemble_case(3, 10, 26032, a.calls, a.warmup, dev)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
