#!/usr/bin/env python3
"""Time the 2-D projections of jvae_compat/inspection.py on the GPU and write profiles/proj2d_bench.json.

    python tools/proj2d_bench.py [--out profiles/proj2d_bench.json] [--max-iter 1000]

  TSNE.fit_transform   N = 2 000 and N = 10 000 points of K = 128 (three seeded blobs), init='pca', the full 1 000 iterations
  PCA.fit_transform    (36 032, 128)
  and the phases of the t-SNE at each N on their own: distances, affinities, one gradient (with and without the KL pass), one
  update.

HIP events around each call, 1 warm-up call, the median (min - max) of 5.  Beside them the file repeats scikit-learn's
recorded wall times (tests/golden/proj2d/timing.json: 300 points on the CPU of the machine that wrote the fixtures - context,
not a bar)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd'), os.path.join(REPO, 'tools'), os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from aggregation_bench import timed as _timed  # noqa: E402
import proj2d_cases as R  # noqa: E402


def timed(fn, calls, warmup, what=''):
    t = _timed(fn, calls, warmup)
    print(what, t, file=sys.stderr, flush=True)          # progress: the large sizes take a while
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--sizes', type=int, nargs='*', default=[2000, 10000])
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'proj2d_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('proj2d_bench needs the GPU: nothing is measured without one')
    from jvae_compat import inspection
    from jvae_hip import ops
    dev = 'cuda:0'
    out = {'metric': 'proj2d_bench', 'device': torch.cuda.get_device_name(0),
           'arch': getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''), 'torch': torch.__version__, 'hip': torch.version.hip,
           'calls': a.calls, 'warmup': a.warmup, 'max_iter': a.max_iter,
           'timing': 'HIP events around each call, median (min - max) of the calls after the warm-up'}
    with open(os.path.join(R.GOLDEN, 'timing.json')) as f:
        out['scikit_learn_cpu_300_points'] = json.load(f)
    K = 128
    for N in a.sizes:
        x = torch.from_numpy(R.blobs(N, K, N)[0]).to(dev)
        rec = {}
        tsne = inspection.TSNE(2, init='pca', max_iter=a.max_iter, device=dev)
        rec['fit_transform'] = timed(lambda: tsne.fit_transform(x), a.calls, a.warmup, f'{N} fit_transform')
        rec['kl_divergence'], rec['n_iter'] = tsne.kl_divergence_, tsne.n_iter_ + 1
        rec['purity'] = R.nearest_neighbour_purity(tsne.embedding_, R.blobs(N, K, N)[1]) if N <= 4000 else None
        rec['distances'] = timed(lambda: ops.pairwise_sqdist(x), a.calls, a.warmup, f'{N} distances')
        d = ops.pairwise_sqdist(x)
        rec['affinities'] = timed(lambda: ops.tsne_affinities(d, 30.), a.calls, a.warmup, f'{N} affinities')
        P = ops.tsne_affinities(d, 30.)[0]
        y = torch.from_numpy(tsne.embedding_).to(dev)
        g, stats = torch.empty_like(y), torch.zeros(2, dtype=torch.float64, device=dev)
        rec['gradient'] = timed(lambda: ops.tsne_gradient(P, y, 1., g=g), a.calls, a.warmup, f'{N} gradient')
        rec['gradient_with_kl'] = timed(lambda: ops.tsne_gradient(P, y, 1., g=g, stats=stats), a.calls, a.warmup, f'{N} gradient_with_kl')
        u, k = torch.zeros_like(y), torch.ones_like(y)
        rec['update'] = timed(lambda: ops.tsne_update(y.clone(), u, k, g, 0.8, 200.), a.calls, a.warmup, f'{N} update')
        out[f'tsne_{N}x{K}'] = rec
        del d, P
    xp = torch.from_numpy(R.blobs(36032, K, 7)[0]).to(dev)
    pca = inspection.PCA(2, device=dev)
    out['pca_36032x128'] = {'fit_transform': timed(lambda: pca.fit_transform(xp), a.calls, a.warmup),
                            'moments': timed(lambda: ops.pca_moments(xp), a.calls, a.warmup)}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
