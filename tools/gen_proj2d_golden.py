#!/usr/bin/env python3
"""Write tests/golden/proj2d/: what scikit-learn (1.7) computes where `jvae_compat.inspection.PCA` / `TSNE` and the kernels of
csrc/embed.hip are its restatement, on seeded blobs.

    python tools/gen_proj2d_golden.py

Runs on the CPU and needs scikit-learn and scipy; the tests that read the files need neither.  Only data is written.  Per case
(N, K, perplexity) of tests/proj2d_cases.py::CASES, `case_<N>_<K>_<perplexity>.npz`:

  x, label            the blobs (fp32) and the blob of every row
  d                   the fp32 squared distances by the rule of the distance kernel (proj2d_cases.sqdist)
  cond_rows, cond     rows of scikit-learn's conditional P (`_binary_search_perplexity` on d), fp64: all rows up to N = 130, every
                      7th beyond
  joint               scikit-learn's joint P (`_joint_probabilities` on d), condensed, fp64
  y_small, y_unit     two embeddings (fp32): the PCA initialisation of TSNE (PCA(2) / std of the first column * 1e-4; a 1e-4
                      normal draw where K = 1) and a unit-scale normal draw
  kl.<y>.<f>, g.<y>.<f>   `_kl_divergence` at each embedding with the factor f = 1 and 12 on P, where P is the fp32 rounding of
                      `joint` widened again - what the device keeps in memory
  pca.mean, pca.components, pca.variance, pca.out   sklearn.decomposition.PCA(min(2, K), svd_solver='full') on the fp64 copy of x
  margin              the smallest ||H - log perplexity| - 1e-5f| over every step of the search: below 1e-9 the case is a knife
                      edge and must be re-seeded (ASSERTED)

and for (300, 16, 30): `init` (= y_small), `kl_exact` = kl_divergence_ of TSNE(method='exact', init=init), `kl_runs` and
`purity_runs`, the same for five inits perturbed at the 1e-6 level, and in timing.json scikit-learn's wall time of the exact
and of the Barnes-Hut run on the machine that wrote the files.

update.npz: 25 iterations of scikit-learn's `_gradient_descent` (momentum 0.8, learning rate 200) from `p0` on the gradients
`base * flip ** t` - half of the entries keep their sign (the gains grow), half change it every iteration (the gains shrink to
the 0.01 clip) - and the `p` it returns."""
import json
import os
import sys
import time

import numpy as np
from sklearn.decomposition import PCA
from sklearn.manifold import TSNE, _t_sne, _utils

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import proj2d_cases as R  # noqa: E402


def update_record():
    rng = np.random.default_rng(3)
    p0, base = (rng.standard_normal(64).astype(np.float32) for _ in range(2))
    flip = np.where(np.arange(64) % 2, -1., 1.).astype(np.float32)
    step = iter(range(25))
    p, _, it = _t_sne._gradient_descent(lambda p, **kw: (0., base * flip ** next(step)), p0.copy(), it=0, max_iter=25, momentum=0.8,
                                        learning_rate=200.)
    assert it == 24 and p.dtype == np.float32
    np.savez(os.path.join(R.GOLDEN, 'update.npz'), p0=p0, base=base, flip=flip, p=p, momentum=0.8, learning_rate=200., steps=25)


def main():
    os.makedirs(R.GOLDEN, exist_ok=True)
    update_record()
    for (N, K, perplexity), seed in R.CASES.items():
        x, label = R.blobs(N, K, seed)
        d = R.sqdist(x)
        cond = _utils._binary_search_perplexity(d, perplexity, 0)
        joint = _t_sne._joint_probabilities(d, perplexity, 0)
        margin = R.search(d, perplexity)[3]
        print(f'case {(N, K, perplexity)}: knife-edge margin {margin:.3g}')
        assert margin > R.KNIFE_EDGE, 're-seed this case'
        rows = np.arange(N) if N <= 130 else np.arange(0, N, 7)
        rng = np.random.default_rng(100 + seed)
        x64 = x.astype(np.float64)
        nc = min(2, K)
        pca = PCA(nc, svd_solver='full')
        out = pca.fit_transform(x64)
        if K >= 2:
            y_small = (out.astype(np.float32) / np.std(out.astype(np.float32)[:, 0]) * 1e-4).astype(np.float32)
        else:
            y_small = (1e-4 * rng.standard_normal((N, 2))).astype(np.float32)
        y_unit = rng.standard_normal((N, 2)).astype(np.float32)
        rec = dict(x=x, label=label, d=d, cond_rows=rows, cond=cond[rows], joint=joint, y_small=y_small, y_unit=y_unit,
                   margin=margin)
        rec.update({'pca.mean': pca.mean_, 'pca.components': pca.components_, 'pca.variance': pca.explained_variance_,
                    'pca.out': out})
        P32 = joint.astype(np.float32).astype(np.float64)
        for name, y in (('small', y_small), ('unit', y_unit)):
            for f in (1, 12):
                kl, g = _t_sne._kl_divergence(y.ravel().copy(), P32 * f, 1, N, 2)
                rec[f'kl.{name}.{f}'], rec[f'g.{name}.{f}'] = kl, g.reshape(N, 2)
                assert g.dtype == np.float32
        if (N, K, perplexity) == (300, 16, 30):
            rec['init'] = y_small
            t0 = time.perf_counter()
            exact = TSNE(2, method='exact', perplexity=perplexity, init=y_small.copy())
            exact.fit(x)
            t_exact = time.perf_counter() - t0
            again = TSNE(2, method='exact', perplexity=perplexity, init=y_small.copy()).fit(x)
            assert np.array_equal(exact.embedding_, again.embedding_), 'the exact method is expected to be deterministic'
            rec['kl_exact'] = exact.kl_divergence_
            t0 = time.perf_counter()
            TSNE(2, method='barnes_hut', perplexity=perplexity, init=y_small.copy()).fit(x)
            t_bh = time.perf_counter() - t0
            kls, purity = [], []
            for _ in range(5):
                init = (y_small * (1. + 1e-6 * rng.standard_normal(y_small.shape))).astype(np.float32)
                run = TSNE(2, method='exact', perplexity=perplexity, init=init).fit(x)
                kls.append(run.kl_divergence_)
                purity.append(R.nearest_neighbour_purity(run.embedding_, label))
            print('five perturbed runs: KL', kls, 'purity', purity)
            rec['kl_runs'], rec['purity_runs'] = np.array(kls), np.array(purity)
            with open(os.path.join(R.GOLDEN, 'timing.json'), 'w') as f:
                json.dump({'case': [N, K, perplexity], 'sklearn_exact_seconds': round(t_exact, 3),
                           'sklearn_barnes_hut_seconds': round(t_bh, 3), 'max_iter': 1000}, f, indent=1)
        np.savez_compressed(R.case_file(N, K, perplexity), **rec)
        print('  wrote', R.case_file(N, K, perplexity), os.path.getsize(R.case_file(N, K, perplexity)), 'bytes')


if __name__ == '__main__':
    main()
