#!/usr/bin/env python3
"""Write tests/golden/rocq/*.npz: score sets and what the REFERENCE's utils/roc_curves.py::roc_curve returns for them in its
tuple mode, two_sided=(f_low, f_up) - the '-a-x-y' OOD methods.

    python tools/gen_rocq_golden.py --reference <checkout of moxime/joint-vae> [--timing]

With validation=0 the reference fits UnivariateSpline(k=3, s=0) through the sorted in-scores and evaluates it at its own
knots: the sorted in-scores again, up to FITPACK's rounding.  Per case and factor pair two records are written:

    a   the reference's roc_curve with ONLY `UnivariateSpline` replaced, in that module's namespace, by a stand-in that
        returns the data at the integer positions it is asked for.  This is what the device ROC reproduces.
    b   the unpatched reference on the same data: the record of how far FITPACK's rounding moves the results ('b_ok' = 0
        where the reference raises, as it does on non-finite in-scores).

Only data is written: the fp32 scores, the kept TPRs, the factor pairs and, per pair and record, the AUC, kept FPR / TPR
and the two threshold vectors.  The reference is fed the scores widened to fp64, which is what the device kernels compute
on.  The score families are those of tools/gen_roc_golden.py (with in-sets of at least 4 scores, the least the spline fit
takes), two tiny in-sets and one continuous set off the 2^-10 grid.

--timing also times the unpatched reference on 4 rows of (10 000, 26 032) scores on this CPU and stores the figure in
tests/golden/rocq/timing.json (the yardstick tools/rocq_bench.py quotes beside the device ROC).
"""
import argparse
import importlib.util
import json
import os
import platform
import time

import numpy as np

from gen_roc_golden import KEPT10, cases as roc_cases, grid_scores

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'rocq')
PAIRS = [(1, 1), (4, 1), (1, 4), (2, 3), (7, 7)]


class KnotValues:
    """Stand-in for scipy.interpolate.UnivariateSpline(x, y, k=3, s=0) asked for its values at its own knots x = 0 .. n - 1."""

    def __init__(self, x, y, k=3, s=0):
        assert len(x) > k and s == 0
        self.y = np.asarray(y)

    def __call__(self, at):
        i = np.rint(at).astype(np.int64)
        assert np.array_equal(i, at)
        return self.y[i]


def cases():
    c = {k: v for k, v in roc_cases().items() if len(v['ins']) >= 4}
    rng = np.random.default_rng(20241017)
    for n_in in (4, 5):
        c[f'gauss_{n_in}_50'] = dict(ins=grid_scores(rng, n_in, 1.), outs=rng.standard_normal(50).astype(np.float32))
    c['continuous_3000_2000'] = dict(ins=(rng.standard_normal(3000) + 1).astype(np.float32),
                                     outs=rng.standard_normal(2000).astype(np.float32))
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds utils/roc_curves.py)')
    ap.add_argument('--timing', action='store_true')
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location('ref_roc_curves', os.path.join(a.reference, 'utils', 'roc_curves.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    fitpack = ref.UnivariateSpline
    os.makedirs(OUT, exist_ok=True)
    for name, case in cases().items():
        kept = np.asarray(case.get('kept', KEPT10), np.float64)
        ins, outs = case['ins'].astype(np.float64), case['outs'].astype(np.float64)
        data = dict(ins=case['ins'], outs=case['outs'], kept=kept, pairs=np.asarray(PAIRS, np.int32))
        for pair in PAIRS:
            tag = '{}_{}'.format(*pair)
            for rec, spline in (('a', KnotValues), ('b', fitpack)):
                ref.UnivariateSpline = spline
                try:
                    auc, fpr, tpr, thr = ref.roc_curve(ins, outs, *kept, two_sided=pair)
                except Exception as e:                     # noqa: BLE001  (b only: FITPACK refuses non-finite data)
                    assert rec == 'b', (name, pair, e)
                    data[f'b_ok_{tag}'] = np.int32(0)
                    print(f'{name:24s} {tag} b: the reference raises {type(e).__name__}: {e}')
                    continue
                finally:
                    ref.UnivariateSpline = fitpack
                data.update({f'{rec}_auc_{tag}': np.float64(auc), f'{rec}_fpr_{tag}': fpr, f'{rec}_tpr_{tag}': tpr,
                             f'{rec}_low_{tag}': thr['low'], f'{rec}_up_{tag}': thr['up']})
                if rec == 'b':
                    data[f'b_ok_{tag}'] = np.int32(1)
                    print(f'{name:24s} {tag}: auc {data[f"a_auc_{tag}"]:.6f}  b - a: auc {auc - data[f"a_auc_{tag}"]:+.2e}  '
                          f'max |fpr| {np.abs(fpr - data[f"a_fpr_{tag}"]).max():.2e}')
        np.savez_compressed(os.path.join(OUT, name + '.npz'), **data)
    if a.timing:
        rng = np.random.default_rng(7)
        pairs = [(1, 1), (4, 1), (1, 1), (4, 1)]              # iws-a-1-1, iws-a-4-1, elbo-a-1-1, elbo-a-4-1
        rows = [(grid_scores(rng, 10000, 1.).astype(np.float64), rng.standard_normal(26032).astype(np.float32).astype(np.float64))
                for _ in pairs]
        t0 = time.perf_counter()
        for (i, o), pair in zip(rows, pairs):
            ref.roc_curve(i, o, *KEPT10, two_sided=pair)
        dt = time.perf_counter() - t0
        json.dump({'what': 'reference utils/roc_curves.py::roc_curve with two_sided=(f_low, f_up), 4 rows in sequence, one CPU core',
                   'n_in': 10000, 'n_out': 26032, 'pairs': pairs, 'seconds': dt, 'machine': platform.machine(),
                   'python': platform.python_version(), 'numpy': np.__version__},
                  open(os.path.join(OUT, 'timing.json'), 'w'), indent=1)
        print(f'reference, 4 quantile rows of (10000, 26032): {dt:.3f} s')


if __name__ == '__main__':
    main()
