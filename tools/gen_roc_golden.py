#!/usr/bin/env python3
"""Write tests/golden/roc/*.npz: score sets and what the REFERENCE's utils/roc_curves.py::roc_curve returns for them.

    python tools/gen_roc_golden.py --reference <checkout of moxime/joint-vae> [--timing]

The reference module is loaded from the given checkout (it needs numpy, scikit-learn and SciPy, nothing else of the
reference); only data is written: the fp32 scores, the kept TPRs and, per mode (0 = one-sided, 1 = 'around-mean'), the
reference's AUC, kept FPR / TPR and the two threshold vectors.  The reference is fed the scores widened to fp64, which is
what the device kernels compute on.

In-scores are integer multiples of 2^-10 with magnitude below 16: their fp64 sum is exact in any order, so the centre of
the around-mean mode is one correctly rounded division and nothing in a golden depends on a summation order.

--timing also times the reference on 11 rows of (10 000, 26 032) scores on this CPU and stores the figure in
tests/golden/roc/timing.json (the yardstick tools/roc_bench.py compares the device ROC against).
"""
import argparse
import importlib.util
import json
import os
import platform
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'roc')
KEPT10 = [pc / 100 for pc in range(90, 100)]                  # cvae.py:1736


def grid_scores(rng, n, mean=0., std=1., levels=None):
    """fp32 multiples of 2^-10 in (-16, 16); `levels`: quantise to that many values first (heavy ties)."""
    v = rng.standard_normal(n) * std + mean
    if levels:
        v = np.round(v * levels / 8) * 8 / levels
    return np.clip(np.round(v * 1024) / 1024, -15.5, 15.5).astype(np.float32)


def cases():
    rng = np.random.default_rng(20240607)
    c = {}
    for n_in, n_out in ((10000, 9000), (1000, 26032), (257, 100), (1, 5), (4096, 1)):
        c[f'gauss_{n_in}_{n_out}'] = dict(ins=grid_scores(rng, n_in, 1.), outs=rng.standard_normal(n_out).astype(np.float32))
    c['separated_500_300'] = dict(ins=grid_scores(rng, 500, 8., .5), outs=(rng.standard_normal(300) * .5 - 8).astype(np.float32))
    same = grid_scores(rng, 400)
    c['identical_400'] = dict(ins=same, outs=same.copy())
    c['ties_2000_1500'] = dict(ins=grid_scores(rng, 2000, .5, 1., levels=64), outs=grid_scores(rng, 1500, -.5, 1., levels=64))
    ins, outs = grid_scores(rng, 300, 1.), rng.standard_normal(200).astype(np.float32)
    ins[[3, 77]], ins[150], outs[[0, 9]], outs[100] = np.inf, -np.inf, -np.inf, np.inf
    c['inf_300_200'] = dict(ins=ins, outs=outs, modes=(0,))      # around-mean: the reference raises on a non-finite in-score
    c['kept11_1000_800'] = dict(ins=grid_scores(rng, 1000, 1.), outs=rng.standard_normal(800).astype(np.float32),
                                kept=KEPT10 + [0.999])
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds utils/roc_curves.py)')
    ap.add_argument('--timing', action='store_true')
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location('ref_roc_curves', os.path.join(a.reference, 'utils', 'roc_curves.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    os.makedirs(OUT, exist_ok=True)
    for name, case in cases().items():
        kept = np.asarray(case.get('kept', KEPT10), np.float64)
        data = dict(ins=case['ins'], outs=case['outs'], kept=kept, modes=np.asarray(case.get('modes', (0, 1)), np.int32))
        for mode in data['modes']:
            auc, fpr, tpr, thr = ref.roc_curve(case['ins'].astype(np.float64), case['outs'].astype(np.float64), *kept,
                                               two_sided='around-mean' if mode else False)
            data.update({f'auc_{mode}': np.float64(auc), f'fpr_{mode}': fpr, f'tpr_{mode}': tpr,
                         f'low_{mode}': thr['low'], f'up_{mode}': thr['up']})
            print(f'{name:24s} mode {mode}: auc {auc:.6f}  fpr@95 {fpr[5]:.4f}')
        np.savez_compressed(os.path.join(OUT, name + '.npz'), **data)
    if a.timing:
        rng = np.random.default_rng(7)
        modes = [m % 2 for m in range(11)]
        rows = [(grid_scores(rng, 10000, 1.).astype(np.float64), rng.standard_normal(26032).astype(np.float32).astype(np.float64))
                for _ in modes]
        t0 = time.perf_counter()
        for (i, o), m in zip(rows, modes):
            ref.roc_curve(i, o, *KEPT10, two_sided='around-mean' if m else False)
        dt = time.perf_counter() - t0
        json.dump({'what': 'reference utils/roc_curves.py::roc_curve, 11 rows in sequence, one CPU core', 'n_in': 10000,
                   'n_out': 26032, 'modes': modes, 'seconds': dt, 'machine': platform.machine(),
                   'python': platform.python_version(), 'numpy': np.__version__},
                  open(os.path.join(OUT, 'timing.json'), 'w'), indent=1)
        print(f'reference, 11 rows of (10000, 26032): {dt:.3f} s')


if __name__ == '__main__':
    main()
