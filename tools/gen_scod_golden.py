#!/usr/bin/env python3
"""Write tests/golden/scod/*.npz: inputs and what the REFERENCE's tests/scod.py computes for them.

    python tools/gen_scod_golden.py --reference <checkout of moxime/joint-vae> [--timing]

The reference module is loaded from the given checkout (it needs torch, scikit-learn and matplotlib, nothing else of the
reference); only data is written:

  curve-*.npz   scores (M, n) fp32, y_true / y_est (n,) int64 and, per row, scrisk's tpr / selective_risk / fpr, the kept figures
                fpr95 / sr95 and the three areas twice: `*_sk` as the reference prints them (sklearn.metrics.auc of its fp32
                curves) and `*_trapz`, the fp64 trapezoid of the same curves.
  rows-*.npz    a recorder's tensors (`t|<name>`), and `row|<r>|<g>|<weight>` = scoring(recorder, r, g, weight, mtype).
  e2e.npz       the tensors of three recorders (`t|<set>|<name>`) and, per variant, the five figures of the command-line block
                (`fig|<r>|<g>|<weight>`: fpr95, sr95, auroc, aust, auscodt as printed; `trapz|...`: the areas as fp64 trapezoids).

--timing also times scrisk on 6 rows of 10 000 + 26 032 scores on one core of this CPU and stores the figure in
tests/golden/scod/timing.json (the yardstick tools/scod_bench.py compares the device call against).
"""
import argparse
import importlib.util
import json
import os
import platform
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'scod')
TILE = 2048                                                    # ROC_TILE of csrc/roc_sort.h
trapezoid = getattr(np, 'trapezoid', None) or np.trapz


def distinct(rng, n, mean=0., std=1.):
    """n fp32 scores without two equal ones."""
    while True:
        v = (rng.standard_normal(n) * std + mean).astype(np.float32)
        if len(np.unique(v)) == n:
            return v


def labels(rng, n_in, n_ood, C=10, wrong=.2):
    """y_true (class, -1 for ood) and y_est of n_in + n_ood samples in a random order; wrong: share of misclassified in-samples
    (0: none, 1: all)."""
    y_true = np.concatenate([rng.integers(0, C, n_in), -np.ones(n_ood, np.int64)]).astype(np.int64)
    y_true = y_true[rng.permutation(n_in + n_ood)]
    y_est = np.where(y_true >= 0, y_true, rng.integers(0, C, n_in + n_ood)).astype(np.int64)
    miss = (rng.random(n_in + n_ood) < wrong) & (y_true >= 0)
    y_est[miss] = (y_est[miss] + 1 + rng.integers(0, C - 1, miss.sum())) % C
    return y_true, y_est


def curve_cases():
    rng = np.random.default_rng(20241019)
    c = {}

    def scores_for(y_true, M=1, levels=None):
        rows = []
        for m in range(M):
            s = distinct(rng, len(y_true)) + np.where(y_true < 0, np.float32(1 + .5 * m), np.float32(0))
            if levels:
                s = rng.integers(0, levels, len(y_true)).astype(np.float32) / 4 + np.where(y_true < 0, np.float32(.5), np.float32(0))
            elif len(np.unique(s)) != len(s):
                raise RuntimeError('equal scores')
            rows.append(s.astype(np.float32))
        return np.stack(rows)

    for name, n_in, n_ood, kw in (('small_5_3', 5, 3, {}), ('tile_minus_1', 1200, TILE - 1 - 1200, {}), ('tile', 1200, TILE - 1200, {}),
                                  ('tile_plus_1', 1200, TILE + 1 - 1200, {}), ('tiles_3000_2000', 3000, 2000, {}),
                                  ('all_correct_700_300', 700, 300, dict(wrong=0.)), ('all_wrong_300_700', 300, 700, dict(wrong=1.))):
        y_true, y_est = labels(rng, n_in, n_ood, **kw)
        c[name] = dict(scores=scores_for(y_true), y_true=y_true, y_est=y_est)
    y_true, y_est = labels(rng, 400, 250)                       # the lowest scores are all OOD: in_cum == 0 at the head
    s = scores_for(y_true)
    low = np.nonzero(y_true < 0)[0][:40]
    s[0, low] = -np.float32(50) - np.arange(40, dtype=np.float32)
    c['ood_head_400_250'] = dict(scores=s, y_true=y_true, y_est=y_est)
    y_true, y_est = labels(rng, 2500, 1700)
    c['rows3_2500_1700'] = dict(scores=scores_for(y_true, M=3), y_true=y_true, y_est=y_est)
    for name, n_in, n_ood in (('ties_300_200', 300, 200), ('ties_2600_1900', 2600, 1900)):
        y_true, y_est = labels(rng, n_in, n_ood)
        c[name] = dict(scores=scores_for(y_true, M=2, levels=8), y_true=y_true, y_est=y_est)
    return c


def figures(ref, auc, y_true, y_est, scores):
    """The command-line block of the reference from scrisk on (scod.py:229-235) -> curves, figures as printed, fp64 trapezoids."""
    tpr, sr, fpr = ref.scrisk(y_true, y_est, scores)
    fpr95 = fpr[tpr >= 0.95].min()
    sr95 = sr[tpr >= 0.95].min()
    auroc = auc(fpr, tpr)
    auscodrt = auc(tpr, 0.5 * sr + 0.5 * fpr)
    ausrt = auc(tpr, sr)
    half = (0.5 * sr + 0.5 * fpr).numpy().astype(np.float64)
    t, s, f = (v.numpy().astype(np.float64) for v in (tpr, sr, fpr))
    trapz = [trapezoid(t, f), trapezoid(s, t), trapezoid(half, t)]
    return (tpr.numpy(), sr.numpy(), fpr.numpy()), [float(fpr95), float(sr95), float(auroc), float(ausrt), float(auscodrt)], trapz


def wim_recorder(rng, n, C=10, at_rows=3, odin=True, y_est=True):
    """Tensors a WIM job's recorder holds (random values): the all-class losses, their `@` partners (zdist@ 2-D), labels."""
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    t = {'zdist': f(C, n).abs() * 20, 'pre-zdist': f(C, n).abs() * 15, 'kl': f(C, n).abs() * 9, 'iws': f(C, n) * 30,
         'zdist@': f(at_rows, n).abs() * 20 if at_rows else f(n).abs() * 20, 'kl@': f(n).abs() * 9, 'iws@': f(n) * 30,
         'cross_y': f(C, n).abs(), 'y_true': torch.from_numpy(rng.integers(0, C, n))}
    if odin:
        t['odin-1-0.0040'] = torch.from_numpy(rng.random(n).astype(np.float32))
    if y_est:
        t['y_est_already'] = torch.from_numpy(rng.integers(0, C, n))
    return t


def name_of(v):
    return 'None' if v is None else str(v)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds tests/scod.py)')
    ap.add_argument('--timing', action='store_true')
    a = ap.parse_args()
    import matplotlib
    matplotlib.use('Agg')
    from sklearn.metrics import auc
    spec = importlib.util.spec_from_file_location('ref_scod', os.path.join(a.reference, 'tests', 'scod.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    os.makedirs(OUT, exist_ok=True)

    for name, case in curve_cases().items():
        data = dict(case)
        y_true, y_est = torch.from_numpy(case['y_true']), torch.from_numpy(case['y_est'])
        got = [figures(ref, auc, y_true, y_est, torch.from_numpy(row)) for row in case['scores']]
        for k, key in enumerate(('tpr', 'selective_risk', 'fpr')):
            data[key] = np.stack([g[0][k] for g in got])
        data['figures'] = np.asarray([g[1] for g in got], np.float64)
        data['trapz'] = np.asarray([g[2] for g in got], np.float64)
        np.savez_compressed(os.path.join(OUT, f'curve-{name}.npz'), **data)
        print(f'{name:22s}', ' '.join(f'{v:.6f}' for v in data['figures'][0]))

    rng = np.random.default_rng(37)
    for fname, mtype, rec, rs, gs in (
            ('wim', 'wim', wim_recorder(rng, 37), (None, 'zdist', 'dist', 'predist', 'logmsp', 'odin-1-0.0040', 'msp'),
             (None, 'elbo', 'iws', 'kl')),
            ('vib', 'vib', wim_recorder(rng, 41, y_est=False), (None, 'odin-1-0.0040', 'dist', 'logmsp'), (None, 'elbo', 'none'))):
        data = {'t|' + k: v.numpy() for k, v in rec.items()}
        if 'y_est_already' not in rec:                           # as the command-line block fills it (scod.py:219-221)
            rec = dict(rec, y_est_already=rec['cross_y'].argmin(0))
        for r in rs:
            for g in gs:
                for w in (0, 1, 0.3):
                    row = ref.scoring(rec, r=r, g=g, weight=w, mtype=mtype)
                    if torch.is_tensor(row):
                        data[f'row|{name_of(r)}|{name_of(g)}|{w}'] = row.numpy()
                    else:
                        data[f'row|{name_of(r)}|{name_of(g)}|{w}'] = np.float64(row)
        data['mtype'] = np.asarray(mtype)
        np.savez_compressed(os.path.join(OUT, f'rows-{fname}.npz'), **data)
        print(fname, len(data), 'entries')

    # end to end: the command-line block on three recorders of a wim job
    rng = np.random.default_rng(2024)
    sets = {'ind': wim_recorder(rng, 200, odin=False), 'ood-a': wim_recorder(rng, 64, odin=False),
            'ood-b': wim_recorder(rng, 137, odin=False, y_est=False)}
    for n_, t in sets.items():                                   # make the sets differ: OOD samples sit further out
        if n_ != 'ind':
            t['zdist'] = t['zdist'] + 6
        else:
            hit = torch.from_numpy(rng.random(200) < .8)
            t['y_est_already'] = torch.where(hit, t['y_true'], t['y_est_already'])
    data = {f't|{s}|{k}': v.numpy() for s, t in sets.items() for k, v in t.items()}
    data['sets'] = np.asarray(list(sets))
    rec = {s: dict(t) for s, t in sets.items()}
    for s in rec:
        if 'y_est_already' not in rec[s]:
            rec[s]['y_est_already'] = rec[s]['cross_y'].argmin(0)
    dset = 'ind'
    y_est = torch.hstack([rec[_]['y_est_already'] for _ in rec])
    y_true = torch.hstack([rec[_]['y_true'] * int(_ == dset) - int(_ != dset) for _ in rec])
    for r in (None, 'dist'):
        for g in (None, 'elbo', 'iws'):
            for w in (1., 0.3):
                scores = torch.hstack([ref.scoring(rec[_], r=r, g=g, weight=w, mtype='wim') for _ in rec])
                assert len(torch.unique(scores)) == len(scores), 'equal scores'
                _, fig, trapz = figures(ref, auc, y_true, y_est, scores)
                data[f'fig|{name_of(r)}|{name_of(g)}|{w}'] = np.asarray(fig, np.float64)
                data[f'trapz|{name_of(r)}|{name_of(g)}|{w}'] = np.asarray(trapz, np.float64)
                print('e2e', r, g, w, ' '.join(f'{v:.6f}' for v in fig))
    np.savez_compressed(os.path.join(OUT, 'e2e.npz'), **data)

    if a.timing:
        torch.set_num_threads(1)
        rng = np.random.default_rng(7)
        n_in, n_ood, M = 10000, 26032, 6
        y_true, y_est = labels(rng, n_in, n_ood)
        y_true, y_est = torch.from_numpy(y_true), torch.from_numpy(y_est)
        rows = [torch.from_numpy(distinct(rng, n_in + n_ood)) for _ in range(M)]
        ref.scrisk(y_true, y_est, rows[0])
        t0 = time.perf_counter()
        for s in rows:
            ref.scrisk(y_true, y_est, s)
        dt = time.perf_counter() - t0
        json.dump({'what': 'reference tests/scod.py::scrisk, 6 rows in sequence, one CPU core (torch.set_num_threads(1))',
                   'n_in': n_in, 'n_ood': n_ood, 'rows': M, 'seconds': dt, 'machine': platform.machine(),
                   'python': platform.python_version(), 'torch': torch.__version__},
                  open(os.path.join(OUT, 'timing.json'), 'w'), indent=1)
        print(f'reference scrisk, {M} rows of {n_in} + {n_ood}: {dt:.4f} s')


if __name__ == '__main__':
    main()
