#!/usr/bin/env python3
"""Time the device ROC (ops.roc_curve, csrc/roc.hip) with strided-quantile rows: M = 11 score rows of (10 000, 26 032) - CIFAR-10
test set against SVHN test set - in the modes of the 11 OOD methods of a 'cvae' with OOD_QUANTILE_METHODS (4 quantile rows:
a-1-1, a-4-1 twice each), against the same 11 rows with the quantile rows made one-sided, and against 11 rows all in one mode
(what one row of each mode costs).

    python tools/rocq_bench.py [--calls 30] [--warmup 5] [--rounds 2] [--parent-lib <libjvae_hip.so of the parent commit>]
                               [--out profiles/rocq_bench.json]

Every library runs in a fresh child process (JVAE_HIP_LIB selects it), the rounds alternate between the libraries, and inside
a process the timed calls go round-robin over the variants, so that drift of the machine hits all of them alike.  HIP events
around every call on the launch stream; median, minimum, maximum and the inter-quartile range are reported.  With --parent-lib
the variant without quantile rows is also timed on the build of the parent commit, which has no quantile mode.  The reference's
CPU time for the 4 quantile rows (tests/golden/rocq/timing.json, tools/gen_rocq_golden.py --timing) is quoted beside.
Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

Q11, Q41, AM = 2 | 1 << 8 | 1 << 16, 2 | 4 << 8 | 1 << 16, 1
TABLE = [AM, Q11, Q41, 0, 0, 0, 0, AM, Q11, Q41, 0]          # iws-2s iws-a-1-1 iws-a-4-1 iws mse elbo soft elbo-2s elbo-a-1-1 elbo-a-4-1 zdist
VARIANTS = {'table_4_quantile_rows': TABLE, 'table_quantile_rows_one_sided': [w if w < 2 else 0 for w in TABLE],
            'all_one_sided': [0] * 11, 'all_around_mean': [AM] * 11, 'all_quantile_1_1': [Q11] * 11, 'all_quantile_4_1': [Q41] * 11}
N_IN, N_OUT = 10000, 26032


def worker(names, calls, warmup):
    import torch
    from jvae_hip import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    ins = torch.randn(11, N_IN, device=dev, generator=g) + 1
    outs = torch.randn(11, N_OUT, device=dev, generator=g)
    kept = torch.tensor([pc / 100 for pc in range(90, 100)], dtype=torch.float64, device=dev)
    modes = {n: torch.tensor(VARIANTS[n], dtype=torch.int32, device=dev) for n in names}
    ms, auc = {n: [] for n in names}, {}
    for i in range(warmup + calls):
        for n in names:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = ops.roc_curve(ins, outs, kept, modes[n])
            t1.record()
            t1.synchronize()
            if i >= warmup:
                ms[n].append(t0.elapsed_time(t1))
            assert int(r['status'].abs().sum()) == 0
            auc[n] = r['auc'].tolist()
    print(json.dumps({'ms': ms, 'auc': auc}))


def stats(ms):
    q1, q3 = np.percentile(ms, [25, 75])
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)), 'ms_iqr': float(q3 - q1),
            'calls': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--worker', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker.split(','), a.calls, a.warmup)
    runs = [('this', None, list(VARIANTS))]
    if a.parent_lib:
        runs.append(('parent', os.path.abspath(a.parent_lib), ['table_quantile_rows_one_sided']))
    ms, auc = {}, {}
    for _ in range(a.rounds):
        for label, lib, names in runs:
            env = dict(os.environ)
            if lib:
                env['JVAE_HIP_LIB'] = lib
            else:
                env.pop('JVAE_HIP_LIB', None)
            done = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', ','.join(names), '--calls', str(a.calls),
                                   '--warmup', str(a.warmup)], env=env, capture_output=True, text=True, timeout=400)
            if done.returncode:
                sys.exit(f'{label}: worker ended with {done.returncode}\n{done.stderr[-2000:]}')
            got = json.loads(done.stdout.strip().splitlines()[-1])
            for n in names:
                ms.setdefault((label, n), []).extend(got['ms'][n])
                auc[(label, n)] = got['auc'][n]
    out = {'metric': 'device_roc_ms', 'rows': 11, 'n_in': N_IN, 'n_out': N_OUT, 'warmup': a.warmup, 'rounds': a.rounds,
           'timing': 'HIP events around each call on the launch stream; round-robin over the variants, fresh process per library and round',
           'variants': {f'{label}:{n}': stats(v) for (label, n), v in ms.items()}}
    med = {k: v['ms_median'] for k, v in out['variants'].items()}
    out['ms_per_row'] = {k.split(':')[1][4:]: med[k] / 11 for k in med if k.startswith('this:all_')}
    out['quantile_row_over_around_mean_row'] = {p: out['ms_per_row'][f'quantile_{p}'] / out['ms_per_row']['around_mean']
                                                for p in ('1_1', '4_1')}
    if a.parent_lib:
        assert auc[('parent', 'table_quantile_rows_one_sided')] == auc[('this', 'table_quantile_rows_one_sided')]
        out['this_over_parent_without_quantile_rows'] = med['this:table_quantile_rows_one_sided'] / med['parent:table_quantile_rows_one_sided']
    ref = os.path.join(REPO, 'tests', 'golden', 'rocq', 'timing.json')
    if os.path.exists(ref):
        out['reference_cpu_ms_4_quantile_rows'] = 1e3 * json.load(open(ref))['seconds']
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
