#!/usr/bin/env python3
"""Time the precision-recall figures (ops.pr_metrics, csrc/prc.hip) beside the device ROC (ops.roc_curve, csrc/roc.hip) on the
shape of tools/roc_bench.py: M = 11 score rows of (10 000, 26 032) - CIFAR-10 test set against SVHN test set, the 11 OOD methods
of a 'cvae'.  Two figures: `ops.roc_curve` alone, which is what an OOD set costs without `DETECTION_PR_METRICS`, and
`ops.roc_curve` followed by `ops.pr_metrics`, which is what it costs with the switch.

    python tools/pr_bench.py [--calls 20] [--warmup 5] [--out profiles/pr_bench.json]

HIP events around every call (or pair of calls) on the launch stream; the medians are reported.  Prints one JSON line."""
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


def timed(fn, calls, warmup):
    for _ in range(warmup):
        r = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return r, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rows', type=int, default=11)
    ap.add_argument('--n-in', type=int, default=10000)
    ap.add_argument('--n-out', type=int, default=26032)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from jvae_hip import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    ins = torch.randn(a.rows, a.n_in, device=dev, generator=g) + 1
    outs = torch.randn(a.rows, a.n_out, device=dev, generator=g)
    kept = torch.tensor([pc / 100 for pc in range(90, 100)], dtype=torch.float64, device=dev)
    modes = torch.tensor([m % 2 for m in range(a.rows)], dtype=torch.int32, device=dev)      # as tools/roc_bench.py
    r, ms_roc = timed(lambda: ops.roc_curve(ins, outs, kept, modes), a.calls, a.warmup)
    (r, p), ms_both = timed(lambda: (ops.roc_curve(ins, outs, kept, modes), ops.pr_metrics(ins, outs, modes)), a.calls, a.warmup)
    p, ms_pr = timed(lambda: ops.pr_metrics(ins, outs, modes), a.calls, a.warmup)
    assert int(r['status'].abs().sum()) == 0 and int(p['status'].abs().sum()) == 0
    out = {'metric': 'device_roc_and_pr_ms', 'rows': a.rows, 'n_in': a.n_in, 'n_out': a.n_out, 'calls': a.calls,
           'warmup': a.warmup, 'roc_curve_ms_median': float(np.median(ms_roc)),
           'roc_curve_then_pr_metrics_ms_median': float(np.median(ms_both)), 'pr_metrics_ms_median': float(np.median(ms_pr)),
           'roc_curve_ms_min_max': [float(np.min(ms_roc)), float(np.max(ms_roc))],
           'roc_curve_then_pr_metrics_ms_min_max': [float(np.min(ms_both)), float(np.max(ms_both))],
           'ratio': float(np.median(ms_both) / np.median(ms_roc)),
           'timing': 'HIP events around each call (pair of calls) on the launch stream',
           'auc_row0': float(r['auc'][0]), **{k + '_row0': float(p[k][0]) for k in ops.PR_FIGURES}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
