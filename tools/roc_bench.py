#!/usr/bin/env python3
"""Time the device ROC (ops.roc_curve, csrc/roc.hip) on M = 11 score rows of (10 000, 26 032) - CIFAR-10 test set against SVHN
test set, the 11 OOD methods of a 'cvae' - and set it against the REFERENCE's roc_curve on the same shape, whose time was
taken on the CPU when the goldens were generated (tests/golden/roc/timing.json, tools/gen_roc_golden.py --timing).

    python tools/roc_bench.py [--calls 20] [--warmup 5] [--out profiles/roc_bench.json]

HIP events around every call on the launch stream; the median is reported.  Prints one JSON line."""
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
    modes = torch.tensor([m % 2 for m in range(a.rows)], dtype=torch.int32, device=dev)      # as in timing.json
    for _ in range(a.warmup):
        r = ops.roc_curve(ins, outs, kept, modes)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r = ops.roc_curve(ins, outs, kept, modes)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    assert int(r['status'].abs().sum()) == 0
    out = {'metric': 'device_roc_ms', 'rows': a.rows, 'n_in': a.n_in, 'n_out': a.n_out, 'calls': a.calls, 'warmup': a.warmup,
           'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)),
           'timing': 'HIP events around each call on the launch stream', 'auc_row0': float(r['auc'][0])}
    ref = os.path.join(REPO, 'tests', 'golden', 'roc', 'timing.json')
    if os.path.exists(ref) and (a.rows, a.n_in, a.n_out) == (11, 10000, 26032):
        t = json.load(open(ref))
        out['reference_cpu_ms'] = 1e3 * t['seconds']
        out['reference_over_device'] = out['reference_cpu_ms'] / out['ms_median']
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
