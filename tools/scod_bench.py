#!/usr/bin/env python3
"""Time the device SCOD curves (ops.scod_curve, csrc/scod.hip) on M = 6 score rows of 10 000 + 26 032 samples - CIFAR-10 test set
against SVHN test set, six score variants - and set it against the REFERENCE's scrisk on the same shape, whose time was taken on
one CPU core when the goldens were generated (tests/golden/scod/timing.json, tools/gen_scod_golden.py --timing), and against
ops.roc_curve at the same M and n (the same sort, on two 32-bit key rows instead of one 64-bit one).

    python tools/scod_bench.py [--calls 20] [--warmup 5] [--out profiles/scod_bench.json]

HIP events around every call on the launch stream; the median is reported.  Host synchronisations inside a call are counted
(Tensor.cpu / item / tolist / numpy).  Prints one JSON line."""
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
    ap.add_argument('--rows', type=int, default=6)
    ap.add_argument('--n-in', type=int, default=10000)
    ap.add_argument('--n-ood', type=int, default=26032)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from jvae_hip import ops
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    n = a.n_in + a.n_ood
    perm = torch.randperm(n, device=dev, generator=g)
    y_true = torch.cat((torch.randint(0, 10, (a.n_in,), device=dev, generator=g),
                        torch.full((a.n_ood,), -1, dtype=torch.int64, device=dev)))[perm]
    y_est = torch.where(torch.rand(n, device=dev, generator=g) < .8, y_true.clamp(min=0), torch.randint(0, 10, (n,), device=dev, generator=g))
    scores = torch.randn(a.rows, n, device=dev, generator=g) + (y_true < 0).float()
    kept = torch.tensor([pc / 100 for pc in range(90, 100)], dtype=torch.float64, device=dev)
    modes = torch.zeros(a.rows, dtype=torch.int32, device=dev)
    ins, outs = scores[:, y_true >= 0].contiguous(), scores[:, y_true < 0].contiguous()

    syncs = {'n': 0}
    for name in ('cpu', 'item', 'tolist', 'numpy'):
        real = getattr(torch.Tensor, name)

        def counted(self, *args, _real=real, **kw):
            syncs['n'] += 1
            return _real(self, *args, **kw)
        setattr(torch.Tensor, name, counted)
    r, ms = timed(lambda: ops.scod_curve(scores, y_true, y_est, n_in=a.n_in), a.calls, a.warmup)
    host_reads = syncs['n']
    _, ms_fig = timed(lambda: ops.scod_curve(scores, y_true, y_est, curves=False, n_in=a.n_in), a.calls, a.warmup)
    _, ms_roc = timed(lambda: ops.roc_curve(ins, outs, kept, modes), a.calls, a.warmup)
    assert int(r['status'].abs().sum()) == 0
    fig = r['figures'][0].tolist()
    out = {'metric': 'device_scod_ms', 'rows': a.rows, 'n_in': a.n_in, 'n_ood': a.n_ood, 'calls': a.calls, 'warmup': a.warmup,
           'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)),
           'figures_only_ms_median': float(np.median(ms_fig)), 'roc_curve_ms_median': float(np.median(ms_roc)),
           'scod_over_roc': float(np.median(ms) / np.median(ms_roc)), 'host_reads_inside_the_calls': host_reads,
           'timing': 'HIP events around each call on the launch stream', 'figures_row0': dict(zip(ops.SCOD_FIGURES, fig))}
    ref = os.path.join(REPO, 'tests', 'golden', 'scod', 'timing.json')
    if os.path.exists(ref) and (a.rows, a.n_in, a.n_ood) == (6, 10000, 26032):
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
