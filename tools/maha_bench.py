#!/usr/bin/env python3
"""Time ops.maha_scores (csrc/maha.hip: whitening on the fp32 matrix cores fused with the class distances, one launch) at the
geometry of config 2 of BASELINE.json - K = 64 latent dimensions, C = 10 classes, N = 512 queries - and in the same process,
interleaved call by call, the COMPOSED path on torch: the subtraction of the mean, ONE torch.mm with the stacked (2K, K) matrix,
torch.cdist to the whitened class means, min (five or so launches, the (N, 2K) and (N, C) intermediates in memory).  Also
ops.maha_moments over a bank of M = 50 000 rows (the fit's device part; the two K x K factorisations are numpy's and are timed
on the host clock beside it), and the share of an ood_detection_rates batch that the Mahalanobis rows add on a config-2 model
(the scoring pass of a batch with and without them).

    python tools/maha_bench.py [--calls 30] [--warmup 5] [--reps 20] [--n 512] [--out profiles/maha_bench.json]

HIP events around `reps` back-to-back calls on the launch stream (one call is tens of microseconds: a window of one would measure
the events), reported per call; medians and min-max over `calls` windows after the warm-up.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def event_ms(fn, reps=1):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def composed_maha(q, fit):
    """The same result from torch ops: the whitened rows (N, 2K) and the distances (N, C) are written to memory on the way."""
    K = q.shape[1]
    y = torch.mm(q - fit['mu0_32'], fit['W32'].t())
    dc = torch.cdist(y[:, :K], fit['m32']).square()
    d, cls = dc.min(1)
    return d, cls, d - (y[:, K:] - fit['m0_32']).square().sum(1)


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_max_ms': [float(np.min(ms)), float(np.max(ms))]}


def synthetic_bank(M, K, C, g, dev):
    labels = torch.randint(0, C, (M,), device=dev, generator=g)
    centres = 3 * torch.randn(C, K, device=dev, generator=g)
    return centres[labels] + torch.randn(M, K, device=dev, generator=g), labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    K, C, M = 64, 10, 50000
    out = {'metric': 'maha_ms', 'N': a.n, 'K': K, 'C': C, 'M': M, 'calls': a.calls, 'warmup': a.warmup, 'reps': a.reps,
           'timing': 'HIP events around `reps` back-to-back calls on the launch stream, per call; fused and composed windows '
                     'interleaved; medians, min-max over the windows',
           'composed': 'q - mu0, torch.mm with the stacked (2K, K) matrix, torch.cdist to the class means, square, min, d0, rel'}
    bank, labels = synthetic_bank(M, K, C, g, dev)
    q = torch.cat([bank[:a.n // 2], bank[:a.n - a.n // 2] + 2 * torch.randn(a.n - a.n // 2, K, device=dev, generator=g)])

    moments = ops.maha_moments(bank, labels, C)
    t0 = time.perf_counter()
    fit = ops.maha_fit(moments)                                  # one read-back, two Cholesky factorisations and inverses in numpy
    out['fit_host_ms'] = (time.perf_counter() - t0) * 1e3
    ms = [event_ms(lambda: ops.maha_moments(bank, labels, C)) for _ in range(a.warmup + a.calls)][a.warmup:]
    out['moments'] = dict(stats(ms), launches=9, note='one call per window')

    d, cls, rel = ops.maha_scores(q, fit)
    cd, ccls, crel = composed_maha(q, fit)
    ms = {'fused': [], 'composed': []}
    for i in range(a.warmup + a.calls):                         # interleaved: fused, composed, fused, ...
        for name, fn in (('fused', lambda: ops.maha_scores(q, fit)), ('composed', lambda: composed_maha(q, fit))):
            t = event_ms(fn, a.reps)
            if i >= a.warmup:
                ms[name].append(t)
    out['scores'] = {'fused': stats(ms['fused']), 'composed': stats(ms['composed']),
                     'fused_over_composed': float(np.median(ms['fused']) / np.median(ms['composed'])),
                     'max_rel_d_difference': float(((d - cd).abs() / cd).max()), 'max_abs_rel_difference': float((rel - crel).abs().max()),
                     'classes_agreeing': float((cls.long() == ccls).float().mean())}
    ops.maha_check_status()

    # the share of a scoring batch: one batch of ood_detection_rates' pass on a config-2 model, with and without the rows
    kw = full_config(2, a.n)['net']
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(dev).eval()
    x = torch.rand(a.n, *kw['input_shape'], device=dev, generator=g)
    net.latent_gaussians = dict(fit, set='synthetic')

    def batch(with_maha):
        with torch.no_grad():
            if not with_maha:
                return net._evaluate_for_scores(x, 0, None)
            got = net._evaluate_for_scores(x, 0, None, with_mu=True)
            return got, net.maha_scores(got[4])
    ms = {False: [], True: []}
    for i in range(a.warmup + a.calls):
        for w in (False, True):
            t = event_ms(lambda: batch(w))
            if i >= a.warmup:
                ms[w].append(t)
    plain, with_maha = float(np.median(ms[False])), float(np.median(ms[True]))
    out['scoring_batch'] = {'model': 'cvae conv32/deconv32 K=64 C=10 batch_norm (BASELINE config 2)', 'without_maha': stats(ms[False]),
                            'with_maha': stats(ms[True]), 'maha_share_of_batch': (with_maha - plain) / with_maha}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
