#!/usr/bin/env python3
"""Time ops.knn (csrc/knn.hip: fp32 matrix-core distances fused with the per-row top-k) at the geometry of config 2 of
BASELINE.json - K = 64 latent dimensions, a bank of the M = 50 000 CIFAR training codes, N = 512 queries, k = 50, normalised - and
in the same process, interleaved call by call, the COMPOSED path on torch: row norms, torch.mm, the 2 - 2 cos epilogue on the
(N, M) matrix, torch.topk.  Also M in {5 000, 500 000} at the same N, and the share of an ood_detection_rates batch that the kNN
rows add on a config-2 model (the scoring pass of a batch with and without them).

    python tools/knn_bench.py [--calls 15] [--warmup 3] [--n 512] [--out profiles/knn_bench.json]

HIP events around every call on the launch stream; medians and min-max after the warm-up.  The fused call includes the query
norms (its three launches); the bank's norms are computed once, outside, for both paths.  Prints one JSON line."""
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


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def composed_knn(q, bank, bank_norm, k):
    """The same result from torch ops: an (N, M) matrix is written by mm, rewritten by the epilogue and read by topk."""
    qn = q.square().sum(1).sqrt().clamp_min(1e-12)
    cos = torch.mm(q, bank.t()) / (qn[:, None] * bank_norm[None, :])
    return (2 - 2 * cos).clamp_min_(0).topk(k, dim=1, largest=False)


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_max_ms': [float(np.min(ms)), float(np.max(ms))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    K = 64
    out = {'metric': 'knn_ms', 'N': a.n, 'K': K, 'k': a.k, 'normalized': True, 'calls': a.calls, 'warmup': a.warmup,
           'timing': 'HIP events around each call on the launch stream, fused and composed interleaved; medians, min-max',
           'composed': 'row norms + torch.mm + (2 - 2 cos).clamp_min(0) + torch.topk', 'banks': []}
    q = torch.randn(a.n, K, device=dev, generator=g)
    for M in (50000, 5000, 500000):
        bank, sq = ops.knn_bank(torch.randn(M, K, device=dev, generator=g))
        norm = sq.sqrt().clamp_min(1e-12)
        d2, idx = ops.knn(q, bank, sq, a.k)
        cd, ci = composed_knn(q, bank, norm, a.k)
        agree = float((idx.long() == ci).float().mean())
        ms = {'fused': [], 'composed': []}
        for i in range(a.warmup + a.calls):                     # interleaved: fused, composed, fused, ...
            for name, fn in (('fused', lambda: ops.knn(q, bank, sq, a.k)), ('composed', lambda: composed_knn(q, bank, norm, a.k))):
                t = event_ms(fn)
                if i >= a.warmup:
                    ms[name].append(t)
        lib_splits = ops.L.load().jvae_knn_workspace_bytes(a.n, M, K, a.k, 0) // (a.n * a.k * 8)
        out['banks'].append({'M': M, 'splits': int(lib_splits), 'fused': stats(ms['fused']), 'composed': stats(ms['composed']),
                             'fused_over_composed': float(np.median(ms['fused']) / np.median(ms['composed'])),
                             'max_abs_d2_difference': float((d2 - cd).abs().max()), 'indices_agreeing': agree,
                             'distance_matrix_MB': a.n * M * 4 / 1e6})
    ops.knn_check_status()

    # the share of a scoring batch: one batch of ood_detection_rates' pass on a config-2 model, with and without the kNN rows
    kw = full_config(2, a.n)['net']
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(dev).eval()
    x = torch.rand(a.n, *kw['input_shape'], device=dev, generator=g)
    bank, sq = ops.knn_bank(torch.randn(50000, kw['latent_dim'], device=dev, generator=g))
    net.latent_bank = {'bank': bank, 'sq': sq, 'labels': torch.zeros(50000, dtype=torch.int64, device=dev), 'set': 'synthetic'}

    def batch(with_knn):
        with torch.no_grad():
            if not with_knn:
                return net._evaluate_for_scores(x, 0, None)
            got = net._evaluate_for_scores(x, 0, None, with_mu=True)
            return got, net.knn_scores(got[4])
    ms = {False: [], True: []}
    for i in range(a.warmup + a.calls):
        for w in (False, True):
            t = event_ms(lambda: batch(w))
            if i >= a.warmup:
                ms[w].append(t)
    plain, with_knn = float(np.median(ms[False])), float(np.median(ms[True]))
    out['scoring_batch'] = {'model': 'cvae conv32/deconv32 K=64 C=10 batch_norm (BASELINE config 2)', 'M': 50000, 'KNN_K': list(net.KNN_K),
                            'without_knn': stats(ms[False]), 'with_knn': stats(ms[True]), 'knn_share_of_batch': (with_knn - plain) / with_knn}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
