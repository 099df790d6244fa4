#!/usr/bin/env python3
"""Time cvae.odin_scores on the full 10 x 21 ODIN grid: a CIFAR-shaped vib (conv32, K = 64, C = 10, L = 16, BatchNorm), N = 100,
one GPU - and, in the same job, the work ODIN cannot avoid: 220 x N image-forwards of the same model through net.forward
(10 batches of N and 10 batches of 21 N rows, slabbed by nothing).  The REFERENCE's time for one such batch was taken on the CPU
when the goldens were generated (tests/golden/odin/timing.json, tools/gen_odin_golden.py --timing).

    python tools/odin_bench.py [--calls 20] [--warmup 3] [--forward-only] [--out profiles/odin_bench.json]

--forward-only skips odin_scores: with JVAE_HIP_LIB pointing at another build of the library (one without the ODIN kernels) it
times the plain forwards there.  HIP events around every call on the launch stream; medians.  Prints one JSON line."""
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
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--n', type=int, default=100)
    ap.add_argument('--forward-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    kw = dict(get_case('eb2_n8_vib_L2')['net'], classifier=[], test_latent_sampling=16)
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(dev).eval()
    T, E = len(getattr(Net, 'ODIN_TEMPS', range(10))), len(getattr(Net, 'ODIN_EPS', range(21)))      # an older tree: the grid's size
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(a.n, *kw['input_shape'], device=dev, generator=g)
    xe = x.repeat(E, 1, 1, 1)

    def forwards():
        with torch.no_grad():
            for _ in range(T):
                net.forward(x, z_output=False)
                net.forward(xe, z_output=False)
    out = {'metric': 'odin_scores_ms', 'model': 'vib conv32 K=64 C=10 L=16 batch_norm', 'N': a.n, 'grid': [T, E],
           'calls': a.calls, 'warmup': a.warmup, 'timing': 'HIP events around each call on the launch stream',
           'lib': os.environ.get('JVAE_HIP_LIB', 'in-tree')}
    fw = timed(forwards, a.calls, a.warmup)
    out.update(forwards_ms_median=float(np.median(fw)), forwards_ms_min=float(np.min(fw)), image_forwards=(T + T * E) * a.n)
    if not a.forward_only:
        ms = timed(lambda: net.odin_scores(x), a.calls, a.warmup)
        out.update(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)),
                   odin_over_forwards=float(np.median(ms) / np.median(fw)))
        ref = os.path.join(REPO, 'tests', 'golden', 'odin', 'timing.json')
        if os.path.exists(ref) and a.n == 100:
            out['reference_cpu_ms'] = 1e3 * json.load(open(ref))['seconds']
            out['reference_over_device'] = out['reference_cpu_ms'] / out['ms_median']
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
