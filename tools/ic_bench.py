#!/usr/bin/env python3
"""Time ops.image_code_length (csrc/ic.hip: the length of a lossless image code, one launch per batch, one workgroup per image)
at the workload's batch, (512, 3, 32, 32), for three kinds of images - natural-like (smooth fields plus Gaussian noise of 4
levels), all-constant (every pixel of an image goes to ONE bin of each histogram: the contended case of the LDS atomics) and
uniform noise - and beside it
  - the share of an ood_detection_rates batch that the `ic-*` rows add on a config-2 model: `_evaluate_for_scores` alone against
    the same plus `ic_scores`;
  - the host alternative on the same batch: the read-back, then per image the shortest of the five PNG filter types (one type
    for the whole image, interleaved channels) under zlib level 9, on the host clock;
  - the mean over the images of device bits / PNG bits, per kind.

    python tools/ic_bench.py [--calls 30] [--warmup 5] [--reps 10] [--n 512] [--out profiles/ic_bench.json]

HIP events around `reps` back-to-back calls on the launch stream, reported per call; medians and min-max over `calls` windows
after the warm-up.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import zlib

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


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_max_ms': [float(np.min(ms)), float(np.max(ms))]}


def images(kind, N, C, H, W, rng):
    """(N, C, H, W) uint8."""
    if kind == 'constant':
        return np.broadcast_to(rng.integers(0, 256, (N, C, 1, 1)), (N, C, H, W)).astype(np.uint8)
    if kind == 'uniform':
        return rng.integers(0, 256, (N, C, H, W)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    f = rng.uniform(.5, 1.5, (2, N, 1, 1, 1))
    ph = rng.uniform(0, 1, (3, N, 1, 1, 1))
    base = 128 + 60 * np.sin(2 * np.pi * (xx / W * f[0] + ph[0])) * np.cos(2 * np.pi * (yy / H * f[1] + ph[1]))
    tint = 25 * np.sin(2 * np.pi * (xx + yy) / (H + W) + rng.uniform(0, 6, (N, C, 1, 1))) + rng.uniform(-20, 20, (N, C, 1, 1))
    return np.clip(np.rint(base + tint + 4. * rng.standard_normal((N, C, H, W))), 0, 255).astype(np.uint8)


def png_bits(img):
    """img (C, H, W) uint8 -> the bits of the shortest zlib-9 stream over the five PNG filter types, one type for all rows."""
    C, H, W = img.shape
    rows = np.ascontiguousarray(img.transpose(1, 2, 0)).reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(rows)
    a[:, C:] = rows[:, :-C]
    b = np.zeros_like(rows)
    b[1:] = rows[:-1]
    c = np.zeros_like(rows)
    c[1:, C:] = rows[:-1, :-C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    best = None
    for t, pred in enumerate((0, a, b, (a + b) >> 1, paeth)):
        body = np.concatenate([np.full((H, 1), t, np.uint8), ((rows - pred) & 255).astype(np.uint8)], 1).tobytes()
        size = len(zlib.compress(body, 9))
        best = size if best is None else min(best, size)
    return 8 * best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    rng = np.random.default_rng(0)
    C, H, W = 3, 32, 32
    out = {'metric': 'ic_ms', 'shape': [a.n, C, H, W], 'calls': a.calls, 'warmup': a.warmup, 'reps': a.reps,
           'timing': 'HIP events around `reps` back-to-back calls on the launch stream, per call; the kinds interleaved window by '
                     'window; medians, min-max over the windows',
           'host': 'read-back of the batch, x 255 to uint8, then per image the shortest zlib level-9 stream over the five PNG '
                   'filter types (one type per image, interleaved channels); host clock, 3 passes'}
    kinds = ('natural', 'constant', 'uniform')
    x = {k: torch.from_numpy(images(k, a.n, C, H, W, rng).astype(np.float32) / np.float32(255.)).to(dev) for k in kinds}
    bits = {k: ops.image_code_length(x[k])[0].cpu().numpy() for k in kinds}
    assert ops.ic_check_status() == 0
    ms = {k: [] for k in kinds}
    for i in range(a.warmup + a.calls):                         # interleaved: natural, constant, uniform, natural, ...
        for k in kinds:
            t = event_ms(lambda: ops.image_code_length(x[k]), a.reps)
            if i >= a.warmup:
                ms[k].append(t)
    out['device'] = {}
    for k in kinds:
        host_ms, png = [], None
        for _ in range(3):
            t0 = time.perf_counter()
            u8 = (x[k] * 255).round().to(torch.uint8).cpu().numpy()
            png = np.array([png_bits(img) for img in u8], dtype=np.float64)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        out['device'][k] = dict(stats(ms[k]), mean_bits_per_dim=float(bits[k].mean() / (C * H * W)),
                                host_png=stats(host_ms), mean_png_bits_per_dim=float(png.mean() / (C * H * W)),
                                mean_device_over_png_bits=float((bits[k] / png).mean()),
                                host_over_device_time=float(np.median(host_ms) / np.median(ms[k])))

    # the share of a scoring batch: one batch of ood_detection_rates' pass on a config-2 model, with and without the rows
    kw = full_config(2, a.n)['net']
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(dev).eval()
    xb = x['natural']

    def batch(with_ic):
        with torch.no_grad():
            got = net._evaluate_for_scores(xb, 0, None)
            return (got, net.ic_scores(got[0], got[2])) if with_ic else got
    ms = {False: [], True: []}
    for i in range(a.warmup + a.calls):
        for w in (False, True):
            t = event_ms(lambda: batch(w))
            if i >= a.warmup:
                ms[w].append(t)
    plain, with_ic = float(np.median(ms[False])), float(np.median(ms[True]))
    out['scoring_batch'] = {'model': 'cvae conv32/deconv32 K=64 C=10 batch_norm (BASELINE config 2)', 'images': 'natural',
                            'without_ic': stats(ms[False]), 'with_ic': stats(ms[True]), 'ic_share_of_batch': (with_ic - plain) / with_ic}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
