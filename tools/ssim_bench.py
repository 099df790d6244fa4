#!/usr/bin/env python3
"""Time ops.ssim (csrc/ssim.hip: the structural similarity of every image of a batch to each of its reconstructions, one launch)
at three shapes (N, R, C, H, W) - the scoring batch (100, 17, 3, 32, 32), a large one (512, 129, 3, 32, 32) and config 5's image
(256, 17, 3, 64, 64) - and beside it
  - a torch expression of the same SSIM on the same inputs: grouped conv2d for the five filtered quantities of the (R N) images,
    then the elementwise chain; interleaved with the kernel calls, call by call;
  - the bytes per second the kernel achieves, 4 N C H W (1 + R) bytes per call (every input read once), against the float4 copy
    rate measured on this chip, 6.29 TB/s;
  - the share of an ood_detection_rates batch that the `ssim*` rows add on a config-2 model at N = 512: `_evaluate_for_scores`
    alone against the same with `with_reco` plus `ssim_scores`.

    python tools/ssim_bench.py [--calls 20] [--warmup 3] [--out profiles/ssim_bench.json]

HIP events around ONE call on the launch stream; medians and min-max over `calls` calls after the warm-up.  Prints one JSON
line."""
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

COPY_RATE = 6.29e12                                             # bytes / s, float4 copy


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_max_ms': [float(np.min(ms)), float(np.max(ms))]}


def torch_ssim(x, y, chunk=64):
    """The same SSIM by torch: x (N, C, H, W), y (R, N, C, H, W) -> (ssim (R, N), cs (R, N)); `chunk` draws at a time, so that the
    five filtered stacks fit beside the inputs."""
    k = torch.arange(11, dtype=torch.float64, device=x.device) - 5
    g = torch.exp(-k * k / 4.5)
    g = (g / g.sum()).float()
    C = x.shape[1]
    wr, wc = g.view(1, 1, 1, 11).repeat(C, 1, 1, 1), g.view(1, 1, 11, 1).repeat(C, 1, 1, 1)

    def f(t):
        return torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, wr, groups=C), wc, groups=C)
    out_s, out_c = [], []
    for r0 in range(0, y.shape[0], chunk):
        yc = y[r0:r0 + chunk]
        R = yc.shape[0]
        xe = x.unsqueeze(0).expand_as(yc).reshape(-1, *x.shape[1:])
        yf = yc.reshape(-1, *x.shape[1:])
        mx, my = f(xe), f(yf)
        vx, vy, cxy = f(xe * xe) - mx * mx, f(yf * yf) - my * my, f(xe * yf) - mx * my
        cs = (2 * cxy + 9e-4) / (vx + vy + 9e-4)
        s = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4) * cs
        out_s.append(s.mean((1, 2, 3)).view(R, -1))
        out_c.append(cs.mean((1, 2, 3)).view(R, -1))
    return torch.cat(out_s), torch.cat(out_c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    out = {'metric': 'ssim_ms', 'calls': a.calls, 'warmup': a.warmup, 'copy_rate_bytes_per_s': COPY_RATE,
           'timing': 'HIP events around one call on the launch stream; the kernel and the torch expression interleaved call by '
                     'call; medians, min-max over the calls', 'shapes': []}
    for N, R, C, H, W in ((100, 17, 3, 32, 32), (512, 129, 3, 32, 32), (256, 17, 3, 64, 64)):
        x = torch.rand((N, C, H, W), generator=g).to(dev)
        y = (x.unsqueeze(0) + 0.1 * torch.randn((R, N, C, H, W), generator=g).to(dev)).contiguous()
        s, cs = ops.ssim(x, y)
        ts, tcs = torch_ssim(x, y)
        ms = {'kernel': [], 'torch': []}
        for i in range(a.warmup + a.calls):
            for name, fn in (('kernel', lambda: ops.ssim(x, y)), ('torch', lambda: torch_ssim(x, y))):
                t = event_ms(fn)
                if i >= a.warmup:
                    ms[name].append(t)
        nbytes = 4 * N * C * H * W * (1 + R)
        k, t = float(np.median(ms['kernel'])), float(np.median(ms['torch']))
        out['shapes'].append({'shape': [N, R, C, H, W], 'strip_rows': ops.ssim_strip_rows(H, W), 'kernel': stats(ms['kernel']),
                              'torch': stats(ms['torch']), 'torch_over_kernel': t / k, 'bytes': nbytes,
                              'kernel_bytes_per_s': nbytes / (k * 1e-3), 'share_of_copy_rate': nbytes / (k * 1e-3) / COPY_RATE,
                              'largest_difference_to_torch': {'ssim': float((s - ts).abs().max()), 'cs': float((cs - tcs).abs().max())}})
        del x, y
    assert ops.ssim_check_status() == 0

    # the share of a scoring batch: one batch of ood_detection_rates' pass on a config-2 model, with and without the rows
    n = 512
    net = Net(**full_config(2, n)['net'])
    load_det_state(net, seed=0)
    net.to(dev).eval()
    xb = torch.rand((n, 3, 32, 32), generator=g).to(dev)

    def batch(with_ssim):
        with torch.no_grad():
            got = net._evaluate_for_scores(xb, 0, None, with_reco=with_ssim)
            return (got, net.ssim_scores(got[0], got[-1])) if with_ssim else got
    ms = {False: [], True: []}
    for i in range(a.warmup + a.calls):
        for w in (False, True):
            t = event_ms(lambda: batch(w))
            if i >= a.warmup:
                ms[w].append(t)
    plain, with_ssim = float(np.median(ms[False])), float(np.median(ms[True]))
    out['scoring_batch'] = {'model': 'cvae conv32/deconv32 K=64 C=10 batch_norm (BASELINE config 2)', 'N': n,
                            'draws': int(batch(True)[0][-1].shape[0]), 'without_ssim': stats(ms[False]),
                            'with_ssim': stats(ms[True]), 'ssim_share_of_batch': (with_ssim - plain) / with_ssim}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
