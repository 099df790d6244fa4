#!/usr/bin/env python3
"""GPU box: time image generation - net.generate() and the two kernels of csrc/sample.hip alone - next to the torch expressions
they replace, on config 2 (conv32 / deconv32, 3 x 32 x 32, K = 64, C = 10).  HIP events, 5 warm-up calls, median of 20.

    python tools/sample_bench.py [--out profiles/sample_bench.json]

Shapes: N = 10 classes with L = 10 draws (the defaults of the reference's command line) and with L = 1000 (a large draw).
  draws    ops.prior_sample (unit mode)           vs  eps + mean.index_select(0, y).view(1, N, K)
  grid     ops.image_grid, prior layout: L draw columns, fp32 + 8-bit grids
           vs  permute / reshape copy of the rows into the grid, then mul, add, clamp, permute and the cast to uint8
  grid_x   ops.image_grid, x layout: input, mean reconstruction, average over the L draws, L draws (Ncol = L + 3)
           vs  cat of [x, x_[0], x_[1:].mean(0), x_[1:]] into the grid, then the same five operations
  generate net.generate(L=L) end to end (draws + decoder in slabs)
One JSON line; times in microseconds.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

WARMUP, CALLS = 5, 20


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return {'median_us': round(statistics.median(times), 1), 'min_us': round(min(times), 1), 'max_us': round(max(times), 1)}


def to_u8(grid):
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import load_det_state
    dev = torch.device('cuda:0')
    kw = full_config(2, 8)['net']
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(dev).eval()
    N, K = kw['num_labels'], kw['latent_dim']
    D, H, W = kw['input_shape']
    mean = net.encoder.prior.mean.detach()
    result = {'device': torch.cuda.get_device_name(0), 'model': 'config 2', 'warmup': WARMUP, 'calls': CALLS, 'shapes': {}}
    torch.manual_seed(0)
    with torch.no_grad():
        for L in (10, 1000):
            eps = torch.randn(L, N, K, device=dev)
            y = torch.arange(N, device=dev)
            labels = y.unsqueeze(0).expand(L, N).reshape(-1).contiguous()
            r = {}
            r['draws_kernel'] = timed(lambda: ops.prior_sample(eps, labels, mean, None, mode='unit'))
            r['draws_torch'] = timed(lambda: eps + mean.index_select(0, y).view(1, N, K))
            assert torch.equal(ops.prior_sample(eps, labels, mean, None, mode='unit'), eps + mean.index_select(0, y).view(1, N, K))
            r['generate'] = timed(lambda: net.generate(L=L, epsilon=eps))
            x_ = net.generate(L=L, epsilon=eps)
            cols = ops.grid_columns([('draw', l) for l in range(L)], dev)
            r['grid_kernel'] = timed(lambda: ops.image_grid(None, x_, cols))

            def torch_grid():
                g = x_.permute(2, 1, 3, 0, 4).reshape(D, N * H, L * W)
                return g, to_u8(g)
            r['grid_torch'] = timed(torch_grid)
            gf, gu = ops.image_grid(None, x_, cols)
            tg, tu = torch_grid()
            assert torch.equal(gf, tg) and torch.equal(gu, tu)
            x = torch.rand(N, D, H, W, device=dev)
            rows = torch.cat([x_[:1], x_])                                   # (L + 1, N, ...): row 0 plays the mean reconstruction
            cols_x = ops.grid_columns([('input',), ('draw', 0), ('average', 1, L)] + [('draw', 1 + l) for l in range(L)], dev)
            r['grid_x_kernel'] = timed(lambda: ops.image_grid(x, rows, cols_x))

            def torch_grid_x():
                cells = torch.cat([x.unsqueeze(0), rows[:1], rows[1:].mean(0, keepdim=True), rows[1:]])
                g = cells.permute(2, 1, 3, 0, 4).reshape(D, N * H, (L + 3) * W)
                return g, to_u8(g)
            r['grid_x_torch'] = timed(torch_grid_x)
            gfx, gux = ops.image_grid(x, rows, cols_x)
            tgx, tux = torch_grid_x()
            keep = torch.ones((L + 3) * W, dtype=torch.bool, device=dev)
            keep[2 * W:3 * W] = False                                        # the average column: another order of summation
            assert torch.equal(gfx[:, :, keep], tgx[:, :, keep]) and float((gfx - tgx).abs().max()) < 1e-5
            r['grid_bytes'] = {'prior': int(x_.numel() * 4 + gf.numel() * 4 + gu.numel()),
                               'x': int((x.numel() + rows.numel() + L * rows[0].numel()) * 4 + gfx.numel() * 4 + gux.numel())}
            result['shapes'][f'N{N}_L{L}'] = r
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
