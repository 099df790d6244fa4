#!/usr/bin/env python3
"""Time what module/cascad.py adds, against the torch expressions of the reference written out, on the same device:

  cascade_mse  `ops.cascade_mse(x, stages)` - every stage-pair row in one pass - against the reference's loop, pair by pair
               (x_i - x_j).pow(2).mean over draws and image, stacked.  Shapes M = 3, L = 16, N = 100, D = 3072 and M = 2,
               L = 128, N = 32, D = 3072; the stages are the [1:] views of (L + 1, N, 3, 32, 32) tensors, as in evaluate().
               Also the peak memory each side adds, the bytes the kernel has to read and the rate that makes of its time.
  evaluate     one `CascadModels.evaluate(x, z_output=True, temps=[1, 5])` of three config-2 models (N = 100, L = 16) beside the
               sum of the three models' own `evaluate(x, z_output=True)` calls on the same stage inputs: the difference is what
               the cascade adds (class posteriors, mutual information, the MSE rows, the stacks).

    python tools/cascad_bench.py [--calls 20] [--warmup 5] [--out profiles/cascad_bench.json]

HIP events around each call on the current stream, after a warm-up; the median of the calls, minimum and maximum beside it.
Prints one JSON line.  No ratio is promised: the figures are whatever was measured."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd'), os.path.join(REPO, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

from aggregation_bench import peak_rise, timed  # noqa: E402


def mse_case(M, L, N, calls, warmup, dev):
    from jvae_hip import ops
    shape = (3, 32, 32)
    D = 3 * 32 * 32
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((N,) + shape, device=dev, generator=g)
    full, prev = [], x.unsqueeze(0).expand(L + 1, N, *shape)
    for i in range(M):
        prev = prev + (.05 + .03 * i) * torch.randn((L + 1, N) + shape, device=dev, generator=g)
        full.append(prev)
    stages = [f[1:] for f in full]
    dims = (0, 2, 3, 4)

    def by_torch():
        rows = []
        for i in range(1, M + 1):
            for j in range(i):
                rows.append((stages[i - 1] - (stages[j - 1] if j else x.unsqueeze(0))).pow(2).mean(dims))
        return torch.stack(rows)

    def kernel():
        return ops.cascade_mse(x, stages)
    out = {'shape': dict(M=M, L=L, N=N, D=D)}
    out['cascade_mse'], out['torch_ops'] = timed(kernel, calls, warmup), timed(by_torch, calls, warmup)
    out['torch_over_kernel'] = out['torch_ops']['ms_median'] / out['cascade_mse']['ms_median']
    read = (M * L + 1) * N * D * 4
    out['bytes_read_by_the_kernel'] = read
    out['kernel_read_rate_GB_per_s'] = read / out['cascade_mse']['ms_median'] / 1e6
    out['peak_bytes'] = {'cascade_mse': peak_rise(kernel), 'torch_ops': peak_rise(by_torch), 'one_stage': L * N * D * 4}
    a, b = kernel(), by_torch()
    out['max_relative_difference'] = float((a - b).abs().max() / b.abs().max())
    return out


def evaluate_case(M, N, L, calls, warmup, dev):
    from cvae import ClassificationVariationalNetwork as Net
    from module.cascad import CascadModels
    from oracle.cases import full_config
    from oracle.det_init import det_inputs, load_det_state
    kw = dict(full_config(2, N)['net'], test_latent_sampling=L)
    nets = []
    for s in range(M):
        torch.manual_seed(0)
        net = Net(**kw)
        load_det_state(net, seed=s)
        nets.append(net.to(dev).eval())
    model = CascadModels(*nets)
    x = det_inputs(N, kw['input_shape'], kw['num_labels'], 1, kw['latent_dim'], seed=3)[0].to(dev)
    temps = [1, 5]
    inputs = [x]
    with torch.no_grad():
        for net in nets[:-1]:
            inputs.append(net.evaluate(inputs[-1])[0][1].clone())

    def cascade():
        with torch.no_grad():
            return model.evaluate(x, z_output=True, temps=temps)

    def alone(i):
        def call():
            with torch.no_grad():
                return nets[i].evaluate(inputs[i], z_output=True)
        return call
    out = {'shape': dict(M=M, N=N, L=nets[0].latent_sampling, C=kw['num_labels'], K=kw['latent_dim'], temps=temps)}
    out['cascade_evaluate'] = timed(cascade, calls, warmup)
    out['model_evaluate'] = [timed(alone(i), calls, warmup) for i in range(M)]
    total = sum(m['ms_median'] for m in out['model_evaluate'])
    out['sum_of_model_evaluates_ms'] = total
    out['added_by_the_cascade_ms'] = out['cascade_evaluate']['ms_median'] - total
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cascad_bench needs the GPU: nothing is measured without one')
    dev = 'cuda:0'
    out = {'metric': 'cascad_bench', 'device': torch.cuda.get_device_name(0),
           'arch': getattr(torch.cuda.get_device_properties(0), 'gcnArchName', ''), 'torch': torch.__version__, 'hip': torch.version.hip,
           'calls': a.calls, 'warmup': a.warmup, 'timing': 'HIP events around each call, median of the calls',
           'cascade_mse': [mse_case(3, 16, 100, a.calls, a.warmup, dev), mse_case(2, 128, 32, a.calls, a.warmup, dev)],
           'evaluate': evaluate_case(3, 100, 16, a.calls, a.warmup, dev)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
