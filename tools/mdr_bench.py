#!/usr/bin/env python3
"""Time misclassification_detection_rates on the device for the default cvae table - 2 prediction methods x 35 methods = 70 rows -
over a recorder of N = 10 000 samples, and print it beside the REFERENCE's time for the same shape, taken on the CPU when the
goldens were generated (tests/golden/mdr/timing.json, tools/gen_mdr_golden.py --timing; that figure includes reading the record
file, this one starts from a recorder on the device).

    python tools/mdr_bench.py [--calls 20] [--warmup 5] [--out profiles/mdr_bench.json]

The call ends with a copy to the host, so it is timed as a whole with the host clock between two device synchronisations; the
median is reported.  Prints one JSON line."""
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


def synth_recorder(C, N, dev, batch=100):
    """All-class losses shaped like a cvae's: the true class is mostly the closest / the most likely one."""
    from jvae_compat.recorders import LossRecorder
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.randint(0, C, (N,), device=dev, generator=g)
    onehot = torch.nn.functional.one_hot(y, C).T.bool()
    hit = torch.rand(2, N, device=dev, generator=g) < .85
    zdist = 6 + 8 * torch.rand(C, N, device=dev, generator=g)
    zdist = torch.where(onehot & hit[0], zdist - 6, zdist)
    kl = .5 * zdist + torch.rand(C, N, device=dev, generator=g)
    total = kl + 40 + 20 * torch.rand(N, device=dev, generator=g)
    iws = -total + torch.randn(C, N, device=dev, generator=g)
    iws = torch.where(onehot & hit[1], iws + 5, iws)
    logits = 2 * torch.randn(C, N, device=dev, generator=g)
    rec = LossRecorder(batch)
    for i in range(0, N, batch):
        rec.append_batch(total=total[:, i:i + batch], kl=kl[:, i:i + batch], zdist=zdist[:, i:i + batch], iws=iws[:, i:i + batch],
                         logits=logits[:, i:i + batch], y_true=y[i:i + batch])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    dev = 'cuda:0'
    net = Net(input_shape=(1, 28, 28), num_labels=10, type='cvae', encoder=[32], decoder=[32], classifier=[], latent_dim=8,
              latent_sampling=1, gamma=0.)
    net.to(dev)
    rec = synth_recorder(10, a.n, dev)

    def call():
        return net.misclassification_detection_rates(recorder=rec, epoch=1, update_self_results=False)
    for _ in range(a.warmup):
        res = call()
    ms = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    rows = sum(len(v) for v in res.values())
    out = {'metric': 'device_mdr_ms', 'rows': rows, 'n': a.n, 'calls': a.calls, 'warmup': a.warmup,
           'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)),
           'timing': 'host clock around each whole call, device synchronised before and after',
           'auc_first_row': float(next(iter(next(iter(res.values())).values()))['auc'])}
    ref = os.path.join(REPO, 'tests', 'golden', 'mdr', 'timing.json')
    if os.path.exists(ref):
        t = json.load(open(ref))
        if (t['rows'], t['n']) == (rows, a.n):
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
