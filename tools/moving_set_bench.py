#!/usr/bin/env python3
"""Time the production of the moving batches of WIMJob.finetune(moving_size=...) in one process on one device: a mixture of four
resident 32x32x3 sets - NHWC uint8 (cifar-like), NCHW uint8 (svhn-like), 28x28 grey resized to 32x32 with g2c (mnist32r-like)
and the synthetic const32 - with equal shares, 8192 items, shuffled, last partial batch dropped, at batch sizes 64 and 512:

  dataloader     `DataLoader(moving_set)`: one launch and one label read-back per IMAGE through `DeviceImageSet.__getitem__`,
                 then the collate - the path the loop had before `mixed_loader`;
  mixed_loader   `torch_load.mixed_loader`: the index batch uploaded, one torch.rand for the synthetic leaf, ONE launch;
  single_set     `torch_load.device_loader` over the 8192 images of the NHWC leaf alone, the floor: the same kind of index
                 batches from a DataLoader over bare positions, their range check and upload, then `ops.imageset_batch`
                 alone - one launch, one layout, no table, no composition of indices;
  kernel         the mixed launch alone at N = 64 and 512, one x per thread against four consecutive x per thread (float4
                 store), and the single-set launch on the NHWC leaf beside them: device events around 200 launches each,
                 the three alternating, median per launch.

    python tools/moving_set_bench.py [--epochs 20] [--warmup 2] [--out profiles/moving_set_bench.json]

Wall clock around each epoch with the device synchronised on both sides; the median of the epochs, minimum and maximum beside
it.  Prints one JSON line and writes it to --out.  Without a GPU it says so and writes that instead of figures.  The only
requirement is that mixed_loader is not slower than the dataloader route at either size; finetune() as a whole is not timed."""
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

N_LEAF, N_ITEMS, BATCHES = 8192, 8192, (64, 512)


def timed(epoch, epochs, warmup):
    for _ in range(warmup):
        epoch()
    s = []
    for _ in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        epoch()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    med = float(np.median(s))
    return {'s_median': med, 's_min': float(np.min(s)), 's_max': float(np.max(s)), 'images_per_s': N_ITEMS / med}


def launches(calls, repeats=200, warmup=20):
    """Median device time per call of each of `calls` (name -> function), the calls alternating."""
    for _ in range(warmup):
        for f in calls.values():
            f()
    times = {k: [] for k in calls}
    for _ in range(repeats):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e-3)
    return {k: {'s_median': float(np.median(v)), 's_min': float(np.min(v)), 's_max': float(np.max(v))} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'moving_set_bench.json'))
    a = ap.parse_args()
    if a.epochs < 20:
        ap.error('--epochs: the median is taken over at least 20 epochs')
    rec = {'metric': 'moving_set_bench', 'items': N_ITEMS, 'leaves': ['nhwc 32x32x3', 'nchw 3x32x32', '28x28 resized to 32x32, g2c', 'const32'],
           'batch_sizes': list(BATCHES), 'epochs': a.epochs, 'warmup': a.warmup,
           'timing': 'synchronised wall clock around each epoch, median of the epochs; kernel: device events, median of 200 launches',
           'finetune_as_a_whole': 'not timed'}
    if not torch.cuda.is_available():
        rec['not_run'] = 'no GPU is visible: nothing was measured'
    else:
        from jvae_compat import torch_load as T
        from jvae_compat.ft_datasets import MixtureDataset
        from jvae_hip import ops
        dev = torch.device('cuda:0')
        g = torch.Generator().manual_seed(0)
        classes = [str(c) for c in range(10)]

        def leaf(name, shape, nhwc, source, **chain):
            data = torch.randint(0, 256, (N_LEAF, *shape), generator=g, dtype=torch.uint8)
            desc = ops.ImagesetDesc(source, nhwc, device=dev, **chain)
            return T.DeviceImageSet(name, data.to(dev), nhwc, torch.randint(0, 10, (N_LEAF,), generator=g).to(dev), None, desc,
                                    desc.shape, classes=classes)
        tables = (*T.pil_bilinear_tables(28, 32), *T.pil_bilinear_tables(28, 32))
        sets = {'nhwc': leaf('nhwc', (32, 32, 3), True, (32, 32, 3)), 'nchw': leaf('nchw', (3, 32, 32), False, (32, 32, 3)),
                'resized': leaf('resized', (1, 28, 28), False, (28, 28, 1), resize=(32, 32, *tables), g2c=True),
                'const32': T.get_dataset('const32', splits=['test'], device=dev)[1]}
        moving = MixtureDataset(mix=1, seed=1, task=0, length=N_ITEMS, **sets)
        alone = sets['nhwc']
        assert len(moving) == len(alone) == N_ITEMS
        props = torch.cuda.get_device_properties(0)
        rec.update(device=props.name, arch=getattr(props, 'gcnArchName', ''), torch=torch.__version__, hip=torch.version.hip)
        rec['batches'] = {}
        for bs in BATCHES:
            def loader_epoch():
                for x, tag in torch.utils.data.DataLoader(moving, batch_size=bs, shuffle=True, drop_last=True, num_workers=0):
                    pass
            fast, floor = T.mixed_loader(moving, bs, True, True), T.device_loader(alone, bs, True)

            def mixed_epoch():
                for x, tag in fast:
                    pass

            def floor_epoch():
                for x, y in floor:
                    pass
            r = {'dataloader': timed(loader_epoch, a.epochs, a.warmup), 'mixed_loader': timed(mixed_epoch, a.epochs, a.warmup),
                 'single_set': timed(floor_epoch, a.epochs, a.warmup)}
            r['dataloader_over_mixed_loader'] = r['dataloader']['s_median'] / r['mixed_loader']['s_median']
            r['mixed_loader_over_single_set'] = r['mixed_loader']['s_median'] / r['single_set']['s_median']
            rec['batches'][str(bs)] = r
        rec['mixed_loader_not_slower'] = all(r['dataloader_over_mixed_loader'] >= 1. for r in rec['batches'].values())
        table = ops.ImagesetMixTable(*moving.resolve(), dev)
        rec['kernel'] = {}
        for bs in BATCHES:
            pos = torch.randint(0, N_ITEMS, (bs,), generator=g).to(dev)
            idx = torch.randint(0, N_LEAF, (bs,), generator=g).to(dev)
            u = torch.rand((bs, 3), device=dev)
            one = sets['nhwc']
            rec['kernel'][str(bs)] = launches({
                'mixed_x1': lambda: ops.imageset_mixed_batch(table, pos, u, vec=1),
                'mixed_x4': lambda: ops.imageset_mixed_batch(table, pos, u, vec=4),
                'single_set': lambda: ops.imageset_batch(one.data, idx, one.desc, one.targets, None)})
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
