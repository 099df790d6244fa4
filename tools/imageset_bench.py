#!/usr/bin/env python3
"""Time the device-resident image sets (jvae_compat/torch_load.py, csrc/imageset.hip) against the path the loops had before
them, in one process on one device, over the same 10 000 synthetic 32x32x3 uint8 images at batch_size 100:

  batches    one epoch of shuffled batch production alone, float32 (100, 3, 32, 32) and labels ready on the device:
             `DataLoader(num_workers=0)` over a plain map-style data set of the raw images (a Python __getitem__ per sample, the
             host collate, a copy per batch, then ops.augment_batch) against `device_loader` (the index batch uploaded, one
             launch);
  accuracy   `accuracy()` of the flagship conv model over the same set, end to end, through either path.

    python tools/imageset_bench.py [--epochs 20] [--warmup 2] [--out profiles/imageset_bench.json]

Wall clock around each epoch with the device synchronised on both sides; the median of the epochs, minimum and maximum beside
it.  Prints one JSON line and writes it to --out.  Without a GPU it says so and writes that instead of figures.  No ratio is
promised: the figures are whatever was measured."""
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

N_IMAGES, BATCH = 10000, 100


class Plain(torch.utils.data.Dataset):
    name = 'synthetic'

    def __init__(self, images, labels):
        self.x, self.y = images, labels.tolist()

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


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
    return {'s_median': med, 's_min': float(np.min(s)), 's_max': float(np.max(s)), 'images_per_s': N_IMAGES / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'imageset_bench.json'))
    a = ap.parse_args()
    if a.epochs < 20:
        ap.error('--epochs: the median is taken over at least 20 epochs')
    rec = {'metric': 'imageset_bench', 'images': N_IMAGES, 'shape': [32, 32, 3], 'batch_size': BATCH, 'epochs': a.epochs,
           'warmup': a.warmup, 'timing': 'synchronised wall clock around each epoch, median of the epochs'}
    if not torch.cuda.is_available():
        rec['not_run'] = 'no GPU is visible: nothing was measured'
    else:
        from cvae import ClassificationVariationalNetwork as Net
        from jvae_compat import torch_load as T
        from jvae_hip import ops
        from oracle.cases import full_config
        dev = torch.device('cuda:0')
        g = torch.Generator().manual_seed(0)
        images = torch.randint(0, 256, (N_IMAGES, 32, 32, 3), generator=g, dtype=torch.uint8)
        labels = torch.randint(0, 10, (N_IMAGES,), generator=g)
        plain = Plain(images, labels)
        resident = T.DeviceImageSet('synthetic', images.to(dev), True, labels.to(dev), None,
                                    ops.ImagesetDesc((32, 32, 3), True, device=dev), (3, 32, 32), classes=[str(c) for c in range(10)])
        net = Net(**full_config(2, 16)['net']).to(dev)
        net.eval()

        def loader_epoch():
            for x, y in torch.utils.data.DataLoader(plain, batch_size=BATCH, shuffle=True, num_workers=0):
                x, y = net._device_batch(x.to(dev)), y.to(dev)

        def device_epoch():
            for x, y in T.device_loader(resident, BATCH, True):
                pass
        props = torch.cuda.get_device_properties(0)
        rec.update(device=props.name, arch=getattr(props, 'gcnArchName', ''), torch=torch.__version__, hip=torch.version.hip)
        rec['batches'] = {'dataloader': timed(loader_epoch, a.epochs, a.warmup), 'device_loader': timed(device_epoch, a.epochs, a.warmup)}
        with torch.no_grad():
            rec['accuracy'] = {
                'dataloader': timed(lambda: net.accuracy(plain, batch_size=BATCH, update_self_testing=False), a.epochs, a.warmup),
                'device_loader': timed(lambda: net.accuracy(resident, batch_size=BATCH, update_self_testing=False), a.epochs, a.warmup)}
        for k in ('batches', 'accuracy'):
            rec[k]['dataloader_over_device_loader'] = rec[k]['dataloader']['s_median'] / rec[k]['device_loader']['s_median']
        rec['device_path_not_slower'] = all(rec[k]['dataloader_over_device_loader'] >= 1. for k in ('batches', 'accuracy'))
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
