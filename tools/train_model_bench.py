"""GPU box: ms per batch of train_model() itself - the entry the reference's train.py calls - with TRAIN_CAPTURED off
(the eager train_step() per batch) and on (replays of the captured step), in ONE process on the same box.

Workload: BASELINE.json configs[1] (CIFAR-10 conv CVAE, batch size 512) on a device-resident synthetic dataset of
`--batches` full batches per epoch (default 64, no ragged batch).  Each mode gets a fresh model from the same seed and runs
`--epochs` epochs (default 3): epoch 0 pays the allocations and, with the switch on, the eager warm-up batches and the
capture; the later epochs are steady state.  A batch is timed from HIP event to HIP event recorded by the loop's test hook
after each batch, so an epoch of B batches gives B - 1 intervals; the epoch boundaries (history, lr, eval()) are left out.
The loader is train_model()'s own torch DataLoader (shuffle, no workers): its per-batch gather is part of both figures.

    python tools/train_model_bench.py [--batches 64] [--epochs 3] [--report-every 10] [--out FILE]

Prints one line per mode and a JSON summary; --out also writes the summary to a text file.  A tool, not a test: bench.py
(the replay of graph_train_step on ONE fixed batch) stays the contract's metric - run it beside this on the same box to
see how far the loop stands from the bare replay."""
import argparse
import json
import os
import socket
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'joint-vae_amd')]
import bench  # noqa: E402

BATCH = 512


def run(captured, data, a, dev):
    torch.manual_seed(0)
    net = bench.build_model(dev)
    net.TRAIN_CAPTURED = captured
    marks = []

    def hook(epoch, i, x, y, eps, losses):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((epoch, i, ev, time.perf_counter()))
    net._train_batch_hook = hook
    t0 = time.time()
    hist = net.train_model(data, epochs=a.epochs, batch_size=BATCH, validation=0, device=dev, report_every=a.report_every)
    torch.cuda.synchronize()
    wall = time.time() - t0
    per_epoch = []
    for e in range(a.epochs):
        m = [r for r in marks if r[0] == e]
        gaps = sorted(m[j][2].elapsed_time(m[j + 1][2]) for j in range(len(m) - 1))
        host = (m[-1][3] - m[0][3]) * 1e3 / (len(m) - 1)
        per_epoch.append({'epoch': e, 'intervals': len(gaps), 'ms_per_batch': sum(gaps) / len(gaps),
                          'median_ms': gaps[len(gaps) // 2], 'min_ms': gaps[0], 'max_ms': gaps[-1], 'host_ms_per_batch': host})
    steady = [p for p in per_epoch if p['epoch'] >= 1] or per_epoch
    n = sum(p['intervals'] for p in steady)
    ms = sum(p['ms_per_batch'] * p['intervals'] for p in steady) / n
    return {'mode': 'captured' if captured else 'eager', 'steady_batches': n, 'ms_per_batch': ms, 'images_per_s': BATCH / ms * 1e3,
            'median_ms': sorted(p['median_ms'] for p in steady)[len(steady) // 2], 'wall_s': wall,
            'captures_built': net._captures_built, 'per_epoch': per_epoch,
            'final_total_loss': hist[a.epochs - 1]['train_loss']['total']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=64, help='full batches per epoch (>= 61 for 60 steady-state intervals)')
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--report-every', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    n = a.batches * BATCH
    protos = torch.rand(10, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (n,), generator=g)
    x = (0.7 * protos[y] + 0.3 * torch.rand(n, 3, 32, 32, generator=g)).clamp(0, 1)
    data = torch.utils.data.TensorDataset(x.to(dev), y.to(dev))
    rows = [run(False, data, a, dev), run(True, data, a, dev)]
    for r in rows:
        print('%-8s %7.3f ms/batch (median %.3f)  %9.0f images/s  over %d steady-state batches  [captures built: %d]'
              % (r['mode'], r['ms_per_batch'], r['median_ms'], r['images_per_s'], r['steady_batches'], r['captures_built']))
    out = {'tool': 'tools/train_model_bench.py', 'workload': 'BASELINE configs[1], batch 512, %d batches/epoch, %d epochs'
           % (a.batches, a.epochs), 'report_every': a.report_every, 'host': socket.gethostname(),
           'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'),
           'captured_over_eager': rows[1]['ms_per_batch'] / rows[0]['ms_per_batch'], 'modes': rows}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
