#!/usr/bin/env python3
"""Write tests/golden/conv_stats/*.npz on the device: for every case of tests/conv_stats_cases.py the seed of its inputs, y, the
BatchNorm partial sums trimmed to the reported nsplit, nsplit and the name of the kernel that ran.

    python tools/gen_conv_stats_golden.py [--out DIR]

Run at the commit whose outputs are the reference (the parent of a change that must not move a bit), with the library built;
tests/test_12_conv_stats_golden_gpu.py then reruns conv_stats_cases.run() on every case and compares the four with the file
bit for bit (a y above 512 KiB: its first image, its last image and the SHA-256 of all its bytes).  Each case runs twice and
must agree with itself before it is written.  The files in the tree were written with a build of 358ed88."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'conv_stats'))
    a = ap.parse_args()
    import conv_stats_cases as sc
    os.makedirs(a.out, exist_ok=True)
    for c in sc.CASES:
        r, again = sc.run(c), sc.run(c)
        for k in ('y', 'stats', 'nsplit'):
            assert np.array_equal(r[k], again[k]), f'{c.name}: two runs differ in {k}'
        assert np.isfinite(r['stats']).all() and (r['y'].dtype == np.uint16 or np.isfinite(r['y']).all()), c.name
        path = os.path.join(a.out, c.name + '.npz')
        np.savez(path, **sc.stored(c, r))
        print(f'{c.name:20s} {str(r["kernel"]):11s} nsplit {int(r["nsplit"]):5d}  y {r["y"].shape}  {os.path.getsize(path)} bytes',
              flush=True)


if __name__ == '__main__':
    main()
