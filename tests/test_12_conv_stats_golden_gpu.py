"""The forward-type convolution kernels with a BatchNorm-sums epilogue against outputs recorded on the device BEFORE that
epilogue, the partial count's return path and the launch helpers were shared (tests/golden/conv_stats/*.npz, written by
tools/gen_conv_stats_golden.py): y, the partial sums, their count and the kernel that ran, equal bit for bit.  No tolerance, no
skip: a case that reaches another kernel fails.  The cases and why they are the smallest that can go wrong: conv_stats_cases.py.

(A y above 512 KiB - the two-tiles-per-workgroup case, 21 MB - is recorded as its first image, its last image and the SHA-256 of
all its bytes: equality of the digest is equality of the bits, and a committed file stays far below the size limit.)"""
import hashlib
import os

import numpy as np
import pytest

import conv_stats_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.name)
def test_conv_stats_golden(case, golden_dir):
    g = np.load(os.path.join(golden_dir, 'conv_stats', case.name + '.npz'))
    assert int(g['seed']) == case.seed
    r = sc.run(case)
    assert str(r['kernel']) == str(g['kernel']) == case.kernel
    assert int(r['nsplit']) == int(g['nsplit'])
    if case.name.startswith('x3_two_tiles'):
        assert int(r['nsplit']) == sc.TWO_TILES_NSPLIT          # the tile count, not the halved grid
    assert r['stats'].dtype == g['stats'].dtype and r['stats'].shape == g['stats'].shape
    assert np.array_equal(r['stats'].view(np.uint32), g['stats'].view(np.uint32)), 'BatchNorm partial sums differ'
    y = r['y']
    bits = np.uint16 if y.dtype == np.uint16 else np.uint32
    if 'y' in g:
        assert y.dtype == g['y'].dtype and y.shape == g['y'].shape
        assert np.array_equal(y.view(bits), g['y'].view(bits)), 'y differs'
    else:
        assert np.array_equal(y[0].view(bits), g['y_head'].view(bits)) and np.array_equal(y[-1].view(bits), g['y_tail'].view(bits))
        assert hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest() == str(g['y_sha256']), 'y differs'
