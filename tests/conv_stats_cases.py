"""The cases of tests/test_12_conv_stats_golden_gpu.py and tools/gen_conv_stats_golden.py: one forward with bias and BatchNorm
partial sums per forward-type kernel that carries the shared stats epilogue (csrc/conv_stats.h), at the smallest shapes at which
each can go wrong.  A plain module, not a conftest.

All maps are 8x8 on the small side and N = 3, so a 128-pixel tile holds more images than exist: the missing images must
contribute exact zeros to the sums.  40 output channels leave the second 32-channel tile half used (the channel guard of the
fold step); the 4-phase fp32 kernels need a multiple of 32.  `x3_two_tiles` is the smallest batch at 8x8 at which launch_x3
gives a workgroup two tiles (grid.x even, grid.x * grid.y >= 2048: 1024 tiles of two images, the last one half empty): its
nsplit must stay the TILE count.  Every case runs plain and with a deferred BatchNorm + ReLU on its input; the fp32 stride-1
ones also with the leaky form (the three instantiations of the launch helper).

Inputs are drawn from the case's seed on the CPU; the recorded outputs are compared bit for bit, nothing here has a tolerance."""
import collections
import hashlib

import numpy as np
import torch

from jvae_hip import lib, ops, ops_b8

Case = collections.namedtuple('Case', 'name kernel cin cout s tr hw N layout split sh16 aff seed')
FULL_Y_BYTES = 512 << 10         # a larger y is recorded as its first and last image plus the SHA-256 of all of it


def _cases():
    base = [
        # name, kernel, Cin, Cout, stride, transposed, input H = W, N, layout, split-bf16 switch, 16x16x32 switch, leaky too
        ('fwd5_s2', 'CK_FWD5', 16, 40, 2, 0, 16, 3, 'f32', 1, 1, False),
        ('fwd5_s1', 'CK_FWD5', 16, 40, 1, 0, 8, 3, 'f32', 0, 1, True),
        ('x3_sh16', 'CK_FWD5_X3', 16, 40, 1, 0, 8, 3, 'f32', 1, 1, True),
        ('x3_sh32', 'CK_FWD5_X3', 16, 40, 1, 0, 8, 3, 'f32', 1, 0, True),
        ('x3_two_tiles', 'CK_FWD5_X3', 16, 40, 1, 0, 8, 2047, 'f32', 1, 1, False),
        ('t2', 'CK_T2', 16, 32, 2, 1, 8, 3, 'f32', 0, 1, False),
        ('t2_x3', 'CK_T2_X3', 16, 32, 2, 1, 8, 3, 'f32', 1, 1, False),
        ('b8', 'CK_B8', 16, 40, 1, 0, 8, 3, 'b8', 1, 1, False),
        ('t2_b8', 'CK_T2_B8', 16, 40, 2, 1, 8, 3, 'b8', 1, 1, False),
    ]
    out = []
    for i, (name, kernel, cin, cout, s, tr, hw, N, layout, split, sh16, leaky) in enumerate(base):
        for aff in (0, 1, 2) if leaky else (0, 1):
            out.append(Case(name + ('', '_relu', '_leaky')[aff], kernel, cin, cout, s, tr, hw, N, layout, split, sh16, aff,
                            20261018 + 16 * i + aff))
    return out


CASES = _cases()
TWO_TILES_NSPLIT = 1024


def spec_of(c):
    return ops.ConvSpec(c.cin, c.cout, 5, c.s, 2, 1 if c.tr else 0, bool(c.tr))


def inputs(c):
    """x, w, bias, (scale, shift) from the case's seed (CPU generator: the same bits everywhere)."""
    g = torch.Generator().manual_seed(c.seed)
    x = torch.randn((c.N, c.cin, c.hw, c.hw), generator=g)
    wshape = (c.cin, c.cout, 5, 5) if c.tr else (c.cout, c.cin, 5, 5)
    w = torch.randn(wshape, generator=g) / (5. * c.cin ** .5)
    b = torch.randn((c.cout,), generator=g)
    sc = .5 + torch.rand((c.cin,), generator=g)
    sh = .5 * torch.randn((c.cin,), generator=g)
    return x, w, b, sc, sh


def run(c, dev='cuda'):
    """-> dict(y, stats, nsplit, kernel): y as stored (uint16 bit patterns of a bf16 output), stats trimmed to nsplit."""
    L = lib.load()
    old = L.jvae_conv2d_set_split_bf16(c.split), L.jvae_conv2d_set_split_shape16(c.sh16)
    try:
        sp = spec_of(c)
        route = ops.conv_route(sp, c.N, c.hw, c.hw, 'fwd', c.layout, bias=True, stats=True, aff=c.aff)
        assert route.kernel == c.kernel, f'{c.name}: expected {c.kernel}, routed to {route.kernel}'
        assert route.aff_ok or not c.aff, f'{c.name}: {route.kernel} reports no deferred BatchNorm'
        x, w, b, sc, sh = (t.to(dev) for t in inputs(c))
        aff = (sc, sh, c.aff) if c.aff else None
        if c.layout == 'b8':
            y, st, ns = ops_b8.conv_fwd_raw(ops_b8.pack(x), w, b, sp, want_stats=True, aff=aff)
            y = y.view(torch.int16)
        elif aff is not None:
            y, st, ns = ops.conv_fwd_aff_raw(x, w, b, sp, aff, True)
        else:
            y, st, ns = ops.conv_fwd_stats_raw(x, w, b, sp)
        assert st is not None and 0 < ns <= route.splits, (c.name, ns, route.splits)
        y = y.cpu().numpy()
        return dict(y=y.view(np.uint16) if y.dtype == np.int16 else y, stats=st[:c.cout * ns * 2].cpu().numpy(),
                    nsplit=np.int32(ns), kernel=np.array(route.kernel))
    finally:
        L.jvae_conv2d_set_split_bf16(old[0])
        L.jvae_conv2d_set_split_shape16(old[1])


def stored(c, r):
    """What the golden file of a case holds."""
    d = dict(seed=np.int64(c.seed), stats=r['stats'], nsplit=r['nsplit'], kernel=r['kernel'])
    y = r['y']
    if y.nbytes <= FULL_Y_BYTES:
        d['y'] = y
    else:
        d.update(y_head=y[0], y_tail=y[-1], y_sha256=np.array(hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()))
    return d
