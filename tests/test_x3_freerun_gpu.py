"""The stride-1 split-bf16 convolution (conv_x3.hip, 16x16x32 form) with its weight fragments loaded from the packed buffer
straight into registers: accuracy against an fp64 torch convolution at the smallest shapes where the fragment addressing can
go wrong, and run-to-run determinism.

Inputs and bound are those of test_split_bf16_conv_is_fp32_accurate (tests/test_0_ops_gpu.py): data with a wide dynamic range
(every (image, channel) plane scaled by exp(2 * randn)), error < 3e-6 of the output scale.

Shapes: Cin 16 / 32 / 40 = one, two, three K steps (the last one ragged: the packed weights of channels 40 .. 47 are zeros);
Cout 32 / 20 / 64 = a full 32-channel block, a partial one, two blockIdx.y blocks (the block offset into the packed weights);
output side 8 / 16 / 32 = the three instantiations; N = 3 = a ragged image group at side 8 (two images per tile).  The dgrad of
every case runs the kernel in the other weight role (swap / flip) with Cout as its K dimension (20: two K steps, ragged)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BOUND = 3e-6          # tests/test_0_ops_gpu.py::test_split_bf16_conv_is_fp32_accurate, split-bf16 mode
LEAKY = 0.01          # JVAE_LEAKY_SLOPE


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def make(cin, cout, tr, H, N):
    g = torch.Generator().manual_seed(cin * 7 + cout + H + (1000 if tr else 0))
    x = torch.randn(N, cin, H, H, generator=g) * torch.exp(2 * torch.randn(N, cin, 1, 1, generator=g))
    w = torch.randn((cin, cout, 5, 5) if tr else (cout, cin, 5, 5), generator=g) / math.sqrt(cin * 25)
    b = torch.randn(cout, generator=g)
    sc = torch.rand(cin, generator=g) + 0.5
    sh = torch.randn(cin, generator=g) * 0.1
    return g, x, w, b, sc, sh


def conv64(a, w, b, tr):
    f = F.conv_transpose2d if tr else F.conv2d
    return f(a.double(), w.double(), None if b is None else b.double(), padding=2)


def act64(x, sc, sh, relu):
    """the deferred BatchNorm(+activation) of the layer input, in fp64"""
    if relu is None:
        return x.double()
    a = x.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    return F.relu(a) if relu == 1 else F.leaky_relu(a, LEAKY) if relu == 2 else a


def check_stats(st, ns, y, b, cout):
    """BatchNorm partial sums of (y - bias) from the kernel epilogue, at the bars of test_split_bf16_conv_is_fp32_accurate"""
    part = st[:cout * ns * 2].view(cout, ns, 2).double().sum(1).cpu()
    yc = y.double().cpu() - b.double().view(1, -1, 1, 1)
    assert float((part[:, 0] - yc.sum((0, 2, 3))).abs().max() / yc.abs().sum((0, 2, 3)).max()) < 1e-5
    assert float((part[:, 1] - (yc * yc).sum((0, 2, 3))).abs().max() / (yc * yc).sum((0, 2, 3)).max()) < 1e-5


def run_forward_modes(ops, xd, wd, bd, scd, shd, spec, x, w, b, sc, sh, tr, cout, modes):
    """every (deferred BatchNorm, stats) mode of `modes` against fp64; -> {mode: error}"""
    errs = {}
    for relu in modes:
        ref = conv64(act64(x, sc, sh, relu), w, b, tr)
        for stats in (False, True):
            if relu is None:
                y, st, ns = ops.conv_fwd_stats_raw(xd, wd, bd, spec) if stats else (ops.conv_fwd_raw(xd, wd, bd, spec), None, 0)
            else:
                y, st, ns = ops.conv_fwd_aff_raw(xd, wd, bd, spec, (scd, shd, relu), stats)
            errs[(relu, stats)] = rel(y, ref)
            if stats:
                assert st is not None and ns > 0
                check_stats(st, ns, y, b, cout)
    return errs


@pytest.mark.parametrize('tr', [False, True], ids=['conv', 'convT'])
@pytest.mark.parametrize('H', [8, 16, 32])
@pytest.mark.parametrize('cout', [32, 20, 64])
@pytest.mark.parametrize('cin', [16, 32, 40])
def test_freerun_conv_matches_fp64(cin, cout, H, tr):
    from jvae_hip import ops
    N = 3
    g, x, w, b, sc, sh = make(cin, cout, tr, H, N)
    spec = ops.ConvSpec(cin, cout, 5, 1, 2, 0, tr)
    assert ops.conv_route(spec, N, H, H, 'fwd', bias=True).kernel == 'CK_FWD5_X3'
    xd, wd, bd, scd, shd = (t.to(DEV) for t in (x, w, b, sc, sh))
    errs = run_forward_modes(ops, xd, wd, bd, scd, shd, spec, x, w, b, sc, sh, tr, cout, (None, 1, 2))
    # the other weight role: the data gradient (K dimension = cout)
    gy = torch.randn(N, cout, H, H, generator=g) * torch.exp(2 * torch.randn(N, cout, 1, 1, generator=g))
    dx = ops.conv_dgrad_raw(gy.to(DEV), wd, spec, xd.shape)
    errs['dgrad'] = rel(dx, conv64(gy, w, None, not tr))
    print(cin, cout, H, tr, {k: '%.2e' % v for k, v in errs.items()})
    assert max(errs.values()) < BOUND, errs


def two_tile_batch(H, cout):
    """smallest N at which launch_x3 takes two tiles per workgroup: an even number of tiles, tiles * (OP / 32) >= 2048
    (conv_x3.hip; tiles = N * OH * OW / PIX with PIX = 128 at side 8, else 256; at side 8 a tile holds two images)"""
    blocks = (cout + 31) // 32
    tiles = -(-2048 // blocks)
    tiles += tiles % 2
    return {8: 2 * tiles - 1, 16: tiles, 32: -(-tiles // 4)}[H]


def test_freerun_second_tile_restarts_weight_stream():
    """two tiles per workgroup: behind the last K step of the first tile the fragment stream starts again at K step 0"""
    from jvae_hip import ops
    cin, cout, H, tr = 32, 256, 8, False              # two K steps: the stream wraps from K step 1 to K step 0
    N = two_tile_batch(H, cout)
    assert N == 511
    g, x, w, b, sc, sh = make(cin, cout, tr, H, N)
    spec = ops.ConvSpec(cin, cout, 5, 1, 2, 0, tr)
    assert ops.conv_route(spec, N, H, H, 'fwd', bias=True).kernel == 'CK_FWD5_X3'
    xd, wd, bd, scd, shd = (t.to(DEV) for t in (x, w, b, sc, sh))
    errs = run_forward_modes(ops, xd, wd, bd, scd, shd, spec, x, w, b, sc, sh, tr, cout, (1,))
    print(N, {k: '%.2e' % v for k, v in errs.items()})
    assert max(errs.values()) < BOUND, errs


@pytest.mark.parametrize('H', [8, 16, 32])
def test_freerun_conv_is_deterministic(H):
    from jvae_hip import ops
    cin, cout, tr, N = 40, 64, False, 3
    g, x, w, b, sc, sh = make(cin, cout, tr, H, N)
    spec = ops.ConvSpec(cin, cout, 5, 1, 2, 0, tr)
    xd, wd, bd, scd, shd = (t.to(DEV) for t in (x, w, b, sc, sh))
    first = None
    for _ in range(8):
        y, st, ns = ops.conv_fwd_aff_raw(xd, wd, bd, spec, (scd, shd, 1), True)
        cur = (y.clone(), st[:cout * ns * 2].clone())
        if first is None:
            first = cur
        assert torch.equal(first[0], cur[0]) and torch.equal(first[1], cur[1])
