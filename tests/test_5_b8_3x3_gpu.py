"""GPU parity of the bf16 ("B8") 3x3 padding-1 kernels and the B8 pooling / up-sampling kernels: the layers of the vgg* /
ivgg* / conv32- / deconv32- stacks in the bf16 mode (net.set_compute_dtype('bf16')).  Reference = an fp64 convolution of the
bf16-ROUNDED operands (the kernels multiply bf16 numbers exactly and accumulate in fp32), with the bars of
test_1_b8_gpu.py: fp32 outputs 2e-5 of the output scale, bf16 outputs 2^-8."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BF_TOL = 2.0 ** -8


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def rbf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def b8_channels(t, C):
    """B8 (N, CB, H, W, 8) -> (N, CB*8, H, W) fp32 on the host, padding channels included."""
    N, CB, H, W, _ = t.shape
    return t.float().cpu().permute(0, 1, 4, 2, 3).reshape(N, CB * 8, H, W)


# (cin, cout, s, op, transposed, H): every 3x3 padding-1 layer of vgg11 / vgg19 features at 3x64x64, ivgg at a 64x64 output,
# conv32- at 3x32x32 and deconv32- (both strides), plus odd channel counts
B8_3X3 = [
    (3, 64, 1, 0, False, 64), (64, 64, 1, 0, False, 64), (64, 128, 1, 0, False, 32), (128, 128, 1, 0, False, 32),
    (128, 256, 1, 0, False, 16), (256, 256, 1, 0, False, 16), (256, 512, 1, 0, False, 8), (512, 512, 1, 0, False, 8),
    (512, 512, 1, 0, False, 4),
    (64, 128, 1, 0, False, 8), (128, 64, 1, 0, False, 16), (64, 32, 1, 0, False, 32), (32, 3, 1, 0, False, 64),
    (3, 32, 1, 0, False, 32), (32, 32, 1, 0, False, 32), (32, 32, 2, 0, False, 32), (32, 64, 1, 0, False, 16),
    (64, 64, 1, 0, False, 16), (64, 64, 2, 0, False, 16),
    (64, 64, 1, 0, True, 8), (64, 64, 2, 1, True, 8), (64, 32, 1, 0, True, 16), (32, 32, 1, 0, True, 16),
    (32, 32, 2, 1, True, 16), (32, 32, 1, 0, True, 32),
    (24, 40, 1, 0, False, 16), (20, 13, 2, 0, False, 16), (13, 20, 2, 1, True, 8),
]


def _conv_ref(tr, s, op):
    if tr:
        return lambda t, w, b: F.conv_transpose2d(t, w, b, stride=s, padding=1, output_padding=op)
    return lambda t, w, b: F.conv2d(t, w, b, stride=s, padding=1)


@pytest.mark.parametrize('cin,cout,s,op,tr,H', B8_3X3)
@pytest.mark.parametrize('N', [3, 8])
def test_b8_3x3_conv_native_directions(cin, cout, s, op, tr, H, N):
    from jvae_hip import ops, ops_b8
    torch.set_num_threads(16)
    g = torch.Generator().manual_seed(cin * 131 + cout * 17 + H + s)
    x = rbf(torch.randn(N, cin, H, H, generator=g))
    wshape = (cin, cout, 3, 3) if tr else (cout, cin, 3, 3)
    w = torch.randn(wshape, generator=g) / math.sqrt(cin * 9)
    b = torch.randn(cout, generator=g)
    spec = ops.ConvSpec(cin, cout, 3, s, 1, op, tr)
    mask = ops_b8.native_mask(spec, N, H, H)
    small = H if tr else H // s                    # the folded grid: a 4x4 one keeps its weight gradient on the fp32 path
    want = ops_b8.FWD | ops_b8.DGRAD | (ops_b8.WGRAD if small >= 8 else 0)
    assert mask == want, (mask, want)

    conv = _conv_ref(tr, s, op)
    xr = x.double().requires_grad_(True)
    wr = rbf(w).double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    yr = conv(xr, wr, br)
    gy = rbf(torch.randn(yr.shape, generator=g))
    yr.backward(gy.double())

    xb = ops_b8.pack(x.to(DEV))
    gyb = ops_b8.pack(gy.to(DEV))
    wd, bd = w.to(DEV), b.to(DEV)
    # forward: fp32 output (not the 4-phase kernel, which writes B8 only), B8 output, BatchNorm partial sums
    f32_out = not (tr and s == 2)
    if f32_out:
        y32, st, ns = ops_b8.conv_fwd_raw(xb, wd, bd, spec, out_f32=True, want_stats=True)
        assert rel(y32, yr) < 2e-5
    yb, st2, ns2 = ops_b8.conv_fwd_raw(xb, wd, bd, spec, want_stats=True)
    if not f32_out:
        st, ns = st2, ns2
    assert ns > 0
    part = st[:cout * ns * 2].view(cout, ns, 2).double().sum(1).cpu()
    d = (yr.detach() - br.detach().view(1, -1, 1, 1))
    assert torch.allclose(part[:, 0], d.sum((0, 2, 3)), rtol=1e-4, atol=1e-3 * float(d.abs().sum((0, 2, 3)).max()))
    assert torch.allclose(part[:, 1], (d * d).sum((0, 2, 3)), rtol=1e-4)
    assert yb.shape == (N, (cout + 7) // 8, yr.shape[2], yr.shape[3], 8)
    assert rel(ops_b8.unpack(yb, cout), yr) < BF_TOL
    assert float(b8_channels(yb, cout)[:, cout:].abs().max() if cout % 8 else 0.) == 0.     # padding channels stay zero
    yb2, _, _ = ops_b8.conv_fwd_raw(xb, wd, bd, spec, want_stats=True)
    assert torch.equal(yb, yb2)                                                            # deterministic
    # input gradient
    gx = ops_b8.conv_dgrad_raw(gyb, wd, spec, N, H, H)
    assert rel(ops_b8.unpack(gx, cin), xr.grad) < BF_TOL
    assert torch.equal(gx, ops_b8.conv_dgrad_raw(gyb, wd, spec, N, H, H))
    # weight / bias gradient
    if mask & ops_b8.WGRAD:
        gw, gb = ops_b8.conv_wgrad_raw(xb, gyb, spec, wshape, True)
        assert rel(gw, wr.grad) < 3e-5
        assert rel(gb, br.grad) < 3e-5
        gw2, gb2 = ops_b8.conv_wgrad_raw(xb, gyb, spec, wshape, True)
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
        slot_w, slot_b = torch.ones(wshape, device=DEV), torch.ones(cout, device=DEV)
        ops_b8.conv_wgrad_raw(xb, gyb, spec, wshape, True, slot_w, slot_b)                 # accumulate in place
        assert rel(slot_w - 1, wr.grad) < 3e-5 and rel(slot_b - 1, br.grad) < 3e-5


def test_fp32_mode_keeps_3x3_layers_and_padding0_heads_off_the_b8_kernels():
    """Only the bf16 layout gained kernels: the 3x3 padding-0 head of conv32+ (config 5) and 3x3 layers on 2x2 maps have none."""
    from jvae_hip import ops, ops_b8
    assert ops_b8.native_mask(ops.ConvSpec(128, 200, 3, 1, 0), 16, 8, 8) == 0
    assert ops_b8.native_mask(ops.ConvSpec(512, 512, 3, 1, 1), 16, 2, 2) == 0
    assert ops_b8.native_mask(ops.ConvSpec(64, 64, 3, 1, 2), 16, 16, 16) == 0


@pytest.mark.parametrize('cin,cout,s,op,tr,H', [(64, 128, 1, 0, False, 16), (32, 32, 2, 0, False, 32),
                                                (64, 64, 2, 1, True, 8), (256, 256, 1, 0, False, 8)])
def test_b8_3x3_conv_with_deferred_batchnorm_input(cin, cout, s, op, tr, H):
    """bf16 conv(relu(x*scale + shift)) with the transform inside the 3x3 kernels (forward and weight gradient) against the
    convolution of the transformed input rounded to bf16 (what the kernels feed the matrix cores)."""
    from jvae_hip import ops, ops_b8
    N = 5
    g = torch.Generator().manual_seed(cin * 11 + cout + H + s)
    x = rbf(torch.randn(N, cin, H, H, generator=g))
    sc = torch.rand(cin, generator=g) + 0.5
    sh = torch.randn(cin, generator=g) * 0.5
    wshape = (cin, cout, 3, 3) if tr else (cout, cin, 3, 3)
    w = torch.randn(wshape, generator=g) / math.sqrt(cin * 9)
    wr = rbf(w).double().requires_grad_(True)
    a = rbf(torch.relu(torch.addcmul(sh.view(1, -1, 1, 1), x, sc.view(1, -1, 1, 1)))).double()
    yr = _conv_ref(tr, s, op)(a, wr, None)
    gy = rbf(torch.randn(yr.shape, generator=g))
    yr.backward(gy.double())
    spec = ops.ConvSpec(cin, cout, 3, s, 1, op, tr)
    assert ops_b8.conv_affine_ok(spec, N, H, H)
    C8 = (cin + 7) // 8 * 8
    coef = torch.zeros(2, C8)
    coef[0, :cin], coef[1, :cin] = sc, sh
    coef = coef.to(DEV)
    aff = (coef[0], coef[1], True)
    xb = ops_b8.pack(x.to(DEV))
    yb, st, ns = ops_b8.conv_fwd_raw(xb, w.to(DEV), None, spec, want_stats=True, aff=aff)
    assert rel(ops_b8.unpack(yb, cout), yr) < 2 * BF_TOL          # an input within rounding of a bf16 tie may round the other way
    part = st[:cout * ns * 2].view(cout, ns, 2).double().sum(1).cpu()
    d = yr.detach()
    assert torch.allclose(part[:, 1], (d * d).sum((0, 2, 3)), rtol=2e-3)
    gw, _ = ops_b8.conv_wgrad_raw(xb, ops_b8.pack(gy.to(DEV)), spec, wshape, False, aff=aff)
    assert rel(gw, wr.grad) < 2e-3


def test_b8_3x3_affine_refused_beyond_the_coefficient_table():
    """512 input channels exceed the 256-channel table of the forward kernels: the route says so (the stack then runs the
    BatchNorm as its own B8 pass), the layer itself stays native."""
    from jvae_hip import ops, ops_b8
    spec = ops.ConvSpec(512, 512, 3, 1, 1)
    assert ops_b8.native_mask(spec, 8, 8, 8) == 7
    assert not ops_b8.conv_affine_ok(spec, 8, 8, 8)


# ----------------------------------------------------------------------------------------- pooling / up-sampling
@pytest.mark.parametrize('N,C,H,K,S,P', [(4, 64, 32, 2, 2, 0), (3, 20, 16, 2, 2, 0), (2, 13, 9, 3, 2, 1), (5, 512, 2, 1, 1, 0),
                                         (2, 24, 8, 3, 1, 1)])
def test_b8_pooling_matches_the_fp32_kernels(N, C, H, K, S, P):
    """B8 max / average pooling against the fp32 kernels on bf16-valued inputs: max pooling routes identically (forward and
    backward bit-identical), average pooling within 2^-8; padding channels stay zero."""
    from jvae_hip import ops, ops_b8
    g = torch.Generator().manual_seed(N * 7 + C + H + K)
    x = rbf(torch.randn(N, C, H, H, generator=g)).to(DEV)
    x[:, :, 1, 1] = x[:, :, 1, 0]                                   # exact ties: the first maximum wins in both
    xb = ops_b8.pack(x)
    for mode in (ops.POOL_MAX, ops.POOL_AVG):
        xf = x.clone().requires_grad_(True)
        yf = ops.pool2d(xf, K, S, P, mode)
        xbg = xb.clone().requires_grad_(True)
        yb = ops_b8.pool2d(xbg, K, S, P, mode)
        assert yb.shape == (N, (C + 7) // 8, yf.shape[2], yf.shape[3], 8)
        gy = rbf(torch.randn(yf.shape, generator=g)).to(DEV)
        yf.backward(gy)
        yb.backward(ops_b8.pack(gy))
        if mode == ops.POOL_MAX:
            assert torch.equal(ops_b8.unpack(yb.detach(), C), yf.detach())
            if K <= S:                                              # disjoint windows: every input gets at most one term
                assert torch.equal(ops_b8.unpack(xbg.grad, C), xf.grad)
            else:
                assert torch.equal(ops_b8.unpack(xbg.grad, C), rbf(xf.grad))
        else:
            assert rel(ops_b8.unpack(yb.detach(), C), yf) < BF_TOL
            assert rel(ops_b8.unpack(xbg.grad, C), xf.grad) < BF_TOL
        if C % 8:
            assert float(b8_channels(yb.detach(), C)[:, C:].abs().max()) == 0.
            assert float(b8_channels(xbg.grad, C)[:, C:].abs().max()) == 0.
        y2 = ops_b8.pool2d(xb, K, S, P, mode)
        assert torch.equal(y2, yb.detach())


@pytest.mark.parametrize('N,C,H,sc', [(4, 64, 4, 2), (3, 20, 8, 2), (2, 13, 5, 3)])
def test_b8_upsampling_matches_the_fp32_kernels(N, C, H, sc):
    from jvae_hip import ops, ops_b8
    g = torch.Generator().manual_seed(N + C + H + sc)
    x = rbf(torch.randn(N, C, H, H, generator=g)).to(DEV)
    xf = x.clone().requires_grad_(True)
    yf = ops.upsample_nearest(xf, sc)
    xbg = ops_b8.pack(x).requires_grad_(True)
    yb = ops_b8.upsample_nearest(xbg, sc)
    assert torch.equal(ops_b8.unpack(yb.detach(), C), yf.detach())
    gy = rbf(torch.randn(yf.shape, generator=g)).to(DEV)
    yf.backward(gy)
    yb.backward(ops_b8.pack(gy))
    assert rel(ops_b8.unpack(xbg.grad, C), xf.grad) < BF_TOL
    if C % 8:
        assert float(b8_channels(yb.detach(), C)[:, C:].abs().max()) == 0.
        assert float(b8_channels(xbg.grad, C)[:, C:].abs().max()) == 0.
    gx2 = ops_b8.upsample_nearest_bwd_raw(ops_b8.pack(gy), sc)
    assert torch.equal(gx2, xbg.grad)


# ----------------------------------------------------------------------------------------- stacks and the model
class _Count:
    """Counts the layout conversions of a stack's forward (ops_b8 functions are looked up at call time)."""

    def __init__(self, monkeypatch):
        from jvae_hip import ops_b8
        self.n = {'to_b8': 0, 'from_b8': 0, 'pack': 0, 'unpack': 0}
        for name in self.n:
            fn = getattr(ops_b8, name)

            def wrapped(*a, _fn=fn, _name=name, **kw):
                self.n[_name] += 1
                return _fn(*a, **kw)
            monkeypatch.setattr(ops_b8, name, wrapped)

    def reset(self):
        for k in self.n:
            self.n[k] = 0


@pytest.mark.parametrize('where,shape,name', [('input', (3, 64, 64), 'vgg11'), ('output', (64, 4, 4), 'ivgg')])
def test_b8_3x3_stack_stays_in_b8_and_matches_fp32(where, shape, name, monkeypatch):
    """A vgg11 feature stack / an ivgg upsampler in the bf16 mode converts once on the way in and at most once on the way
    out (pooling and up-sampling included), and tracks the same stack in fp32: output within 3 % in L2, parameter gradients by
    direction.  vgg11 is deeper than conv32+ (8 BatchNorm+ReLU boundaries and 5 max pools, each flipping the mask or the
    argmax of the activations within bf16 rounding of a tie): ONE bf16-sized perturbation of the input alone, in fp32 on both
    sides, already moves its first layers' gradients to cosine 0.935-0.96; the bf16 mode, which rounds at every layer,
    measures 0.89-0.95 there and 0.975 at the last convolution.  Bars: cosine > 0.85 everywhere, > 0.95 for the last
    convolution."""
    from module.vae_layers.conv import build_de_conv_layers
    torch.manual_seed(0)
    a = build_de_conv_layers(shape, name, batch_norm=True, where=where).to(DEV)
    b = build_de_conv_layers(shape, name, batch_norm=True, where=where).to(DEV)
    b.load_state_dict(a.state_dict())
    b.compute_dtype = 'bf16'
    x = torch.rand(6, *shape, device=DEV)
    ya = a(x)
    cnt = _Count(monkeypatch)
    yb = b(x)
    if name == 'vgg11':
        assert cnt.n['to_b8'] == 1 and cnt.n['from_b8'] == 1, cnt.n
    else:
        assert cnt.n['to_b8'] == 1 and cnt.n['from_b8'] <= 1, cnt.n
    assert cnt.n['pack'] == cnt.n['to_b8'] and cnt.n['unpack'] == cnt.n['from_b8'], cnt.n   # no conversion inside the stack
    assert yb.dtype == torch.float32 and yb.shape == ya.shape
    err = float((ya - yb).detach().norm() / ya.detach().norm())
    assert err < 3e-2, (name, err)
    g = torch.randn_like(ya)
    ya.backward(g)
    yb.backward(g)
    cosines = {}
    for (n_, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if pa.grad is None or float(pa.grad.norm()) < 1e-6 * pa.numel() ** 0.5:
            continue          # dead biases in front of a BatchNorm
        cosines[n_] = float((pa.grad * pb.grad).sum() / (pa.grad.norm() * pb.grad.norm()))
    last = [n_ for n_, _ in b.named_parameters() if n_.endswith('.weight') and b[int(n_.split('.')[0])].__class__.__name__
            in ('HipConv2d', 'HipConvTranspose2d')][-1]
    assert min(cosines.values()) > 0.85 and cosines[last] > 0.95, (name, last, cosines)


def test_b8_vgg11_ivgg_training_sequence_tracks_fp32():
    """A cvae with vgg11 features and an ivgg upsampler (3x64x64, BatchNorm) trains 24 steps in the bf16 mode against the
    same run in fp32 with the robust bars of test_b8_training_sequence_tracks_fp32's un-chosen case: the median step within
    5 %, at most one step beyond 25 %, the last six steps within 3 %; both runs fall and the bf16 run is bit-reproducible."""
    from oracle.cases import get_case
    from oracle.det_init import load_det_state
    from cvae import ClassificationVariationalNetwork as Net
    kw = get_case('c5_n4')['net']
    kw.update(features='vgg11', upsampler='ivgg', latent_dim=256)     # 16 x 4 x 4 in front of the upsampler
    N = 32
    torch.manual_seed(1)
    data = torch.rand(4, N, *kw['input_shape'], device=DEV)
    lab = torch.randint(0, kw['num_labels'], (4, N), device=DEV)

    def run(dtype):
        net = Net(**kw)
        load_det_state(net, seed=0)
        net.to(DEV).train()
        net.set_compute_dtype(dtype)
        torch.manual_seed(7)
        torch.cuda.manual_seed(7)
        hist = []
        for step in range(24):
            losses, _ = net.train_step(data[step % 4], lab[step % 4])
            hist.append(losses['total'].detach().mean())
        hist = [float(h) for h in hist]
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
        return hist, torch.cat([p.detach().flatten() for p in net.parameters()])
    h32, _ = run('fp32')
    h16, p16 = run('bf16')
    h16b, p16b = run('bf16')
    assert h16 == h16b and torch.equal(p16, p16b)
    diffs = sorted(abs(a - b) / abs(a) for a, b in zip(h32, h16))
    median = diffs[len(diffs) // 2]
    tail = abs(sum(h16[-6:]) - sum(h32[-6:])) / sum(h32[-6:])
    assert diffs[-2] < 0.25 and median < 0.05 and tail < 3e-2, (diffs[-2:], median, tail, h32, h16)
    assert all(np.isfinite(h16)) and all(np.isfinite(h32))
    assert h32[-1] < 0.7 * h32[0] and h16[-1] < 0.7 * h16[0], (h32, h16)
    print(f'vgg11/ivgg bf16 vs fp32 over 24 steps: median step difference {median:.2e}, last six steps {tail:.2e}')
