"""Image generation on the device: the two kernels of csrc/sample.hip (ops.prior_sample, ops.image_grid), GaussianPrior.sample,
net.generate() and module.sample.sample(), against the fp64 restatement and the inputs of tests/test_sample_restatement.py,
the CPU oracle, and what the REFERENCE's sample() returned (tools/gen_sample_golden.py -> tests/golden/sample).

Bars.  Prior draws: UNIT / SCALAR / DIAG bit-identical to the fp32 torch expression; FULL within 4 x the error fp32
torch.linalg.solve_triangular on the CPU shows against the fp64 solve on the same inputs (relative to max |z|; a differently
ordered fp32 sum is as good as torch's - the margin tests/test_14_wim_gpu.py gives its `soft~` and `@` rows).  Grid: INPUT and
DRAW cells bit-identical to their sources, AVERAGE cells within the bound of a sequential fp32 sum and one division,
((n - 1) u sum |x_l|) / n + u |avg|, u = 2^-24; the 8-bit grid bit-identical to floor(clamp(255 v + 0.5, 0, 255)) of the kernel's
own fp32 grid.  Models: 1e-4 relative against the oracle and the golden, the bar of the evaluation goldens.

Measured on the MI355X, FULL mode, worst case over C, R, t and labels given / not given per K - error against the fp64 solve
relative to max |z|, the kernel's (and fp32 solve_triangular's on the same inputs):
    K = 1     7.64e-08 (7.64e-08)
    K = 5     9.87e-08 (1.56e-07)
    K = 64    9.27e-08 (1.01e-07)
    K = 200   7.26e-08 (1.42e-07)
    K = 256   7.80e-08 (1.34e-07)
and in the wider register tiers (C = 2, R = 5, t = 0.7, labels given):
    K = 300   4.69e-08 (6.70e-08)
    K = 1000  5.31e-08 (8.18e-08)
    K = 1024  5.07e-08 (1.30e-07)"""
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state
from test_sample_restatement import (CLASS_NAMES, MODEL_CASES, NAMED, PS_C, PS_K, PS_R, PS_T, average_bound, decode_png, full_errors,
                                     grid64, grid_columns_for, grid_inputs, load_golden, oracle_decode, oracle_model,
                                     prior_inputs, quantise)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RTOL = 1e-4


def rel(a, b):
    a = np.asarray(a.detach().double().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().double().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def same_bits(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(p):
    return {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}


def torch_draw(p, mode, t, with_y):
    """The fp32 torch expression of the three element-wise modes, on the CPU (one rounding per operation)."""
    y = torch.from_numpy(p['y']) if with_y else torch.zeros(len(p['eps']), dtype=torch.int64)
    e = torch.tensor(t, dtype=torch.float32) * torch.from_numpy(p['eps'])
    if mode == 'scalar':
        e = e / torch.from_numpy(p['scalar'])[y].unsqueeze(-1)
    elif mode == 'diag':
        e = e / torch.from_numpy(p['diag'])[y]
    return torch.from_numpy(p['means'])[y] + e


# ---------------------------------------------------------------------------------------------- 1. prior draws
@pytest.mark.parametrize('K', PS_K)
def test_prior_sample_against_torch_and_the_fp64_solve(K):
    from jvae_hip import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = (0., 0.)
    for C in PS_C:
        for R in PS_R:
            p = prior_inputs(K, C, R)
            d = dev(p)
            for t in PS_T:
                for with_y in (False, True):
                    y = d['y'] if with_y else None
                    for mode in ('unit', 'scalar', 'diag'):
                        z = ops.prior_sample(d['eps'], y, d['means'], d.get(mode), mode=mode, temperature=t, status=status)
                        assert same_bits(z, torch_draw(p, mode, t, with_y)), (mode, C, R, t, with_y)
                    z = ops.prior_sample(d['eps'], y, d['means'], d['full'], mode='full', temperature=t, status=status)
                    again = ops.prior_sample(d['eps'], y, d['means'], d['full'], mode='full', temperature=t, status=status)
                    assert same_bits(z, again)
                    top, referr, err = full_errors(p, t, with_y, z.cpu().numpy())
                    print(f'full K={K} C={C} R={R} t={t} y={with_y}: kernel {err / top:.3e} solve_triangular {referr / top:.3e}')
                    assert err <= 4 * referr, (C, R, t, with_y, err / top, referr / top)
                    if err / top > worst[0]:
                        worst = (err / top, referr / top)
    print(f'full K={K} worst: kernel {worst[0]:.2e} (solve_triangular {worst[1]:.2e})')
    assert int(status) == 0


@pytest.mark.parametrize('K', [300, 1000, 1024])
def test_full_mode_in_the_wide_register_tiers(K):
    """K above 256: the instantiations that keep 8 and 16 values of u per lane (K <= 512, K <= 1024), same bar."""
    from jvae_hip import ops
    p = prior_inputs(K, 2, 5)
    d = dev(p)
    z = ops.prior_sample(d['eps'], d['y'], d['means'], d['full'], mode='full', temperature=.7)
    top, referr, err = full_errors(p, .7, True, z.cpu().numpy())
    print(f'full K={K}: kernel {err / top:.3e} solve_triangular {referr / top:.3e}')
    assert 0. < referr / top < 1e-5 and err <= 4 * referr
    assert same_bits(ops.prior_sample(d['eps'], d['y'], d['means'], d['diag'], mode='diag', temperature=.7),
                     torch_draw(p, 'diag', .7, True))


def test_full_mode_rows_do_not_depend_on_the_launch():
    """The rows of a 650-row launch equal the same rows drawn alone (one wave per row: the order of every sum is K's alone)."""
    from jvae_hip import ops
    d = dev(prior_inputs(200, 10, 650))
    whole = ops.prior_sample(d['eps'], d['y'], d['means'], d['full'], mode='full', temperature=.7)
    for r0, r1 in ((0, 1), (17, 38), (649, 650)):
        part = ops.prior_sample(d['eps'][r0:r1], d['y'][r0:r1], d['means'], d['full'], mode='full', temperature=.7)
        assert same_bits(part, whole[r0:r1])


@pytest.mark.parametrize('mode', ['unit', 'scalar', 'diag', 'full'])
def test_prior_sample_writes_its_rows_only_and_flags_a_bad_label(mode):
    from jvae_hip import ops
    K, C, R = 5, 10, 21
    p = prior_inputs(K, C, R)
    d = dev(p)
    sentinel = torch.arange((R + 9) * K, dtype=torch.float32, device=DEV).view(R + 9, K) * -1.5 - 7.
    buf = sentinel.clone()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    good = ops.prior_sample(d['eps'], d['y'], d['means'], d.get(mode), mode=mode, status=status)
    out = ops.prior_sample(d['eps'], d['y'], d['means'], d.get(mode), mode=mode, out=buf[4:4 + R], status=status)
    assert out.data_ptr() == buf[4:4 + R].data_ptr() and int(status) == 0
    assert same_bits(buf[4:4 + R], good) and torch.equal(buf[:4], sentinel[:4]) and torch.equal(buf[4 + R:], sentinel[4 + R:])
    for bad in (C, -1, 1 << 40):
        y = d['y'].clone()
        y[7] = bad
        status.zero_()
        z = ops.prior_sample(d['eps'], y, d['means'], d.get(mode), mode=mode, status=status)
        assert int(status) & 1 and bool(torch.isnan(z[7]).all())
        keep = torch.arange(R, device=DEV) != 7
        assert same_bits(z[keep], good[keep])
        with pytest.raises(ops.L.JvaeHipError):
            ops.wim_check_status(status)
        assert int(status) == 0                                # read and cleared
    with pytest.raises(ops.L.JvaeHipError):
        ops.prior_sample(d['eps'], d['y'].int(), d['means'], d.get(mode), mode=mode)
    with pytest.raises(ops.L.JvaeHipError):
        ops.prior_sample(torch.zeros(2, 1025, device=DEV), None, torch.zeros(1, 1025, device=DEV), None, mode='unit')


def test_gaussian_prior_sample():
    from module.priors import GaussianPrior, TiltedGaussianPrior, UniformWithGaussianTailPrior
    K, C, N, L = 5, 10, 21, 3
    p = prior_inputs(K, C, N)
    eps = torch.from_numpy(prior_inputs(K, C, L * N)['eps']).view(L, N, K)
    y = torch.from_numpy(p['y'])
    for var_dim in ('scalar', 'diag', 'full'):
        pr = GaussianPrior(K, var_dim=var_dim, num_priors=C, init_mean=1.)
        with torch.no_grad():
            pr.mean.copy_(torch.from_numpy(p['means']))
            pr._var_parameter.copy_(torch.from_numpy(p[var_dim]))
        pr.to(DEV)
        q = dict(p, eps=eps.reshape(L * N, K).numpy(), y=np.tile(p['y'], L))
        z = pr.sample(y.to(DEV), epsilon=eps.to(DEV), temperature=.7)
        assert tuple(z.shape) == (L, N, K) and z.is_cuda
        if var_dim == 'full':
            top, referr, err = full_errors(q, .7, True, z.reshape(L * N, K).cpu().numpy())
            assert err <= 4 * referr
            flat_y = torch.from_numpy(q['y']).to(DEV)                       # sample() is the inverse of whiten()
            white = pr.whiten(z.reshape(L * N, K) - pr.mean.detach()[flat_y], flat_y)
            assert rel(white, .7 * eps.reshape(L * N, K)) < 1e-5
        else:
            assert same_bits(z.reshape(L * N, K), torch_draw(q, var_dim, .7, True))
        unit = pr.sample(y.to(DEV), epsilon=eps.to(DEV), with_variance=False)
        assert same_bits(unit, eps + torch.from_numpy(p['means'])[y].unsqueeze(0))
        drawn = pr.sample(y.to(DEV), L=4)
        assert tuple(drawn.shape) == (4, N, K) and bool(torch.isfinite(drawn).all())
        with pytest.raises(ValueError):
            pr.sample(L=2)
    single = GaussianPrior(K, var_dim='diag', num_priors=1, init_mean=1.).to(DEV)
    z = single.sample(n=N, epsilon=eps.to(DEV))
    assert same_bits(z, single.mean.detach().cpu().view(1, 1, K) + eps / single._var_parameter.detach().cpu())
    assert tuple(single.sample(n=7, L=2).shape) == (2, 7, K)
    for cls in (TiltedGaussianPrior, UniformWithGaussianTailPrior):
        pr = cls(K, num_priors=C, init_mean=1.).to(DEV)
        with pytest.raises(NotImplementedError):
            pr.sample(y.to(DEV), epsilon=eps.to(DEV))
        z = pr.sample(y.to(DEV), epsilon=eps.to(DEV), with_variance=False)
        assert same_bits(z, eps + pr.mean.detach().cpu()[y].unsqueeze(0))


# ---------------------------------------------------------------------------------------------- 2. the grid
def check_grid(x_in, x_out, cols, gf, gu):
    Rr, N, D, H, W = x_out.shape
    gf_h = gf.cpu().numpy()
    exact = grid64(x_in, x_out, cols)
    assert gf_h.shape == exact.shape and gf_h.dtype == np.float32
    for c, col in enumerate(cols):
        cell = gf_h[:, :, c * W:(c + 1) * W].reshape(D, N, H, W).transpose(1, 0, 2, 3)
        if col[0] != 'average':
            src = x_in if col[0] == 'input' else x_out[col[1]]
            assert same_bits(np.ascontiguousarray(cell), src), col
        else:
            want = exact[:, :, c * W:(c + 1) * W].reshape(D, N, H, W).transpose(1, 0, 2, 3)
            bound = average_bound(x_out, col[1], col[2])
            finite = np.isfinite(want)
            assert np.array_equal(np.isnan(cell), ~finite), col
            err = np.abs(cell.astype(np.float64) - want)[finite]
            assert (err <= bound[finite]).all(), (col, float((err / np.maximum(bound[finite], 1e-300)).max()))
            if col[1] == col[2]:
                assert same_bits(np.ascontiguousarray(cell), x_out[col[1]])          # an average over one row is the row
    if gu is not None:
        gu_h = gu.cpu()
        assert tuple(gu_h.shape) == (N * H, len(cols) * W, D) and gu_h.dtype == torch.uint8
        assert torch.equal(gu_h, quantise(gf_h))               # the expression on the kernel's own fp32 grid
        for c, col in enumerate(cols):
            if col[0] != 'average':                            # ... and, for the copies, on the sources
                src = x_in if col[0] == 'input' else x_out[col[1]]
                q = quantise(np.ascontiguousarray(src.transpose(1, 0, 2, 3)).reshape(D, N * H, W))
                assert torch.equal(gu_h[:, c * W:(c + 1) * W], q), col


@pytest.mark.parametrize('D', [1, 3])
@pytest.mark.parametrize('H,W', [(5, 7), (28, 28), (32, 32)])
@pytest.mark.parametrize('N', [1, 3])
def test_image_grid(D, H, W, N):
    from jvae_hip import ops
    for Rr in (2, 3, 130):
        x_in, x_out = grid_inputs(D, H, W, N, Rr)
        assert np.isnan(x_out[0]).any() and (x_out[0] < 0).any() and (x_out[0] > 1).any()
        cols = grid_columns_for(Rr)
        xi, xo = torch.from_numpy(x_in).to(DEV), torch.from_numpy(x_out).to(DEV)
        gf, gu = ops.image_grid(xi, xo, cols)
        check_grid(x_in, x_out, cols, gf, gu)
        gf2, none = ops.image_grid(xi, xo, ops.grid_columns(cols, xo.device), u8=False)
        none2, gu2 = ops.image_grid(xi, xo, cols, f32=False)
        assert none is None and none2 is None and same_bits(gf2, gf) and torch.equal(gu2, gu)
        no_in = [c for c in cols if c[0] != 'input']
        gf3, gu3 = ops.image_grid(None, xo, no_in)
        check_grid(None, x_out, no_in, gf3, gu3)


def test_image_grid_on_unaligned_tensors_takes_the_scalar_path():
    """W a multiple of 4 but the rows 4 bytes off a 16-byte boundary: the same values through the scalar path."""
    from jvae_hip import ops
    D, H, W, N, Rr = 3, 28, 28, 3, 3
    x_in, x_out = grid_inputs(D, H, W, N, Rr)
    cols = grid_columns_for(Rr)
    base = torch.zeros(x_out.size + 1, device=DEV)
    base[1:] = torch.from_numpy(x_out).to(DEV).reshape(-1)
    xo = base[1:].view(Rr, N, D, H, W)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    gf, gu = ops.image_grid(torch.from_numpy(x_in).to(DEV), xo, cols)
    check_grid(x_in, x_out, cols, gf, gu)


def test_image_grid_limits():
    from jvae_hip import ops
    x_in, x_out = grid_inputs(5, 5, 7, 2, 3)
    xi, xo = torch.from_numpy(x_in).to(DEV), torch.from_numpy(x_out).to(DEV)
    cols = grid_columns_for(3)
    with pytest.raises(ops.L.JvaeHipError, match='unsupported'):          # D = 5 with an 8-bit grid: ENOTSUP
        ops.image_grid(xi, xo, cols)
    gf, gu = ops.image_grid(xi, xo, cols, u8=False)                        # any D for the fp32 grid alone
    check_grid(x_in, x_out, cols, gf, None)
    for bad in ([('draw', 3)], [('draw', -1)], [('average', 0, 3)], [('average', 2, 1)], [('draw', 0), ('average', -1, 1)]):
        with pytest.raises(ops.L.JvaeHipError, match='invalid argument'):  # EINVAL, checked on the host copy of the specs
            ops.image_grid(xi, xo, bad, u8=False)
    with pytest.raises(ops.L.JvaeHipError, match='invalid argument'):      # a kind-0 column without x_in
        ops.image_grid(None, xo, [('input',)], u8=False)
    with pytest.raises(ops.L.JvaeHipError):
        ops.image_grid(xi, xo, [('mean', 0, 1)], u8=False)
    with pytest.raises(ops.L.JvaeHipError):
        ops.image_grid(xi, xo, [('draw', 0)] * 1025, u8=False)
    gf, _ = ops.image_grid(xi, xo, [('draw', 1)] * 1024, u8=False)
    assert same_bits(gf[:, :5, -7:], x_out[1, 0])


# ---------------------------------------------------------------------------------------------- 3. generate()
def build(name):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**get_case(name)['net'])
    load_det_state(net, seed=0)
    net.to(DEV)
    net.eval()
    net.job_number = int(load_golden(name, 'prior')['job_number'])
    net.training_parameters['set'] = load_golden(name, 'prior')['dset'].item()
    return net


def cells_of(grid, N, H, W):
    """(D, N H, Ncol W) -> (Ncol, N, D, H, W)"""
    D = grid.shape[0]
    return grid.reshape(D, N, H, -1, W).transpose(3, 1, 0, 2, 4)


@pytest.mark.parametrize('name', MODEL_CASES)
def test_generate_against_the_oracle_and_the_reference(name, monkeypatch):
    g = load_golden(name, 'prior')
    kw = get_case(name)['net']
    net = build(name)
    eps = torch.from_numpy(g['eps'])
    L, N, K = eps.shape
    x, z = net.generate(L=L, epsilon=eps.to(DEV), z_output=True)
    assert tuple(x.shape) == (L, N, *kw['input_shape']) and x.dtype == torch.float32 and x.is_cuda and not x.requires_grad
    sp, P = oracle_model(name)
    assert same_bits(z, eps + P['encoder.prior.mean'].unsqueeze(0))        # the reference's z + mean, bit for bit
    assert rel(x, oracle_decode(sp, P, z.cpu())) < RTOL
    D, H, W = kw['input_shape']
    assert rel(x, cells_of(g['grid'], N, H, W)) < RTOL
    monkeypatch.setenv('JVAE_EVAL_SLAB_ROWS', '7')
    calls = []
    orig = net._decode_rows
    monkeypatch.setattr(net, '_decode_rows', lambda t: (calls.append(t.shape[0]), orig(t))[1])
    slabbed = net.generate(L=L, epsilon=eps.to(DEV))
    rows = L * N
    assert calls == [7] * (rows // 7) + ([rows % 7] if rows % 7 else []) and same_bits(slabbed, x)
    monkeypatch.delenv('JVAE_EVAL_SLAB_ROWS')
    net.train()
    in_train = net.generate(L=L, epsilon=eps.to(DEV))
    assert net.training and net.latent_sampling == net._latent_samplings['train'] and same_bits(in_train, x)
    net.eval()
    net.generate(L=L, epsilon=eps.to(DEV))
    assert not net.training
    own = net.generate(y=torch.tensor([3, 3, 0], device=DEV), L=2, temperature=.5)
    assert tuple(own.shape) == (2, 3, *kw['input_shape']) and bool(torch.isfinite(own).all())


def test_generate_with_the_variance_of_a_diag_prior_and_refusals():
    from cvae import ClassificationVariationalNetwork as Net
    from module.priors import GaussianPrior
    net = build('e2_n8_L3')
    K, C = net.latent_dim, net.num_labels
    p = prior_inputs(K, C, 21)
    alt = GaussianPrior(K, var_dim='diag', num_priors=C, init_mean=1.)
    with torch.no_grad():
        alt.mean.copy_(torch.from_numpy(p['means']))
        alt._var_parameter.copy_(torch.from_numpy(p['diag']))
    alt.to(DEV)
    eps = torch.from_numpy(p['eps']).view(1, 21, K)
    x, z = net.generate(y=torch.from_numpy(p['y']).to(DEV), epsilon=eps.to(DEV), prior_variance=True, prior=alt, z_output=True)
    assert same_bits(z.reshape(21, K), torch_draw(p, 'diag', 1., True)) and tuple(x.shape) == (1, 21, 3, 32, 32)
    net.set_compute_dtype('bf16')
    with pytest.raises(NotImplementedError):
        net.generate()
    vib = Net(**get_case('b2_n8_vib')['net'])
    with pytest.raises(ValueError):
        vib.generate()


# ---------------------------------------------------------------------------------------------- 4. module.sample.sample()
def inject(monkeypatch, eps):
    """The next torch.randn of eps's shape returns eps (on the device asked for)."""
    def fake(*size, **kw):
        size = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        assert size == tuple(eps.shape), (size, tuple(eps.shape))
        return eps.clone().to(kw.get('device', 'cpu'))
    monkeypatch.setattr(torch, 'randn', fake)


@pytest.mark.parametrize('branch', ['prior', 'x'])
@pytest.mark.parametrize('name', MODEL_CASES)
def test_sample_against_the_reference(name, branch, monkeypatch, tmp_path):
    from module.sample import sample
    g = load_golden(name, branch)
    kw = get_case(name)['net']
    net = build(name)
    D, H, W = kw['input_shape']
    inject(monkeypatch, torch.from_numpy(g['eps']))
    root = os.path.join(str(tmp_path), '%j', 'samples')
    if branch == 'prior':
        args, more, directory = (net,), dict(N=20, L=10), 'generate'
    else:
        N = int(g['N'])
        x, y, _ = det_inputs(N, kw['input_shape'], kw['num_labels'], kw['test_latent_sampling'], kw['latent_dim'])
        args, directory = (net, x.to(DEV), y.to(DEV)), 'test'
        more = dict(N=N, L={'e2_n8_L3': 2, 'c1_n16_mlp': 10}[name])
        if NAMED[name]:
            more.update(in_classes=CLASS_NAMES, out_classes=CLASS_NAMES)
    images = sample(*args, root=root, directory=directory, **more)
    assert [im['name'] for im in images] == g['names'].tolist()
    grid = images[0]['tensor']
    assert grid.is_cuda and grid.dtype == torch.float32 and tuple(grid.shape) == g['grid'].shape
    assert rel(grid, g['grid']) < RTOL
    with_tex = [im for im in images if 'tex' in im]
    assert [im['name'] for im in with_tex] == g['cell_names'].tolist() and [im['tex'] for im in with_tex] == g['tex'].tolist()
    dir_path = os.path.join(str(tmp_path), '%06d' % int(g['job_number']), 'samples', directory)
    assert open(os.path.join(dir_path, 'params.tex')).read() == g['params_tex'].item()
    written = sorted(os.listdir(dir_path))
    assert written == sorted(['params.tex'] + [im['name'] + '.png' for im in images] + [im['name'] + '.tex' for im in with_tex])
    per_row = (len(images) - 1) // int(g['N'])
    for i, im in enumerate(images):
        t = im['tensor']
        assert set(im) <= {'name', 'tensor', 'tex'}
        assert t.untyped_storage().data_ptr() == grid.untyped_storage().data_ptr()          # a view into the one grid
        if i:
            r, c = divmod(i - 1, per_row)
            assert tuple(t.shape) == (D, H, W) and t.data_ptr() == grid[:, r * H:, c * W:].data_ptr()
        png = decode_png(open(os.path.join(dir_path, im['name'] + '.png'), 'rb').read())
        assert np.array_equal(png, quantise(t.cpu()).numpy()), im['name']
        if 'tex' in im:
            assert open(os.path.join(dir_path, im['name'] + '.tex')).read() == im['tex']
    # save=False: the same list, nothing written
    quiet_root = os.path.join(str(tmp_path), 'quiet', '%j')
    quiet = sample(*args, root=quiet_root, directory=directory, save=False, **more)
    assert [im['name'] for im in quiet] == [im['name'] for im in images] and same_bits(quiet[0]['tensor'], grid)
    assert not os.path.exists(os.path.join(str(tmp_path), 'quiet'))


def test_sample_refuses_a_model_without_decoder():
    from cvae import ClassificationVariationalNetwork as Net
    from module.sample import sample
    vib = Net(**get_case('b2_n8_vib')['net'])
    with pytest.raises(ValueError):
        sample(vib, save=False)
