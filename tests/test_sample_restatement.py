"""Image generation on the host (no GPU): an fp64 restatement of the two kernels of csrc/sample.hip (prior draws, image grid)
and of the grid layout of module/sample.py, held to what the REFERENCE's sample() returned (tools/gen_sample_golden.py ->
tests/golden/sample).  Checked: the names and their order, the column order, every grid value (1e-4 relative, the bar of the
evaluation goldens: the decoded rows come from the CPU oracle here), the average column, the .tex strings and params.tex.

Also here: the inputs the GPU test (tests/test_16_sample_gpu.py) reuses for the kernels, and the check that the yardstick of
the FULL mode - the error of fp32 torch.linalg.solve_triangular on the CPU against fp64 - is nonzero and small on them."""
import os

import numpy as np
import pytest
import torch

from oracle import jvae_oracle as O
from oracle.cases import get_case
from oracle.det_init import det_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sample')
MODEL_CASES = ['e2_n8_L3', 'c1_n16_mlp']
CLASS_NAMES = ['class-%d' % c for c in range(10)]          # tools/gen_sample_golden.py: given to the x branch of e2_n8_L3
NAMED = {'e2_n8_L3': True, 'c1_n16_mlp': False}
RTOL = 1e-4
U = 2. ** -24
_cache = {}


def load_golden(name, branch):
    key = (name, branch)
    if key not in _cache:
        g = np.load(os.path.join(GOLDEN, f'{name}_{branch}.npz'))
        _cache[key] = {k: g[k] for k in g.files}
    return _cache[key]


# ------------------------------------------------------------------------------------------ restatement of the kernels
def prior_draw64(eps, y, means, T, mode, t):
    """jvae_prior_sample_f32 in fp64 on fp32 inputs: eps (R, K), y (R,) or None, means (C, K), T by mode."""
    eps, means = np.asarray(eps, np.float64), np.asarray(means, np.float64)
    y = np.zeros(eps.shape[0], np.int64) if y is None else np.asarray(y)
    e = np.float64(np.float32(t)) * eps
    if mode == 'unit':
        u = e
    elif mode == 'scalar':
        u = e / np.asarray(T, np.float64)[y][:, None]
    elif mode == 'diag':
        u = e / np.asarray(T, np.float64)[y]
    else:
        tri = torch.from_numpy(np.tril(np.asarray(T, np.float64))[y])
        u = torch.linalg.solve_triangular(tri, torch.from_numpy(e).unsqueeze(-1), upper=False).squeeze(-1).numpy()
    return means[y] + u


def grid64(x_in, x_out, columns):
    """jvae_image_grid_f32 in fp64: x_in (N, D, H, W) or None, x_out (Rr, N, D, H, W) -> (D, N H, Ncol W)."""
    x_out = np.asarray(x_out, np.float64)
    Rr, N, D, H, W = x_out.shape
    grid = np.empty((D, N * H, len(columns) * W))
    for c, col in enumerate(columns):
        if col[0] == 'input':
            cell = np.asarray(x_in, np.float64)
        elif col[0] == 'draw':
            cell = x_out[col[1]]
        else:
            cell = x_out[col[1]:col[2] + 1].sum(0) / (col[2] - col[1] + 1)
        grid[:, :, c * W:(c + 1) * W] = cell.transpose(1, 0, 2, 3).reshape(D, N * H, W)
    return grid


def quantise(grid):
    """torchvision's save_image arithmetic on an fp32 tensor (D, h, w) -> (h, w, D) uint8; NaN gives 0."""
    t = torch.as_tensor(grid, dtype=torch.float32)
    q = t.mul(255).add_(0.5).clamp_(0, 255)
    q = torch.where(torch.isnan(q), torch.zeros_like(q), q)
    return q.permute(1, 2, 0).to(torch.uint8)


def layout(N, L, latent_sampling, x_branch):
    """Names of list_of_images after the grid, in order, and the column specs of a row (module/sample.py:47-51,88-153)."""
    wN = int(np.log10(N - 1)) + 1
    wL = 1 if L <= 1 else int(np.log10(L - 1)) + 1
    if not x_branch:
        return [f'x{r:0{wN}}_out_{l:0{wL}}' for r in range(N) for l in range(L)], [('draw', l) for l in range(L)]
    avg = latent_sampling > 1
    tails = ['in', 'out_mean'] + (['out_average'] if avg else []) + [f'out_{l:0{wL}}' for l in range(L)]
    cols = [('input',), ('draw', 0)] + ([('average', 1, latent_sampling)] if avg else []) + [('draw', 1 + l) for l in range(L)]
    return [f'x_{r:0{wN}}_{t}' for r in range(N) for t in tails], cols


# ------------------------------------------------------------------------------------------ the model side (CPU oracle)
def oracle_model(name):
    if ('model', name) not in _cache:
        sp = O.make_spec(**get_case(name)['net'])
        _cache['model', name] = (sp, {k: v.detach() for k, v in O.init_state(sp, seed=0).items()})
    return _cache['model', name]


def oracle_decode(sp, P, z):
    """The eval-mode decoder of oracle/jvae_oracle.py::evaluate on given latents z (..., K) -> (..., *input_shape)."""
    act = sp.get('act', 'relu')
    h = z.reshape(-1, z.shape[-1])
    with torch.no_grad():
        for j in range(len(sp['dec'])):
            h = O._act(torch.nn.functional.linear(h, P[f'decoder.{2 * j}.weight'], P[f'decoder.{2 * j}.bias']), act)
        if sp['imager']:
            xr = O.run_stack(P, 'imager', sp['imager'], sp['bn_d'], h.reshape(-1, *sp['imager_in']), sp['out_act'], False,
                             hidden_act=act)
        else:
            xr = O._act(torch.nn.functional.linear(h, P['imager.0.weight'], P['imager.0.bias']), sp['out_act'])
    return xr.reshape(*z.shape[:-1], *sp['input_shape'])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize('name', MODEL_CASES)
def test_prior_branch_restated(name):
    g = load_golden(name, 'prior')
    kw = get_case(name)['net']
    sp, P = oracle_model(name)
    L, N, K = g['eps'].shape
    assert (N, L) == (int(g['N']), int(g['L'])) == (kw['num_labels'], min(10, kw['test_latent_sampling']))
    names, cols = layout(N, L, kw['test_latent_sampling'], False)
    assert g['names'].tolist() == [f'grid-{N}x{L}'] + names and g['saved'].tolist() == [n + '.png' for n in g['names'].tolist()]
    assert g['cell_names'].size == 0                           # no .tex beside generated images
    y = np.tile(np.arange(N), L)
    z = prior_draw64(g['eps'].reshape(L * N, K), y, P['encoder.prior.mean'].numpy(), None, 'unit', 1.).reshape(L, N, K)
    z32 = (torch.from_numpy(g['eps']) + P['encoder.prior.mean'].unsqueeze(0)).numpy()
    assert np.array_equal(z.astype(np.float32), z32)           # one fp32 sum: the restatement rounds to the reference's z
    x_out = oracle_decode(sp, P, torch.from_numpy(z32))
    grid = grid64(None, x_out.numpy(), cols)
    assert grid.shape == g['grid'].shape and rel(grid, g['grid']) < RTOL
    assert g['params_tex'].item() == r'\def\modelsigma{%s}\def\modellatentdim{%d}\def\modeldset{%s}' % (
        '1->rmse[l] (1)' if name == 'e2_n8_L3' else '0.1', K, g['dset'].item())


@pytest.mark.parametrize('name', MODEL_CASES)
def test_x_branch_restated(name):
    g = load_golden(name, 'x')
    kw = get_case(name)['net']
    sp, P = oracle_model(name)
    Ls, N, L = kw['test_latent_sampling'], int(g['N']), int(g['L'])
    x, y, eps = det_inputs(N, kw['input_shape'], kw['num_labels'], Ls, kw['latent_dim'])
    assert np.array_equal(eps.numpy(), g['eps']) and L == min({'e2_n8_L3': 2, 'c1_n16_mlp': 10}[name], Ls)
    names, cols = layout(N, L, Ls, True)
    assert g['names'].tolist() == [f'grid-{N}x{L}'] + names and g['cell_names'].tolist() == names
    with torch.no_grad():
        x_reco, y_est, losses, _ = O.evaluate_all_classes(sp, P, x, eps)
    grid = grid64(x.numpy(), x_reco.numpy(), cols)
    assert grid.shape == g['grid'].shape and rel(grid, g['grid']) < RTOL
    D, H, W = kw['input_shape']
    assert np.array_equal(g['grid'][:, :, :W], x.numpy().transpose(1, 0, 2, 3).reshape(D, N * H, W))       # inputs are copies
    if Ls > 1:                                                 # the average column, against the reference's own draw columns
        draws = np.stack([g['grid'][:, :, (3 + l) * W:(4 + l) * W] for l in range(L)]).astype(np.float64)
        assert L < Ls                                          # the average runs over ALL Ls draws, more than the L shown
        assert rel(grid[:, :, 2 * W:3 * W], g['grid'][:, :, 2 * W:3 * W]) < RTOL
        assert np.abs(draws.mean(0) - g['grid'][:, :, 2 * W:3 * W]).max() > 1e-6
    # .tex: the class of the input, then the predicted class on every output of the row
    y_ = O.predict(losses, y_est, 'iws' if 'iws' in losses else 'closest')
    assert np.array_equal(np.asarray(y_), g['y_'])
    per_row = len(names) // N
    for i, (n, tex) in enumerate(zip(g['cell_names'].tolist(), g['tex'].tolist())):
        r, c = divmod(i, per_row)
        label = int(y[r]) if c == 0 else int(g['y_'][r])
        shown = CLASS_NAMES[label] if NAMED[name] else str(label)
        assert tex == r'\def\y{%s}' % shown, n


# ------------------------------------------------------------------------------------------ inputs of the kernel tests
PS_K, PS_C, PS_R, PS_T = [1, 5, 64, 200, 256], [1, 10], [1, 21, 650], [1., 0.7]


def prior_inputs(K, C, R, seed=0):
    """eps (R, K), y (R,), means (C, K) and the three factors; `full`: diagonal in [0.5, 2] with either sign kept positive,
    small off-diagonals (row sums of |off-diagonal| below 0.25: well conditioned), an upper triangle of junk the kernel must
    not read."""
    rng = np.random.default_rng([seed, K, C, R])
    eps = rng.standard_normal((R, K)).astype(np.float32)
    y = rng.integers(0, C, R).astype(np.int64)
    means = rng.normal(0., 2., (C, K)).astype(np.float32)
    scalar = rng.uniform(.5, 2., C).astype(np.float32)
    diag = rng.uniform(.5, 2., (C, K)).astype(np.float32)
    full = rng.uniform(-1., 1., (C, K, K)) * (.25 / max(K - 1, 1))
    full = np.tril(full, -1) + np.triu(rng.uniform(5., 9., (C, K, K)), 1)
    full[:, np.arange(K), np.arange(K)] = rng.uniform(.5, 2., (C, K))
    return dict(eps=eps, y=y, means=means, scalar=scalar, diag=diag, full=full.astype(np.float32))


def full_errors(p, t, with_y, z_kernel=None):
    """-> (max |z| of the fp64 solve, error of fp32 torch.linalg.solve_triangular on the CPU against it[, the kernel's])."""
    y = p['y'] if with_y else None
    exact = prior_draw64(p['eps'], y, p['means'], p['full'], 'full', t)
    idx = p['y'] if with_y else np.zeros(len(p['eps']), np.int64)
    tri = torch.from_numpy(p['full']).tril()[torch.from_numpy(idx)]
    rhs = (torch.tensor(t, dtype=torch.float32) * torch.from_numpy(p['eps'])).unsqueeze(-1)
    z32 = torch.from_numpy(p['means'])[torch.from_numpy(idx)] + torch.linalg.solve_triangular(tri, rhs, upper=False).squeeze(-1)
    out = (float(np.abs(exact).max()), float(np.abs(z32.double().numpy() - exact).max()))
    return out if z_kernel is None else out + (float(np.abs(np.asarray(z_kernel, np.float64) - exact).max()),)


@pytest.mark.parametrize('K', PS_K)
def test_the_full_mode_yardstick_is_nonzero_and_small(K):
    for C in PS_C:
        for R in PS_R:
            p = prior_inputs(K, C, R)
            for t in PS_T:
                for with_y in (False, True):
                    top, err = full_errors(p, t, with_y)
                    assert 0. < err / top < 1e-5, (K, C, R, t, with_y, err / top)


SPECIAL = np.float32([(k + .5) / 255 for k in range(256)])
SPECIAL = np.concatenate([SPECIAL, np.nextafter(SPECIAL, np.float32(-1)), np.nextafter(SPECIAL, np.float32(2)),
                          np.float32([-.22, -1e-9, -0., 0., 1., 1. + 2. ** -23, 1.7, 300., -300., np.nan])])


def grid_inputs(D, H, W, N, Rr, seed=0):
    """x_in (N, D, H, W), x_out (Rr, N, D, H, W) in about [-0.2, 1.2]; every value of SPECIAL (each 8-bit rounding point and
    its two fp32 neighbours, values outside [0, 1], a NaN) is planted in x_in and in x_out[0] when they have the room, else as
    many as fit; the rows an average may read stay finite."""
    rng = np.random.default_rng([seed, D, H, W, N, Rr])
    x_in = rng.uniform(-.2, 1.2, (N, D, H, W)).astype(np.float32)
    x_out = rng.uniform(-.2, 1.2, (Rr, N, D, H, W)).astype(np.float32)
    for t in (x_in, x_out[0]):
        flat = t.reshape(-1)
        n = min(flat.size, SPECIAL.size)
        flat[rng.permutation(flat.size)[:n]] = SPECIAL[::-1][:n]          # the NaN and the out-of-range values first
    return x_in, x_out


def grid_columns_for(Rr):
    """All three kinds: the input, row 0 (the special values), an average over ONE row, one over rows 1 .. Rr - 1, the last row."""
    return [('draw', 0), ('input',), ('average', 1, 1), ('average', 1, Rr - 1), ('draw', Rr - 1), ('average', 0, Rr - 1)]


def average_bound(x_out, a, b):
    """Sequential fp32 sum of n terms and one division: ((n - 1) u sum |x_l|) / n + u |avg|, elementwise (N, D, H, W)."""
    rows = np.asarray(x_out[a:b + 1], np.float64)
    n = b - a + 1
    return (n - 1) * U * np.abs(rows).sum(0) / n + U * np.abs(rows.sum(0) / n)


def test_restated_grid_and_quantisation_on_the_kernel_inputs():
    x_in, x_out = grid_inputs(3, 5, 7, 3, 3)
    cols = grid_columns_for(3)
    g = grid64(x_in, x_out, cols)
    assert g.shape == (3, 15, 42) and np.isnan(g).any()
    assert np.array_equal(g[:, 5:10, 7:14], x_in[1].astype(np.float64), equal_nan=True)
    assert np.array_equal(g[:, 5:10, 14:21], x_out[1, 1].astype(np.float64))                    # an average over one row is the row
    q = quantise(np.float32([[SPECIAL]])).reshape(-1).numpy()
    assert q.dtype == np.uint8 and q[-1] == 0 and q[-2] == 0 and q[-3] == 255
    exact = np.floor(np.clip(np.float32(SPECIAL[:-1] * np.float32(255)) + np.float32(.5), 0, 255))
    assert np.array_equal(q[:-1], exact.astype(np.uint8))
    assert set(q[:768].tolist()) == set(range(1, 256)) and 0 in q[768:]          # every level is reached


def test_png_writer_round_trip():
    """The standard-library PNG writer of module/sample.py: signature, IHDR, filter-0 rows that inflate to the pixels, CRCs."""
    import struct
    import zlib
    from module.sample import job_to_str, png_bytes
    rng = np.random.default_rng(5)
    for d in (1, 3):
        img = rng.integers(0, 256, (5, 7, d), dtype=np.uint8)
        assert np.array_equal(decode_png(png_bytes(img)), img)
    with pytest.raises(ValueError):
        png_bytes(np.zeros((2, 2, 2), np.uint8))
    data = png_bytes(np.zeros((1, 1, 1), np.uint8))
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and data[12:16] == b'IHDR' and data[-8:-4] == b'IEND'
    assert struct.unpack('>I', data[29:33])[0] == zlib.crc32(data[12:29]) & 0xffffffff
    assert job_to_str(42, 'a/%j/b') == 'a/000042/b' and job_to_str('x7', 'a/%j') == 'a/x7'


def decode_png(data):
    """Bytes of an 8-bit grey / RGB PNG with filter type 0 on every row -> (H, W, D) uint8 (zlib and struct only)."""
    import struct
    import zlib
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, head = 8, b'', None
    while pos < len(data):
        n, tag = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b'IHDR':
            head = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    w, h, depth, color, comp, filt, interlace = head
    assert (depth, comp, filt, interlace) == (8, 0, 0, 0) and color in (0, 2)
    d = 1 if color == 0 else 3
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * d)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, d)


def test_entry_points_refuse_malformed_arguments_on_the_host():
    """The argument checks of csrc/sample.hip run before anything is launched: -1 (EINVAL) / -2 (ENOTSUP) without a device.
    The pointers are never dereferenced on these paths (the specs are read from the HOST copy)."""
    import ctypes
    from jvae_hip import lib
    L = lib.load()
    p = ctypes.c_void_p(4096)                                  # any non-NULL address
    ps = L.jvae_prior_sample_f32
    assert ps(p, None, p, None, p, p, 4, 0, 1, 1., 0, None) == -1          # K < 1
    assert ps(p, None, p, None, p, p, 4, 1025, 1, 1., 0, None) == -1       # K > 1024
    assert ps(p, None, p, None, p, p, 4, 8, 0, 1., 0, None) == -1          # C < 1
    assert ps(p, None, p, None, p, p, 4, 8, 1, 1., 4, None) == -1          # unknown mode
    assert ps(p, None, p, None, p, p, 4, 8, 1, 1., 2, None) == -1          # a factor is needed beyond the unit mode
    assert ps(p, None, p, None, p, None, 4, 8, 1, 1., 0, None) == -1       # no status word
    assert ps(p, None, p, None, p, p, 0, 8, 1, 1., 0, None) == 0           # no rows: nothing to do

    def grid(specs, x_in=p, gf=p, gu=None, D=3, Rr=3, ncol=None):
        flat = [v for s in specs for v in s]
        host = (ctypes.c_int * max(len(flat), 1))(*flat)
        return L.jvae_image_grid_f32(x_in, p, p, host, len(specs) if ncol is None else ncol, gf, gu, 2, D, 5, 7, Rr, None)
    assert grid([(1, 3, 3)]) == -1 and grid([(1, -1, 0)]) == -1            # a outside [0, Rr)
    assert grid([(2, 0, 3)]) == -1 and grid([(2, 2, 1)]) == -1             # b outside, b < a
    assert grid([(3, 0, 0)]) == -1 and grid([(-1, 0, 0)]) == -1            # unknown kind
    assert grid([(0, 0, 0)], x_in=None) == -1                              # an input column without inputs
    assert grid([(1, 0, 0)], gf=None) == -1                                # nothing to write
    assert grid([(1, 0, 0)], ncol=0) == -1 and grid([(1, 0, 0)] * 1025) == -1
    assert grid([(1, 0, 0)], gu=p, D=5) == -2                              # the 8-bit grid holds at most 4 channels
    assert grid([(1, 3, 3)], gu=p, D=5) == -1                              # a malformed spec comes first
