"""Chained models on the host (no GPU): an fp64 numpy restatement of the two kernels of csrc/cascad.hip (the stage-pair mean
squared errors, the sequential Bayesian update), held to what the REFERENCE's module/cascad.py returned
(tools/gen_cascad_golden.py -> tests/golden/cascad).

The (M, L + 1, N, D) reconstructions of the chains are not stored (size), so the restatement meets the golden `mse` only
through the error the generator measured with these very functions on the reference's reconstructions: `mse_err`, the
reference's own fp32 error against fp64, is capped here (ERR_CAP) so that a bad regeneration cannot pass as rounding.  With
L = 3 and L = 32 no stored row can be recomputed from the stored stage inputs (they are single draws); the row order is
checked by construction on inputs whose rows are known in closed form, and on the golden rows by the triangle inequality that
the root mean squares of the three stage pairs of a cascade obey.  The golden `iterate_with_prior` is recomputed from its
seeded input.

Also here: the inputs the GPU test (tests/test_18_cascad_gpu.py) reuses, the ABI of the entry points and their argument
checks (they run before anything is launched, so without a device), the import surface of module.cascad and the save() /
load() round trip of a cascade of stub models."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cascad')
# chain: (case of oracle/cases.py, the load_det_state seed of every stage)
CHAINS = {'e2L3x3': ('e2_n8_L3', (0, 1, 2)), 'e3L32x2': ('e3_n8_L32', (0, 1))}
CHAIN_N = 8
CHAIN_TEMPS = [1, 5]
CHAIN_X_SEED = 1234                    # det_inputs seed of x; stage i draws its noise with seed CHAIN_X_SEED + 1 + i
ERR_CAP = 1e-6                         # upper cap of a stored reference error, relative to the tensor's magnitude: 8 fp32 ulps
ITER_GOLDEN = (3, 10, 65)              # (M, C, N) of the stored iterate_with_prior
# (M, L, N, D): one element; odd D below a chunk; the image size (12 chunks, 16-byte loads); D = 257 = a chunk + 1 with all 36
# rows; L beyond the four waves with N beyond a fold block's wave; many samples of a small D
MSE_SHAPES = [(1, 1, 1, 1), (2, 3, 7, 75), (3, 3, 8, 3072), (8, 2, 5, 257), (3, 16, 65, 192), (2, 1, 300, 12)]
ITER_SHAPES = [(1, 1, 1), (2, 2, 7), (3, 10, 65), (8, 128, 300), (5, 100, 1)]
_cache = {}


def load_golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        _cache[name] = {k: g[k] for k in g.files}
    return _cache[name]


def pairs(M):
    """The reference's row order: for i in 1..M: for j in 0..i-1 (stage 0 is the input)."""
    return [(i, j) for i in range(1, M + 1) for j in range(i)]


# ------------------------------------------------------------------------------------------ restatement of the kernels
def mse64(x, stages):
    """jvae_cascade_mse_f32 in fp64 on fp32 inputs: x (N, D), stages M x (L, N, D) -> (M (M + 1) / 2, N)."""
    s = [np.asarray(x, np.float64)[None]] + [np.asarray(r, np.float64) for r in stages]
    return np.stack([((s[i] - s[j]) ** 2).mean((0, 2)) for i, j in pairs(len(stages))])


def torch_mse(x, stages):
    """The reference's expressions in fp32 torch on the CPU: pair by pair, (x_i - x_j).pow(2).mean over draws and image."""
    s = [torch.from_numpy(np.ascontiguousarray(x)).unsqueeze(0)] + [torch.from_numpy(np.ascontiguousarray(r)) for r in stages]
    return torch.stack([(s[i] - s[j]).pow(2).mean((0, 2)) for i, j in pairs(len(stages))]).numpy()


def iter64(p):
    """jvae_iterate_prior_f32 in fp64: p (M, C, N) -> (M, C, N); a class sum of 0 gives NaN from that stage on."""
    p = np.asarray(p, np.float64)
    prior = np.full(p.shape[1:], 1. / p.shape[1])
    out = np.zeros_like(p)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(p.shape[0]):
            joint = p[i] * prior
            out[i] = joint / joint.sum(0, keepdims=True)
            prior = out[i]
    return out


def torch_iter(p):
    """The reference's iterate_with_prior written out in fp32 torch on the CPU."""
    p = torch.from_numpy(np.ascontiguousarray(p))
    M, C, N = p.shape
    prior = torch.ones(C, N) / C
    posterior = torch.zeros_like(p)
    for i in range(M):
        joint = p[i] * prior
        posterior[i] = joint / joint.sum(0, keepdim=True)
        prior = posterior[i]
    return posterior.numpy()


# ------------------------------------------------------------------------------------------ inputs of the kernel tests
def mse_inputs(M, L, N, D, seed=0):
    """x (N, D) in [0, 1) and M stages (L, N, D): each the stage before plus a draw-dependent error of a size of its own, as
    the reconstructions of a cascade are."""
    rng = np.random.default_rng([seed, M, L, N, D, 53])
    x = rng.uniform(0., 1., (N, D)).astype(np.float32)
    stages, prev = [], x[None].repeat(L, 0)
    for i in range(M):
        prev = (prev + (.05 + .03 * i) * rng.standard_normal((L, N, D))).astype(np.float32)
        stages.append(prev)
    return x, stages


def iter_inputs(M, C, N, seed=0):
    """Class likelihoods (M, C, N): exponentials of Gaussian logits, so that a few classes carry each sample."""
    rng = np.random.default_rng([seed, M, C, N, 59])
    return np.exp(2. * rng.standard_normal((M, C, N))).astype(np.float32)


# ------------------------------------------------------------------------------------------ restatement against itself
def test_row_order_by_construction():
    """Stage i = x + i c: row (i, j) is ((i - j) c)^2 exactly (powers of two), whatever L, N, D."""
    x = np.zeros((3, 5), np.float32)
    stages = [np.full((2, 3, 5), i * .5, np.float32) for i in range(1, 5)]
    want = np.array([((i - j) * .5) ** 2 for i, j in pairs(4)])
    assert pairs(3) == [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
    got = mse64(x, stages)
    assert got.shape == (10, 3) and np.array_equal(got, want[:, None].repeat(3, 1))
    assert np.array_equal(torch_mse(x, stages), got.astype(np.float32))


@pytest.mark.parametrize('shape', MSE_SHAPES, ids=str)
def test_mse_restatement_and_torch_agree(shape):
    x, stages = mse_inputs(*shape)
    exact = mse64(x, stages)
    M, L, N, D = shape
    assert exact.shape == (M * (M + 1) // 2, N) and np.isfinite(exact).all() and (exact > 0).all()
    assert np.abs(torch_mse(x, stages) - exact).max() <= 1e-5 * np.abs(exact).max()


@pytest.mark.parametrize('shape', ITER_SHAPES, ids=str)
def test_iterate_restatement_and_torch_agree(shape):
    p = iter_inputs(*shape)
    exact = iter64(p)
    assert np.allclose(exact.sum(1), 1., rtol=0, atol=1e-12)
    assert np.abs(torch_iter(p) - exact).max() <= 1e-5
    # the constant prior of the first stage cancels: stage 0 is the normalised likelihood
    assert np.allclose(exact[0], p[0].astype(np.float64) / p[0].astype(np.float64).sum(0), rtol=1e-14, atol=0)
    # a zero stage: NaN from that stage on in that sample only
    if shape[0] > 1 and shape[2] > 1:
        q = p.copy()
        q[1, :, 0] = 0.
        z = iter64(q)
        assert np.isfinite(z[0]).all() and np.isnan(z[1:, :, 0]).all() and np.array_equal(z[:, :, 1:], exact[:, :, 1:])


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('chain', list(CHAINS))
def test_chain_goldens(chain):
    from oracle.cases import get_case
    g = load_golden(chain)
    name, seeds = CHAINS[chain]
    kw = get_case(name)['net']
    M, N, C, K = len(seeds), CHAIN_N, kw['num_labels'], kw['latent_dim']
    L, D = kw['test_latent_sampling'], int(np.prod(kw['input_shape']))
    for i in range(M):
        assert g[f'eps{i}'].shape == (L + 1, N, K) and g[f'eps{i}'].dtype == np.float32
    assert g['stage_in'].shape == (M, N, D) and g['stage_in'].dtype == np.float32
    assert g['y_'].shape == (M, N, C)
    P, Q = M * (M + 1) // 2, M * (M - 1) // 2
    assert g['mse'].shape == (P, N) and g['mse'].dtype == np.float32 and np.isfinite(g['mse']).all() and (g['mse'] > 0).all()
    for T in CHAIN_TEMPS:
        assert g[f'Im-{T}'].shape == (Q, N) and np.isfinite(g[f'Im-{T}']).all()
    for k in ('kl', 'zdist', 'var_kl', 'total', 'iws'):
        assert g['loss.' + k].shape == (M, C, N), k
    for k in ('wmse', 'cross_x', 'dzdist'):
        assert g['loss.' + k].shape == (M, N), k
    assert all(g[k].shape == (M,) for k in g if k.startswith('measure.')) and 'measure.rmse' in g
    # the yardstick of the GPU test: the reference's own fp32 error, and its cap
    top = float(np.abs(g['mse']).max())
    assert 0. < float(g['mse_err']) < ERR_CAP * top, float(g['mse_err']) / top
    # root mean squares over (l, d) are distances: every triple of stages obeys the triangle inequality in the stored order
    rms = {ij: np.sqrt(g['mse'][p].astype(np.float64)) for p, ij in enumerate(pairs(M))}
    for a in range(M + 1):
        for b in range(a):
            for c in range(b):
                sides = [rms[(a, b)], rms[(a, c)], rms[(b, c)]]
                for s in range(3):
                    assert (sides[s] <= sum(sides) - sides[s] + 1e-6).all(), (a, b, c)
    # stage_in[k] is the first draw of stage k (k = 0: x itself), one of the L terms whose mean is row (k, k - 1)
    for k in range(1, M):
        first = ((g['stage_in'][k].astype(np.float64) - g['stage_in'][k - 1]) ** 2).mean(-1)
        assert (first <= L * g['mse'][pairs(M).index((k, k - 1))] * (1 + 1e-5)).all() and (first > 0).all()


def test_iterate_golden():
    g = load_golden('iterate')
    p = iter_inputs(*ITER_GOLDEN)
    exact = iter64(p)
    assert g['posterior'].shape == ITER_GOLDEN and g['posterior'].dtype == np.float32
    assert 0. < float(g['err']) < ERR_CAP
    assert np.abs(g['posterior'] - exact).max() <= float(g['err'])
    assert np.array_equal(g['posterior'], torch_iter(p)) or np.abs(g['posterior'] - torch_iter(p)).max() <= 2. ** -23


# ------------------------------------------------------------------------------------------ ABI and argument checks
NEW_SYMBOLS = ('jvae_cascade_mse_workspace_bytes', 'jvae_cascade_mse_f32', 'jvae_iterate_prior_f32')


def test_new_symbols_are_exported_and_declared():
    import ctypes
    import re
    from jvae_hip import lib
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(repo, 'include', 'jvae_hip.h')).read(), flags=re.S)
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name + ' is not exported'
        proto = re.search(r'\b' + name + r'\s*\(([^;{]*?)\)\s*;', src, flags=re.S)
        assert proto, name + ' is not declared in include/jvae_hip.h'
        assert name in lib._SIGS and len(lib._SIGS[name][1]) == len(proto.group(1).split(','))


def test_entry_points_refuse_malformed_arguments_on_the_host():
    """-1 (EINVAL) / -3 (EWORKSPACE) before anything is launched: no device is needed, no pointer is dereferenced."""
    import ctypes
    from jvae_hip import lib
    L = lib.load()
    p = ctypes.c_void_p(4096)
    srcs = (ctypes.c_void_p * 9)(*([4096] * 9))
    holes = (ctypes.c_void_p * 2)(4096, None)
    odd = (ctypes.c_void_p * 2)(4096, 4098)

    def mse(x=p, s=srcs, M=3, out=p, Ls=2, N=4, D=10, ws=p, nbytes=1 << 20):
        return L.jvae_cascade_mse_f32(x, s, M, out, Ls, N, D, ws, nbytes, None)
    assert mse(x=None) == -1 and mse(s=None) == -1 and mse(out=None) == -1 and mse(ws=None) == -1 and mse(s=holes, M=2) == -1
    assert mse(M=0) == -1 and mse(M=9) == -1 and mse(Ls=0) == -1 and mse(N=-1) == -1 and mse(D=0) == -1
    assert mse(s=odd, M=2) == -1 and mse(x=ctypes.c_void_p(4097)) == -1 and mse(ws=ctypes.c_void_p(4100)) == -1
    assert mse(N=1 << 24) == -1 and mse(D=65535 * 256 + 1) == -1
    assert mse(N=(1 << 24) - 1, D=257) == -1 and mse(N=1 << 22, D=1024) == -1        # N * chunks * 256 threads reach 2^32
    assert mse(N=0) == 0 and mse(N=0, ws=None) == 0
    assert L.jvae_cascade_mse_workspace_bytes(3, 7, 257) == 8 * 2 * 6 * 7 and L.jvae_cascade_mse_workspace_bytes(9, 7, 257) == 0
    assert mse(M=3, N=7, D=257, nbytes=8 * 2 * 6 * 7 - 1) == -3

    def it(q=p, out=ctypes.c_void_p(8192), M=2, C=3, N=4):
        return L.jvae_iterate_prior_f32(q, out, M, C, N, None)
    assert it(q=None) == -1 and it(out=None) == -1 and it(out=p) == -1
    assert it(M=0) == -1 and it(M=9) == -1 and it(C=0) == -1 and it(C=129) == -1 and it(N=-1) == -1 and it(N=0) == 0


# ------------------------------------------------------------------------------------------ the public interface
class Stub(torch.nn.Module):
    """What CascadModels reads of a model, without a network."""

    def __init__(self, job_number, saved_dir=None, **over):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(2))
        self.input_shape, self.input_dim, self.num_labels, self.latent_sampling = (3, 4, 4), 3, 10, 5
        self.training_parameters = {'set': 'letters'}
        self.job_number, self.saved_dir = job_number, saved_dir
        self.__dict__.update(over)

    @classmethod
    def load(cls, dir_name, *a, **kw):
        return cls(int(os.path.basename(dir_name)), saved_dir=dir_name)


def test_surface_and_no_cpu_path():
    from jvae_hip import JvaeHipError, ops
    from module import cascad
    for name in ('CascadModels', 'iterate_with_prior', 'record_sets'):
        assert hasattr(cascad, name), name
    x = torch.rand(4, 6)
    for call in (lambda: ops.cascade_mse(x, [x.view(1, 4, 6)]), lambda: ops.iterate_prior(torch.rand(2, 3, 4)),
                 lambda: cascad.iterate_with_prior(torch.rand(2, 3, 4)),
                 lambda: ops.cascade_mse(x, [x.view(1, 4, 6)] * 9), lambda: ops.iterate_prior(torch.rand(9, 3, 4)),
                 lambda: ops.iterate_prior(torch.rand(2, 129, 4)), lambda: ops.cascade_mse(x, [])):
        with pytest.raises(JvaeHipError):
            call()


def test_cascade_of_stubs_holds_its_models_and_refuses_by_name():
    from module.cascad import CascadModels
    a, b = Stub(11), Stub(12)
    m = CascadModels(a, b)
    assert len(m) == 2 and m._models == (a, b) and dict(m.named_children()) == {'0': a, '1': b}
    assert len(list(m.parameters())) == 2 and m.predict_methods == ['iter'] and m.testing == {} and m.ood_results == {}
    assert m.input_shape == (3, 4, 4) and m.input_dim == 3 and m.num_labels == 10 and m.latent_sampling == 5
    assert m.training_parameters is b.training_parameters and m.saved_dir is None
    m.eval()
    assert not a.training and not b.training
    with pytest.raises(ValueError, match='input_shape'):
        CascadModels(a, Stub(13, input_shape=(1, 4, 4)))
    with pytest.raises(ValueError, match='latent_sampling'):
        CascadModels(a, Stub(13, latent_sampling=2))
    with pytest.raises(NotImplementedError, match='coded labels'):
        CascadModels(a, Stub(13, y_is_coded=True))
    with pytest.raises(NotImplementedError, match='categorical'):
        CascadModels(Stub(13, output_distribution='categorical'), a)
    with pytest.raises(ValueError, match='decoder'):
        CascadModels(a, Stub(13, is_vib=True, x_is_generated=False))
    with pytest.raises(NotImplementedError, match='without labels'):
        m.evaluate(torch.zeros(2, 3, 4, 4), torch.zeros(2, dtype=torch.int64))
    # with z_output every prior is looked at before any stage runs (the stubs could not run one)
    import types
    a.encoder = types.SimpleNamespace(prior=types.SimpleNamespace(distribution='gaussian', conditional=True))
    for prior, word in ((types.SimpleNamespace(distribution='gaussian', conditional=False), 'non-conditional gaussian'),
                        (types.SimpleNamespace(distribution='uniform', conditional=True), 'uniform')):
        b.encoder = types.SimpleNamespace(prior=prior)
        with pytest.raises(NotImplementedError, match='model 1 has a ' + word):
            m.evaluate(torch.zeros(2, 3, 4, 4), z_output=True)


def test_save_and_load_round_trip_the_three_files(tmp_path):
    from module.cascad import CascadModels
    dirs = [str(tmp_path / 'jobs' / str(j)) for j in (11, 12, 13)]
    m = CascadModels(*[Stub(j, saved_dir=d) for j, d in zip((11, 12, 13), dirs)])
    m.testing = {0: {'iter': {'n': 100, 'epochs': 0, 'accuracy': .5}}}
    m.ood_results = {0: {'other': {'iws': {'auc': .75}}}}
    where = m.save(job_dir=str(tmp_path / 'cascad-jobs'))
    assert where == m.saved_dir == os.path.join(str(tmp_path / 'cascad-jobs'), 'letters', '11-12-13')
    assert sorted(os.listdir(where)) == ['ood.json', 'params.json', 'test.json']
    assert json.load(open(os.path.join(where, 'params.json'))) == {'0': dirs[0], '1': dirs[1], '2': dirs[2]}
    back = CascadModels.load(where, model_class=Stub)
    assert [s.job_number for s in back._models] == [11, 12, 13] and [s.saved_dir for s in back._models] == dirs
    assert back.testing == m.testing and back.ood_results == m.ood_results and back.saved_dir == where
    os.remove(os.path.join(where, 'ood.json'))
    assert CascadModels.load(where, model_class=Stub).ood_results == {}
    other = m.save(dir_name=str(tmp_path / 'elsewhere'))
    assert other == str(tmp_path / 'elsewhere') and os.path.exists(os.path.join(other, 'params.json'))
