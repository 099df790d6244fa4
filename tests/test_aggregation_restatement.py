"""Model ensembles on the host (no GPU): an fp64 numpy restatement of the three kernels of csrc/aggregate.hip (class posteriors of
latent draws, pairwise latent mutual information, score aggregation), held to what the REFERENCE's module/aggregation.py
returned (tools/gen_aggregation_golden.py -> tests/golden/aggregation): the restatement agrees with every stored fp32 result
within the error that result itself shows against fp64 on the same inputs.  The generator takes that error with these very
functions, so the agreement pins golden files and restatement to each other; what keeps a bad regeneration from widening the
GPU test's bars is the cap on every stored error (ERR_CAP, SCORE_ERR_CAP).

Also here: the inputs the GPU test (tests/test_17_aggregation_gpu.py) reuses, the ABI of the three entry points and their
argument checks (they run before anything is launched, so without a device), and the import surface of module.aggregation."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'aggregation')
PAIRS = {'e2L3_e2L3': ('e2_n8_L3', 'e2_n8_L3'), 'e2L3_e2L16': ('e2_n8_L3', 'e2_n16_L16'), 'e3L32_e3L32': ('e3_n8_L32', 'e3_n8_L32')}
PAIR_N = 8
PAIR_SEEDS = (0, 1)                    # load_det_state seeds of the two models
PAIR_EPS_SEEDS = (1234, 4321)          # det_inputs seeds of the two noises (x: the first)
MI_TEMPS = [1, 5]
AGG_TEMPS = [-1, 1, 5, 100]
NAN_TEMPS = [None, -1, 0]
# (E, C, N): every C with every N once, every E with every C
SCORE_CASES = [(1, 2, 1), (2, 2, 7), (3, 2, 65), (5, 2, 300), (2, 10, 1), (3, 10, 7), (5, 10, 65), (1, 10, 300), (3, 100, 1),
               (5, 100, 7), (1, 100, 65), (2, 100, 300)]
KEEP_COLS = 8                          # columns of every posterior the golden keeps (the maxima and their classes: all)
GAP = 1e-3
ERR_CAP = 1e-6                         # upper cap of a stored reference error, relative to the tensor's magnitude: 8 fp32 ulps
SCORE_ERR_CAP = 1e-5                   # ... of a score slot
_cache = {}


def load_golden(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        _cache[name] = {k: g[k] for k in g.files}
    return _cache[name]


def is_nan_temp(t):
    return t is None or t in (-1, 0)


# ------------------------------------------------------------------------------------------ restatement of the kernels
def log_det64(T, var_dim, K):
    T = np.asarray(T, np.float64)
    if var_dim == 'scalar':
        return -2 * K * np.log(T)
    if var_dim == 'diag':
        return -2 * np.log(np.abs(T)).sum(-1)
    return -2 * np.log(np.abs(np.diagonal(T, axis1=-2, axis2=-1))).sum(-1)


def logp64(z, means, T, log_det, var_dim):
    """jvae_class_posterior_f32's logp in fp64 on fp32 inputs: z (R, K), means (C, K), T by var_dim, log_det (C,) -> (C, R)."""
    z, means, T = np.asarray(z, np.float64), np.asarray(means, np.float64), np.asarray(T, np.float64)
    K = z.shape[-1]
    d = z[None] - means[:, None]
    if var_dim == 'scalar':
        wd = d * T[:, None, None]
    elif var_dim == 'diag':
        wd = d * T[:, None, :]
    else:
        wd = np.einsum('ckj,crj->crk', np.tril(T), d)
    return -K / 2 * np.log(2 * np.pi) - (wd ** 2).sum(-1) / 2 - np.asarray(log_det, np.float64)[:, None] / 2


def softmax64(logits, temps):
    """(C, ...) -> (nT, C, ...): softmax over axis 0 of logits / T, the logits themselves for a temperature of NAN_TEMPS."""
    logits = np.asarray(logits, np.float64)
    out = []
    for t in temps:
        if is_nan_temp(t):
            out.append(logits)
            continue
        x = logits / t
        e = np.exp(x - x.max(0))
        out.append(e / e.sum(0))
    return np.stack(out)


def im64(P0, P1):
    """jvae_latent_mi_f32 in fp64: P0 (nT, C, L0, N), P1 (nT, C, L1, N) -> (nT, N); log 0 = -inf."""
    P0, P1 = np.asarray(P0, np.float64), np.asarray(P1, np.float64)
    with np.errstate(divide='ignore'):
        return np.log(np.einsum('tcan,tcbn->tabn', P0, P1)).mean((1, 2))


def agg64(sources, mode, f, temps, C=None):
    """jvae_aggregate_scores_f32 in fp64 -> (post (nT, C, N), a (C, N) or None)."""
    E = len(sources)
    if mode == 'vote':
        a = sum((np.asarray(s)[None] == np.arange(C)[:, None]).astype(np.float64) for s in sources) / E
        return np.stack([a] * len(temps)), a
    x = f * np.stack([np.asarray(s, np.float64) for s in sources])
    if mode == 'mean_soft':
        return np.stack([softmax64(xe, temps) for xe in x]).mean(0), None
    if mode == 'mean':
        m = x.max(0)
        a = m + np.log(np.exp(x - m).mean(0))
    else:
        a = x.sum(0)
    return softmax64(a, temps), a


def argmax_lowest(row):
    """Lowest index of the maximum over axis 0 (numpy's rule)."""
    return np.argmax(row, axis=0)


def top_two_gap(row):
    if row.shape[0] < 2:
        return np.full(row.shape[1:], np.inf)
    s = np.sort(row, axis=0)
    return s[-1] - s[-2]


# ------------------------------------------------------------------------------------------ inputs of the kernel tests
CP_K, CP_C, CP_R = [1, 5, 64, 200], [1, 2, 10, 128], [1, 7, 65, 300]
MI_L, MI_C, MI_N = [(1, 1), (3, 5), (16, 3), (128, 128), (7, 18)], [1, 10, 128], [1, 7, 65]


def posterior_inputs(K, C, R, seed=0):
    """z (R, K), means (C, K), the three factors (full: an upper triangle of junk the kernel must not read) and their fp32
    log-determinants as GaussianPrior.log_det_per_class computes them."""
    rng = np.random.default_rng([seed, K, C, R, 17])
    z = (1.5 * rng.standard_normal((R, K))).astype(np.float32)
    means = rng.normal(0., 1., (C, K)).astype(np.float32)
    scalar = rng.uniform(.5, 2., C).astype(np.float32)
    diag = (rng.uniform(.5, 2., (C, K)) * rng.choice([-1., 1.], (C, K))).astype(np.float32)
    full = rng.uniform(-1., 1., (C, K, K)) * (.25 / max(K - 1, 1))
    full = np.tril(full, -1) + np.triu(rng.uniform(5., 9., (C, K, K)), 1)
    full[:, np.arange(K), np.arange(K)] = rng.uniform(.5, 2., (C, K)) * rng.choice([-1., 1.], (C, K))
    p = dict(z=z, means=means, scalar=scalar, diag=diag, full=full.astype(np.float32))
    t = torch.from_numpy(p['full']).tril()
    p['log_det_scalar'] = (-2 * K * torch.from_numpy(scalar).log()).numpy()
    p['log_det_diag'] = (-2 * torch.from_numpy(diag).abs().log().sum(-1)).numpy()
    p['log_det_full'] = (-2 * torch.diagonal(t, dim1=-2, dim2=-1).abs().log().sum(-1)).numpy()
    return p


def torch_logp(p, var_dim, temps):
    """The fp32 torch expressions on the CPU (the yardstick where no golden exists): GaussianPrior.log_density's formula
    with the quadratic form written out, and (logp / T).softmax(0)."""
    z, m = torch.from_numpy(p['z']), torch.from_numpy(p['means'])
    K = z.shape[1]
    d = z.unsqueeze(0) - m.unsqueeze(1)
    if var_dim == 'scalar':
        wd = d * torch.from_numpy(p['scalar'])[:, None, None]
    elif var_dim == 'diag':
        wd = d * torch.from_numpy(p['diag'])[:, None, :]
    else:
        wd = torch.matmul(torch.from_numpy(p['full']).tril().unsqueeze(1), d.unsqueeze(-1)).squeeze(-1)
    u = wd.pow(2).sum(-1)
    logp = -np.log(2 * np.pi) * K / 2 - u / 2 - torch.from_numpy(p['log_det_' + var_dim]).unsqueeze(-1) / 2
    post = torch.stack([logp.clone() if is_nan_temp(t) else (logp / t).softmax(0) for t in temps])
    return logp.numpy(), post.numpy()


def mi_inputs(C, L0, L1, N, nT=2, seed=0):
    """Two stacks of class posteriors (nT, C, L, N): soft-maxes of Gaussian logits, sharper in the first slot."""
    rng = np.random.default_rng([seed, C, L0, L1, N, 29])
    out = []
    for L in (L0, L1):
        logits = torch.from_numpy((4. * rng.standard_normal((C, L, N))).astype(np.float32))
        out.append(torch.stack([(logits / t).softmax(0) for t in (1, 5, 25)[:nT]]).numpy())
    return out


def torch_im(P0, P1):
    """The reference's arithmetic in fp32 torch on the CPU: the broadcast product, sum over classes, log, mean over the pairs."""
    a, b = torch.from_numpy(P0), torch.from_numpy(P1)
    return (a.unsqueeze(3) * b.unsqueeze(2)).sum(1).log().mean((1, 2)).numpy()


def score_inputs(E, C, N, seed=0):
    """Synthetic recorder tensors of E models: iws about -1e3, zdist and kl positive tens, each (C, N) fp32, and the models'
    votes (the argmax of their iws).  A column whose aggregated row (fp64: log_mean_exp of iws, -sum zdist / 2, the mean of
    -kl) has a top-two gap below GAP of its magnitude is redrawn, so the predicted class of every column is beyond rounding."""
    rng = np.random.default_rng([seed, E, C, N, 41])

    def draw(n):
        return dict(iws=(-1000. + 30. * rng.standard_normal((E, C, n))).astype(np.float32),
                    zdist=np.abs(30. + 8. * rng.standard_normal((E, C, n))).astype(np.float32),
                    kl=np.abs(20. + 5. * rng.standard_normal((E, C, n))).astype(np.float32))
    s = draw(N)
    for _ in range(100):
        close = np.zeros(N, bool)
        for key, mode, f in (('iws', 'mean', 1.), ('zdist', 'joint', -.5), ('kl', 'mean_soft', -1.)):
            post, a = agg64(list(s[key]), mode, f, [-1])
            row = post[0]
            close |= top_two_gap(row) < GAP * np.abs(row).max(0)
        if not close.any():
            break
        fresh = draw(int(close.sum()))
        for key in s:
            s[key][:, :, close] = fresh[key]
    else:
        raise AssertionError('columns with close maxima remain')
    out = {k: [np.ascontiguousarray(v[e]) for e in range(E)] for k, v in s.items()}
    out['y'] = [argmax_lowest(v).astype(np.int64) for v in out['iws']]
    return out


SCORE_MODES = (('iws', 'mean', 1.), ('zdist', 'joint', -.5), ('kl', 'mean_soft', -1.))


def score_name(E, C, N):
    return f'E{E}_C{C}_N{N}'


# ------------------------------------------------------------------------------------------ goldens
def prior_of(name, seed):
    """(means (C, K), T (C,), log_det (C,)) of a drop-in model's prior under load_det_state(seed): fp32 numpy."""
    from oracle.cases import get_case
    from oracle.det_init import det_tensor
    kw = get_case(name)['net']
    C, K = kw['num_labels'], kw['latent_dim']
    assert kw['prior'].get('var_dim', 'scalar') == 'scalar'
    means = det_tensor('encoder.prior.mean', (C, K), seed)
    T = det_tensor('encoder.prior._var_parameter', (C,), seed)
    return means.numpy(), T.numpy(), (-2 * K * T.log()).numpy()


@pytest.mark.parametrize('pair', list(PAIRS))
def test_latent_goldens_restated(pair):
    g, gl = load_golden(pair), load_golden(pair + '_logp')
    for i, name in enumerate(PAIRS[pair]):
        means, T, log_det = prior_of(name, PAIR_SEEDS[i])
        z = g[f'z{i}']
        L, N, K = z.shape
        assert N == PAIR_N and g[f'eps{i}'].shape == (L + 1, N, K)
        logp = logp64(z.reshape(L * N, K), means, T, log_det, 'scalar').reshape(-1, L, N)
        ref = gl[f'logp{i}']
        assert ref.dtype == np.float32 and ref.shape == logp.shape
        assert np.abs(logp - ref).max() <= float(g[f'logp{i}_err']) and 0. < float(g[f'logp{i}_err']) < 1e-5 * np.abs(ref).max()
    P = [softmax64(gl[f'logp{i}'], MI_TEMPS) for i in range(2)]
    Im = im64(P[0], P[1])
    for j, t in enumerate(MI_TEMPS):
        assert np.abs(Im[j] - g[f'Im_{t}']).max() <= float(g[f'Im_{t}_err']), (t, np.abs(Im[j] - g[f'Im_{t}']).max())
        # the stored errors are the GPU test's yardsticks: a regeneration that inflates them must not pass (8 fp32 ulps)
        assert 0. < float(g[f'Im_{t}_err']) < ERR_CAP * np.abs(g[f'Im_{t}']).max()
        assert all(0. < float(g[f'P{i}_err'][j]) < ERR_CAP for i in range(2))
        assert g[f'Im_{t}'].dtype == np.float32 and g[f'Im_{t}'].shape == (PAIR_N,) and np.isfinite(g[f'Im_{t}']).all()
        assert 0. < float(g[f'im_sens_{t}']) < 1e-2
    mean = gl['logp0'].astype(np.float64).mean(1)
    gap = top_two_gap(mean)
    assert np.allclose(gap, g['y_gap'], rtol=1e-4, atol=1e-6)
    sure = g['y_gap'] > 2 * 1e-4 * np.abs(gl['logp0']).max()
    assert np.array_equal(argmax_lowest(mean)[sure], g['y_'][sure])
    if pair != 'e3L32_e3L32':
        assert sure.all()


@pytest.mark.parametrize('case', SCORE_CASES, ids=lambda c: score_name(*c))
def test_score_goldens_restated(case):
    E, C, N = case
    g = load_golden('scores')
    s = score_inputs(E, C, N)
    name = score_name(E, C, N)
    keep = min(N, KEEP_COLS)
    for key, mode, f in SCORE_MODES:
        post, a = agg64(s[key], mode, f, AGG_TEMPS)
        ref = g[f'{name}.{mode}.post']
        assert ref.shape == (len(AGG_TEMPS), C, keep) and ref.dtype == np.float32
        for j, t in enumerate(AGG_TEMPS):
            err = float(g[f'{name}.{mode}.err'][j])
            assert np.abs(post[j][:, :keep] - ref[j]).max() <= err, (mode, t)
            # yardsticks of the GPU test: the soft-max slots carry the rounding of a / T through exp (a about 1e3: 4e-6 seen)
            assert err <= SCORE_ERR_CAP * float(g[f'{name}.{mode}.top'][j]), (mode, t, err)
            assert np.isclose(float(g[f'{name}.{mode}.top'][j]), np.abs(post[j]).max(), rtol=1e-12)
        assert np.array_equal(argmax_lowest(post[0]), g[f'{name}.{mode}.y'])
        gap = top_two_gap(post[0])
        assert (gap >= GAP * np.abs(post[0]).max(0)).all()
        if mode == 'mean':
            assert np.abs(a.max(0) - g[f'{name}.log_p_x_y']).max() <= float(g[f'{name}.log_p_x_y_err'])
            assert float(g[f'{name}.log_p_x_y_err']) < ERR_CAP * np.abs(a).max()
    post, a = agg64(s['y'], 'vote', None, [None], C=C)
    assert np.array_equal(a[:, :keep].astype(np.float32), g[f'{name}.vote.post'])          # count / E: the same fp32 value
    assert np.array_equal(argmax_lowest(a), g[f'{name}.vote.y'])


# ------------------------------------------------------------------------------------------ ABI and argument checks
NEW_SYMBOLS = ('jvae_class_posterior_f32', 'jvae_latent_mi_workspace_bytes', 'jvae_latent_mi_f32', 'jvae_aggregate_scores_f32')


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
    temps = (ctypes.c_float * 16)(*([1.] * 16))
    many = (ctypes.c_float * 17)(*([1.] * 17))

    def cp(z=p, means=p, T=p, ld=p, tp=temps, nT=1, logp=p, P=p, R=4, K=8, C=3, var=0):
        return L.jvae_class_posterior_f32(z, means, T, ld, tp, nT, logp, P, R, K, C, var, None)
    assert cp(z=None) == -1 and cp(means=None) == -1 and cp(T=None) == -1 and cp(ld=None) == -1
    assert cp(logp=None, P=None) == -1 and cp(tp=None) == -1
    assert cp(C=0) == -1 and cp(C=129) == -1 and cp(K=0) == -1 and cp(K=1025) == -1
    assert cp(var=3) == -1 and cp(var=-1) == -1 and cp(nT=17, tp=many) == -1 and cp(nT=0) == -1 and cp(R=-1) == -1
    assert cp(R=0) == 0 and cp(nT=0, P=None, R=0) == 0

    def mi(P0=p, P1=p, Im=p, nT=1, C=3, L0=2, L1=2, N=4, ws=p, nbytes=1 << 20):
        return L.jvae_latent_mi_f32(P0, P1, Im, nT, C, L0, L1, N, ws, nbytes, None)
    assert mi(P0=None) == -1 and mi(P1=None) == -1 and mi(Im=None) == -1 and mi(ws=None) == -1
    assert mi(C=0) == -1 and mi(C=129) == -1 and mi(nT=0) == -1 and mi(nT=17) == -1 and mi(L0=0) == -1 and mi(L1=0) == -1
    assert mi(N=-1) == -1 and mi(N=0) == 0
    assert L.jvae_latent_mi_workspace_bytes(2, 5, 7) == 8 * 2 * 2 * 7 and mi(nT=2, L0=5, N=7, nbytes=8 * 2 * 2 * 7 - 1) == -3

    srcs = (ctypes.c_void_p * 9)(*([4096] * 9))
    holes = (ctypes.c_void_p * 2)(4096, None)
    fac = (ctypes.c_float * 9)(*([1.] * 9))

    def ag(s=srcs, f=fac, E=2, mode=0, tp=temps, nT=2, post=p, a=p, amax=p, arg=p, slot=0, C=3, N=4, status=p):
        return L.jvae_aggregate_scores_f32(s, f, E, mode, tp, nT, post, a, amax, arg, slot, C, N, status, None)
    assert ag(s=None) == -1 and ag(f=None) == -1 and ag(s=holes) == -1 and ag(tp=None) == -1
    assert ag(E=0) == -1 and ag(E=9) == -1 and ag(mode=4) == -1 and ag(mode=-1) == -1
    assert ag(C=0) == -1 and ag(C=129) == -1 and ag(nT=17, tp=many) == -1 and ag(N=-1) == -1
    assert ag(slot=2) == -1 and ag(slot=-2) == -1 and ag(post=None, a=None, amax=None, arg=None) == -1
    assert ag(mode=2) == -1 and ag(mode=2, a=None, slot=-1) == -1          # MEAN_SOFT has no aggregated row
    assert ag(mode=3, status=None) == -1 and ag(nT=0, slot=-1) == -1       # votes need the status word; post needs a temperature
    assert ag(N=0) == 0 and ag(mode=2, a=None, N=0) == 0


# ------------------------------------------------------------------------------------------ the public interface
def test_module_aggregation_surface_and_no_cpu_path():
    from jvae_hip import JvaeHipError, ops
    from module import aggregation as A
    for name in ('TEMPS', 'NAN_TEMPS', 'log_mean_exp', 'posterior', 'joint_posterior', 'mean_posterior', 'voting_posterior',
                 'compute_latent_mutual_info', 'latent_mutual_info', 'mean_of_posteriors', 'ensemble'):
        assert hasattr(A, name), name
    assert A.TEMPS == [None, 1, 5] and A.NAN_TEMPS == NAN_TEMPS
    x = torch.randn(3, 5)
    y = torch.zeros(5, dtype=torch.int64)
    for call in (lambda: A.log_mean_exp(x, x), lambda: A.posterior(x), lambda: A.joint_posterior(x, x),
                 lambda: A.mean_posterior(x, x), lambda: A.mean_of_posteriors(x, x), lambda: A.voting_posterior(y, y),
                 lambda: A.voting_posterior(y, num_classes=3), lambda: A.compute_latent_mutual_info(x.view(3, 1, 5), x.view(3, 1, 5)),
                 lambda: A.ensemble({'iws': [x, x]}, 'mean'), lambda: A.ensemble({'y': [y]}, 'vote'),
                 lambda: ops.class_posterior(x, x, torch.ones(3), torch.zeros(3)),
                 lambda: ops.latent_mutual_info(x.view(1, 3, 1, 5), x.view(1, 3, 1, 5)),
                 lambda: ops.aggregate_scores([x], 'mean', temps=[1])):
        with pytest.raises(JvaeHipError):
            call()
    with pytest.raises(JvaeHipError):
        ops.aggregate_scores([x] * 9, 'mean', temps=[1])
    with pytest.raises(JvaeHipError):
        ops.aggregate_scores([x], 'median', temps=[1])

    class Tilted:
        distribution, conditional = 'tilted', True
    with pytest.raises(NotImplementedError, match='tilted'):
        A.class_posteriors(Tilted(), x)
