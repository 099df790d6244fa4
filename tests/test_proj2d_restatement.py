"""proj2d on the host: the numpy fp64 restatement of csrc/embed.hip (tests/proj2d_cases.py) held to what scikit-learn computed
(tests/golden/proj2d, written by tools/gen_proj2d_golden.py), the bookkeeping of `jvae_compat.inspection.proj2d` with a stub
model, and the refusals that need no device.  The GPU tests (test_25_proj2d_gpu.py) hold the kernels to the same files and to
this restatement.

Bars: conditional and joint P 1e-12 relative on the entries above eps (the restatement sums with numpy's pairwise order,
scikit-learn in sequence: a few 1e-16); the PCA 1e-9 of the largest coordinate (scikit-learn's own rounding: an SVD there, an
eigen-decomposition of the covariance here)."""
import os
import re

import numpy as np
import pytest
import torch

import proj2d_cases as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('jvae_pairwise_sqdist_f32', 'jvae_tsne_affinities_f32', 'jvae_tsne_gradient_f32', 'jvae_tsne_update_f32',
               'jvae_pca_moments_f32', 'jvae_project_f32')


def load(case):
    with np.load(R.case_file(*case)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module', params=list(R.CASES), ids=lambda c: 'N%d-K%d-p%d' % c)
def golden(request):
    return request.param, load(request.param)


def close(a, b, rtol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    big = np.abs(b) > R.EPS
    assert np.array_equal(big, np.abs(a) > R.EPS)
    err = float(np.max(np.abs(a[big] - b[big]) / np.abs(b[big]))) if big.any() else 0.
    assert err <= rtol, err


def test_the_fixture_inputs_are_the_seeded_blobs(golden):
    (N, K, perplexity), g = golden
    x, label = R.blobs(N, K, R.CASES[(N, K, perplexity)])
    assert np.array_equal(x, g['x']) and np.array_equal(label, g['label'])
    d = R.sqdist(x)
    assert np.array_equal(d, g['d']) and np.array_equal(d, d.T) and not d.diagonal().any()
    assert float(g['margin']) > R.KNIFE_EDGE


def test_search_and_joint_restatement_against_scikit_learn(golden):
    (N, K, perplexity), g = golden
    cond, beta, S, margin = R.search(g['d'], perplexity)
    assert margin == float(g['margin'])
    close(cond[g['cond_rows']], g['cond'], 1e-12)
    close(R.condensed(R.joint(cond)), g['joint'], 1e-12)
    assert np.abs(R.entropies(g['d'], beta) - np.log(perplexity)).max() <= 1e-5
    assert np.allclose(cond.sum(1), 1., rtol=0, atol=1e-12) and not cond.diagonal().any()


@pytest.mark.parametrize('name', ('small', 'unit'))
@pytest.mark.parametrize('f', (1, 12))
def test_kl_and_gradient_restatement_against_scikit_learn(golden, name, f):
    (N, K, perplexity), g = golden
    P = R.expand(g['joint'].astype(np.float32).astype(np.float64), N)
    kl, grad, terms, norm = R.kl_and_gradient(P, g['y_' + name], f)
    ref_kl, ref_g = float(g[f'kl.{name}.{f}']), g[f'g.{name}.{f}']
    assert abs(kl - ref_kl) <= N * N * 2. ** -52 * abs(ref_kl)
    assert (np.abs(grad.astype(np.float64) - ref_g) <= 2. ** -23 * np.abs(ref_g) + 2. ** -50 * terms).all()
    assert norm == pytest.approx(float(np.linalg.norm(ref_g.astype(np.float64))), rel=1e-6)


def test_update_restatement_is_the_step_of_scikit_learn():
    """25 iterations of scikit-learn's own loop (update.npz) against the restatement: both gain branches and the clip."""
    with np.load(os.path.join(R.GOLDEN, 'update.npz')) as z:
        g = {k: z[k] for k in z.files}
    y, upd, gains = g['p0'].copy(), np.zeros(64, np.float32), np.ones(64, np.float32)
    for t in range(int(g['steps'])):
        y, upd, gains, _ = R.update(y, upd, gains, g['base'] * g['flip'] ** t, float(g['momentum']), float(g['learning_rate']))
    assert np.array_equal(y, g['p'])
    assert (gains == np.float32(0.01)).any() and (gains > 1.).any()              # the clip and the growing branch were reached


def test_update_restatement_branches():
    y = np.zeros(6, np.float32)
    upd = np.array([1, 1, -1, 0, 1e-30, 1], np.float32)
    g = np.array([-1, 1, -1, 1, -1e-30, 1], np.float32)
    gains = np.array([1, 1, 1, 1, 1, 0.011], np.float32)
    y1, u1, k1, g1 = R.update(y, upd, gains, g, 0.8, 200.)
    f = np.float32
    assert np.array_equal(k1, np.array([f(1) + f(0.2), f(0.8), f(0.8), f(0.8), f(0.8), f(0.01)], np.float32))
    assert np.array_equal(g1, g * k1) and np.array_equal(u1, f(0.8) * upd - f(200.) * g1) and np.array_equal(y1, u1)


def test_pca_restatement_against_scikit_learn(golden):
    from jvae_compat import inspection
    (N, K, perplexity), g = golden
    mean, cov, _ = R.covariance(g['x'])
    comp, var = inspection.principal_axes(cov, min(2, K))
    out = (g['x'].astype(np.float64) - mean) @ comp.T
    bar = 1e-9 * np.abs(g['pca.out']).max()
    assert np.abs(out - g['pca.out']).max() <= bar
    assert np.abs(mean - g['pca.mean']).max() <= 1e-12 * np.abs(g['pca.mean']).max()
    assert np.abs(comp - g['pca.components']).max() <= 1e-9 and np.allclose(var, g['pca.variance'], rtol=1e-9, atol=0)
    big = np.abs(comp).argmax(1)
    assert (comp[np.arange(len(comp)), big] > 0).all()


# ----------------------------------------------------------------------------------------------------- proj2d's bookkeeping
class Recorder(dict):
    def __init__(self, mu, y, **aux):
        super().__init__(mu=mu, y=y)
        self._aux = aux


class Stub:
    """Model(2).fit_transform: the row number and its first coordinate."""
    seen = None

    def __init__(self, n):
        assert n == 2

    def fit_transform(self, X):
        Stub.seen = np.array(X)
        return np.stack([np.arange(len(X), dtype=np.float64), np.asarray(X)[:, 0]], 1)


def recorders(shift):
    rng = np.random.default_rng(7)
    cent = torch.from_numpy(rng.standard_normal((9, 4)).astype(np.float32))
    alt = torch.from_numpy(rng.standard_normal(4).astype(np.float32))
    out = {}
    for name, n in (('cifar10-3', 25), ('svhn', 9), ('cifar10-3-extra', 25)):
        mu = torch.from_numpy(rng.standard_normal((n, 4)).astype(np.float32)) + shift
        out[name] = Recorder(mu, torch.from_numpy(rng.integers(0, 9, n)), centroids=cent, alternate=alt)
    return out


@pytest.mark.parametrize('alternate', (False, True))
def test_proj2d_bookkeeping_with_a_stub_model(tmp_path, alternate):
    from jvae_compat import inspection
    from jvae_compat.torch_load import get_classes_by_name
    pre, ft = recorders(0.), recorders(1.)
    tset, N, N_ = 'cifar10-3', 20, 3
    classes = get_classes_by_name(tset)
    assert len(classes) == 9 and 'cat' not in classes
    csv = str(tmp_path / 'p.csv')
    mu_, y_ = inspection.proj2d(pre, ft, tset, include_alternate=alternate, N=N, N_=N_, Model=Stub, csv_file=csv)
    C = 9
    block = C + (1 if alternate else 0)
    want = ['centroids'] + (['alternate'] if alternate else [])
    want += [f'{s}-{w}' for w in ('pre', 'ft') for s in pre]
    assert sorted(mu_) == sorted(want) and list(mu_) == list(y_)
    cent = pre[tset]._aux['centroids'].numpy()
    start, stack = 0, Stub.seen
    for w, recs in (('pre', pre), ('ft', ft)):
        for s in recs:
            n = N if s.startswith(tset) else N // 10
            for c in range(N_):                                          # N_ copies of the centroid block
                assert np.array_equal(stack[start + c * block:start + c * block + C], cent)
                if alternate:
                    assert np.array_equal(stack[start + c * block + C], pre[tset]._aux['alternate'].numpy())
            last = start
            start += N_ * block
            k = f'{s}-{w}'
            assert np.array_equal(stack[start:start + n], recs[s]['mu'].numpy()[:n])
            assert np.array_equal(mu_[k][:, 0], np.arange(start, start + n))          # the slice bounds
            if s == tset:
                assert list(y_[k]) == [classes[i] for i in recs[s]['y'].numpy()[:n]]
            else:
                assert list(y_[k]) == [s] * n
            start += n
    assert start == len(stack)
    assert np.array_equal(mu_['centroids'][:, 0], np.arange(last, last + C)) and list(y_['centroids']) == list(classes)
    if alternate:
        assert mu_['alternate'][:, 0].tolist() == [last + C] and y_['alternate'] == ['ood']
    text = open(csv).read().splitlines()
    assert text[0] == 'x1,x2,y,set,dist,ft' and len(text) == 1 + sum(len(v) for v in mu_.values())
    tails = {}
    for line in text[1:]:
        f = line.split(',')
        assert len(f) == 6 and float(f[0]) == int(float(f[0]))
        tails.setdefault(tuple(f[3:]), 0)
        tails[tuple(f[3:])] += 1
    want_rows = {('centroids', 'ind', 'both'): C, ('cifar10-3', 'ind', 'pre'): N, ('cifar10-3', 'ind', 'ft'): N,
                 ('svhn', 'ood', 'pre'): N // 10, ('svhn', 'ood', 'ft'): N // 10,
                 ('cifar10-3-extra', 'ood', 'pre'): N, ('cifar10-3-extra', 'ood', 'ft'): N}
    if alternate:
        want_rows[('alt', 'ood', 'both')] = 1
    assert tails == want_rows
    row = text[1 + (C + (1 if alternate else 0))].split(',')            # the first set row: x1, x2 and the class name
    assert row[2] == classes[int(pre[tset]['y'][0])]


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('name', NEW_SYMBOLS)
def test_new_symbols_are_declared_and_bound(name):
    from jvae_hip import lib
    with open(os.path.join(REPO, 'include', 'jvae_hip.h')) as f:
        header = f.read()
    decl = re.search(r'^int ' + name + r'\(([^;]*)\);', header, re.M | re.S)
    assert decl, name + ' is not declared in include/jvae_hip.h'
    restype, argtypes = lib._SIGS[name]
    assert len(argtypes) == len(decl.group(1).split(',')) and argtypes[-1] is lib.P


def test_host_side_refusals():
    from jvae_compat import inspection
    from jvae_hip import lib, ops
    x = torch.zeros(8, 3)
    for call in (lambda: ops.pairwise_sqdist(x), lambda: ops.tsne_affinities(torch.zeros(8, 8), 2.),
                 lambda: ops.tsne_gradient(torch.zeros(8, 8), torch.zeros(8, 2)),
                 lambda: ops.tsne_update(*(torch.zeros(8, 2) for _ in range(4)), 0.5, 50.),
                 lambda: ops.pca_moments(x), lambda: ops.project(x, torch.zeros(3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64)),
                 lambda: ops.pairwise_sqdist(x.double())):
        with pytest.raises(lib.JvaeHipError):
            call()
    with pytest.raises(NotImplementedError):
        inspection.TSNE(3)
    assert inspection.TSNE().perplexity == 30. and inspection.TSNE().max_iter == 1000 and inspection.PCA().n_components == 2
    for k in ('proj2d', 'plot2d', 'PCA', 'TSNE'):
        assert callable(getattr(inspection, k))
    doc = inspection.__doc__
    assert 'stay in the reference' in doc and 'proj2d' not in doc.split('stay in the reference')[0].splitlines()[-1]
