"""proj2d on the device: the kernels of csrc/embed.hip (ops.pairwise_sqdist, tsne_affinities, tsne_gradient, tsne_update,
pca_moments, project) and `jvae_compat.inspection.PCA` / `TSNE` / `proj2d` over them, held to scikit-learn's records
(tests/golden/proj2d, tools/gen_proj2d_golden.py) at the fixture sizes and to the fp64 restatement (tests/proj2d_cases.py,
itself held to the same records by test_proj2d_restatement.py) at N = 257: no multiple of a tile, a wave or a workgroup.

Bars (none of them is taken from what the kernels gave):
  distances      bit for bit the rule fp32(sum_k (double(x_ik) - double(x_jk))^2), k ascending
  affinities     every row's entropy within 1e-5 of log(perplexity) (the search's stopping rule); the joint P within 1 fp32 ulp of
                 the fp32 rounding of scikit-learn's fp64 value (formed in fp64 here and rounded once; the two fp64 values differ
                 by summation order, which can move the rounding by one step)
  gradient       the kernel is given the fp32 rounding of scikit-learn's joint P - what the device keeps - and the records were
                 taken at that P: |g - g_ref| <= 2^-23 |g_ref| + 2^-50 sum_j (|f P qn dy| + |Q qn dy|), the one fp32 rounding and
                 the fp64 sums, against the abs-sum because the attractive and the repulsive part cancel
  KL             N^2 2^-52 relative
  update         bit for bit numpy's fp32 execution of scikit-learn's step
  covariance     N K 2^-52 of sum |terms|;  PCA.fit_transform (2^-23 + 1e-9) of the largest coordinate
  TSNE           on the 300-point fixture from its stored init: the same bits twice; every point's nearest embedded neighbour in
                 its own blob (all five recorded scikit-learn runs meet this); the final KL at most the records' largest plus
                 their spread.  Measured KL: see DESIGN.md 7m.
"""
import functools
import os

import numpy as np
import pytest
import torch

import proj2d_cases as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURES = list(R.CASES)
IDS = ['N%d-K%d-p%d' % c for c in FIXTURES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def golden(case):
    with np.load(R.case_file(*case)) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case257():
    """(x, d, joint P fp64 full, y (257, 2) fp32) of the N = 257 input; computed once, never written to."""
    x, d, cond, beta, S = R.case257()
    y = np.random.default_rng(257).standard_normal((257, 2)).astype(np.float32)
    return x, d, R.joint(cond), y


def ulps(a, b):
    """Distance in fp32 steps between two arrays of positive floats."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------ 1. distances
@pytest.mark.parametrize('K', (1, 3, 37, 128))
@pytest.mark.parametrize('N', (2, 5, 64, 65, 257))
def test_distances_bit_for_bit(N, K):
    from jvae_hip import ops
    x, _ = R.blobs(N, K, 10 * N + K)
    d = ops.pairwise_sqdist(dev(x)).cpu().numpy()
    want = R.sqdist(x)
    assert d.dtype == np.float32 and np.array_equal(d.view(np.int32), want.view(np.int32))
    assert np.array_equal(d, d.T) and not d.diagonal().any() and (d[~np.eye(N, dtype=bool)] > 0).all()


# ----------------------------------------------------------------------------------------------------------- 2. affinities
def check_affinities(d, perplexity, joint_full):
    from jvae_hip import ops
    N = len(d)
    P, beta, S = (t.cpu().numpy() for t in ops.tsne_affinities(dev(d), perplexity))
    H = R.entropies(d, beta)
    worst_h = np.abs(H - np.log(perplexity)).max()
    off = ~np.eye(N, dtype=bool)
    step = ulps(P[off], joint_full.astype(np.float32)[off])
    print(f'affinities N={N}: worst |H - log perplexity| {worst_h:.3g}, worst fp32 steps {step.max()}, '
          f'steps > 0 in {np.mean(step > 0):.3%}')
    assert worst_h <= 1e-5
    assert step.max() <= 1
    assert np.array_equal(P, P.T) and (P.diagonal() == np.float32(R.EPS)).all() and (P >= np.float32(R.EPS)).all()
    again = ops.tsne_affinities(dev(d), perplexity)[0].cpu().numpy()
    assert np.array_equal(again.view(np.int32), P.view(np.int32))


@pytest.mark.parametrize('case', FIXTURES, ids=IDS)
def test_affinities_against_scikit_learn(case):
    g = golden(case)
    check_affinities(g['d'], case[2], R.expand(g['joint'], case[0]))


def test_affinities_against_the_restatement_at_257():
    x, d, joint, y = case257()
    check_affinities(d, 30., joint)


# ------------------------------------------------------------------------------------------------- 3. gradient, KL, norm
def check_gradient(P32, y, f, ref_kl, ref_g):
    from jvae_hip import ops
    N = len(y)
    stats = torch.zeros(2, dtype=torch.float64, device=DEV)
    g = ops.tsne_gradient(dev(P32), dev(y), float(f), stats=stats).cpu().numpy()
    kl, norm = stats.tolist()
    terms = R.kl_and_gradient(P32.astype(np.float64), y, f)[2]
    bar = 2. ** -23 * np.abs(ref_g) + 2. ** -50 * terms
    err = np.abs(g.astype(np.float64) - ref_g)
    print(f'gradient N={N} f={f}: worst err / bar {np.max(err / bar):.3g}, KL {kl:.17g} (ref {ref_kl:.17g}, '
          f'rel {abs(kl - ref_kl) / abs(ref_kl):.3g}, bar {N * N * 2. ** -52:.3g})')
    assert (err <= bar).all()
    assert abs(kl - ref_kl) <= N * N * 2. ** -52 * abs(ref_kl)
    assert abs(norm - np.linalg.norm(g.astype(np.float64))) <= 1e-12 * norm
    plain = ops.tsne_gradient(dev(P32), dev(y), float(f)).cpu().numpy()        # without the second pass: the same gradient
    assert np.array_equal(plain.view(np.int32), g.view(np.int32))


@pytest.mark.parametrize('f', (1, 12))
@pytest.mark.parametrize('name', ('small', 'unit'))
@pytest.mark.parametrize('case', FIXTURES, ids=IDS)
def test_gradient_and_kl_against_scikit_learn(case, name, f):
    g = golden(case)
    P32 = R.expand(g['joint'].astype(np.float32), case[0])
    check_gradient(P32, g['y_' + name], f, float(g[f'kl.{name}.{f}']), g[f'g.{name}.{f}'].astype(np.float64))


@pytest.mark.parametrize('f', (1, 12))
def test_gradient_and_kl_against_the_restatement_at_257(f):
    x, d, joint, y = case257()
    P32 = joint.astype(np.float32)
    kl, grad, _, _ = R.kl_and_gradient(P32.astype(np.float64), y, f)
    check_gradient(P32, y, f, kl, grad.astype(np.float64))


# --------------------------------------------------------------------------------------------------------------- 4. update
def test_update_bit_for_bit():
    from jvae_hip import ops
    rng = np.random.default_rng(4)
    N = 700
    y, upd, g = (rng.standard_normal((N, 2)).astype(np.float32) for _ in range(3))
    gains = rng.uniform(0.005, 2., (N, 2)).astype(np.float32)              # some at and below the clip
    upd[:5] = 0.
    upd[5:10], g[5:10] = 1e-30, -1e-30                                     # the fp32 product underflows: no increase
    for momentum, lr in ((0.5, 50.), (0.8, 208.33333333333334)):
        want = R.update(y, upd, gains, g, momentum, lr)
        assert (want[2] == np.float32(0.01)).any() and (want[2] > gains).any() and (want[2] < gains).any()
        t = [dev(a.copy()) for a in (y, upd, gains, g)]
        norm = torch.zeros(1, dtype=torch.float64, device=DEV)
        ops.tsne_update(*t, momentum, lr, norm=norm)
        for have, ref, what in zip(t, want, ('y', 'update', 'gains', 'g')):
            assert np.array_equal(have.cpu().numpy().view(np.int32), ref.view(np.int32)), what
        ref_norm = np.linalg.norm(want[3].astype(np.float64))
        assert abs(float(norm) - ref_norm) <= 1e-12 * ref_norm


# ------------------------------------------------------------------------------------------------------------------ 5. PCA
@pytest.mark.parametrize('shape', ((5, 3), (65, 1), (257, 128), (300, 1024)), ids=str)
def test_pca_moments_against_fp64(shape):
    from jvae_hip import ops
    N, K = shape
    x, _ = R.blobs(N, K, N + K)
    mean, cov = (t.cpu().numpy() for t in ops.pca_moments(dev(x)))
    ref_mean, ref_cov, terms = R.covariance(x)
    print(f'pca_moments {shape}: worst cov err / bar {np.max(np.abs(cov - ref_cov) / (N * K * 2. ** -52 * terms)):.3g}')
    assert (np.abs(mean - ref_mean) <= N * 2. ** -52 * np.abs(x.astype(np.float64)).mean(0)).all()
    assert (np.abs(cov - ref_cov) <= N * K * 2. ** -52 * terms).all()
    assert np.array_equal(cov, cov.T)
    again = ops.pca_moments(dev(x))[1].cpu().numpy()
    assert np.array_equal(again, cov)


@pytest.mark.parametrize('case', FIXTURES, ids=IDS)
def test_pca_fit_transform_against_scikit_learn(case):
    from jvae_compat import inspection
    g = golden(case)
    pca = inspection.PCA(min(2, case[1]), device=DEV)
    out = pca.fit_transform(g['x'])
    top = np.abs(g['pca.out']).max()
    assert out.dtype == np.float32 and out.shape == g['pca.out'].shape
    print(f'PCA {case}: worst err / largest coordinate {np.abs(out - g["pca.out"]).max() / top:.3g}')
    assert np.abs(out - g['pca.out']).max() <= (2. ** -23 + 1e-9) * top
    assert np.abs(pca.components_ - g['pca.components']).max() <= 1e-9
    assert np.allclose(pca.explained_variance_, g['pca.variance'], rtol=1e-9, atol=0)
    assert np.allclose(pca.mean_, g['pca.mean'], rtol=0, atol=1e-12 * np.abs(g['pca.mean']).max())
    assert np.array_equal(inspection.PCA(min(2, case[1])).fit_transform(dev(g['x'])), out)      # a device tensor, the default device


# ----------------------------------------------------------------------------------------------------------------- 6. TSNE
def test_tsne_on_the_300_point_fixture():
    from jvae_compat import inspection
    from jvae_hip import ops
    case = (300, 16, 30)
    g = golden(case)
    runs = []
    for _ in range(2):
        tsne = inspection.TSNE(2, perplexity=30., init=g['init'], device=DEV)
        runs.append((tsne.fit_transform(g['x']), tsne.kl_divergence_, tsne.n_iter_))
    (emb, kl, n_iter), (emb2, kl2, n_iter2) = runs
    assert emb.dtype == np.float32 and emb.shape == (300, 2) and np.isfinite(emb).all()
    assert np.array_equal(emb.view(np.int32), emb2.view(np.int32)) and kl == kl2 and n_iter == n_iter2
    purity = R.nearest_neighbour_purity(emb, g['label'])
    top, spread = g['kl_runs'].max(), g['kl_runs'].max() - g['kl_runs'].min()
    print(f'TSNE 300: KL {kl:.6f} after {n_iter + 1} iterations (scikit-learn: {g["kl_runs"]}, exact {float(g["kl_exact"]):.6f}), '
          f'purity {purity}')
    assert purity == 1.0
    assert kl <= top + spread
    assert tsne.learning_rate_ == 50. and tsne.embedding_ is emb2
    P = ops.tsne_affinities(ops.pairwise_sqdist(dev(g['x'])), 30.)[0]
    assert inspection.TSNE.kl_divergence(P, dev(emb)) == kl
    with pytest.raises(ValueError):
        inspection.TSNE(2, perplexity=300.).fit_transform(g['x'])
    seeded = inspection.TSNE(2, init='random', random_state=5, max_iter=250, device=DEV)
    y0 = seeded._initial(dev(g['x']))
    assert np.array_equal(y0, 1e-4 * np.random.RandomState(5).standard_normal(size=(300, 2)).astype(np.float32))


# --------------------------------------------------------------------------------------------------------------- 7. proj2d
def test_proj2d_end_to_end_with_pca(tmp_path):
    from jvae_compat import inspection
    from jvae_compat.recorders import SampleRecorder
    from jvae_compat.torch_load import get_classes_by_name
    from jvae_hip import ops
    tset, C, K = 'cifar10+0+1+2', 3, 8
    classes = get_classes_by_name(tset)
    assert len(classes) == C
    rng = np.random.default_rng(11)
    cent = torch.from_numpy((4. * rng.standard_normal((C, K))).astype(np.float32))
    alt = torch.from_numpy(rng.standard_normal(K).astype(np.float32))

    def recorders(shift):
        out = {}
        for name, n in ((tset, 40), ('svhn', 12)):
            y = torch.from_numpy(rng.integers(0, C, n))
            mu = cent[y] + torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)) + shift
            rec = SampleRecorder(n, mu=mu, y=y)
            rec.append_batch(mu=mu, y=y)
            rec.add_auxiliary(centroids=cent, alternate=alt)
            out[name] = rec
        return out
    pre, ft = recorders(0.), recorders(0.5)
    seen = {}

    class Model(inspection.PCA):
        def fit_transform(self, X):
            seen['model'], seen['stack'] = self, np.array(X)
            return super().fit_transform(X)
    csv = str(tmp_path / 'proj.csv')
    N, N_ = 30, 2
    mu_, y_ = inspection.proj2d(pre, ft, tset, include_alternate=True, N=N, N_=N_, Model=Model, csv_file=csv)
    model = seen['model']
    assert seen['stack'].shape == (2 * (2 * N_ * (C + 1) + N + N // 10), K)

    def project(block):
        return ops.project(dev(np.asarray(block, np.float32)), dev(model.mean_), dev(model.components_)).cpu().numpy()
    assert np.array_equal(mu_['centroids'], project(cent.numpy())) and np.array_equal(mu_['alternate'], project(alt.numpy()[None]))
    for w, recs in (('pre', pre), ('ft', ft)):
        for s, n in ((tset, N), ('svhn', N // 10)):
            assert np.array_equal(mu_[f'{s}-{w}'], project(recs[s]['mu'].numpy()[:n])), (s, w)
    assert list(y_[tset + '-ft']) == [classes[i] for i in ft[tset]['y'].numpy()[:N]] and list(y_['svhn-pre']) == ['svhn'] * (N // 10)
    rows = [line.split(',') for line in open(csv).read().splitlines()]
    assert rows[0] == ['x1', 'x2', 'y', 'set', 'dist', 'ft']
    count = {}
    for r in rows[1:]:
        count[tuple(r[3:])] = count.get(tuple(r[3:]), 0) + 1
    assert count == {('centroids', 'ind', 'both'): C, ('alt', 'ood', 'both'): 1, (tset, 'ind', 'pre'): N, (tset, 'ind', 'ft'): N,
                     ('svhn', 'ood', 'pre'): N // 10, ('svhn', 'ood', 'ft'): N // 10}
    assert [np.float32(v) for v in rows[1][:2]] == list(mu_['centroids'][0]) and rows[1][2] == classes[0]


# ------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_outputs_untouched():
    from jvae_hip import lib, ops
    L = lib.load()
    st = lib.stream_ptr()
    x = torch.zeros(64, 4, device=DEV)
    out = torch.full((64, 64), 7., device=DEV)
    f64 = torch.full((4096,), 7., dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    p, n = lib.ptr, ws.numel()
    assert L.jvae_pairwise_sqdist_f32(p(x), p(out), 16385, 4, st) == -2
    assert L.jvae_pairwise_sqdist_f32(p(x), p(out), 64, 1025, st) == -2
    assert L.jvae_pairwise_sqdist_f32(p(x), p(out), 1, 4, st) == -1
    assert L.jvae_tsne_affinities_workspace_bytes(16385) == 0 and L.jvae_tsne_gradient_workspace_bytes(16385) == 0
    assert L.jvae_tsne_affinities_f32(p(out), p(out), p(f64), p(f64), 30., 16385, p(ws), n, st) == -2
    assert L.jvae_tsne_gradient_f32(p(out), p(x), p(out), 1., 16385, None, p(ws), n, st) == -2
    assert L.jvae_tsne_update_f32(p(out), p(out), p(out), p(out), 0.5, 50., 16385, None, st) == -2
    assert L.jvae_pca_moments_workspace_bytes(64, 1025) == 0
    assert L.jvae_pca_moments_f32(p(x), p(f64), p(f64), 64, 1025, p(ws), n, st) == -2
    assert L.jvae_pca_moments_f32(p(x), p(f64), p(f64), 1, 4, p(ws), n, st) == -1
    assert L.jvae_project_f32(p(x), p(f64), p(f64), p(out), 64, 1025, 2, st) == -2
    assert L.jvae_project_f32(p(x), p(f64), p(f64), p(out), 64, 4, 17, st) == -2
    torch.cuda.synchronize()
    assert (out == 7.).all() and (f64 == 7.).all() and not x.any() and not ws.any()
    cpu = torch.zeros(8, 3)
    for call in (lambda: ops.pairwise_sqdist(cpu), lambda: ops.pca_moments(cpu), lambda: ops.tsne_affinities(torch.zeros(8, 8), 2.),
                 lambda: ops.pairwise_sqdist(x.double()), lambda: ops.pca_moments(x[:1]),
                 lambda: ops.pairwise_sqdist(torch.zeros(4, 1025, device=DEV))):
        with pytest.raises(lib.JvaeHipError):
            call()
