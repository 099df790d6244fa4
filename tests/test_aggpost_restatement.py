"""The fp64 restatement of the aggregate-posterior density (ops.aggpost_logdensity, csrc/aggpost.hip) and of
net.elbo_decomposition (module/scoring.py), the data cases, and the tolerance of the GPU test
(tests/test_36_aggpost_gpu.py).  No code under test runs here: the closed forms below check the restatement itself.

Restatement.  For a query z and the bank rows n of its set S (all rows, or the rows of its group):
  Q_n = sum_k log_var_nk + sum_k (z_k - mu_nk)^2 exp(-log_var_nk),   log q(z) = logsumexp_n(-Q_n / 2) - log |S| - (K / 2) log 2 pi,
and for one coordinate the same with q_nk = log_var_nk + (z_k - mu_nk)^2 exp(-log_var_nk) and K = 1; all in fp64 from the fp32 inputs.

Tolerance.  |error| <= u B with u = 2^-24.  B is the first-order error of the kernel's own arithmetic, evaluated in fp64 on the
case's inputs (as test_dose_restatement.dose_c is):
  * a pair's Q is the chain acc = fmaf(d * d, w, acc) from acc = c = fp32(sum_k log_var) on: c carries u |c|; a term t_k = d^2 w
    carries 4 u t_k before the fmaf (d: 1, its rounded square: 2 + 1, w = fp32(exp(-log_var)): 1); every step of the chain rounds
    to u |acc_k|.  EQ_n = |c_n| + 4 sum_k t_k + sum_k |c_n + sum_{j<=k} t_j|, and Q_n moves log q by p_n / 2 per unit, p_n the
    term's share of the sum;
  * the shift: the computed result does not depend on WHICH shift is used (it cancels), only on the roundings of the exponent
    -log2(e)/2 (Q - a): the difference, the constant and the product, 3 u |x|, added up over a term's way from its group's shift
    to the final one: 3 u (Q_n - A) / 2 in natural units, again weighted by p_n;
  * the sums: every level a term passes (an addition, a product with a scale factor, the factor's own v_exp_f32) costs at most u
    (2 u for an exponential: 1 ulp) of the whole sum, i.e. of 1 in log q.  Levels: the term's exponential 2, the tree of 16 (8)
    terms 4 (3), a fold 4 (two exponentials of which one is exactly 1, a product, a sum) for each of the 16 (32) groups of a wave
    in a piece and the 2 levels of the four waves, the merge 3 + 2 ceil(log2 pieces);
  * the end is fp64; the final rounding costs u |log q|.
  B = sum_n p_n (EQ_n / 2 + 3 (Q_n - A) / 2) + LEVELS + |log q|.
Limit.  EQ_n <= (K + 4)(|c_n| + T_n), T_n = sum_k t_k = Q_n - c_n; sum_n p_n Q_n <= A + 2 log N and |A| <= 2 |log q| + 2 log N + K
log 2 pi, so with |log_var| <= V:  B / (1 + |log q|) <= (K + 4)(1 + (V + 0.92) K + 3 log N) + 3 log N + LEVELS + 1 = b_limit(K, N, V),
asserted on every case (a coordinate: K = 1).  The bound cannot be widened to fit a result: it has no free constant."""
import functools
import math

import numpy as np
import pytest

U = 2. ** -24
P = 1024                                               # ops.aggpost_partition(), asserted by the GPU test
LOG2PI = math.log(2 * math.pi)
V_DATA = -math.log(1e-4)                               # |log_var| of the data cases: variances from 1e-4 to 1
V_MODEL = 20.                                          # the clip of the latent kernel
JOINT_GROUPS, DIMS_GROUPS = 16, 32                     # groups of rows a wave folds in a piece: 1024 / 4 / 16 and 1024 / 4 / 8


def pieces_of(N):
    return -(-N // P)


def levels(N, dims):
    merge = 3 + 2 * max(1, math.ceil(math.log2(pieces_of(N))))
    return 2 + (3 + 4 * (DIMS_GROUPS + 2) if dims else 4 + 4 * (JOINT_GROUPS + 2)) + merge


def b_limit(K, N, V, dims=False):
    k = 1 if dims else K
    return (k + 4) * (1 + (V + 0.92) * k + 3 * math.log(max(N, 2))) + 3 * math.log(max(N, 2)) + levels(N, dims) + 1


def aggpost_reference(mu, lv, group, z, zgroup=None, conditional=False):
    """fp32 arrays -> {'logq' (M,), 'logq_dims' (M, K), 'B' (M,), 'B_dims' (M, K)} in fp64; a query whose set is empty: -inf, B 0."""
    mu, lv, z = (np.asarray(a, dtype=np.float64) for a in (mu, lv, z))
    N, K = mu.shape
    M = z.shape[0]
    w, c = np.exp(-lv), lv.sum(1)
    out = {'logq': np.full(M, -np.inf), 'logq_dims': np.full((M, K), -np.inf), 'B': np.zeros(M), 'B_dims': np.zeros((M, K))}
    for m in range(M):
        sel = np.asarray(group) == zgroup[m] if conditional else np.ones(N, dtype=bool)
        n = int(sel.sum())
        if not n:
            continue
        d = z[m] - mu[sel]
        t = d * d * w[sel]
        cs, lvs = c[sel], lv[sel]
        Q = cs + t.sum(1)
        A = Q.min()
        y = 0.5 * (Q - A)
        e = np.exp(-y)
        p = e / e.sum()
        logq = -0.5 * A + math.log(e.sum()) - math.log(n) - 0.5 * K * LOG2PI
        EQ = np.abs(cs) + 4 * t.sum(1) + np.abs(cs[:, None] + np.cumsum(t, 1)).sum(1)
        out['logq'][m] = logq
        out['B'][m] = (p * (0.5 * EQ + 3 * y)).sum() + levels(N, False) + abs(logq)
        q = lvs + t
        Ak = q.min(0)
        yk = 0.5 * (q - Ak)
        ek = np.exp(-yk)
        pk = ek / ek.sum(0)
        lk = -0.5 * Ak + np.log(ek.sum(0)) - math.log(n) - 0.5 * LOG2PI
        out['logq_dims'][m] = lk
        out['B_dims'][m] = (pk * (0.5 * (4 * t + np.abs(q)) + 3 * yk)).sum(0) + levels(N, True) + np.abs(lk)
    return out


def assert_limit(ref, K, N, V):
    """The fixed ceiling of the derived bound, on every output of a case."""
    fin = np.isfinite(ref['logq'])
    assert (ref['B'][fin] <= b_limit(K, N, V) * (1 + np.abs(ref['logq'][fin]))).all()
    assert (ref['B_dims'][fin] <= b_limit(K, N, V, True) * (1 + np.abs(ref['logq_dims'][fin]))).all()


# ------------------------------------------------------------------------------------------------------------- data cases
# (K, N, M, groups, empty): every K of {1, 3, 64, 65, 200}, N of {1, 2, 63, 64, 65, P - 1, P, P + 1, 2 P + 3}, M of {1, 64, 65, 129},
# groups of {1, 3, 10}; `empty`: group 1 of 3 has no bank row and some queries ask for it
CASES = [(1, 1, 1, 1, False), (3, 2, 64, 1, False), (64, 63, 65, 3, False), (65, 64, 129, 10, False), (200, 65, 64, 3, False),
         (3, P - 1, 65, 10, False), (64, P, 64, 3, False), (65, P + 1, 129, 1, False), (200, 2 * P + 3, 65, 10, False),
         (64, 2 * P + 3, 129, 3, True)]


def case_id(c):
    return 'K{}_N{}_M{}_G{}{}'.format(*c[:4], '_empty' if c[4] else '')


@functools.lru_cache(maxsize=None)
def aggpost_case(K, N, M, G, empty=False, seed=0):
    """-> mu, lv (N, K) fp32, group (N,) int32, z (M, K) fp32, zgroup (M,) int32.  Variances log-uniform in [1e-4, 1] with both
    ends present; a query is a draw of a bank row (its group the row's), every fifth one far from it: 8 sigma and 10^4 sigma of
    that row in every coordinate, in turn."""
    rng = np.random.default_rng(1000 * K + N + M + G + seed)
    lv = rng.uniform(-V_DATA, 0., (N, K))
    lv[0, 0], lv[-1, -1] = -V_DATA, 0. if N * K > 1 else -V_DATA
    lv = lv.astype(np.float32)
    mu = rng.normal(0., 1., (N, K)).astype(np.float32)
    group = rng.integers(0, G, N).astype(np.int32)
    group[:min(G, N)] = np.arange(min(G, N))
    if empty:
        group[group == 1] = 2
    src = rng.integers(0, N, M)
    src[0] = 0
    f = rng.normal(0., 1., (M, K))
    far = np.arange(M) % 5 == 4
    sign = np.where(rng.random((M, K)) < .5, -1., 1.)
    f[far] = sign[far] * np.where(np.arange(M) % 10 == 4, 8., 1e4)[far, None]
    z = (mu[src].astype(np.float64) + np.exp(0.5 * lv[src].astype(np.float64)) * f).astype(np.float32)
    zgroup = group[src].copy()
    if empty:
        zgroup[1::7] = 1
    return mu, lv, group, z, zgroup


@functools.lru_cache(maxsize=None)
def case_reference(case, conditional):
    mu, lv, group, z, zgroup = aggpost_case(*case)
    return aggpost_reference(mu, lv, group, z, zgroup, conditional)


def unshifted_fp32(mu, lv, z):
    """What a plain fp32 sum of exponentials gives (no shift): the far queries come out as -inf."""
    mu, lv, z = (np.asarray(a, dtype=np.float32) for a in (mu, lv, z))
    with np.errstate(divide='ignore', over='ignore'):
        E = np.stack([-0.5 * (((zm - mu) ** 2 * np.exp(-lv)).sum(1) + lv.sum(1)) for zm in z])
        return np.log(np.exp(E).sum(1, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------- elbo_decomposition
def gaussian_prior(means, T=1., var_dim='scalar', conditional=False):
    """The prior as the restatement reads it: means (C, K), the whitening factor T in the layout of var_dim ((), (K,), (K, K), with
    a leading class axis when conditional) - GaussianPrior's mean and inv_trans."""
    means = np.asarray(means, dtype=np.float64)
    means = means.reshape(-1, means.shape[-1])
    C, K = means.shape
    T = np.asarray(T, dtype=np.float64)
    tail = {'scalar': (), 'diag': (K,), 'full': (K, K)}[var_dim]
    return dict(means=means, T=np.broadcast_to(T.reshape((-1,) + tail) if conditional else T.reshape((1,) + tail), (C,) + tail), var_dim=var_dim,
                conditional=conditional)


def _whiten(prior, x, y):
    T = prior['T'][y]
    if prior['var_dim'] == 'full':
        return np.einsum('mij,mj->mi', np.tril(T), x)
    return x * (T if prior['var_dim'] == 'diag' else T[:, None])


def _log_det(prior, y, K):
    T = prior['T'][y]
    if prior['var_dim'] == 'full':
        return -2 * np.log(np.abs(np.diagonal(T, axis1=-2, axis2=-1))).sum(-1)
    return -2 * np.log(np.abs(T)).sum(-1) if prior['var_dim'] == 'diag' else -2 * K * np.log(T)


def prior_log_density(prior, z, y):
    K = z.shape[1]
    return -0.5 * K * LOG2PI - 0.5 * (_whiten(prior, z - prior['means'][y], y) ** 2).sum(1) - 0.5 * _log_det(prior, y, K)


def prior_kl(prior, mu, lv, y):
    """KL(N(mu, diag e^lv) || p(. | y)) = 1/2 (|T (mu - m)|^2 + tr(T^T T diag(var)) - sum lv + log |Sigma_y| - K)."""
    K = mu.shape[1]
    T = prior['T'][y]
    diag = (np.tril(T) ** 2).sum(-2) if prior['var_dim'] == 'full' else (T ** 2 if prior['var_dim'] == 'diag' else (T ** 2)[:, None])
    return 0.5 * ((_whiten(prior, mu - prior['means'][y], y) ** 2).sum(1) + (diag * np.exp(lv)).sum(1) - lv.sum(1) + _log_det(prior, y, K) - K)


def elbo_restatement(mu, lv, labels, prior, eps, rows=None, z=None, dims=True):
    """The figures of net.elbo_decomposition in fp64 from the bank (fp32 mu, lv, labels), the queried rows (None: all), the noise
    eps (M, K) and - where the caller has them - the fp32 codes z the model drew (else fp32(mu + exp(lv / 2) eps)).  -> the figures
    and, under 'bound', u-free first-order bounds of the KERNEL's share of each figure's error (the means of B)."""
    mu, lv, eps = (np.asarray(a, dtype=np.float32) for a in (mu, lv, eps))
    labels = np.asarray(labels).astype(np.int64)
    N, K = mu.shape
    rows = np.arange(N) if rows is None else np.asarray(rows)
    M = len(rows)
    qm, ql, e = mu[rows].astype(np.float64), lv[rows].astype(np.float64), eps.astype(np.float64)
    if z is None:
        z = (qm + np.exp(0.5 * ql) * e).astype(np.float32)
    z = np.asarray(z, dtype=np.float32)
    cond = prior['conditional']
    y = labels[rows] if cond else np.zeros(M, dtype=np.int64)
    lqzx = -0.5 * (e * e + ql + LOG2PI).sum(1)
    ref = aggpost_reference(mu, lv, labels, z, y, cond)
    logq, qsum = ref['logq'], ref['logq_dims'].sum(1)
    logp = prior_log_density(prior, z.astype(np.float64), y)
    kl_rows = prior_kl(prior, qm, ql, y)
    out = {'kl': kl_rows.mean(), 'kl_mc': (lqzx - logp).mean(), 'mi': (lqzx - logq).mean(), 'kl_marginal': (logq - logp).mean(),
           'tc': (logq - qsum).mean() if dims else None, 'dwkl': None, 'dwkl_per_dim': None, 'mi_bound': math.log(N), 'n': N, 'm': M}
    bound = {'mi': ref['B'].mean(), 'kl_marginal': ref['B'].mean(), 'tc': (ref['B'] + ref['B_dims'].sum(1)).mean(),
             'dwkl': ref['B_dims'].sum(1).mean(), 'dwkl_per_dim': ref['B_dims'].mean(0)}
    if dims and prior['var_dim'] in ('scalar', 'diag'):
        T = prior['T'][y] if prior['var_dim'] == 'diag' else np.repeat(prior['T'][y][:, None], K, 1)
        logp_k = -0.5 * LOG2PI - 0.5 * ((z.astype(np.float64) - prior['means'][y]) * T) ** 2 + np.log(np.abs(T))
        out['dwkl'], out['dwkl_per_dim'] = (qsum - logp).mean(), (ref['logq_dims'] - logp_k).mean(0)
    if cond:
        C = prior['means'].shape[0]
        count = np.bincount(y, minlength=C)
        with np.errstate(invalid='ignore', divide='ignore'):
            out['per_class'] = {'count': count, 'mi': np.bincount(y, lqzx - logq, C) / count,
                                'kl_marginal': np.bincount(y, logq - logp, C) / count}
            bound['per_class'] = np.bincount(y, ref['B'], C) / count
        un = aggpost_reference(mu, lv, labels, z)
        out['mi_unconditional'] = (lqzx - un['logq']).mean()
        bound['mi_unconditional'] = un['B'].mean()
    # the prior's own fp32 arithmetic (its log_density and kl run in the latent kernel: a whitening of at most K products per
    # coordinate, a sum of K squares, a handful of sums): (2 K + 8) roundings of the sum of the sizes of its terms
    dist = (_whiten(prior, z.astype(np.float64) - prior['means'][y], y) ** 2).sum(1)
    ld = np.abs(_log_det(prior, y, K))
    bound['logp'] = ((2 * K + 8) * 0.5 * (dist + ld + K * LOG2PI)).mean()
    bound['kl'] = ((2 * K + 8) * 0.5 * (2 * kl_rows + 2 * np.abs(ql).sum(1) + 2 * ld + 2 * K)).mean()
    out.update(bound=bound, summand_kl_mc=lqzx - logp, kl_rows=kl_rows, z=z, logp=logp, ref=ref)
    return out


# ------------------------------------------------------------------------------------------------------------- closed forms
SEED = 7                                               # the committed seed of the statistical checks


def identical_bank(N=40, K=5):
    """All rows equal: q(z) is that one Gaussian."""
    rng = np.random.default_rng(3)
    m0, l0 = rng.normal(0., 1., K).astype(np.float32), rng.uniform(-3., 0., K).astype(np.float32)
    labels = np.zeros(N, dtype=np.int64)
    return np.tile(m0, (N, 1)), np.tile(l0, (N, 1)), labels


def lattice_bank(N=27, K=3, sigma=0.05):
    """Means on a cubic lattice of spacing g in the first three coordinates (0 in the others) with g^2 / sigma^2 = 400 >= 200: a
    draw within 4 sigma of its row sees every other row at more than (20 - 4)^2 / 2 = 128 nats below its own."""
    side = round(N ** (1 / 3))
    assert side ** 3 == N and K >= 3
    g = 20 * sigma
    mu = np.zeros((N, K), dtype=np.float32)
    mu[:, :3] = np.stack(np.meshgrid(*[np.arange(side) * g] * 3, indexing='ij'), -1).reshape(N, 3)
    return mu, np.full((N, K), 2 * math.log(sigma), dtype=np.float32), np.zeros(N, dtype=np.int64)


def noise(M, K, seed=SEED, clip=None):
    e = np.random.default_rng(seed).normal(0., 1., (M, K))
    return (np.clip(e, -clip, clip) if clip else e).astype(np.float32)


def check_identical(res, bank, prior, z=None):
    """Closed form 1 on a result (the restatement's here, the model's in the GPU test): mi = tc = 0 within the bound,
    kl_marginal = KL(that Gaussian || prior) within 5 standard errors of its summand."""
    mu, lv, labels = bank
    ref = elbo_restatement(mu, lv, labels, prior, noise(len(mu), mu.shape[1]), z=z)
    assert abs(res['mi']) <= U * ref['bound']['mi'] and abs(res['tc']) <= U * ref['bound']['tc']
    exact = prior_kl(prior, mu[:1].astype(np.float64), lv[:1].astype(np.float64), np.asarray(labels[:1], dtype=np.int64))[0]
    summand = ref['ref']['logq'] - ref['logp']
    se = summand.std(ddof=1) / math.sqrt(len(summand))
    print('identical posteriors: mi', res['mi'], 'tc', res['tc'], 'kl_marginal', res['kl_marginal'], 'closed form', exact, 'se', se)
    assert abs(res['kl_marginal'] - exact) <= 5 * se + U * ref['bound']['kl_marginal']
    return ref


def check_separated(res, bank, prior, z=None):
    """Closed form 2: mi = log N within the bound (every foreign term is below e^-100)."""
    mu, lv, labels = bank
    ref = elbo_restatement(mu, lv, labels, prior, noise(len(mu), mu.shape[1], clip=4.), z=z)
    print('separated posteriors: mi', res['mi'], 'log N', math.log(len(mu)), 'bound', U * ref['bound']['mi'])
    assert abs(res['mi'] - math.log(len(mu))) <= U * ref['bound']['mi'] + 1e-40
    assert res['mi_bound'] == math.log(len(mu))
    return ref


def check_identities(res):
    # fp64 means of M summands of a size of up to a few hundred nats: 1024 roundings of the figures' sizes
    tol = 1024 * 2. ** -52 * (1 + abs(res['kl_mc']) + abs(res['mi']) + abs(res['kl_marginal']) + abs(res['tc'] or 0.))
    assert abs(res['kl_mc'] - (res['mi'] + res['kl_marginal'])) <= tol
    if res['dwkl'] is not None:
        assert abs(res['kl_marginal'] - (res['tc'] + res['dwkl'])) <= tol + 1024 * 2. ** -52 * abs(res['dwkl'])


STD_PRIOR = gaussian_prior(np.zeros((1, 5)))


def test_identical_posteriors():
    bank = identical_bank()
    res = elbo_restatement(*bank, STD_PRIOR, noise(40, 5))
    check_identical(res, bank, STD_PRIOR)
    check_identities(res)
    assert res['dwkl'] is not None and abs(res['dwkl_per_dim'].sum() - res['dwkl']) <= 1e-12


def test_separated_posteriors():
    bank = lattice_bank()
    prior = gaussian_prior(np.zeros((1, 3)))
    res = elbo_restatement(*bank, prior, noise(27, 3, clip=4.))
    check_separated(res, bank, prior)
    check_identities(res)


@pytest.mark.parametrize('var_dim', ['scalar', 'diag', 'full'])
def test_identities_and_the_statistical_check(var_dim):
    """kl_mc is an unbiased estimate of kl row by row: |kl_mc - kl| <= 5 standard errors of the summand at the committed seed (a
    condition with a false alarm below 1e-6, not a measurement); a conditional prior of every variance layout."""
    rng = np.random.default_rng(11)
    N, K, C = 300, 4, 3
    mu, lv = rng.normal(0., 1., (N, K)).astype(np.float32), rng.uniform(-4., 0., (N, K)).astype(np.float32)
    labels = rng.integers(0, C, N)
    T = {'scalar': rng.uniform(.5, 2., C), 'diag': rng.uniform(.5, 2., (C, K)), 'full': np.tril(rng.normal(0., .3, (C, K, K))) + np.eye(K)}
    prior = gaussian_prior(rng.normal(0., 1., (C, K)), T[var_dim], var_dim, True)
    res = elbo_restatement(mu, lv, labels, prior, noise(N, K))
    check_identities(res)
    d = res['summand_kl_mc'] - res['kl_rows']
    se = d.std(ddof=1) / math.sqrt(N)
    print(var_dim, 'kl', res['kl'], 'kl_mc', res['kl_mc'], 'se', se)
    assert abs(res['kl_mc'] - res['kl']) <= 5 * se
    assert (res['dwkl'] is None) == (var_dim == 'full') and res['per_class']['count'].sum() == N
    assert 0 <= res['mi'] <= res['mi_unconditional'] + 5 * se <= math.log(N) + 5 * se
    sub = elbo_restatement(mu, lv, labels, prior, noise(50, K), rows=np.arange(50) * 3)
    check_identities(sub)
    assert sub['m'] == 50 and sub['n'] == N


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_the_bound_stays_below_its_limit(case):
    K, N, M, G, empty = case
    mu, lv, group, z, zgroup = aggpost_case(*case)
    assert mu.shape == lv.shape == (N, K) and z.shape == (M, K) and len(set(group.tolist())) == (min(G, N) - (1 if empty else 0))
    assert np.isclose(np.exp(lv.astype(np.float64)).min(), 1e-4) and (N * K == 1 or np.exp(lv).max() == 1.)
    for conditional in (False, True):
        ref = case_reference(case, conditional)
        assert_limit(ref, K, N, V_DATA)
        gone = ~np.isfinite(ref['logq'])
        assert gone.any() == (empty and conditional) and (not gone.any() or (zgroup[gone] == 1).all())
        assert np.isfinite(ref['logq_dims'][~gone]).all()
        print(case_id(case), 'conditional' if conditional else 'whole bank', 'B / (1 + |ref|) at most',
              float((ref['B'][~gone] / (1 + np.abs(ref['logq'][~gone]))).max()), 'limit', b_limit(K, N, V_DATA))


def test_the_far_queries_need_the_shift():
    case = CASES[3]
    mu, lv, group, z, zgroup = aggpost_case(*case)
    plain = unshifted_fp32(mu, lv, z)
    far = np.arange(len(z)) % 10 == 9                  # 10^4 sigma
    assert far.any() and np.isinf(plain[far]).all() and np.isfinite(case_reference(case, False)['logq']).all()
