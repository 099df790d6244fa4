"""The Mahalanobis scores (ops.maha_moments / maha_fit / maha_scores, csrc/maha.hip) restated in numpy
fp64, the error bars the kernel is held to, and the kernel's own formula as an fp32 chain - no code under test runs here; the GPU
tests (tests/test_29_maha_gpu.py) import the data, the restatement and the bars from this file.

Data, `maha_case(K, N, M, C, offset, seed)`: A = (I + 0.3 G / sqrt(K)) with its rows scaled by linspace(0.5, 2, K), class centres
3 g + offset, bank and queries centre[label] + g A^T in fp32, the second half of the queries with 2 g of extra noise.

Restatement: the moments as ops.maha_moments defines them, d_c = (q - mu_c)^T S^-1 (q - mu_c) through np.linalg.inv of the
regularised matrices, a stable argmin.

Bars, u = 2^-24, W the inverse Cholesky factor: a_k = sum_j |W_kj| |q_j - mean0_j|, eta_ck = (K + 4) u (a_k + |m_ck|),
bar_c = sum_k (2 |e_ck| eta_ck + eta_ck^2) + (K + 2) u d_c with e_c = W (q - mu_c) and m_c the fp64 whitened centred class mean;
bar_0 the same with W0 and m = 0.  eta bounds the error of one y_k - m_ck for any summation order - the rounding of W, of x and
of m, a K-term fp32 accumulation, the subtraction - and the last term the squares and their sum.  min is 1-Lipschitz in the sup
norm: d is held to max_c bar_c, rel to max_c bar_c + bar_0, a per-class entry to its own bar_c, and cls must name a class whose
fp64 distance is within 2 max_c bar_c of the fp64 minimum.  So that a bar cannot hide a wrong result, max_c bar_c <= 5e-3 min_c d_c
is asserted for every row of every shape."""
import numpy as np
import pytest

U = 2. ** -24
# (K, N, M, C, offset, shrinkage): the smallest at which the 32-row tiling, the padding of K, the chunking above 64 columns, the
# class limit and the offset can go wrong
SHAPES = [(1, 3, 5, 1, 0., 0.), (3, 5, 40, 2, 0., 0.), (16, 130, 500, 10, 30., 0.), (64, 67, 1000, 10, 0., 0.),
          (64, 67, 1000, 10, 30., 0.), (65, 33, 700, 3, 30., 0.), (130, 40, 2000, 10, 0., 0.), (256, 33, 3000, 128, 30., 0.),
          (64, 67, 100, 10, 30., 1e-3)]
SEED = 7


def maha_case(K, N, M, C, offset, seed=SEED):
    """-> (q (N, K) fp32, bank (M, K) fp32, labels (M,) int64): every class has a row when M >= C."""
    rng = np.random.default_rng([seed, K, N, M, C])
    A = (np.eye(K) + 0.3 * rng.standard_normal((K, K)) / np.sqrt(K)) * np.linspace(0.5, 2., K)[:, None]
    centres = 3. * rng.standard_normal((C, K)) + offset
    yb = rng.permutation(np.arange(M) % C).astype(np.int64)
    yq = rng.integers(0, C, N)
    bank = centres[yb] + rng.standard_normal((M, K)) @ A.T
    q = centres[yq] + rng.standard_normal((N, K)) @ A.T
    q[N // 2:] += 2. * rng.standard_normal((N - N // 2, K))
    return q.astype(np.float32), bank.astype(np.float32), yb


_CASES = {}


def case(shape):
    """The data, the fp64 moments, the restated scores and the bars of one shape, computed once and never modified."""
    if shape not in _CASES:
        K, N, M, C, offset, shrinkage = shape
        q, bank, labels = maha_case(K, N, M, C, offset)
        mom = moments_restatement(bank, labels, C)
        _CASES[shape] = dict(q=q, bank=bank, labels=labels, mom=mom, ref=scores_restatement(q, mom, shrinkage),
                             bars=bars(q, mom, shrinkage))
    return _CASES[shape]


def moments_restatement(bank, labels, C):
    """fp64: counts (C,), means (C, K) (zeros for an empty class), mean0 (K,), Sw and St (K, K), both divided by M."""
    b = bank.astype(np.float64)
    M = b.shape[0]
    counts = np.bincount(labels, minlength=C).astype(np.int64)
    means = np.zeros((C, b.shape[1]))
    for c in np.flatnonzero(counts):
        means[c] = b[labels == c].mean(0)
    mean0 = b.mean(0)
    xw, xt = b - means[labels], b - mean0
    return dict(counts=counts, means=means, mean0=mean0, Sw=xw.T @ xw / M, St=xt.T @ xt / M)


def regularised(S, shrinkage):
    return S + shrinkage * (np.trace(S) / S.shape[0]) * np.eye(S.shape[0])


def whitener(S, shrinkage):
    return np.linalg.inv(np.linalg.cholesky(regularised(S, shrinkage)))


def scores_restatement(q, mom, shrinkage):
    """fp64 -> dict(dc (N, C) with +inf for an empty class, d0 (N,), d (N,), cls (N,), rel (N,))."""
    x = q.astype(np.float64)
    Si, S0i = np.linalg.inv(regularised(mom['Sw'], shrinkage)), np.linalg.inv(regularised(mom['St'], shrinkage))
    diff = x[:, None, :] - mom['means'][None]
    dc = np.einsum('nck,kl,ncl->nc', diff, Si, diff)
    dc[:, mom['counts'] == 0] = np.inf
    x0 = x - mom['mean0']
    d0 = np.einsum('nk,kl,nl->n', x0, S0i, x0)
    return dict(dc=dc, d0=d0, d=dc.min(1), cls=dc.argmin(1), rel=(dc - d0[:, None]).min(1))


def bars(q, mom, shrinkage):
    """-> dict(bar (N, C), +inf for an empty class: never the largest; bar0 (N,); top (N,) = the largest bar_c of a row)."""
    x0 = q.astype(np.float64) - mom['mean0']
    K = x0.shape[1]
    W, W0 = whitener(mom['Sw'], shrinkage), whitener(mom['St'], shrinkage)
    m = (mom['means'] - mom['mean0']) @ W.T                                  # (C, K)
    y = x0 @ W.T
    e = y[:, None, :] - m[None]                                              # W (q - mu_c)
    a = np.abs(x0) @ np.abs(W).T
    eta = (K + 4) * U * (a[:, None, :] + np.abs(m)[None])
    dc = (e * e).sum(2)
    bar = (2 * np.abs(e) * eta + eta * eta).sum(2) + (K + 2) * U * dc
    kept = mom['counts'] > 0
    e0 = x0 @ W0.T
    eta0 = (K + 4) * U * (np.abs(x0) @ np.abs(W0).T)
    bar0 = (2 * np.abs(e0) * eta0 + eta0 * eta0).sum(1) + (K + 2) * U * (e0 * e0).sum(1)
    return dict(bar=np.where(kept[None], bar, np.inf), bar0=bar0, top=bar[:, kept].max(1))


def operands(mom, shrinkage):
    """What the host prepares once per fit: fp64, rounded once to fp32 -> (mu0_32, W32, W0_32, m32 of the non-empty classes,
    m0_32, cmap); m0 = W0 (mean0 - mu0_32), the whitened rounding error of mu0_32, is to d0 what a class mean is to d_c: with it
    the rounding of mean0 cancels in d0 as well (without it a row near mean0 leaves bar_0: K = 1, |mean0| u / sigma against a
    distance of 6e-4)."""
    kept = np.flatnonzero(mom['counts'] > 0)
    W, W0 = np.tril(whitener(mom['Sw'], shrinkage)), np.tril(whitener(mom['St'], shrinkage))
    mu0 = mom['mean0'].astype(np.float32)
    m = (mom['means'][kept] - mu0.astype(np.float64)) @ W.T
    m0 = W0 @ (mom['mean0'] - mu0.astype(np.float64))
    return mu0, W.astype(np.float32), W0.astype(np.float32), m.astype(np.float32), m0.astype(np.float32), kept


def fma32(a, b, c):
    """fp32(a * b + c) with one rounding: the product of two fp32 values is exact in fp64 (the sum's fp64 rounding is at 2^-29
    of an fp32 ulp and moves the result in no case that matters to a bar)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_chain(q, mom, shrinkage):
    """The kernel's formula in fp32: x = q - mu0_32, y_k and y0_k fmaf chains over j ascending, d_c = chain over k ascending of
    (y_k - m_ck)^2, d0 = chain of (y0_k - m0_k)^2 -> dict(dc (N, C) with +inf for an empty class, d, cls, rel)."""
    mu0, W, W0, m, m0, kept = operands(mom, shrinkage)
    x = q - mu0
    N, K = x.shape
    y, y0 = np.zeros((N, K), np.float32), np.zeros((N, K), np.float32)
    for j in range(K):
        y, y0 = fma32(x[:, j:j + 1], W[None, :, j], y), fma32(x[:, j:j + 1], W0[None, :, j], y0)
    dk, d0 = np.zeros((N, len(kept)), np.float32), np.zeros(N, np.float32)
    for k in range(K):
        t, t0 = y[:, k:k + 1] - m[None, :, k], y0[:, k] - m0[k]
        dk, d0 = fma32(t, t, dk), fma32(t0, t0, d0)
    dc = np.full((N, len(mom['counts'])), np.inf, np.float32)
    dc[:, kept] = dk
    return dict(dc=dc, d=dk.min(1), cls=kept[dk.argmin(1)], rel=(dk - d0[:, None]).min(1))


def check_scores(got, ref, bar, tag, bad=None):
    """`got` (d, cls, rel, and dc or None, as arrays) against the restatement `ref` inside the bars `bar`, every figure printed
    before it is asserted; bad: the rows that have to be NaN / -1 -> the worst error / bar of the case."""
    N = ref['d'].shape[0]
    good = np.ones(N, bool) if bad is None else ~bad
    d, cls, rel = (np.asarray(got[k]) for k in ('d', 'cls', 'rel'))
    assert d.shape == rel.shape == cls.shape == (N,)
    assert np.isnan(d[~good]).all() and np.isnan(rel[~good]).all() and (cls[~good] == -1).all()
    top, bar0 = bar['top'][good], bar['bar0'][good]
    ratios = {'d': np.abs(d[good].astype(np.float64) - ref['d'][good]) / top,
              'rel': np.abs(rel[good].astype(np.float64) - ref['rel'][good]) / (top + bar0)}
    kept = np.isfinite(ref['dc'][0])
    assert ((cls[good] >= 0) & (cls[good] < kept.size)).all() and kept[cls[good]].all()          # never an empty class
    named = ref['dc'][good, cls[good]]
    ratios['cls (held to 2)'] = (named - ref['d'][good]) / top
    if got.get('dc') is not None:
        dc = np.asarray(got['dc'])
        assert dc.shape == ref['dc'].shape and (dc[good][:, ~kept] == np.inf).all() and np.isnan(dc[~good]).all()
        ratios['per class'] = (np.abs(dc[good][:, kept].astype(np.float64) - ref['dc'][good][:, kept]) / bar['bar'][good][:, kept]).max(1)
    worst = {k: float(v.max()) if v.size else 0. for k, v in ratios.items()}
    print(tag, 'worst error / bar:', worst, 'largest bar / d', float((bar['top'] / ref['d']).max()))
    assert all(v <= (2. if k.startswith('cls') else 1.) for k, v in worst.items()), (tag, worst)
    return max(v for k, v in worst.items() if not k.startswith('cls'))


@pytest.mark.parametrize('shape', SHAPES)
def test_the_restatement_agrees_with_itself(shape):
    K, N, M, C, offset, shrinkage = shape
    c = case(shape)
    mom, ref = c['mom'], c['ref']
    assert mom['counts'].sum() == M and (mom['counts'] > 0).all()
    assert np.allclose(mom['St'], np.cov(c['bank'].astype(np.float64).T, bias=True).reshape(K, K), rtol=1e-9, atol=1e-12)
    # the whitened form of the bars is the inverse form of the restatement
    W = whitener(mom['Sw'], shrinkage)
    e = (c['q'].astype(np.float64)[:, None, :] - mom['means'][None]) @ W.T
    cond = np.linalg.cond(regularised(mom['Sw'], shrinkage))
    print(shape, 'condition number of Sw', float(cond))
    assert np.allclose((e * e).sum(2), ref['dc'], rtol=1e-13 * cond + 1e-12)
    assert (ref['cls'] == ref['dc'].argmin(1)).all() and (ref['rel'] == ref['d'] - ref['d0']).all()
    if shrinkage:
        assert not np.allclose(scores_restatement(c['q'], mom, 0.)['d'], ref['d'], rtol=1e-6)


@pytest.mark.parametrize('shape', SHAPES)
def test_a_bar_cannot_hide_a_wrong_result(shape):
    c = case(shape)
    ratio = c['bars']['top'] / c['ref']['d']
    print(shape, 'largest bar / smallest distance per row: worst', float(ratio.max()))
    assert (c['bars']['top'] <= 5e-3 * c['ref']['d']).all()


@pytest.mark.parametrize('shape', SHAPES)
def test_the_fp32_chain_sits_inside_the_bars(shape):
    c = case(shape)
    worst = check_scores(kernel_chain(c['q'], c['mom'], shape[5]), c['ref'], c['bars'], f'chain {shape}')
    assert worst <= 1.


def test_an_empty_class_is_never_the_argmin():
    q, bank, labels = maha_case(16, 20, 300, 5, 0.)
    keep = labels != 2
    mom = moments_restatement(bank[keep], labels[keep], 5)
    ref = scores_restatement(q, mom, 0.)
    assert mom['counts'][2] == 0 and (mom['means'][2] == 0).all() and np.isinf(ref['dc'][:, 2]).all() and (ref['cls'] != 2).all()
    chain = kernel_chain(q, mom, 0.)
    assert np.isinf(chain['dc'][:, 2]).all() and (chain['cls'] != 2).all()
    check_scores(chain, ref, bars(q, mom, 0.), 'chain, class 2 empty')
