"""The density-of-states scores (ops.kde_fit / ops.kde_logdensity, csrc/dose.hip) restated in numpy fp64,
the data of the kernel tests and the tolerance the kernel is held to - no code under test runs here; the GPU tests
(tests/test_31_dose_gpu.py) import the data, the restatement and the tolerance from this file.

Data, `dose_case(S, M, N)`: row s of the bank is offset_s + scale_s g in fp32 with the offsets (-3000, 30, 25, 0.01, -2990) and
the scales (40, 3, 2, 1e-3, 40) (rows 5 .. 7 take them again from the start); a query is offset_s + f scale_s g with f = 8 for
every fifth query from the fourth and f = 1e4 for every fifth from the fifth, else 1.

Tolerance, u = 2^-24: c u (1 + |ref|) with c = `dose_c(...)`, the first-order bound of DESIGN.md section 7s evaluated in fp64 on
the inputs of the case, over every marginal and joint entry (with w_m the weights exp(E_m) / sum exp(E) of a query's terms):
  operands     sum_m w_m |d_m| (|t| + |z_m| + |d_m|)   t, z rounded once (u |t|, u |z_m|), the difference rounded (u |d_m|)
  squares      sum_m w_m d_m^2 / 2                     the square, rounded (the smallest square is subtracted as computed)
  shifts       5 sum_m w_m (E_max - E_m) + 2 |E_max|   d^2 - min d^2, the constant -log2(e) / 2 and the product, u times
                                                       their size each; a = fp32(k min d^2): the constant and the product
                                                       again, on the piece's and on the query's largest exponent
  chain        12 + 2 ceil(log2 pieces)                the roundings on the way of one term through the pairwise sums
  the rest     5 + 2 ln(sum) + |ref| + 1               v_exp_f32 (1 ulp), exp2f and the product of the merge, log2f, the
                                                       result rounded once, and 1 for what the fp64 steps leave
(the joint row: the operands summed over s with the factor (h1 / hS)^2, S roundings on |E_m| for its fmaf chain instead of the
one of a square), divided by 1 + |ref|.  `dose` is the fp64 sum of its marginals rounded once: it is held to the sum of their
tolerances - under cancellation the derivation gives no bound relative to |dose| itself - and, besides, to the limit of the form
itself, 64 u (1 + |dose|): whichever is smaller.  The typicality rows are fp64 rounded once: c = 2."""
import math

import numpy as np
import pytest

U = 2. ** -24
OFFSETS = (-3000., 30., 25., 0.01, -2990.)
SCALES = (40., 3., 2., 1e-3, 40.)
C_LIMIT = 64.                   # a derived c above it means the summation chain is too long
# (S, M, N): one bank value pair, sizes around the 64 queries of a workgroup and the 16 / 256 values of the inner sums, more
# than one piece of the bank
SHAPES = [(1, 2, 1), (1, 2, 3), (5, 63, 1), (5, 64, 64), (5, 65, 65), (3, 257, 129), (8, 4096, 257)]
SEED = 11


def dose_case(S, M, N, seed=SEED):
    """-> (stats (S, N) fp32, bank (S, M) fp32)."""
    rng = np.random.default_rng([seed, S, M, N])
    off = np.array([OFFSETS[s % 5] for s in range(S)])[:, None]
    scale = np.array([SCALES[s % 5] for s in range(S)])[:, None]
    bank = off + scale * rng.standard_normal((S, M))
    i = np.arange(N)
    far = np.where(i % 5 == 4, 1e4, np.where(i % 5 == 3, 8., 1.))
    stats = off + scale * far * rng.standard_normal((S, N))
    return stats.astype(np.float32), bank.astype(np.float32)


def fit_restatement(bank, bandwidth=1.0):
    """fp64: centre, sigma (ddof = 1), h1 = bandwidth sigma M^(-1/5), hS = bandwidth sigma M^(-1/(S+4)), lognorm (S + 1,)."""
    b = np.asarray(bank, dtype=np.float64)
    S, M = b.shape
    centre, sigma = b.mean(1), b.std(1, ddof=1)
    h1, hS = bandwidth * sigma * M ** (-1. / 5), bandwidth * sigma * M ** (-1. / (S + 4))
    lognorm = np.append(np.log(M * h1 * math.sqrt(2 * math.pi)), math.log(M) + np.log(hS).sum() + 0.5 * S * math.log(2 * math.pi))
    return dict(centre=centre, sigma=sigma, h1=h1, hS=hS, lognorm=lognorm)


def _lse(E):
    top = E.max(1, keepdims=True)
    shift = np.where(np.isneginf(top), 0., top)                     # every term exp(-inf) = 0: log 0 = -inf, not inf - inf
    with np.errstate(divide='ignore'):
        return shift[:, 0] + np.log(np.exp(E - shift).sum(1))


def dose_restatement(stats, bank, bandwidth=1.0):
    """The definitions in fp64: stats (S, N), bank (S, M) -> (2 S + 2, N): the marginal log-densities, `dose`, `dose-joint`, the
    typicality rows.  A non-finite statistic gives NaN / -inf by the arithmetic itself."""
    T, B = np.asarray(stats, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    S, N = T.shape
    f = fit_restatement(B, bandwidth)
    out = np.empty((2 * S + 2, N))
    joint = np.zeros((N, B.shape[1]))
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(S):
            out[s] = _lse(-0.5 * ((T[s][:, None] - B[s][None]) / f['h1'][s]) ** 2) - f['lognorm'][s]
            joint += -0.5 * ((T[s][:, None] - B[s][None]) / f['hS'][s]) ** 2
            out[S + 2 + s] = -np.abs(T[s] - f['centre'][s]) / f['sigma'][s]
        out[S] = sum(out[s] for s in range(S))
        out[S + 1] = _lse(joint) - f['lognorm'][S]
    return out


def chain_depth(M, partition):
    """Roundings on the way of one term through the kernel's sums: 16 values as a tree (4), four of those and four of those in
    sequence (3 + 3), the four waves as a tree (2), the pieces pairwise (at most 2 ceil(log2 pieces))."""
    pieces = -(-M // partition)
    return 12 + (2 * math.ceil(math.log2(pieces)) if pieces > 1 else 0)


def dose_c(stats, bank, bandwidth, partition):
    """The derived c of the module docstring for one case: the largest bound / (u (1 + |ref|)) over the finite marginal and
    joint entries."""
    T, B = np.asarray(stats, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    S, N = T.shape
    M = B.shape[1]
    f = fit_restatement(B, bandwidth)
    ref = dose_restatement(stats, bank, bandwidth)
    depth = chain_depth(M, partition)
    ratio2 = (f['h1'][0] / f['hS'][0]) ** 2
    worst = 0.
    EJ, opJ = np.zeros((N, M)), np.zeros((N, M))
    for s in range(S + 1):
        if s < S:
            t, z = (T[s] - f['centre'][s]) / f['h1'][s], (B[s] - f['centre'][s]) / f['h1'][s]
            d = t[:, None] - z[None]
            E = -0.5 * d * d
            op = np.abs(d) * (np.abs(t)[:, None] + np.abs(z)[None] + np.abs(d))
            squares = -E
            EJ += ratio2 * E
            opJ += ratio2 * op
        else:
            E, op, squares = EJ, opJ, S * -EJ
        top = E.max(1, keepdims=True)
        w = np.exp(E - top)
        total = w.sum(1)
        w /= total[:, None]
        size = np.abs(ref[s if s < S else S + 1])
        bound = ((w * (op + squares + 5 * (top - E))).sum(1) + 2 * np.abs(top[:, 0]) + depth + 5 + 2 * np.log(total) + size + 1)
        worst = max(worst, float((bound / (1 + size)).max()))
    return worst


def tolerance(ref, c):
    """(2 S + 2, N) absolute tolerances for the restated `ref`: c u (1 + |ref|) on the marginal and joint rows; on `dose` the sum
    of the marginals' and never more than C_LIMIT u (1 + |dose|); 2 u (1 + |ref|) on the typicality rows."""
    S = (ref.shape[0] - 2) // 2
    tol = c * U * (1 + np.abs(ref))
    tol[S] = np.minimum(tol[:S].sum(0), C_LIMIT * U * (1 + np.abs(ref[S])))
    tol[S + 2:] = 2 * U * (1 + np.abs(ref[S + 2:]))
    return tol


def rank_auc(ins, outs):
    """P(in > out) + P(in = out) / 2."""
    ins, outs = np.asarray(ins)[:, None], np.asarray(outs)[None]
    return float((ins > outs).mean() + 0.5 * (ins == outs).mean())


def test_marginals_are_scipy_s_gaussian_kde():
    stats_mod = pytest.importorskip('scipy.stats')
    stats, bank = dose_case(5, 300, 40)
    near = stats[:, np.arange(40) % 5 < 3].astype(np.float64)        # scipy's logpdf underflows on the far queries: it does not shift
    ref = dose_restatement(near, bank)
    for s in range(5):
        kde = stats_mod.gaussian_kde(bank[s].astype(np.float64))
        np.testing.assert_allclose(ref[s], kde.logpdf(near[s]), rtol=1e-12, atol=0)
    # a bandwidth factor is scipy's bw_method relative to Scott's
    ref2 = dose_restatement(near, bank, 0.5)
    kde = stats_mod.gaussian_kde(bank[1].astype(np.float64), bw_method=0.5 * 300 ** (-1. / 5))
    np.testing.assert_allclose(ref2[1], kde.logpdf(near[1]), rtol=1e-12, atol=0)


def test_two_bank_values_by_hand():
    a, b, T = 1.5, 4.0, np.array([0.5, 2.0, 9.0])
    ref = dose_restatement(T[None], np.array([[a, b]]))
    sigma = abs(a - b) / math.sqrt(2.)
    h = sigma * 2. ** (-1. / 5)
    by_hand = np.log((np.exp(-0.5 * ((T - a) / h) ** 2) + np.exp(-0.5 * ((T - b) / h) ** 2)) / (2 * h * math.sqrt(2 * math.pi)))
    assert ref.shape == (4, 3)
    np.testing.assert_allclose(ref[0], by_hand, rtol=1e-14)
    assert np.array_equal(ref[1], ref[0])                            # `dose` of one statistic is its marginal
    np.testing.assert_allclose(ref[2], by_hand, rtol=1e-14)          # ... and so is the joint row: h(S) = h(1) at S = 1
    np.testing.assert_allclose(ref[3], -np.abs(T - 2.75) / sigma, rtol=1e-15)


def test_the_definitions_of_the_joint_row_and_of_dose():
    stats, bank = dose_case(3, 50, 7)
    ref = dose_restatement(stats, bank, 0.7)
    f = fit_restatement(bank, 0.7)
    T, B = stats.astype(np.float64), bank.astype(np.float64)
    for i in range(7):
        dens = np.prod([np.exp(-0.5 * ((T[s, i] - B[s]) / f['hS'][s]) ** 2) / (f['hS'][s] * math.sqrt(2 * math.pi)) for s in range(3)],
                       axis=0).mean()
        if dens > 1e-300:
            assert abs(ref[4, i] - math.log(dens)) <= 1e-12 * (1 + abs(ref[4, i]))
    np.testing.assert_allclose(ref[3], ref[0] + ref[1] + ref[2], rtol=1e-15)
    np.testing.assert_allclose(f['hS'], 0.7 * B.std(1, ddof=1) * 50 ** (-1. / 7), rtol=1e-15)
    assert np.all(np.isfinite(ref)) and ref[:5].min() < -1e7         # the far queries: finite and far down


def test_a_score_that_is_too_good_ranks_last():
    """In-scores and bank from N(0, 1), out-scores from N(3, 0.3^2): the raw one-sided score ranks the outliers FIRST."""
    rng = np.random.default_rng(5)
    bank, ins, outs = rng.standard_normal(2000), rng.standard_normal(500), 3 + 0.3 * rng.standard_normal(500)
    r_in, r_out = dose_restatement(ins[None], bank[None]), dose_restatement(outs[None], bank[None])
    raw, dose, typ = rank_auc(ins, outs), rank_auc(r_in[1], r_out[1]), rank_auc(r_in[3], r_out[3])
    print(f'AUC raw {raw:.4f} dose {dose:.4f} typicality {typ:.4f}')
    assert raw < 0.05 and dose > 0.95 and typ > 0.95


def test_non_finite_statistics_by_the_arithmetic():
    stats, bank = dose_case(3, 20, 4)
    stats = stats.copy()
    stats[1, 2], stats[0, 3] = np.inf, np.nan
    ref = dose_restatement(stats, bank)
    assert ref[1, 2] == -np.inf and ref[3, 2] == -np.inf and ref[4, 2] == -np.inf and ref[6, 2] == -np.inf
    assert np.isfinite(ref[[0, 2, 5, 7], 2]).all()
    assert np.isnan(ref[[0, 3, 4, 5], 3]).all() and np.isfinite(ref[[1, 2, 6, 7], 3]).all()
    assert np.isfinite(ref[:, :2]).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_the_derived_c_stays_below_the_limit(shape):
    """The tolerance of the kernel tests for every shape they use, at the kernel's partition of 1024 values."""
    S, M, N = shape
    stats, bank = dose_case(S, M, N)
    c = dose_c(stats, bank, 1.0, 1024)
    print(f'shape {shape}: derived c = {c:.1f}')
    assert 1 < c <= C_LIMIT
    assert chain_depth(1023, 1024) == chain_depth(1024, 1024) == 12 and chain_depth(1025, 1024) == 14 and chain_depth(50000, 1024) == 24
