"""The k nearest neighbours of ops.knn (csrc/knn.hip) restated without the code under test (no GPU):

`knn_distances`     the (N, M) squared distances in numpy fp64, in the direct form sum_k (q_k - b_k)^2 (of the normalised rows in
                    the normalised mode) - no cancellation, whatever the offset of the data.
`knn_restatement`   the k smallest per row by a stable argsort (ties: the lower bank row), +inf / -1 where the bank has fewer than
                    k rows, a bank row at a non-finite distance never selected, a non-finite query row NaN / -1.  Held here to
                    torch.cdist + topk in fp64 on the fixed cases.
`plain_bar`, `normalized_bar`   the bars of tests/test_28_knn_gpu.py, with u = 2^-24:
      plain       bar_ij = 2 (K + 3) u (|q_i|^2 + |b_j|^2): the worst-case bound gamma_K of a K-term fp32 accumulation, applied to
                  the three summands |q|^2, |b|^2 and 2 q.b (|2 q.b| <= |q|^2 + |b|^2), plus the two additions and the rounding
                  of the result; it holds for any order of summation.
      normalised  bar = 4 (K + 4) u: the same bound on the cosine (|cos| <= 1): twice the dot product's (K u), plus the two
                  norms, the square roots, the product and the division.
    An order statistic is 1-Lipschitz in the sup norm, so slot j of a row is held to max_j' bar_ij' with no element left out.
`kernel_chain`      the kernel's formula as a plain fp32 k-ordered chain in numpy (every fma = one fp64 product and sum rounded to
                    fp32), to show that the formula itself sits inside the bars on the cases the GPU test uses."""
import numpy as np
import pytest
import torch

U = 2.0 ** -24
# (K, N, M, k): the smallest shapes at which tiling (32 bank rows, 32 query rows per wave, 128 per workgroup), the zero padding
# of K (steps of 2, groups of 8, chunks of 64), the partition merge and the list (k = 64: every lane) can go wrong
SHAPES = [(1, 1, 1, 1), (3, 5, 63, 64), (64, 33, 64, 64), (65, 67, 65, 2), (130, 130, 1000, 50), (64, 67, 4099, 50), (2, 1, 4099, 1)]
VARIANT_SHAPE = (64, 67, 4099, 50)
VARIANTS = ('copies', 'duplicates', 'offset', 'nan')
COPIES = ((5, 0), (2000, 33), (4098, 66))           # (bank row, query row) of the 'copies' variant
NAN_BANK_ROW, NAN_QUERY_ROW = 77, 10


def knn_case(K, N, M, variant=None, seed=None):
    """-> (q (N, K), bank (M, K)) fp32 numpy arrays; a property of the shape (and the variant) alone."""
    g = np.random.default_rng(1000 * K + 10 * N + M if seed is None else seed)
    q = g.standard_normal((N, K)).astype(np.float32)
    bank = g.standard_normal((M, K)).astype(np.float32)
    if variant == 'copies':
        for b, i in COPIES:
            bank[b] = q[i]
    elif variant == 'duplicates':
        bank[-200:] = bank[:200]
    elif variant == 'offset':                        # the cancellation case: |q|^2 + |b|^2 is 900 K times the distance's scale
        q, bank = (30 + q).astype(np.float32), (30 + bank).astype(np.float32)
    elif variant == 'nan':
        bank[NAN_BANK_ROW, 3] = np.nan
        q[NAN_QUERY_ROW, K - 1] = np.nan
    elif variant is not None:
        raise KeyError(variant)
    return q, bank


def _unit(x):
    n = np.sqrt((x * x).sum(1, keepdims=True))
    return x / np.maximum(n, 1e-12)


def knn_distances(q, bank, normalized):
    """(N, M) fp64 squared distances, direct form, one query row at a time."""
    q, bank = np.asarray(q, np.float64), np.asarray(bank, np.float64)
    if normalized:
        q, bank = _unit(q), _unit(bank)
    out = np.empty((q.shape[0], bank.shape[0]))
    with np.errstate(invalid='ignore'):
        for i in range(q.shape[0]):
            d = bank - q[i]
            out[i] = (d * d).sum(1)
    return out


def select(D, k, bad_query=None):
    """The k smallest of each row of D (N, M) -> (d2 (N, k) fp64 ascending, idx (N, k) int64): stable, a non-finite distance
    never selected, +inf / -1 in the slots nothing fills, NaN / -1 in the rows of `bad_query`."""
    N, M = D.shape
    key = np.where(np.isfinite(D), D, np.inf)
    order = np.argsort(key, axis=1, kind='stable')[:, :k]
    d2 = np.full((N, k), np.inf)
    idx = np.full((N, k), -1, np.int64)
    got = np.take_along_axis(key, order, 1)
    d2[:, :order.shape[1]] = got
    idx[:, :order.shape[1]] = np.where(np.isfinite(got), order, -1)
    if bad_query is not None:
        d2[bad_query] = np.nan
        idx[bad_query] = -1
    return d2, idx


def knn_restatement(q, bank, k, normalized):
    q = np.asarray(q, np.float64)
    return select(knn_distances(q, bank, normalized), k, ~np.isfinite(q).all(1))


def plain_bar(q, bank, K=None):
    """(N,) fp64: max over the finite bank rows j of 2 (K + 3) u (|q_i|^2 + |b_j|^2)."""
    q, bank = np.asarray(q, np.float64), np.asarray(bank, np.float64)
    K = q.shape[1] if K is None else K
    bs = (bank * bank).sum(1)
    top = np.nanmax(np.where(np.isfinite(bs), bs, np.nan)) if bank.shape[0] else 0.
    return 2 * (K + 3) * U * ((q * q).sum(1) + top)


def normalized_bar(K):
    return 4 * (K + 4) * U


def row_bars(q, bank, normalized):
    return np.full(q.shape[0], normalized_bar(q.shape[1])) if normalized else plain_bar(q, bank)


# ------------------------------------------------------------------------------------------- the kernel's formula in fp32
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def chain_sqnorms(x):
    s = np.zeros(x.shape[0], np.float32)
    for k in range(x.shape[1]):
        s = _fma32(x[:, k], x[:, k], s)
    return s


def kernel_chain(q, bank, normalized):
    """(N, M) fp32: csrc/knn.hip's distance of every pair - norms and dot product as k-ordered fmaf chains, then the epilogue."""
    q, bank = np.asarray(q, np.float32), np.asarray(bank, np.float32)
    qs, bs = chain_sqnorms(q), chain_sqnorms(bank)
    dot = np.zeros((q.shape[0], bank.shape[0]), np.float32)
    for k in range(q.shape[1]):
        dot = _fma32(q[:, k][:, None], bank[:, k][None, :], dot)
    two = np.float32(2)
    with np.errstate(invalid='ignore', divide='ignore'):
        if normalized:
            qn, bn = (np.maximum(np.sqrt(s), np.float32(1e-12)) for s in (qs, bs))
            den = (qn[:, None] * bn[None, :]).astype(np.float32)
            d = _fma32(-two, (dot / den).astype(np.float32), two)
        else:
            d = _fma32(-two, dot, (qs[:, None] + bs[None, :]).astype(np.float32))
        return np.where(d < 0, np.float32(0), d)


# ------------------------------------------------------------------------------------------- checks
ALL_CASES = [(s, None) for s in SHAPES] + [(VARIANT_SHAPE, v) for v in VARIANTS]


@pytest.mark.parametrize('normalized', [False, True])
@pytest.mark.parametrize('shape,variant', ALL_CASES)
def test_restatement_against_cdist_topk(shape, variant, normalized):
    K, N, M, k = shape
    q, bank = knn_case(K, N, M, variant)
    d2, idx = knn_restatement(q, bank, k, normalized)
    assert d2.shape == (N, k) and idx.shape == (N, k)
    tq, tb = torch.from_numpy(q).double(), torch.from_numpy(bank).double()
    if normalized:
        tq, tb = torch.nn.functional.normalize(tq, dim=1), torch.nn.functional.normalize(tb, dim=1)
    ok_q = np.isfinite(q).all(1)
    ok_b = np.isfinite(bank).all(1)
    D = torch.cdist(tq[ok_q], tb[ok_b], compute_mode='donot_use_mm_for_euclid_dist') ** 2
    kk = min(k, int(ok_b.sum()))
    top, where = D.topk(kk, dim=1, largest=False)
    where = torch.from_numpy(np.flatnonzero(ok_b))[where]
    scale = max(1., float(top.max()))
    assert np.abs(d2[ok_q][:, :kk] - top.numpy()).max() <= 1e-12 * scale
    # the rows named are at the distances named; the same rows as topk's where no tie is involved (topk's order among ties is
    # not the stable one: the two tie variants are held to the stable order below)
    full = np.full((int(ok_q.sum()), M), np.inf)
    full[:, ok_b] = D.numpy()
    assert np.abs(np.take_along_axis(full, idx[ok_q][:, :kk], 1) - d2[ok_q][:, :kk]).max() <= 1e-12 * scale
    if variant not in ('duplicates', 'copies'):
        assert np.array_equal(idx[ok_q][:, :kk], where.numpy())
    assert np.isinf(d2[ok_q][:, kk:]).all() and (idx[ok_q][:, kk:] == -1).all()
    assert np.isnan(d2[~ok_q]).all() and (idx[~ok_q] == -1).all()
    fin = idx[ok_q][:, :kk]
    assert ((fin >= 0) & (fin < M)).all() and all(len(set(r)) == len(r) for r in fin.tolist())
    if variant == 'nan':
        assert not (idx == NAN_BANK_ROW).any() and (~ok_q).sum() == 1
    if variant == 'duplicates':                       # a duplicated row and its copy: adjacent, the lower row first
        for r in idx:
            r = r.tolist()
            for j, b in enumerate(r):
                if 0 <= b < 200 and j + 1 < k:
                    assert r[j + 1] == b + M - 200
    if variant == 'copies':
        for b, i in COPIES:
            assert idx[i, 0] == b and d2[i, 0] == 0.


def test_ties_go_to_the_lower_row_and_short_banks_are_padded():
    q = np.zeros((2, 3), np.float32)
    bank = np.ones((5, 3), np.float32)
    bank[3] = 0
    d2, idx = knn_restatement(q, bank, 7, False)
    assert idx.tolist() == [[3, 0, 1, 2, 4, -1, -1]] * 2
    assert d2[0].tolist() == [0., 3., 3., 3., 3., np.inf, np.inf]
    d2, idx = knn_restatement(q, bank, 2, True)      # a zero row normalises to zero: distance 1 to every unit row, 0 to itself
    assert idx.tolist() == [[3, 0]] * 2 and np.allclose(d2, [[0., 1.]] * 2, atol=1e-15)


@pytest.mark.parametrize('normalized', [False, True])
@pytest.mark.parametrize('shape,variant', [c for c in ALL_CASES if c[1] != 'nan'])
def test_fp32_chain_of_the_formula_is_inside_the_bars(shape, variant, normalized):
    """The kernel's formula as a plain fp32 chain against the fp64 restatement, slot by slot, on the GPU test's cases: what the
    bars leave to the formula (on these cases: at most 0.21 of the bar, at K = 3 normalised; 0.11 and less elsewhere)."""
    K, N, M, k = shape
    q, bank = knn_case(K, N, M, variant)
    ref, _ = knn_restatement(q, bank, k, normalized)
    got, _ = select(kernel_chain(q, bank, normalized).astype(np.float64), k)
    bars = row_bars(q, bank, normalized)
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all()
    with np.errstate(invalid='ignore'):              # inf - inf in the padded slots, which `fin` leaves out
        err = np.abs(got - ref)
    ratio = float((err[fin] / np.broadcast_to(bars[:, None], ref.shape)[fin]).max())
    print(shape, variant, 'normalized' if normalized else 'plain', 'worst error / bar', ratio)
    assert ratio <= 1.
    if variant == 'copies' and not normalized:
        for b, i in COPIES:
            assert 0. <= got[i, 0] <= bars[i]


def test_bars_are_the_stated_formulas():
    q, bank = knn_case(3, 2, 4)
    want = 2 * 6 * U * ((q.astype(np.float64) ** 2).sum(1) + (bank.astype(np.float64) ** 2).sum(1).max())
    assert np.array_equal(plain_bar(q, bank), want)
    assert normalized_bar(64) == 4 * 68 * U and np.array_equal(row_bars(q, bank, True), np.full(2, 4 * 7 * U))
    from jvae_hip import ops
    assert ops.KNN_MAX_K == 64 and ops.KNN_MAX_DIM == 4096          # the limits the shapes above are chosen against
