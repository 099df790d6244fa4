"""Closed-form numpy restatement of the reference's ROC (utils/roc_curves.py:38-210) against the goldens the reference wrote
(tools/gen_roc_golden.py -> tests/golden/roc/*.npz).  No GPU.  `roc_restatement` is also the checker of the GPU tests
(tests/test_4_roc_gpu.py) where the reference itself is not available."""
import glob
import os

import numpy as np
import pytest


def roc_restatement(ins, outs, kept_tpr, around_mean=False):
    """-> auc, kept_fpr, kept_tpr, low, up of roc_curve(ins, outs, *kept_tpr, two_sided='around-mean' if around_mean else False)
    on the fp32 scores widened to fp64: searchsorted counts in place of the pointer loops, the kept-TPR cursor walked per slot,
    the trapezoid summed over integer counts."""
    ins, outs = (np.asarray(v, np.float32).astype(np.float64) for v in (ins, outs))
    kept = np.sort(np.asarray(kept_tpr, np.float64))
    n_in, n_out = len(ins), len(outs)
    s_in, s_out = np.sort(ins), np.sort(outs)
    if around_mean:
        c = ins.mean()
        d = np.concatenate([[0], np.sort(abs(ins - c)), [np.inf]])
        low, up = -d[::-1] + c, d + c
    else:
        low = np.concatenate([[-np.inf], s_in])
        up = np.ones_like(low) * np.inf
    nt, upr = len(low), up[::-1]                               # upr[it] = up[-1 - it]
    going = (low < upr)[:nt - 1]
    V = nt - 1 if going.all() else int(np.argmin(going))       # iterations of the while loop (at least one)

    def neg(s, n):                                             # where the pointer loops stop: one short of the end
        c_low = np.minimum(n - 1, np.searchsorted(s, low[:V], 'left'))
        c_up = np.minimum(n - 1, n - np.searchsorted(s, upr[:V], 'right'))
        return c_low + c_up
    neg_in, neg_out = neg(s_in, n_in), neg(s_out, n_out)
    tpr, fpr = 1 - neg_in / n_in, 1 - neg_out / n_out
    K = len(kept)
    k_fpr, k_tpr, k_low, k_up = np.ones(K), np.zeros(K), -np.inf * np.ones(K), np.inf * np.ones(K)
    start = 0
    for j in range(K - 1, -1, -1):                             # the cursor of roc_curves.py:181-189
        if start >= V:
            break
        below = np.nonzero(tpr[start:] < kept[j])[0]
        e = start + int(below[0]) if len(below) else V         # iteration at which the cursor leaves slot j
        if e > start:                                          # iteration e - 1 wrote last: its rates, the NEXT thresholds
            k_fpr[j], k_tpr[j], k_low[j], k_up[j] = fpr[e - 1], tpr[e - 1], low[e], upr[e]
        start = e + 1
    F = np.append(n_out - neg_out, 0).astype(np.int64)
    T = np.append(n_in - neg_in, 0).astype(np.int64)
    auc = int(((F[:-1] - F[1:]) * (T[:-1] + T[1:])).sum()) / (2 * n_in * n_out)
    return auc, k_fpr, k_tpr, k_low, k_up


def auc_bound(n_in):
    """|auc - auc_ref|: the reference sums at most n_in + 1 non-negative fp64 trapezoids whose total is at most 1, each built
    from two rounded ratios, so its own error is below (n_in + 1) * 4 * 2^-53; the restated value is exact up to one division."""
    return (n_in + 2) * 2.0 ** -50


def golden_cases(golden_dir):
    """[(id, ins, outs, kept, mode, (auc, fpr, tpr, low, up))] of every golden file and mode."""
    out = []
    for f in sorted(glob.glob(os.path.join(golden_dir, 'roc', '*.npz'))):
        g = np.load(f)
        for mode in g['modes']:
            ref = tuple(g[f'{k}_{mode}'] for k in ('auc', 'fpr', 'tpr', 'low', 'up'))
            out.append((f'{os.path.basename(f)[:-4]}-{mode}', g['ins'], g['outs'], g['kept'], int(mode), ref))
    return out


def test_goldens_cover_the_cases(golden_dir):
    ids = [c[0] for c in golden_cases(golden_dir)]
    assert len(ids) == 19
    for name in ('gauss_10000_9000', 'gauss_1000_26032', 'gauss_257_100', 'gauss_1_5', 'gauss_4096_1', 'separated_500_300',
                 'identical_400', 'ties_2000_1500', 'kept11_1000_800'):
        assert f'{name}-0' in ids and f'{name}-1' in ids
    assert 'inf_300_200-0' in ids and 'inf_300_200-1' not in ids
    g = np.load(os.path.join(golden_dir, 'roc', 'kept11_1000_800.npz'))
    assert len(g['kept']) == 11 and g['ins'].dtype == np.float32 and g['outs'].dtype == np.float32
    assert 0.99 < float(np.load(os.path.join(golden_dir, 'roc', 'separated_500_300.npz'))['auc_0']) < 1


def test_restatement_reproduces_every_golden(golden_dir):
    for cid, ins, outs, kept, mode, (auc, fpr, tpr, low, up) in golden_cases(golden_dir):
        a, f, t, lo, hi = roc_restatement(ins, outs, kept, around_mean=bool(mode))
        assert np.array_equal(f, fpr), cid
        assert np.array_equal(t, tpr), cid
        assert np.array_equal(lo, low), cid
        assert np.array_equal(hi, up), cid
        assert abs(a - float(auc)) <= auc_bound(len(ins)), (cid, a, float(auc))


@pytest.mark.parametrize('n_in,n_out', [(1, 1), (2, 3), (63, 65), (65, 63), (1025, 7)])
def test_restatement_small_sizes_are_well_formed(n_in, n_out):
    rng = np.random.default_rng(n_in * 131 + n_out)
    ins, outs = rng.standard_normal(n_in).astype(np.float32), rng.standard_normal(n_out).astype(np.float32)
    for mode in (False, True):
        a, f, t, lo, hi = roc_restatement(ins, outs, [.9, .95, .99], around_mean=mode)
        assert 0 <= a <= 1 and np.all((0 <= f) & (f <= 1)) and np.all((0 <= t) & (t <= 1)) and np.all(lo <= hi)
