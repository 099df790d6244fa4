"""Closed-form numpy restatement of the reference's ROC in its tuple mode, two_sided=(f_low, f_up) (utils/roc_curves.py:74-83,
the '-a-x-y' OOD methods), on the noise-free thresholds: against the goldens of tools/gen_rocq_golden.py ->
tests/golden/rocq/*.npz.  No GPU.  Record (a) of a golden is the reference's own loop with only its spline replaced by the
values at the knots, record (b) the unpatched reference.  `roc_restatement_quantile` is also the checker of the GPU tests
(tests/test_8_rocq_gpu.py) where no golden exists."""
import glob
import os

import numpy as np
import pytest

from test_roc_restatement import auc_bound

PAIRS = [(1, 1), (4, 1), (1, 4), (2, 3), (7, 7)]
NAMES = ['gauss_10000_9000', 'gauss_1000_26032', 'gauss_257_100', 'gauss_4096_1', 'separated_500_300', 'identical_400',
         'ties_2000_1500', 'inf_300_200', 'kept11_1000_800', 'gauss_4_50', 'gauss_5_50', 'continuous_3000_2000']


def roc_restatement_quantile(ins, outs, kept_tpr, factors):
    """-> auc, kept_fpr, kept_tpr, low, up of roc_curve(ins, outs, *kept_tpr, two_sided=factors) with the spline's values at
    its knots taken as the sorted in-scores themselves, on the fp32 scores widened to fp64: searchsorted counts in place of
    the pointer loops, the kept-TPR cursor walked per slot, the trapezoid summed over integer counts."""
    ins, outs = (np.asarray(v, np.float32).astype(np.float64) for v in (ins, outs))
    kept = np.sort(np.asarray(kept_tpr, np.float64))
    n_in, n_out = len(ins), len(outs)
    s_in, s_out = np.sort(ins), np.sort(outs)
    low, up = (np.concatenate([[-np.inf], s_in[::f], [np.inf]]) for f in factors)
    nt = min(len(low), len(up))
    low, upr = low[:nt], up[::-1][:nt]                         # upr[it] = up[-1 - it]
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


def golden_cases(golden_dir, record='a'):
    """[(id, ins, outs, kept, (f_low, f_up), (auc, fpr, tpr, low, up))] of every golden file and factor pair; record 'b' lists
    the pairs on which the unpatched reference returned."""
    out = []
    for f in sorted(glob.glob(os.path.join(golden_dir, 'rocq', '*.npz'))):
        g = np.load(f)
        for pair in g['pairs']:
            tag = '{}_{}'.format(*pair)
            if record == 'b' and not int(g[f'b_ok_{tag}']):
                continue
            ref = tuple(g[f'{record}_{k}_{tag}'] for k in ('auc', 'fpr', 'tpr', 'low', 'up'))
            out.append((f'{os.path.basename(f)[:-4]}-{tag}', g['ins'], g['outs'], g['kept'], (int(pair[0]), int(pair[1])), ref))
    return out


def test_goldens_cover_the_cases(golden_dir):
    ids = [c[0] for c in golden_cases(golden_dir)]
    assert sorted(ids) == sorted(f'{n}-{a}_{b}' for n in NAMES for a, b in PAIRS)
    for name in NAMES:
        g = np.load(os.path.join(golden_dir, 'rocq', name + '.npz'))
        assert g['ins'].dtype == np.float32 and g['outs'].dtype == np.float32 and len(g['ins']) >= 4
        assert (len(g['ins']), len(g['outs'])) == tuple(int(v) for v in name.split('_')[1:]) or name == 'identical_400'
    assert len(np.load(os.path.join(golden_dir, 'rocq', 'kept11_1000_800.npz'))['kept']) == 11
    inf = np.load(os.path.join(golden_dir, 'rocq', 'inf_300_200.npz'))['ins']
    assert np.isposinf(inf).any() and np.isneginf(inf).any()
    off_grid = np.load(os.path.join(golden_dir, 'rocq', 'continuous_3000_2000.npz'))['ins'].astype(np.float64) * 1024
    assert np.mean(off_grid != np.round(off_grid)) > .9
    ties = np.load(os.path.join(golden_dir, 'rocq', 'ties_2000_1500.npz'))['ins']
    assert len(np.unique(ties)) < len(ties) / 10


def test_restatement_reproduces_every_golden(golden_dir):
    for cid, ins, outs, kept, pair, (auc, fpr, tpr, low, up) in golden_cases(golden_dir):
        a, f, t, lo, hi = roc_restatement_quantile(ins, outs, kept, pair)
        assert np.array_equal(f, fpr), cid
        assert np.array_equal(t, tpr), cid
        assert np.array_equal(lo, low), cid
        assert np.array_equal(hi, up), cid
        assert abs(a - float(auc)) <= auc_bound(len(ins)), (cid, a, float(auc))


def test_goldens_hold_unwritten_kept_slots(golden_dir):
    """On small or tied sets the reference's cursor passes slots without writing them (TPR 0, FPR 1): the goldens have them."""
    unwritten = [c[0] for c in golden_cases(golden_dir) if np.any((c[5][2] == 0) & (c[5][1] == 1))]
    assert any(i.startswith('gauss_257_100') for i in unwritten) and any(i.startswith('ties_2000_1500') for i in unwritten)


def test_the_unpatched_reference_differs(golden_dir):
    """Why the mode is opt-in: FITPACK's rounding of the spline at its own knots moves the reference's results."""
    a = {c[0]: c[5] for c in golden_cases(golden_dir, 'a')}
    b = {c[0]: c[5] for c in golden_cases(golden_dir, 'b')}
    assert len(b) >= len(a) - len(PAIRS)
    differ = [cid for cid in b if any(not np.array_equal(x, y) for x, y in zip(a[cid], b[cid]))]
    print(len(differ), 'of', len(b), 'records differ')
    assert differ
    assert any(not np.array_equal(a[cid][1], b[cid][1]) for cid in b if cid.startswith('gauss_10000_9000'))


@pytest.mark.parametrize('n_in,n_out', [(1, 1), (2, 3), (4, 5), (63, 65), (65, 63), (1025, 7)])
def test_restatement_small_sizes_are_well_formed(n_in, n_out):
    rng = np.random.default_rng(n_in * 131 + n_out)
    ins, outs = rng.standard_normal(n_in).astype(np.float32), rng.standard_normal(n_out).astype(np.float32)
    for pair in PAIRS + [(255, 1), (1, 255)]:
        a, f, t, lo, hi = roc_restatement_quantile(ins, outs, [.9, .95, .99], pair)
        assert 0 <= a <= 1 and np.all((0 <= f) & (f <= 1)) and np.all((0 <= t) & (t <= 1))

