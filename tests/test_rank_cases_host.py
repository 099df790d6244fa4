"""tests/rank_cases.py on the CPU: the table reaches the regimes it names, every discriminating row can tell a wrong kernel from a
right one, the restatements that serve as references agree with a second, naive definition of the same quantity, and the closed
forms of the two long rows are the restatements on the same data.  No GPU."""
import math

import numpy as np
import pytest

import rank_cases as rc
from rank_cases import F32

SMALL = [r for r in rc.ROWS if max(r.n_in, r.n_out) <= 4097]


# ------------------------------------------------------------------------------------------------------------ the table
def test_the_table_reaches_every_regime_for_every_user():
    assert len({r.name for r in rc.ROWS}) == len(rc.ROWS) and len({r.seed for r in rc.ROWS}) == len(rc.ROWS)
    assert [rc.padded(n) for n in rc.TIEFREE_SIZES] == [2048] * 4 + [4096] * 2 + [8192, 16384, 32768]
    assert [rc.stages(n) for n in rc.TIEFREE_SIZES] == [0, 0, 0, 0, 1, 1, 2, 3, 4]
    for user in rc.ALL:
        fed = [r for r in rc.ROWS if user in r.users]
        tiefree = {r.n_in for r in fed if r.kind == 'tiefree' and r.n_in == r.n_out}
        assert tiefree == set(rc.TIEFREE_SIZES), user
        assert {rc.stages(r.n_in) for r in fed} >= {0, 1, 2, 3, 4}, user
        kinds = {r.kind for r in fed}
        assert kinds >= set(rc.ON_GRID), user
        if user != 'roc1':
            assert 'extremes' in kinds or user in ('rocq', 'mdr')
            assert {'denormals', 'adjacent_bits'} <= kinds, user
        for kind in ('all_equal', 'sorted_asc', 'sorted_desc', 'organ_pipe'):
            assert {r.n_in for r in fed if r.kind == kind} == {4097, 8193}, (user, kind)
        assert {r.arg for r in fed if r.kind == 'straddle'} == set(rc.STRADDLE_ENDS), user
        assert {r.n_in for r in fed if r.kind == 'signed_zeros'} == {64, 4097}, user
    for user in ('roc0', 'roc1', 'rocq', 'pr'):                # the two sides in different padded lengths
        pairs = {(r.n_in, r.n_out) for r in rc.ROWS if user in r.users and r.n_in != r.n_out}
        assert pairs == set(rc.PAIRS), user
        assert all(rc.padded(a) != rc.padded(b) for a, b in pairs)
    # the 64-bit network (PR, SCOD, the around-mean deltas) above 8192 padded keys
    for user in ('pr', 'scod', 'roc1'):
        assert max(rc.padded(r.n_in) for r in rc.ROWS if user in r.users) == 32768, user
    # quantile rows below their factor, and every factor pair
    assert rc.FACTORS == [(1, 1), (4, 1), (3, 7), (255, 255)]
    assert {r.n_in for r in rc.ROWS if 'rocq' in r.users} >= {1, 2, 3}
    # the scan blocks of the misclassification split, and the halves the ROC behind misclass_rates sorts
    mdr = [r for r in rc.ROWS if 'mdr' in r.users]
    assert {min(3, -(-r.n_in // rc.SCAN)) for r in mdr} == {1, 2, 3}
    assert {rc.stages(int(rc.mask(r.n_in).sum())) for r in mdr} >= {0, 1, 2, 3}
    for r in mdr:
        assert 0 < rc.mask(r.n_in).sum() < r.n_in
    for r in rc.ROWS:
        if 'scod' in r.users:
            y_true, _ = rc.labels(r.n_in)
            assert 0 < (y_true >= 0).sum() < r.n_in


def test_around_mean_rows_are_on_the_grid_and_the_others_are_kept_out():
    for r in rc.ROWS:
        v = rc.values(r, 0).astype(np.float64)
        on = bool(np.all(np.isfinite(v)) and np.array_equal(v * 1024, np.round(v * 1024)) and np.abs(v).max() < 16)
        assert on == (r.kind in rc.ON_GRID), r.name
        assert ('roc1' in r.users) <= on, r.name
        if on:                                                 # the centre does not depend on the order of the sum
            assert v.sum() == v[::-1].sum() == math.fsum(v) == np.sort(v).sum()


def test_the_value_kinds_hold_what_they_name():
    for r in rc.ROWS:
        for side in (0, 1):
            v = rc.values(r, side)
            assert v.dtype == F32 and v.shape == ((r.n_in, r.n_out)[side],) and not np.isnan(v).any(), r.name
            assert np.array_equal(v.view(np.uint32), rc.values(r, side).view(np.uint32)), r.name          # seeded
            bits = v.view(np.uint32)
            if r.kind in ('tiefree', 'sorted_asc', 'sorted_desc', 'organ_pipe'):
                assert len(np.unique(v)) == len(v), r.name
            if r.kind == 'sorted_asc':
                assert np.all(np.diff(v) > 0)
            if r.kind == 'sorted_desc':
                assert np.all(np.diff(v) < 0)
            if r.kind == 'organ_pipe':
                top = int(np.argmax(v))
                assert np.all(np.diff(v[:top + 1]) > 0) and np.all(np.diff(v[top:]) < 0) and 0 < top < len(v) - 1
            if r.kind == 'signed_zeros':
                assert set(bits.tolist()) == {0x0, 0x80000000, 0x3F800000, 0xBF800000}
            if r.kind == 'denormals':
                assert set(bits.tolist()) == {s | k for s in (0, 0x80000000) for k in list(range(9)) + [0x00800000]}
            if r.kind == 'extremes':
                for x in (rc.FLT_MAX, -rc.FLT_MAX, np.inf, -np.inf):
                    assert (v == F32(x)).sum() == len(v) // 16
            if r.kind == 'adjacent_bits' and side == 0:
                want = set(range(1500)) | {0x80000000 | k for k in range(1500)} | set(range(0x3F800000 - 1500, 0x3F800000 + 1500))
                assert set(bits.tolist()) == want and len(v) == 6000
                s = np.sort(v)                                 # consecutive floats: nothing fits between two neighbours
                assert np.all(np.nextafter(s[:2999], F32(np.inf)) >= s[1:3000]) and s[1499] == 0 and s[1500] == 0
            if r.kind == 'all_equal':
                assert len(np.unique(v)) == 1 and len(v) > rc.TILE
    z = rc.values(rc.BY_NAME['signed_zeros_64'], 0)            # the two zeros interleave, and the labels differ across them
    y_true, y_est = rc.labels(64)
    code = np.where(y_true < 0, 2, (y_true != y_est).astype(int))
    neg, pos = np.nonzero((z == 0) & np.signbit(z))[0], np.nonzero((z == 0) & ~np.signbit(z))[0]
    assert any(code[a] != code[b] for a in neg for b in pos if a > b)


# ------------------------------------------------------------------------------------------------------------ rows discriminate
def differs(a, b):
    """Two results of one restatement differ in a count-valued part"""
    if isinstance(a, dict):
        return any(differs(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return any(differs(x, y) for x, y in zip(a, b))
    return not np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize('name', ['signed_zeros_64', 'signed_zeros_4097'])
def test_signed_zero_rows_tell_the_stable_order_from_the_order_of_the_raw_key(name):
    s = rc.values(rc.BY_NAME[name], 0)
    y_true, y_est = rc.labels(len(s))
    (tpr, sr, fpr), fig = rc.scod_restatement(s, y_true, y_est)
    (tpr_k, sr_k, fpr_k), fig_k = rc.scod_restatement(rc.raw_key_image(s), y_true, y_est)
    print(name, 'positions that differ: tpr', int((tpr != tpr_k).sum()), 'sr', int((sr != sr_k).sum()), 'fpr', int((fpr != fpr_k).sum()))
    assert (tpr != tpr_k).any() and (sr != sr_k).any() and (fpr != fpr_k).any()
    # and IEEE-equal zeros are one value to every other user: giving every zero one sign changes nothing
    r = rc.BY_NAME[name]
    ins, outs = rc.values(r, 0), rc.values(r, 1)
    for mode in rc.roc_modes(r):
        assert not differs(rc.roc_ref(ins, outs, mode), rc.roc_ref(ins + F32(0), outs + F32(0), mode)), mode      # -0. + 0. = +0.
    assert rc.pr_ref(ins, outs, False) == rc.pr_ref(ins + F32(0), outs + F32(0), False)


@pytest.mark.parametrize('b', rc.STRADDLE_ENDS)
def test_straddle_rows_end_their_first_group_where_the_name_says(b):
    r = rc.BY_NAME[f'straddle_{b}']
    for side in (0, 1):
        s = np.sort(rc.values(r, side))
        assert s[b - 1] == F32(0.25) and s[b] == F32(0.75) and s[0] == F32(0.25) and s[-1] == F32(0.75)
        assert not np.array_equal(rc.values(r, side), s)       # shuffled
    assert rc.padded(r.n_in) == 8192 and min(abs(b - 2048), abs(b - 4096)) <= 1


def test_the_denormal_row_tells_a_kernel_that_flushes_to_zero():
    r = rc.BY_NAME['denormals_2049']
    ins, outs = rc.values(r, 0), rc.values(r, 1)
    assert (rc.flush(ins) != ins).sum() > r.n_in // 2 and set(np.abs(rc.flush(ins)).tolist()) == {0., rc.FLT_MIN}
    assert differs(rc.roc_ref(ins, outs, False)[1:3], rc.roc_ref(rc.flush(ins), rc.flush(outs), False)[1:3])
    for a, b in rc.FACTORS:
        mode = ('quantile', a, b)
        assert differs(rc.roc_ref(ins, outs, mode), rc.roc_ref(rc.flush(ins), rc.flush(outs), mode)), mode
    assert differs(rc.pr_ref(ins, outs, False), rc.pr_ref(rc.flush(ins), rc.flush(outs), False))
    assert differs(rc.scod_ref(ins)[0], rc.scod_ref(rc.flush(ins))[0])
    got, flushed = rc.mdr_ref(ins), rc.mdr_ref(rc.flush(ins))
    assert differs((got['tp'], got['fp']), (flushed['tp'], flushed['fp'])) and differs((got['fpr'], got['tpr']), (flushed['fpr'], flushed['tpr']))


def test_adjacent_bit_rows_tell_a_key_that_breaks_at_the_sign_change():
    """A key that ordered negative floats by their raw bits (the classic mistake) reverses the 1500 patterns below zero."""
    s = rc.values(rc.BY_NAME['adjacent_bits_6000'], 0)
    wrong = s.copy()
    neg = np.signbit(s) & (np.abs(s) < 1e-30)
    wrong[neg] = rc.bits_f32(np.uint32(0x80000000) | (np.uint32(1499) - (s[neg].view(np.uint32) & np.uint32(0x7FFFFFFF))))
    assert differs(rc.scod_ref(s)[0], rc.scod_ref(wrong)[0])


# ------------------------------------------------------------------------------------------------------------ naive definitions
def naive_roc(ins, outs, mode):
    """The ROC as its definition reads: every count a direct comparison in fp64, the walk and the kept-TPR cursor one iteration
    at a time, the area a floating-point trapezoid."""
    ins, outs = np.asarray(ins, F32).astype(np.float64), np.asarray(outs, F32).astype(np.float64)
    n_in, n_out, s = len(ins), len(outs), sorted(ins.tolist())
    inf = math.inf
    if mode == 'around-mean':
        c = math.fsum(ins) / n_in
        d = [0.] + sorted(abs(x - c) for x in ins.tolist()) + [inf]
        low, up = [c - x for x in d[::-1]], [c + x for x in d]
    elif isinstance(mode, tuple):
        low, up = [-inf] + s[::mode[1]] + [inf], [-inf] + s[::mode[2]] + [inf]
    else:
        low = [-inf] + s
        up = [inf] * len(low)
    nt = min(len(low), len(up))
    upr = up[::-1]
    lo, hi = np.array(low[:nt]), np.array(upr[:nt])
    neg_in = np.minimum(n_in - 1, (ins[None] < lo[:, None]).sum(1)) + np.minimum(n_in - 1, (ins[None] > hi[:, None]).sum(1))
    neg_out = np.minimum(n_out - 1, (outs[None] < lo[:, None]).sum(1)) + np.minimum(n_out - 1, (outs[None] > hi[:, None]).sum(1))
    K = len(rc.KEPT)
    k_fpr, k_tpr, k_low, k_up = [1.] * K, [0.] * K, [-inf] * K, [inf] * K
    j, it, xs, ys = K - 1, 0, [], []
    while it < nt - 1 and low[it] < upr[it]:
        tpr, fpr = 1 - neg_in[it] / n_in, 1 - neg_out[it] / n_out
        xs.append(fpr), ys.append(tpr)
        if j >= 0:
            if tpr < rc.KEPT[j]:
                j -= 1
            else:
                k_fpr[j], k_tpr[j], k_low[j], k_up[j] = fpr, tpr, low[it + 1], upr[it + 1]
        it += 1
    xs, ys = np.array(xs + [0.]), np.array(ys + [0.])
    auc = float(-np.sum(np.diff(xs) * (ys[1:] + ys[:-1]) / 2))
    return auc, np.array(k_fpr), np.array(k_tpr), np.array(k_low), np.array(k_up)


def naive_pr(ins, outs, mode):
    """The PR figures by the threshold definition: one threshold per distinct positive score, every count a direct comparison"""
    ins, outs = np.asarray(ins, F32).astype(np.float64), np.asarray(outs, F32).astype(np.float64)
    if mode == 'around-mean':
        c = math.fsum(ins) / len(ins)
        ins, outs = -abs(ins - c), -abs(outs - c)

    def side(pos, neg):
        ap = trap = r_prev = 0.
        p_prev, errs = 1., []
        thr = np.array(sorted(set(pos.tolist()) | set(neg.tolist()), reverse=True))    # every score is a threshold
        tps, fps = (pos[None] >= thr[:, None]).sum(1).tolist(), (neg[None] >= thr[:, None]).sum(1).tolist()
        for tp, fp in zip(tps, fps):
            r, p = tp / len(pos), tp / (tp + fp)               # the curve starts at (0, 1); negatives in front: (0, 0)
            ap += (r - r_prev) * p
            trap += (r - r_prev) * (p + p_prev) / 2
            errs.append(0.5 * (1 - r) + 0.5 * fp / len(neg))
            r_prev, p_prev = r, p
        return ap, trap, min(errs)
    ap_in, trap_in, err = side(ins, outs)
    ap_out, trap_out, _ = side(-outs, -ins)
    return [ap_in, ap_out, trap_in, trap_out, min(0.5, err)]


def naive_scod(scores, y_true, y_est):
    s = np.asarray(scores, F32)
    order = sorted(range(len(s)), key=lambda i: (float(s[i]), i))
    n_in = int((y_true >= 0).sum())
    n_ood = len(s) - n_in
    inn = wrong = ood = 0
    tpr, sr, fpr = [], [], []
    for i in order:
        inn += y_true[i] >= 0
        ood += y_true[i] < 0
        wrong += y_true[i] >= 0 and y_true[i] != y_est[i]
        tpr.append(F32(inn) / F32(n_in)), fpr.append(F32(ood) / F32(n_ood)), sr.append(F32(wrong) / F32(inn) if inn else F32(0))
    tpr, sr, fpr = (np.array(v, F32) for v in (tpr, sr, fpr))
    half = (F32(0.5) * sr + F32(0.5) * fpr).astype(np.float64)
    t, r, f = (v.astype(np.float64) for v in (tpr, sr, fpr))

    def area(y, x):
        return math.fsum(((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2).tolist())
    keep = tpr >= F32(0.95)
    return (tpr, sr, fpr), [float(fpr[keep].min()), float(sr[keep].min()), area(t, f), area(r, t), area(half, t)]


def same_roc(got, want, n_in, what):
    print(what, 'auc', got[0], want[0], 'diff', abs(got[0] - want[0]), 'bound', rc.auc_bound(n_in))
    for g, w in zip(got[1:3], want[1:3]):
        assert g.tobytes() == w.tobytes(), what
    for g, w in zip(got[3:], want[3:]):
        assert np.array_equal(g, w), what
    assert abs(got[0] - want[0]) <= rc.auc_bound(n_in), what


@pytest.mark.parametrize('r', SMALL, ids=rc.ids)
def test_the_restatements_agree_with_a_naive_definition(r):
    ins, outs = rc.values(r, 0), rc.values(r, 1)
    for mode in rc.roc_modes(r):
        same_roc(rc.roc_ref(ins, outs, mode), naive_roc(ins, outs, mode), r.n_in, (r.name, mode))
    for mode in rc.pr_modes(r):
        got, want = rc.pr_ref(ins, outs, mode), naive_pr(ins, outs, mode)
        for k, g, w, b in zip(rc.PR_FIGURES, got, want, rc.pr_bounds(r.n_in, r.n_out)):
            print(r.name, mode, k, g, w, 'diff', abs(g - w), 'bound', b)
            assert abs(g - w) <= b, (r.name, mode, k)
    if 'scod' in r.users:
        y_true, y_est = rc.labels(r.n_in)
        (curves, fig), (ncurves, nfig) = rc.scod_ref(ins), naive_scod(ins, y_true, y_est)
        for g, w in zip(curves, ncurves):
            assert g.dtype == F32 and g.tobytes() == w.tobytes(), r.name
        assert fig[:2] == nfig[:2]
        for g, w in zip(fig[2:], nfig[2:]):
            print(r.name, 'area', g, w, 'diff', abs(g - w), 'bound', rc.area_bound(r.n_in, w))
            assert abs(g - w) <= rc.area_bound(r.n_in, w), r.name
    if 'mdr' in r.users:
        m, got = rc.mask(r.n_in), rc.mdr_ref(ins)
        want = naive_roc(ins[m], ins[~m], False)
        same_roc((got['auc'], got['fpr'], got['tpr'], got['low'], got['low']), want[:4] + (want[3],), int(m.sum()), (r.name, 'mdr'))
        wide = ins.astype(np.float64)
        for k, t in enumerate(want[3]):
            assert got['tp'][k] == sum(1 for x, c in zip(wide.tolist(), m) if c and x >= t)
            assert got['fp'][k] == sum(1 for x, c in zip(wide.tolist(), m) if not c and x >= t)


# ------------------------------------------------------------------------------------------------------------ the long rows
def test_the_long_rows_reach_the_branches_they_are_for():
    n = rc.SCOD_LONG_N
    tiles = rc.padded(n) // rc.TILE
    assert n == 2 ** 21 + 1 and tiles == 2048 and -(-tiles // rc.SCAN) == 2          # per = ceil(T / 1024) of scod_offsets_kernel
    assert -(-rc.padded(2 ** 21) // rc.TILE // rc.SCAN) == 1                            # and one sample fewer would not
    assert tiles > rc.SCAN                                                             # scod_figures_kernel strides a second time
    N = rc.MDR_LONG_N
    assert N == 2 ** 20 + 1025 and -(-N // rc.SCAN) == 1026 > rc.SCAN                   # a second chunk of misclass_offsets_kernel
    assert max(n, N) < 2 ** 24
    for size in (n, N):
        s = rc.long_scores(size)
        assert s.dtype == F32 and math.gcd(rc.LONG_A, size) == 1
        order = rc.long_order(size)
        assert np.array_equal(s[order], np.arange(size, dtype=F32))                    # a permutation, and its inverse
        assert not np.array_equal(order[:64], np.sort(order[:64]))


def test_the_closed_form_of_the_long_scod_row_is_the_restatement():
    n = rc.SCOD_LONG_N
    y_true, y_est = rc.scod_long_labels()
    curves, fig = rc.scod_restatement(rc.long_scores(n), y_true, y_est)
    ccurves, cfig = rc.scod_long_closed_form()
    for g, w in zip(ccurves, curves):
        assert g.tobytes() == w.tobytes()
    assert cfig == fig
    assert 0 < (y_true >= 0).sum() < n and ((y_true >= 0) & (y_true != y_est)).any()
    assert len(np.unique(curves[1])) > 1000


def test_the_closed_form_of_the_long_misclassification_row_is_the_restatement():
    N = rc.MDR_LONG_N
    s, m = rc.long_scores(N), rc.mdr_long_mask()
    r = rc.mdr_restatement(s, m, rc.KEPT)
    tp, fp = rc.mdr_long_counts(r['low'])
    assert np.array_equal(tp, r['tp']) and np.array_equal(fp, r['fp']) and tp.dtype == np.int32
    tp, fp = rc.mdr_long_counts(rc.MDR_LONG_THR)
    wide = s.astype(np.float64)
    assert tp.tolist() == [int((wide[m] >= t).sum()) for t in rc.MDR_LONG_THR]
    assert fp.tolist() == [int((wide[~m] >= t).sum()) for t in rc.MDR_LONG_THR]
    assert tp[0] == m.sum() and fp[0] == N - m.sum() and tp[-1] == fp[-1] == 0 and len(set(tp.tolist())) >= 6
