"""Numpy restatement of the reference's SCOD evaluation (tests/scod.py: scoring_r, scoring_g, scoring, scrisk and the figures of
its command-line block) against the goldens the reference wrote (tools/gen_scod_golden.py -> tests/golden/scod/*.npz).  No GPU.
The restatement pins the goldens independently of the device code; it is also the checker of tests/test_21_scod_gpu.py where
the reference leaves a result unspecified (the order inside a group of equal scores).

Curves and the kept figures are compared bit for bit.  The areas are compared with the fp64 trapezoid of the reference's own
curves: the terms are the same, so only the order of at most n fp64 additions of non-negative terms can differ - a relative
n * 2^-52, plus an absolute term of the same size (`area_bound`).  The value sklearn returned for the reference is its own fp32
summation and is printed, not held to a bar."""
import glob
import os

import numpy as np
import torch

F32 = np.float32
FIGURES = ('fpr95', 'sr95', 'auroc', 'aust', 'auscodt')
trapezoid = getattr(np, 'trapezoid', None) or np.trapz


def scod_restatement(scores, y_true, y_est):
    """-> (tpr, selective_risk, fpr) fp32, [fpr95, sr95, auroc, aust, auscodt] of one score row; equal scores in the order of
    their positions."""
    scores, y_true, y_est = np.asarray(scores, F32), np.asarray(y_true), np.asarray(y_est)
    order = np.argsort(scores, kind='stable')
    y_, e_ = y_true[order], y_est[order]
    wrong = np.cumsum((y_ != e_) & (y_ >= 0))
    ood = np.cumsum(y_ < 0)
    inn = np.cumsum(y_ >= 0)
    n_in, n_ood = int((y_true >= 0).sum()), int((y_true < 0).sum())
    tpr = inn.astype(F32) / F32(n_in)
    fpr = ood.astype(F32) / F32(n_ood)
    sr = np.where(inn > 0, wrong.astype(F32) / np.maximum(inn, 1).astype(F32), F32(0)).astype(F32)
    kept = tpr >= F32(0.95)
    half = F32(0.5) * sr + F32(0.5) * fpr
    assert half.dtype == F32 and tpr.dtype == F32 and fpr.dtype == F32
    t, s, f, h = (v.astype(np.float64) for v in (tpr, sr, fpr, half))
    figures = [float(fpr[kept].min()), float(sr[kept].min()), float(trapezoid(t, f)), float(trapezoid(s, t)), float(trapezoid(h, t))]
    return (tpr, sr, fpr), figures


def area_bound(n, ref):
    return n * 2.0 ** -52 * abs(ref) + n * 2.0 ** -52


def tie_group_ends(scores):
    """Sorted positions that end a group of equal scores (all of them on tie-free scores)."""
    s = np.sort(np.asarray(scores, F32), kind='stable')
    return np.concatenate([s[1:] != s[:-1], [True]])


def curve_cases(golden_dir):
    """[(id, scores (n,), y_true, y_est, (tpr, sr, fpr), figures (5,), trapz (3,))] of every row of every curve golden."""
    out = []
    for f in sorted(glob.glob(os.path.join(golden_dir, 'scod', 'curve-*.npz'))):
        g = np.load(f)
        for m in range(g['scores'].shape[0]):
            out.append((f'{os.path.basename(f)[6:-4]}-{m}', g['scores'][m], g['y_true'], g['y_est'],
                        (g['tpr'][m], g['selective_risk'][m], g['fpr'][m]), g['figures'][m], g['trapz'][m]))
    return out


def check_figures(cid, figures, golden_figures, golden_trapz, n):
    """fpr95 / sr95 exact, the three areas against the fp64 trapezoid of the reference's curves at `area_bound`."""
    assert figures[0] == golden_figures[0] and figures[1] == golden_figures[1], (cid, figures[:2], golden_figures[:2])
    for k in range(3):
        print(cid, FIGURES[2 + k], figures[2 + k], 'trapezoid of the reference curves', golden_trapz[k], 'diff',
              abs(figures[2 + k] - golden_trapz[k]), 'bound', area_bound(n, golden_trapz[k]), '| to sklearn',
              abs(figures[2 + k] - golden_figures[2 + k]))
        assert abs(figures[2 + k] - golden_trapz[k]) <= area_bound(n, golden_trapz[k]), (cid, FIGURES[2 + k])


def parse_name(v):
    return None if v == 'None' else v


def row_records(golden_dir, which):
    """tensors {name: array}, mtype, [((r, g, weight), row)] of tests/golden/scod/rows-<which>.npz."""
    g = np.load(os.path.join(golden_dir, 'scod', f'rows-{which}.npz'))
    tensors = {k[2:]: g[k] for k in g.files if k.startswith('t|')}
    rows = []
    for k in g.files:
        if k.startswith('row|'):
            _, r, gg, w = k.split('|')
            rows.append(((parse_name(r), parse_name(gg), float(w) if '.' in w else int(w)), g[k]))
    return tensors, str(g['mtype']), rows


def scoring_restatement(t, r, g, weight, mtype):
    """scoring(losses, r, g, weight, mtype=mtype) on numpy arrays (y_est_already present).  The class-axis log-sum-exp of `logmsp`
    is torch's, as everywhere in this project."""
    defaults = {'wim': ('zdist', 'elbo'), 'vib': ('odin-1-0.0040', 'none')}
    y = t['y_est_already']
    n = np.arange(len(y))
    r = defaults[mtype][0] if r is None else r
    g = defaults[mtype][1] if g is None else g
    if r.startswith('odin'):
        rr = F32(1) - t[r]
    elif r == 'predist':
        rr = F32(0.5) * t['pre-zdist'][y, n]
    elif r == 'dist':
        rr = F32(0.5) * t['zdist'][y, n]
    elif r == 'logmsp':
        rr = F32(0.5) * t['zdist'][y, n] - (-0.5 * torch.from_numpy(t['zdist'])).logsumexp(0).numpy()
    else:
        rr = 0.
    if mtype == 'wim':
        key, sign = ('zdist', F32(0.5)) if g == 'elbo' else (g, F32(-1) if g == 'iws' else F32(1))
        alt = t[key + '@']
        gg = sign * (t[key][y, n] - (alt[0] if alt.ndim == 2 else alt))
    else:
        gg = 0.
    wg = (F32(weight) * gg) if isinstance(gg, np.ndarray) else weight * gg
    out = rr + wg
    return out.astype(F32) if isinstance(out, np.ndarray) else out


def e2e_record(golden_dir):
    """sets {name: {tensor name: array}} in recorder order, {(r, g, weight): (figures (5,), trapz (3,))} of e2e.npz."""
    g = np.load(os.path.join(golden_dir, 'scod', 'e2e.npz'))
    sets = {str(s): {} for s in g['sets']}
    for k in g.files:
        if k.startswith('t|'):
            _, s, name = k.split('|')
            sets[s][name] = g[k]
    figs = {}
    for k in g.files:
        if k.startswith('fig|'):
            _, r, gg, w = k.split('|')
            figs[(parse_name(r), parse_name(gg), float(w))] = (g[k], g['trapz|' + k[4:]])
    return sets, figs


# ------------------------------------------------------------------------------------------------------------------ tests
def test_goldens_cover_the_cases(golden_dir):
    ids = [c[0] for c in curve_cases(golden_dir)]
    for name in ('small_5_3-0', 'tile_minus_1-0', 'tile-0', 'tile_plus_1-0', 'tiles_3000_2000-0', 'ood_head_400_250-0',
                 'all_correct_700_300-0', 'all_wrong_300_700-0', 'rows3_2500_1700-0', 'rows3_2500_1700-1', 'rows3_2500_1700-2',
                 'ties_300_200-0', 'ties_300_200-1', 'ties_2600_1900-0', 'ties_2600_1900-1'):
        assert name in ids
    assert len(ids) == 15
    by = {c[0]: c for c in curve_cases(golden_dir)}
    assert [len(by[f'{k}-0'][1]) for k in ('tile_minus_1', 'tile', 'tile_plus_1')] == [2047, 2048, 2049]
    _, s, y_true, _, (tpr, sr, _), _, _ = by['ood_head_400_250-0']
    assert np.all(y_true[np.argsort(s)[:40]] < 0) and np.all(tpr[:40] == 0) and np.all(sr[:40] == 0)       # the 0 / 0 -> 0 branch
    assert np.all(by['all_correct_700_300-0'][4][1] == 0) and by['all_wrong_300_700-0'][5][1] == 1
    for cid, s, *_ in curve_cases(golden_dir):
        assert s.dtype == F32 and (len(np.unique(s)) == len(s)) == (not cid.startswith('ties')), cid
        if cid.startswith('ties'):
            assert len(np.unique(s)) <= 16
    assert len(row_records(golden_dir, 'wim')[2]) == 7 * 4 * 3 and len(row_records(golden_dir, 'vib')[2]) == 4 * 3 * 3
    t = row_records(golden_dir, 'wim')[0]
    assert t['zdist'].shape == (10, 37) and t['zdist@'].ndim == 2 and 'y_est_already' in t
    t = row_records(golden_dir, 'vib')[0]
    assert 'odin-1-0.0040' in t and 'y_est_already' not in t
    sets, figs = e2e_record(golden_dir)
    assert list(sets) == ['ind', 'ood-a', 'ood-b'] and len(figs) == 12
    assert all(64 <= len(t['y_true']) <= 200 for t in sets.values())


def test_restatement_reproduces_every_curve_golden(golden_dir):
    for cid, scores, y_true, y_est, curves, figures, trapz in curve_cases(golden_dir):
        got, fig = scod_restatement(scores, y_true, y_est)
        ends = tie_group_ends(scores)
        assert cid.startswith('ties') or ends.all()
        for name, a, b in zip(('tpr', 'selective_risk', 'fpr'), got, curves):
            assert a.dtype == b.dtype == F32 and np.array_equal(a[ends], b[ends]), (cid, name)
        if not cid.startswith('ties'):                        # inside a tie group the reference's curves are unspecified
            check_figures(cid, fig, figures, trapz, len(scores))


def test_restatement_reproduces_every_score_row(golden_dir):
    for which in ('wim', 'vib'):
        t, mtype, rows = row_records(golden_dir, which)
        if 'y_est_already' not in t:
            t = dict(t, y_est_already=t['cross_y'].argmin(0))
        for (r, g, w), want in rows:
            got = scoring_restatement(t, r, g, w, mtype)
            if want.ndim == 0:
                assert not isinstance(got, np.ndarray) and float(got) == float(want), (which, r, g, w)
            else:
                assert got.dtype == want.dtype == F32 and got.tobytes() == want.tobytes(), (which, r, g, w)
    # the reference's default r of a wim, the name 'zdist', matches no branch: the row is weight * g alone
    t, mtype, rows = row_records(golden_dir, 'wim')
    by = dict(rows)
    assert by[(None, 'elbo', 1)].tobytes() == by[('msp', 'elbo', 1)].tobytes() == by[('zdist', None, 1)].tobytes()
    # weight 0.3 tells a fused multiply-add from two rounded operations on some sample
    r, g = F32(0.5) * t['zdist'][t['y_est_already'], np.arange(37)], by[(None, 'elbo', 1)]
    fused = (r.astype(np.float64) + np.float64(F32(0.3)) * g.astype(np.float64)).astype(F32)
    assert fused.tobytes() != by[('dist', 'elbo', 0.3)].tobytes()


def test_restatement_reproduces_the_end_to_end_figures(golden_dir):
    sets, figs = e2e_record(golden_dir)
    sets = {s: (t if 'y_est_already' in t else dict(t, y_est_already=t['cross_y'].argmin(0))) for s, t in sets.items()}
    y_est = np.hstack([t['y_est_already'] for t in sets.values()])
    y_true = np.hstack([t['y_true'] if s == 'ind' else -np.ones_like(t['y_true']) for s, t in sets.items()])
    for (r, g, w), (figures, trapz) in figs.items():
        scores = np.hstack([scoring_restatement(t, r, g, w, 'wim') for t in sets.values()])
        _, fig = scod_restatement(scores, y_true, y_est)
        check_figures(('e2e', r, g, w), fig, figures, trapz, len(scores))
