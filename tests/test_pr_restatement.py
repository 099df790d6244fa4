"""Closed-form numpy restatement of the precision-recall figures of csrc/prc.hip (jvae_hip.ops.pr_metrics) against the goldens
scikit-learn wrote (tools/gen_pr_golden.py -> tests/golden/pr/*.npz).  No GPU, no scikit-learn.  `pr_restatement` is also the
checker of the GPU tests (tests/test_26_pr_gpu.py), and it defines the answer where scikit-learn refuses to give one (infinite
scores)."""
import glob
import os

import numpy as np
import pytest

PR_FIGURES = ('aupr_in', 'aupr_out', 'aucpr_in', 'aucpr_out', 'dete')
CASES = ('small_1_1', 'small_5_3', 'tile', 'tile_minus_1', 'tile_plus_1', 'tiles_5000_3000', 'ties_2600_1900', 'identical_400',
         'separated_500_300', 'reversed_300_500', 'zeros_pm', 'rows3', 'around_mean_1500_1200', 'inf_300_200')


def _side(pos, neg):
    """(sum dR * P, sum dR * (P + P') / 2, the detection errors) over the distinct values v of `pos` (positive = kept at
    score >= v), both rows fp64."""
    pos, neg = np.sort(pos), np.sort(neg)
    n_pos, n_neg = len(pos), len(neg)
    v = np.unique(pos)
    tp, fp = n_pos - np.searchsorted(pos, v, 'left'), n_neg - np.searchsorted(neg, v, 'left')           # >= v
    tq, fq = n_pos - np.searchsorted(pos, v, 'right'), n_neg - np.searchsorted(neg, v, 'right')         # > v
    P = tp / (tp + fp)
    Q = np.where(tq + fq > 0, tq / np.maximum(tq + fq, 1), 1.0)
    dR = (tp - tq) / n_pos
    err = 0.5 * ((n_pos - tp) / n_pos) + 0.5 * (fp / n_neg)
    return float(np.sum(dR * P)), float(np.sum(dR * (P + Q) / 2)), err


def pr_restatement(ins, outs, mode=0):
    """-> [aupr_in, aupr_out, aucpr_in, aucpr_out, dete] of one row of fp32 scores widened to fp64.  mode: the mode word of the
    ROC - 0 one-sided, 1 'around-mean' (the score of a sample is -|s - mean(ins)|), anything else (a quantile row): NaN."""
    ins, outs = (np.asarray(v, np.float32).astype(np.float64) for v in (ins, outs))
    if mode not in (0, 1):
        return [np.nan] * 5
    if mode == 1:
        c = ins.mean()
        ins, outs = -abs(ins - c), -abs(outs - c)
    ap_in, trap_in, err = _side(ins, outs)
    ap_out, trap_out, _ = _side(-outs, -ins)                   # out = positive, score negated
    return [ap_in, ap_out, trap_in, trap_out, float(min(0.5, err.min()))]


def pr_bounds(n_in, n_out):
    """Absolute bounds on |figure - scikit-learn's|, derived, not measured: an AUPR / AUCPR is a sum of at most n terms with
    total at most 1, each formed with three roundings, so either side stays within (n + 3) * 2^-53 of the exact value; dete is
    two divisions, two (exact) halvings and a sum."""
    return [(n_in + n_out + 3) * 2.0 ** -52] * 4 + [2.0 ** -50]


def golden_cases(golden_dir):
    """{name: dict(ins, outs, modes, figures, refused)} of every golden file"""
    out = {}
    for f in sorted(glob.glob(os.path.join(golden_dir, 'pr', '*.npz'))):
        g = np.load(f)
        out[os.path.basename(f)[:-4]] = {k: g[k] for k in ('ins', 'outs', 'modes', 'figures', 'refused')}
    return out


def test_goldens_cover_the_cases(golden_dir):
    cases = golden_cases(golden_dir)
    assert sorted(cases) == sorted(CASES)
    for name, c in cases.items():
        M = len(c['modes'])
        assert c['ins'].dtype == np.float32 and c['outs'].dtype == np.float32 and c['ins'].shape[0] == c['outs'].shape[0] == M
        assert c['figures'].shape == (M, 5) and c['figures'].dtype == np.float64
        assert c['ins'].nbytes + c['outs'].nbytes <= 32 * 1024 + 64
        assert os.path.getsize(os.path.join(golden_dir, 'pr', name + '.npz')) < 64 * 1024
    shapes = {n: (c['ins'].shape[1], c['outs'].shape[1]) for n, c in cases.items()}
    assert shapes['small_1_1'] == (1, 1) and shapes['small_5_3'] == (5, 3) and shapes['tile'] == (2048, 2048)
    assert shapes['tile_minus_1'] == (2047, 2049) and shapes['tile_plus_1'] == (2049, 2047)
    assert shapes['tiles_5000_3000'] == (5000, 3000) and shapes['ties_2600_1900'] == (2600, 1900)
    assert shapes['around_mean_1500_1200'] == (1500, 1200) and shapes['inf_300_200'] == (300, 200)
    assert list(cases['rows3']['modes']) == [0, 1, 0] and list(cases['around_mean_1500_1200']['modes']) == [1]
    assert list(cases['inf_300_200']['refused']) == [1] and np.isinf(cases['inf_300_200']['ins']).sum() == 3
    assert all(not c['refused'].any() for n, c in cases.items() if n != 'inf_300_200')
    z = cases['zeros_pm']
    for row in (z['ins'][0], z['outs'][0]):                    # both zeros and the 1 in both rows
        assert (np.signbit(row) & (row == 0)).any() and (~np.signbit(row) & (row == 0)).any() and (row == 1).any()
    t = cases['ties_2600_1900']
    assert set(np.unique(t['ins'])) <= set(range(12)) and set(np.unique(t['outs'])) <= set(range(12))
    r = cases['rows3']
    assert all(np.array_equal(np.sort(r['ins'][0]), np.sort(r['ins'][m])) for m in (1, 2))
    assert all(np.array_equal(np.sort(r['outs'][0]), np.sort(r['outs'][m])) for m in (1, 2))
    assert np.array_equal(r['figures'][0], r['figures'][2])
    a = cases['around_mean_1500_1200']['ins']
    assert np.array_equal(a * 1024, np.round(a * 1024)) and np.abs(a).max() < 1024


def test_restatement_reproduces_every_golden(golden_dir):
    for name, c in golden_cases(golden_dir).items():
        for m, mode in enumerate(c['modes']):
            if c['refused'][m]:
                continue
            got = pr_restatement(c['ins'][m], c['outs'][m], int(mode))
            for k, g, w, b in zip(PR_FIGURES, got, c['figures'][m], pr_bounds(c['ins'].shape[1], c['outs'].shape[1])):
                assert abs(g - w) <= b, (name, m, k, g, w, abs(g - w) / b)


def test_restatement_on_the_closed_cases(golden_dir):
    cases = golden_cases(golden_dir)
    got = pr_restatement(cases['separated_500_300']['ins'][0], cases['separated_500_300']['outs'][0])
    assert all(abs(g - w) <= b for g, w, b in zip(got, [1., 1., 1., 1., 0.], pr_bounds(500, 300))) and got[4] == 0.
    got = pr_restatement(cases['identical_400']['ins'][0], cases['identical_400']['outs'][0])
    assert got == [0.5, 0.5, 0.75, 0.75, 0.5]                  # one tie group: P = 1/2, the trapezoid runs up to P' = 1
    got = pr_restatement(cases['reversed_300_500']['ins'][0], cases['reversed_300_500']['outs'][0])
    assert got[4] == 0.5 and got[0] < 300 / 800 + 1e-12 and got[1] < 500 / 800 + 1e-12
    assert np.isnan(pr_restatement([1., 2.], [0.], 2 | 4 << 8 | 1 << 16)).all()
    # the two zeros are one tie group: the figures do not change when every zero gets one sign
    z = cases['zeros_pm']
    assert pr_restatement(z['ins'][0], z['outs'][0]) == pr_restatement(np.abs(z['ins'][0]), np.abs(z['outs'][0]))


def test_restatement_defines_the_infinite_scores(golden_dir):
    """scikit-learn raises ValueError on infinite scores; here they are ordinary values that tie with themselves: replacing
    them by finite values beyond every other score changes nothing."""
    c = golden_cases(golden_dir)['inf_300_200']
    assert np.isnan(c['figures']).all()
    got = pr_restatement(c['ins'][0], c['outs'][0])
    finite = [np.where(np.isinf(v), np.sign(v) * 100, v).astype(np.float32) for v in (c['ins'][0], c['outs'][0])]
    assert got == pr_restatement(*finite)
    assert all(0 <= g <= 1 for g in got) and got[4] < 0.5


def test_pr_metrics_off_the_gpu_is_an_error():
    import torch
    from jvae_compat import roc_curves
    from jvae_hip import lib, ops
    assert ops.PR_FIGURES == PR_FIGURES
    with pytest.raises(lib.JvaeHipError):
        ops.pr_metrics(torch.zeros(8), torch.zeros(8))
    with pytest.raises(lib.JvaeHipError):
        roc_curves.pr_metrics([0., 1.], np.zeros(3), device='cpu')


def test_the_switch_is_off_on_the_class():
    from cvae import ClassificationVariationalNetwork as Net
    from module.scoring import ScoringMixin
    assert ScoringMixin.DETECTION_PR_METRICS is False and Net.DETECTION_PR_METRICS is False
    assert Net.MISCLASS_PR_KEYS == ('aupr_correct', 'aupr_error', 'aucpr_correct', 'aucpr_error', 'dete')


def test_the_abi_names_are_bound():
    from jvae_hip import lib
    L = lib.load()
    assert L.jvae_pr_workspace_bytes(1, 1, 1) > 0
    for bad in ((0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, (1 << 24) + 1, 1), (1, 1, (1 << 24) + 1)):
        assert L.jvae_pr_workspace_bytes(*bad) == 0, bad
    assert L.jvae_pr_workspace_bytes(11, 1 << 24, 1 << 24) > 0
