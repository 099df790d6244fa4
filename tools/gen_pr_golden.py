#!/usr/bin/env python3
"""Write tests/golden/pr/*.npz: score rows and scikit-learn's precision-recall figures for them.

    python tools/gen_pr_golden.py

Needs numpy and scikit-learn (the tests read the files and import neither scikit-learn nor this tool).  Each file holds
`ins` (M, n_in) and `outs` (M, n_out) fp32, `modes` (M,) int32 - the mode words of jvae_roc_curve_f32: 0 one-sided,
1 'around-mean' - `figures` (M, 5) fp64 in the order of jvae_hip.ops.PR_FIGURES, `refused` (M,) int32 and the versions:

    aupr_in    average_precision_score(y, s)          y = 1 for an in-sample, s the scores widened exactly to fp64
    aupr_out   average_precision_score(1 - y, -s)
    aucpr_in   auc(recall, precision) of precision_recall_curve(y, s)
    aucpr_out  the same of precision_recall_curve(1 - y, -s)
    dete       min 0.5 (1 - tpr) + 0.5 fpr over roc_curve(y, s, drop_intermediate=False)

For an around-mean row s = -|score - c| in fp64, c the fp64 mean of the row's in-scores.  In-scores are integer multiples of
2^-10 with magnitude below 16: their fp64 sum is exact in any order, so c is one correctly rounded division and no golden hangs
on a summation order.  Where scikit-learn refuses the input (infinite scores: ValueError) the row's figures are NaN and
`refused` is 1; the numpy restatement in tests/test_pr_restatement.py defines the answer there.
"""
import os

import numpy as np
import sklearn
from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_curve

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'pr')


def grid_scores(rng, n, mean=0., std=1.):
    """fp32 multiples of 2^-10 in (-16, 16)"""
    return np.clip(np.round((rng.standard_normal(n) * std + mean) * 1024) / 1024, -15.5, 15.5).astype(np.float32)


def cases():
    """name -> (ins (M, n_in), outs (M, n_out), modes)"""
    rng = np.random.default_rng(20250311)
    c = {}

    def gauss(n_in, n_out, mode=0):
        return grid_scores(rng, n_in, 1.)[None], rng.standard_normal(n_out).astype(np.float32)[None], [mode]
    for name, n_in, n_out in (('small_1_1', 1, 1), ('small_5_3', 5, 3), ('tile', 2048, 2048), ('tile_minus_1', 2047, 2049),
                              ('tile_plus_1', 2049, 2047), ('tiles_5000_3000', 5000, 3000)):
        c[name] = gauss(n_in, n_out)
    c['ties_2600_1900'] = (rng.integers(0, 12, (1, 2600)).astype(np.float32), rng.integers(0, 12, (1, 1900)).astype(np.float32), [0])
    c['identical_400'] = (np.full((1, 400), 0.75, np.float32), np.full((1, 400), 0.75, np.float32), [0])
    c['separated_500_300'] = (grid_scores(rng, 500, 8., .5)[None], (rng.standard_normal(300) * .5 - 8).astype(np.float32)[None], [0])
    c['reversed_300_500'] = (grid_scores(rng, 300, -8., .5)[None], (rng.standard_normal(500) * .5 + 8).astype(np.float32)[None], [0])
    levels = np.array([-0.0, 0.0, 1.0], np.float32)
    c['zeros_pm'] = (levels[rng.integers(0, 3, 600)][None], levels[rng.integers(0, 3, 500)][None], [0])
    ins, outs = grid_scores(rng, 700, 1.), rng.standard_normal(500).astype(np.float32)
    c['rows3'] = (np.stack([ins, ins[::-1], rng.permutation(ins)]), np.stack([outs, rng.permutation(outs), outs[::-1]]), [0, 1, 0])
    c['around_mean_1500_1200'] = (grid_scores(rng, 1500, 1., .5)[None], (rng.standard_normal(1200) * 2).astype(np.float32)[None], [1])
    ins, outs = grid_scores(rng, 300, 1.), rng.standard_normal(200).astype(np.float32)
    ins[[3, 77]], ins[150], outs[[0, 9]], outs[100] = np.inf, -np.inf, -np.inf, np.inf
    c['inf_300_200'] = (ins[None], outs[None], [0])
    return c


def sklearn_figures(ins, outs, mode):
    ins, outs = ins.astype(np.float64), outs.astype(np.float64)
    if mode:
        centre = ins.mean()
        ins, outs = -abs(ins - centre), -abs(outs - centre)
    y, s = np.r_[np.ones(len(ins)), np.zeros(len(outs))], np.r_[ins, outs]
    p_in, r_in, _ = precision_recall_curve(y, s)
    p_out, r_out, _ = precision_recall_curve(1 - y, -s)
    fpr, tpr, _ = roc_curve(y, s, drop_intermediate=False)
    return [average_precision_score(y, s), average_precision_score(1 - y, -s), auc(r_in, p_in), auc(r_out, p_out),
            np.min(0.5 * (1 - tpr) + 0.5 * fpr)]


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (ins, outs, modes) in cases().items():
        figures, refused = np.full((len(modes), 5), np.nan), np.zeros(len(modes), np.int32)
        for m, mode in enumerate(modes):
            try:
                figures[m] = sklearn_figures(ins[m], outs[m], mode)
            except ValueError as err:
                refused[m] = 1
                print(f'{name} row {m}: scikit-learn refuses: {err}')
        np.savez_compressed(os.path.join(OUT, name + '.npz'), ins=np.ascontiguousarray(ins), outs=np.ascontiguousarray(outs),
                            modes=np.asarray(modes, np.int32), figures=figures, refused=refused,
                            sklearn_version=np.array(sklearn.__version__), numpy_version=np.array(np.__version__))
        for m, f in enumerate(figures):
            print(f'{name:24s} row {m} mode {modes[m]}: ' + ' '.join(f'{v:.6f}' for v in f))


if __name__ == '__main__':
    main()
