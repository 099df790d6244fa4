"""The public names of the reference's `utils/roc_curves.py` on the device ROC (jvae_hip.ops.roc_curve, csrc/roc.hip).

`roc_curve` takes what the reference's takes (array-likes or tensors, on any device: they are moved to the GPU as fp32, the
precision in which the model produces its scores) and returns numpy values of the same shapes.  What the reference computes
through a SciPy spline (`two_sided=(a, b)`), a validation split or reversed scores raises there; `roc_curve_quantile` is the
tuple mode on the spline's noise-free values, under a name of its own because its numbers are not the reference's.

Public names: `fpr_at_tpr`, `tpr_at_fpr`, `roc_curve`, `roc_curve_quantile` and `pr_metrics` - the precision-recall side the
reference's scripts take from scikit-learn (AUPR-in / -out, AUCPR, detection error), computed by jvae_hip.ops.pr_metrics.
"""
import numpy as np
import torch

from jvae_hip import ops


def fpr_at_tpr(fpr, tpr, a, thresholds=None, return_threshold=False):
    """fpr and tpr in ascending order (utils/roc_curves.py:8-27)."""
    assert not return_threshold or thresholds is not None
    i_ = np.where(np.asarray(tpr) >= a)[0].min()
    fpr_ = np.asarray(fpr)[i_]
    return (fpr_, thresholds[i_]) if return_threshold else fpr_


def tpr_at_fpr(fpr, tpr, a):
    """utils/roc_curves.py:30-35"""
    return np.asarray(tpr)[np.where(np.asarray(fpr) <= a)[0]].max()


def roc_curve(ins, outs, *kept_tpr, two_sided=False, validation=0, debug=False, ins_are_higher=True, device=None):
    """-> (auc, kept_fpr, kept_tpr, {'low': ..., 'up': ...}) of utils/roc_curves.py:38-210; ValueError on a NaN score (and on
    a non-finite in-score with two_sided='around-mean', where the reference fails as well)."""
    if validation:
        raise NotImplementedError('roc_curve: a validation split of the in-scores is not built')
    if not ins_are_higher:
        raise NotImplementedError('roc_curve: ins_are_higher=False is not built')
    if isinstance(two_sided, tuple):
        raise NotImplementedError('roc_curve: the spline thresholds (two_sided=(a, b)) are not built')
    return _one_row(ins, outs, kept_tpr, 'around-mean' if two_sided == 'around-mean' else False, device)


def roc_curve_quantile(ins, outs, *kept_tpr, factors=(1, 1), device=None):
    """What `roc_curve(ins, outs, *kept_tpr, two_sided=factors)` of the reference computes (utils/roc_curves.py:74-83, the
    '-a-x-y' OOD methods) when its spline through the sorted in-scores returns them unchanged: every factors[0]-th one is a
    lower threshold, every factors[1]-th one an upper threshold, met from the two ends.  The reference's own numbers carry
    FITPACK's rounding of that spline on top and differ slightly.  Same return tuple as `roc_curve`;
    ValueError on a NaN score and for fewer than 4 in-scores, where the reference's cubic fit fails."""
    n_in = ins.numel() if torch.is_tensor(ins) else np.size(ins)
    if n_in < 4:
        raise ValueError(f'roc_curve_quantile: {n_in} in-distribution scores, the cubic spline of the reference needs 4')
    return _one_row(ins, outs, kept_tpr, ('quantile',) + tuple(factors), device)


def pr_metrics(ins, outs, two_sided=False, device=None):
    """-> {'aupr_in', 'aupr_out', 'aucpr_in', 'aucpr_out', 'dete'} as plain floats: scikit-learn's average_precision_score and
    auc(recall, precision) with in, resp. out and the negated score, as the positive class, and the smallest detection error
    0.5 (1 - tpr) + 0.5 fpr over all thresholds (jvae_hip.ops.pr_metrics, csrc/prc.hip).  two_sided: False or
    'around-mean' (the score of a sample is then -|s - mean(ins)|).  ValueError on a NaN score, as for `roc_curve`."""
    if isinstance(two_sided, tuple):
        raise NotImplementedError('pr_metrics: quantile thresholds (two_sided=(a, b)) give no scalar score')
    rows = _rows(ins, outs, device)
    r = ops.pr_metrics(rows[0], rows[1], 'around-mean' if two_sided == 'around-mean' else False)
    host = ops.read_back(r)
    ops.roc_check_status([int(host['status'])])
    return {k: float(host[k]) for k in ops.PR_FIGURES}


def _rows(ins, outs, device):
    device = device or ('cuda' if torch.cuda.is_available() else 'cpu')      # off the GPU the op raises JvaeHipError
    return [torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(device=device, dtype=torch.float32).reshape(-1)
            for v in (ins, outs)]


def _one_row(ins, outs, kept_tpr, mode, device):
    rows = _rows(ins, outs, device)
    r = ops.roc_curve(rows[0], rows[1], sorted(kept_tpr), mode)
    host = ops.read_back(r)
    ops.roc_check_status([int(host['status'])])
    return float(host['auc']), host['fpr'], host['tpr'], {'low': host['low'], 'up': host['up']}
