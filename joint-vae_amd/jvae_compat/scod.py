"""SCOD: selective classification in the presence of out-of-distribution data, on the device (reference tests/scod.py).

One rejection score - the HIGHer the more likely to REJECT - is applied to the union of the in-distribution test set and all
OOD sets of a fine-tuned (WIM) or `vib` job; sweeping it gives the selective risk and the false-positive rate as functions of
the coverage.  The figures are FPR@95, SR@95, AuROC, AuST and AuSCODT.

`scoring_r`, `scoring_g`, `scoring`, `scrisk` and `default_scores` keep the reference's names, signatures and return values;
`scod_rates` does what the reference's command-line block does with the recorders of a job.  The arithmetic runs in
csrc/scod.hip (`ops.scod_scores`, `ops.scod_curve`): there is no CPU path.  No plotting, no command line.
"""
import itertools
import logging
import os

import torch

from jvae_hip import ops
from jvae_hip import lib as _lib
from module.score_rows import ODIN

default_scores = {'wim': {'r': 'zdist', 'g': 'elbo'},
                  'vib': {'r': 'odin-1-0.0040', 'g': 'none'}}


def _host_lse(zdist):
    """logsumexp_c(-0.5 zdist) of `logmsp` as the reference takes it: torch's expression on the HOST, whose last bits the
    device's torch.logsumexp does not reproduce (other exp / log routines: up to 5e-7 apart on an MI355X, enough to move a
    last bit of the score and with it the order of two samples).  Costs one copy of `zdist` to the host and one row back."""
    return (-0.5 * zdist.cpu()).logsumexp(0).to(zdist.device)


def _r_spec(losses, score, mtype, cache=None):
    """The r side of a variant -> (kind of ops.SCOD_R_KINDS, source, aux).  The branches are the reference's (scod.py:77-105):
    a name none of them matches - 'zdist', the default of a wim, among them - is 0.  cache: a dict that keeps the log-sum-exp
    row of `logmsp` between the variants of one set."""
    if score is None:
        score = default_scores[mtype]['r']
    logging.debug('r score is %s', score)
    if score and score.startswith(ODIN.prefix):
        return 'odin', losses[score], None
    if score == 'predist':
        return 'half_y', losses['pre-zdist'], None
    if score == 'dist':
        return 'half_y', losses['zdist'], None
    if score == 'logmsp':
        zdist = losses['zdist']
        cache = {} if cache is None else cache
        if 'lse' not in cache:
            cache['lse'] = _host_lse(zdist)                        # the class-axis log-sum-exp stays a torch row
        return 'logmsp', zdist, cache['lse']
    return 'zero', None, None


def _g_spec(losses, score, mtype):
    """The g side of a variant -> (kind of ops.SCOD_G_KINDS, source, alternate) (scod.py:108-144)."""
    if score is None:
        score = default_scores[mtype]['g']
    logging.debug('g score is %s', score)
    key, kind = score, 'plain'
    if score == 'elbo':
        key, kind = 'zdist', 'half'
    if score == 'iws':
        kind = 'neg'
    if mtype != 'wim':
        return 'zero', None, None
    return kind, losses[key], losses[key + '@']


def _classes(spec):
    """C of a variant's all-class tensors (1 when it reads none)."""
    for src in (spec[1], spec[4]):
        if src is not None and src.dim() == 2:
            return src.shape[0]
    return 1


def scoring_r(losses, score='msp', y_est=None, mtype='cvae'):
    """Estimation of 1 - max P(y|x): a (N,) device row, or 0. where the reference returns 0."""
    spec = _r_spec(losses, score, mtype)
    if spec[0] == 'zero':
        return 0.
    if y_est is None and spec[0] != 'odin':
        y_est = losses['y_est_already']
    N = spec[1].shape[-1]
    C = spec[1].shape[0] if spec[1].dim() == 2 else 1
    return ops.scod_scores([spec + (None, None, None, 0.)], y_est, C, N)[0]


def scoring_g(losses, score='elbo', y_est=None, mtype='wim'):
    """Estimation of pOut / pIn: a (N,) device row, or 0. for any type but 'wim'."""
    if y_est is None:
        y_est = losses['y_est_already']
    spec = _g_spec(losses, score, mtype)
    if spec[0] == 'zero':
        return 0.
    C, N = spec[1].shape
    return ops.scod_scores([(None, None, None) + spec + (1.,)], y_est, C, N)[0]


def _variants(losses, variants, kw_r, kw_g):
    """The (r, g, weight) variants of one set as the tuples `ops.scod_scores` takes."""
    cache = {}
    return [_r_spec(losses, r, cache=cache, **kw_r) + _g_spec(losses, g, **kw_g) + (weight,) for r, g, weight in variants]


def scoring(losses, r=None, g='elbo', weight=1, **kw):
    """r + weight * g, reject if high: a (N,) device row (0. where both sides are 0. for the reference too)."""
    try:
        y_est = losses['y_est_already']
        kw_r = dict({'mtype': 'cvae'}, **kw)
        kw_g = dict({'mtype': 'wim'}, **kw)
        spec, = _variants(losses, [(r, g, weight)], kw_r, kw_g)
        if spec[0] == 'zero' and spec[3] == 'zero':
            return 0. + weight * 0.
        return ops.scod_scores([spec], y_est, _classes(spec), y_est.shape[0])[0]
    except KeyError as e:
        logging.error('Possibles keys')
        logging.error(' -- '.join(losses))
        raise e


def scrisk(y_true, y_est, scores):
    """Computation of the sc(od) risk.  y_true: class for indist, -1 for ood; y_est: estimated class; scores: the HIGHer the
    more likely to REJECT.  -> (tpr, selective_risk, fpr), fp32 tensors on the device of the inputs.  Equal scores are taken in
    the order of their positions (the reference's torch.sort leaves that order unspecified)."""
    res = ops.scod_curve(scores, y_true, y_est, curves=True, figures=False)
    ops.scod_check_status(res['status'].cpu())
    return res['tpr'], res['selective_risk'], res['fpr']


class _Losses:
    """The tensors of one recorder on the device, fetched once each; `y_est_already` from `cross_y` where it was not recorded."""

    def __init__(self, recorder, device):
        self._rec, self._dev, self._got = recorder, device, {}

    def __iter__(self):
        return iter(self._rec)

    def __contains__(self, k):
        return k in self._got or k in list(self._rec)

    def __getitem__(self, k):
        if k not in self._got:
            if k == 'y_est_already' and k not in list(self._rec):
                self._got[k] = self['cross_y'].argmin(0)
            else:
                self._got[k] = self._rec[k].to(self._dev)
        return self._got[k]


def scod_rates(recorders, dset, mtype=None, r=None, g=None, weight=1., curves=False, device=None):
    """The SCOD figures of a job from its recorders {set name: LossRecorder or dict of tensors}, as the reference's command-line
    block computes them (scod.py:215-235): `y_est_already` is filled from `cross_y.argmin(0)` where a recorder lacks it, all sets
    are concatenated in recorder order, y_true is the class for `dset` and -1 for every other set, the scores are
    `scoring(recorder, r=r, g=g, weight=weight, mtype=mtype)`.

    -> {'fpr95', 'sr95', 'auroc', 'aust', 'auscodt'} (floats); with `curves` also 'tpr', 'selective_risk', 'fpr' ((n,) fp32
    device tensors).  r, g and weight may be lists: every combination goes through the same launches - ONE `ops.scod_scores` per
    set (per 32 variants), ONE `ops.scod_curve` - and the result is {(r, g, weight): that dictionary}.  The only values read
    back are the figures and the status words, in one copy - and, where an r is 'logmsp', each set's `zdist` once (`_host_lse`).  mtype None: each side of the score uses its own default type, as
    `scoring()` called without one does."""
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
    device = torch.device(device)
    as_lists = [isinstance(v, (list, tuple)) for v in (r, g, weight)]
    variants = list(itertools.product(*[list(v) if many else [v] for v, many in zip((r, g, weight), as_lists)]))
    kw = {} if mtype is None else {'mtype': mtype}
    kw_r, kw_g = dict({'mtype': 'cvae'}, **kw), dict({'mtype': 'wim'}, **kw)
    names = list(recorders)
    sets = {s: _Losses(recorders[s], device) for s in names}
    try:
        y_est = torch.hstack([sets[s]['y_est_already'] for s in names])
    except KeyError as e:
        logging.error('Possibles keys')
        logging.error(' -- '.join(str(k) for s in names for k in sets[s]))
        raise e
    _lib.ptr(y_est)                                                # there is no CPU path
    y_true = torch.hstack([sets[s]['y_true'] * int(s == dset) - int(s != dset) for s in names])
    sizes = [sets[s]['y_est_already'].shape[0] for s in names]
    n, n_in = sum(sizes), sum(k for s, k in zip(names, sizes) if s == dset)
    if n_in < 1 or n_in >= n:
        raise _lib.JvaeHipError(f'scod_rates: {n_in} samples of {dset!r} and {n - n_in} OOD samples: neither side may be empty')
    if n > ops.SCOD_MAX_N:
        raise _lib.JvaeHipError(f'scod_rates: {n} samples, at most {ops.SCOD_MAX_N}')
    M = len(variants)
    scores = torch.empty((M, n), dtype=torch.float32, device=device)
    word = torch.zeros(1, dtype=torch.int32, device=device)
    col = 0
    for s, k in zip(names, sizes):
        losses = sets[s]
        try:
            specs = _variants(losses, variants, kw_r, kw_g)
        except KeyError as e:
            logging.error('Possibles keys')
            logging.error(' -- '.join(str(_) for _ in losses))
            raise e
        ops.scod_scores(specs, losses['y_est_already'], max(_classes(sp) for sp in specs), k, out=scores, col=col, status=word)
        col += k
    res = ops.scod_curve(scores, y_true.to(torch.int64), y_est.to(torch.int64), curves=curves, figures=True, n_in=n_in)
    host = ops.read_back({'figures': res['figures'], 'status': res['status'], 'word': word})     # the one read-back
    ops.wim_check_status(int(host['word'][0]))
    ops.scod_check_status([int(v) for v in host['status']])
    out = {}
    for m, v in enumerate(variants):
        out[v] = dict(zip(ops.SCOD_FIGURES, host['figures'][m].tolist()))
        if curves:
            out[v].update({k: res[k][m] for k in ('tpr', 'selective_risk', 'fpr')})
    return out if any(as_lists) else out[variants[0]]


def job_scod_rates(net, sample_dir=None, epoch='last', **kw):
    """`scod_rates` on the `record-*.pth` files of a saved job (what `ScoringMixin.scod_rates` calls): `sample_dir`, or
    `saved_dir/samples/<epoch:04d>` - `epoch='last'`: `samples/last` where it holds records, else the largest epoch directory
    that does.  dset is the job's training set, mtype its type, 'wim' for a fine-tuned job."""
    from jvae_compat.recorders import LossRecorder

    def has_records(d):
        return os.path.isdir(d) and bool(LossRecorder.loadall(d, output='paths'))
    if sample_dir is None:
        root = os.path.join(getattr(net, 'saved_dir', None) or '', 'samples')
        if epoch == 'last':
            sample_dir = os.path.join(root, 'last')
            if not has_records(sample_dir):
                found = [d for d in (os.listdir(root) if os.path.isdir(root) else [])
                         if d.isdigit() and has_records(os.path.join(root, d))]
                if not found:
                    raise FileNotFoundError(f'scod_rates: no record-*.pth under {root}')
                sample_dir = os.path.join(root, max(found, key=int))
        else:
            sample_dir = os.path.join(root, '{:04d}'.format(int(epoch)))
    recorders = LossRecorder.loadall(sample_dir, map_location=net.device)
    if not recorders:
        raise FileNotFoundError(f'scod_rates: no record-*.pth in {sample_dir}')
    from jvae_compat.wim import WIMJob
    kw.setdefault('mtype', 'wim' if isinstance(net, WIMJob) else net.type)
    kw.setdefault('device', net.device)
    return scod_rates(recorders, net.training_parameters['set'], **kw)
