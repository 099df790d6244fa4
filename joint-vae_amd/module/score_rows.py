"""What an OOD / misclassification / WIM method name means, in one place: `parse()` turns a name such as `softkl-10`, `iws-2s`,
`elbo-a-4-1`, `zdist~` or `elbo@` into a `Row` (the loss it reads, its kernel row, its torch expression, its ROC mode) and
`write_rows()` computes the rows of a batch: kernel rows by one launch per source tensor, the others by their torch expression.

The torch expressions are the reference's (cvae.py:972-1085, ft/wim.py:145-192), written once per KIND of row; a name is an entry
of the table below: source, kind, constant."""
import math
from collections import namedtuple
from dataclasses import dataclass

import torch

from jvae_hip import ops

# what the form of a row depends on besides its name
# (OOD_REGRET_METHODS, OOD_KNN_METHODS, OOD_IC_METHODS, OOD_SSIM_METHODS, OOD_DOSE_METHODS, OOD_MAHA_METHODS: the model's opt-in
# switches of the recorded `regret-*` / `knn-*` / `ic-*` / `ssim*` / `dose*` / `maha*` rows; off where a caller does not say.  The
# switches are read by name, their order means nothing.)
Traits = namedtuple('Traits', 'losses_might_be_computed_for_each_class is_vae is_jvae num_labels OOD_REGRET_METHODS OOD_KNN_METHODS '
                    'OOD_IC_METHODS OOD_SSIM_METHODS OOD_DOSE_METHODS OOD_MAHA_METHODS',
                    defaults=(False, False, False, False, False, False))


# One family of RECORDED score rows: a model method computes them once per batch, the pass records them with the losses, reads
# them back from a full recorder and copies them into the score buffer as they are.  prefix: a name that starts with it is the
# family's (`_ood_methods` refuses it unless the model lists it); is_row: name without its thresholding suffix -> whether it is a
# well-formed row (`parse` accepts nothing else); starred: the name that expands to the model's list; switch, types: the NAMES of
# the model's opt-in switch and, if only some model types have the rows, of its tuple of those types - `on(model)` and
# `trait(traits)` say whether the family is switched on, from a model and from a Traits value (no switch: `odin*`, on where the
# type's own table lists it); names, scores: the NAMES of the model methods (looked up at each call) that list the rows and compute
# {row: (N,) scores} from the keywords `args` - `x`, `logits`, `losses` (the batch and its label-free evaluation), `mu` (its
# posterior means), `x_reco` (its reconstructions); off, unlisted: the refusals where the family is off / the model does not list
# the name
class Family(namedtuple('Family', 'prefix is_row starred switch types names scores args off unlisted')):
    __slots__ = ()

    def on(self, model):
        if self.switch is None:
            return self.starred in model.ood_methods
        return bool(getattr(model, self.switch)) and (self.types is None or model.type in getattr(model, self.types))

    def trait(self, t):
        return self.switch is None or getattr(t, self.switch)


# in the order in which 'all' and the starred names expand and the per-batch calls run.  Callers read `score_rows.FAMILIES` at the
# call: a test takes a family out by replacing the attribute
FAMILIES = (
    Family('odin', lambda m: m.startswith('odin'), 'odin*', None, None,      # cvae.py:1076-1078, 1645-1663
           '_odin_names', 'odin_scores', ('x',),
           '{m}: spline-threshold (-a-x-y) and ODIN OOD methods are outside this build',
           '{m}: not on the ODIN grid of this model (ODIN_TEMPS x ODIN_EPS)'),
    Family('regret', lambda m: m.startswith('regret-'), 'regret*', 'OOD_REGRET_METHODS', 'REGRET_TYPES',
           '_regret_names', 'regret_scores', ('x', 'logits', 'losses'),
           '{m}: the likelihood-regret rows are an opt-in (OOD_REGRET_METHODS) of the types {types}',
           '{m}: not among the (steps, lr) pairs of this model (REGRET_PARAMS)'),
    Family('knn', lambda m: m.startswith('knn-') and m[4:].isdigit(), 'knn*', 'OOD_KNN_METHODS', None,
           '_knn_names', 'knn_scores', ('mu',),
           '{m}: the nearest-neighbour rows are an opt-in (OOD_KNN_METHODS)',
           '{m}: not among the neighbour counts of this model (KNN_K)'),
    Family('maha', lambda m: m in ('maha', 'maha-rel'), 'maha*', 'OOD_MAHA_METHODS', None,
           '_maha_names', 'maha_scores', ('mu',),
           '{m}: the Mahalanobis rows are an opt-in (OOD_MAHA_METHODS)',
           '{m}: not among the Mahalanobis rows of this model (`maha`; `maha-rel` with more than one fitted class)'),
    Family('ic-', lambda m: m in ('ic-bits', 'ic-elbo', 'ic-iws'), 'ic*', 'OOD_IC_METHODS', 'IC_TYPES',
           '_ic_names', 'ic_scores', ('x', 'losses'),
           '{m}: the input-complexity rows are an opt-in (OOD_IC_METHODS) of the types with a decoder (IC_TYPES)',
           '{m}: not among the input-complexity rows of this model (`ic-bits`, `ic-elbo`, `ic-iws`)'),
    Family('dose', lambda m: m == 'dose' or m.startswith('dose-'), 'dose*', 'OOD_DOSE_METHODS', 'DOSE_TYPES',
           '_dose_names', 'dose_scores', ('logits', 'losses'),
           '{m}: the density-of-states rows are an opt-in (OOD_DOSE_METHODS) of the types of DOSE_TYPES',
           '{m}: not among the density-of-states rows of this model (`dose`, `dose-joint`, `dose-<stat>` and `dose-typ-<stat>` for '
           'the statistics of DOSE_STATS)'),
    Family('ssim', lambda m: m in ('ssim', 'ssim-mu', 'ssim-cs'), 'ssim*', 'OOD_SSIM_METHODS', 'SSIM_TYPES',
           '_ssim_names', 'ssim_scores', ('x', 'x_reco'),
           '{m}: the SSIM rows are an opt-in (OOD_SSIM_METHODS) of the types with a decoder (SSIM_TYPES)',
           '{m}: not among the SSIM rows of this model (`ssim`, `ssim-mu`, `ssim-cs`)'))
ODIN = FAMILIES[0]
odin_name = (ODIN.prefix + '-{:.0f}-{:.4f}').format            # (T, eps) -> `odin-T-eps` as the reference formats it (cvae.py:124-127)


def claimed_by(name):
    """The family whose prefix claims `name` (or whose starred name it is), or None."""
    return next((f for f in FAMILIES if name.startswith(f.prefix) or name == f.starred), None)


def recorded_by(name):
    """The family `name` (no thresholding suffix) is a well-formed row of, or None."""
    for f in FAMILIES:
        if f.is_row(name):
            return f


def traits_of(model):
    opt = Traits._field_defaults
    return Traits(*(getattr(model, f, opt[f]) if f in opt else getattr(model, f) for f in Traits._fields))


# name -> (source, kind of ops.misclass_scores, its temperature or additive constant) where the model type has no say
_ROWS = {'max': ('total', 'max-', 1.), 'softiws': ('iws', 'soft+', 1.), 'soft': ('kl', 'soft-', 1.), 'softkl': ('kl', 'soft-', 1.),
         'mse': ('cross_x', 'neg', 0.), 'wmse': ('wmse', 'neg', 0.), 'logits': ('logits', 'max+', 1.), 'hyz': ('logits', 'hyz', 1.),
         'sum': ('total', 'lse-', 0.),                         # cvae.py:1020-1068: the class-axis scores, all from -losses['total']
         **{m: ('total', m, 0.) for m in ('mean', 'std', 'nstd', 'mag', 'IYx')}}
_OOD_ONLY = ('elbo', 'mse', 'wmse')                            # no rows of the misclassification pass
# WIM family -> (source, the factor of the family on its loss, ft/wim.py:145); `elbo` is -total
_WIM = {'kl': ('kl', -1.), 'zdist': ('zdist', -0.5), 'iws': ('iws', 1.), 'elbo': ('total', 1.)}


def roc_mode(name):
    """The `two_sided` value of ops.roc_curve for a method name (cvae.py:1850-1854)."""
    if name.endswith('-2s'):
        return 'around-mean'
    if '-a-' not in name:
        return False
    factors = name.split('-a-')[1].split('-')
    if len(factors) != 2 or not all(f.isdigit() and 1 <= int(f) <= 255 for f in factors):
        raise ValueError(f'{name}: <score>-a-<x>-<y> with x and y in 1 .. 255 expected')
    return ('quantile', int(factors[0]), int(factors[1]))


def _plain_entry(m, t):
    """(source, kind, const) of the score `m` (no thresholding suffix) on a model with the traits `t`; None: no such score."""
    per_class = t.losses_might_be_computed_for_each_class
    family = recorded_by(m)
    if family is not None:                                     # recorded by the family's method; off: no such score
        return (m, None, None) if family.trait(t) else None
    if m == 'elbo':
        return ('total', 'max-', 1.) if per_class else ('total', 'neg', 0.)
    if m == 'iws':                                             # cvae.py:1013-1019: log C unless is_jvae
        return ('iws', 'lse+', 0. if t.is_jvae else math.log(t.num_labels)) if per_class else ('iws', 'id', 0.)
    if m in ('zdist', 'kl'):
        return (m, 'neg', 0.) if t.is_vae else (m, 'max-', 1.)
    if m in _ROWS:
        return _ROWS[m]
    if m.startswith('soft') and '-' in m:                      # cvae.py:1040-1043: soft<loss>-T
        return m.split('-')[0][4:], 'soft-', float(m.split('-')[-1])
    if m.startswith('baseline'):
        return 'logits', 'soft+', float(m.split('-')[-1]) if '-' in m else 1.
    return None


def _wim_entry(m):
    """'zdist~' -> Y, 'softkl~' -> SOFT_Y, 'elbo@' -> LSE_AT, 'iws~@' -> Y_AT of ops.wim_scores, on the family's source."""
    if m.endswith('~@'):
        k, kind = m[:-2], 'Y_AT'
    elif m.endswith('@'):
        k, kind = m[:-1], 'LSE_AT'
    elif m.startswith('soft'):
        k, kind = m[4:-1], 'SOFT_Y'
    else:
        k, kind = m[:-1], 'Y'
    if k not in _WIM:
        raise NotImplementedError(f'{m}: WIM score outside this build')
    return _WIM[k][0], kind, _WIM[k][1]


@dataclass(frozen=True)
class Row:
    """One score row.  base: the name without the '-2s' / '-a-x-y' suffix, which only names the thresholding done downstream
    (`roc_mode`); source: the key of the losses the row reads, `logits`, or the name itself for a recorded `odin-*` / `regret-*` /
    `knn-*` / `maha*` / `ic-*` / `dose*` / `ssim*` row; kind,
    const: its row of ops.misclass_scores (temperature or additive constant) or of ops.wim_scores (the family's factor), kind
    None where there is no kernel row."""
    name: str
    base: str
    roc_mode: object
    source: str
    kind: object
    const: object
    num_labels: int

    def torch_row(self, sources):
        """The reference's torch expression on `sources` (the losses; `logits` as (N, C), reduced over its last axis: a softmax
        summed over the other layout may round differently).  A constant of 0 adds nothing: -0. + 0. would be +0."""
        kind, c = self.kind, self.const
        if kind in ops.WIM_KINDS:
            return self._wim_torch_row(sources)
        v = sources[self.source]
        ax = -1 if self.source == 'logits' else 0
        if kind is None or kind == 'id':
            return v
        if kind == 'neg':
            return -v
        if kind in ('max+', 'max-'):
            return (v if kind == 'max+' else -v).max(ax)[0]
        if kind in ('soft+', 'soft-', 'hyz'):
            x = v if kind != 'soft-' else -v
            p = (x if c == 1. else x / c).softmax(ax)
            return (p * p.log()).sum(ax) if kind == 'hyz' else p.max(ax)[0]
        logp = v if kind == 'lse+' else -v                     # the class-axis rows
        if kind == 'std':
            return logp.std(0)
        top = logp.max(0)[0]
        if kind == 'mag':
            return top - logp.median(0)[0]
        d = logp - top
        if kind in ('lse-', 'lse+'):
            r = d.exp().sum(0).log() + top
            return r + c if c else r
        if kind == 'mean':
            return d.exp().mean(0).log() + top
        if kind == 'nstd':
            return (d.exp().std(0).log() - d.exp().mean(0).log()).exp().pow(2)
        d_x = d.exp().mean(0).log()                            # IYx
        return (d * d.exp()).sum(0) / (self.num_labels * d_x.exp()) - d_x

    def _wim_torch_row(self, losses):
        f, elbo = self.const, self.source == 'total'
        y = losses['y_est_already'].unsqueeze(0)
        v = -losses['total'] if elbo else losses[self.source]
        if self.kind in ('LSE_AT', 'Y_AT'):
            alt = -losses['total@'] if elbo else losses[self.source + '@']
        if self.kind == 'Y':
            return f * v.gather(0, y).squeeze(0)
        if self.kind == 'SOFT_Y':
            return (v * f).softmax(0).gather(0, y).squeeze(0)
        if self.kind == 'LSE_AT':
            return (v * f).logsumexp(0) - f * alt
        return f * v.gather(0, y).squeeze(0) - f * alt


def parse(name, traits, misclass=False):
    """Method name -> Row.  A name ending in `~` / `@` is a WIM row; any other is looked up without its thresholding suffix.
    Unknown: NotImplementedError, or ValueError with `misclass` (the misclassification pass asks: no WIM, `elbo`, `mse` rows)."""
    mode = roc_mode(name)
    base = name[:-3] if name.endswith('-2s') else name
    base = base.split('-')[0] if '-a-' in base else base
    wim = name[-1] in '~@'
    row = None if wim or (misclass and base in _OOD_ONLY) else _plain_entry(base, traits)
    if misclass and row is None:
        raise ValueError(f'{name}: unknown misclassification method')
    if wim:
        row = _wim_entry(name)
    if row is None:
        raise NotImplementedError(f'{name}: OOD method outside this build')
    return Row(name, base, mode, *row, traits.num_labels)


def _kernel_source(rec, sources, torch_rows):
    """The tensor ops.misclass_scores computes `rec` from ((C, N), `logits` as the recorder stores them; (N,) for `neg` / `id`), or
    None: no kernel row, a name the caller keeps on torch, a source that is not fp32 or has more classes than the kernel stages."""
    src = sources.get(rec.source)
    if rec.kind is None or rec.base.startswith(tuple(torch_rows)) or not torch.is_tensor(src) or src.dtype != torch.float32:
        return None
    if rec.source == 'logits' and src.dim() == 2:
        src = src.T
    flat = rec.kind in ('neg', 'id')
    return src if (src.dim() == 1 if flat else src.dim() == 2 and src.shape[0] <= ops.MISCLASS_MAX_CLASSES) else None


def write_rows(records, rows, logits, losses, out=None, col=0, torch_rows=(), wim_status=None):
    """The score rows `records` of one batch -> [(N,) tensor per record].  With `out` (a dense (M, n) fp32 buffer) record i is
    written into out[rows[i], col:col + N] and that view is returned.  A row with a kernel form whose source is fp32 with at most
    ops.MISCLASS_MAX_CLASSES classes goes through ops.misclass_scores, ONE launch per source tensor, unless its name starts with
    one of `torch_rows`; the WIM rows through their ONE ops.wim_scores launch (`wim_status(name, device)` gives its status word,
    or refuses); every other row is its torch expression.  Without `out` each launch fills a new buffer and the torch rows are
    returned as computed."""
    sources = dict(losses, logits=logits)
    res = [None] * len(records)

    def launch(op, idx, n, *args, **kw):
        got = op(*args, out=out, rows=None if out is None else [rows[i] for i in idx], col=col, **kw)
        for j, i in enumerate(idx):
            res[i] = got[j] if out is None else out[rows[i], col:col + n]

    by_source, wim = {}, []
    for i, rec in enumerate(records):
        if rec.kind in ops.WIM_KINDS:
            wim.append(i)
        elif _kernel_source(rec, sources, torch_rows) is not None:
            by_source.setdefault(rec.source, []).append(i)
    for idx in by_source.values():
        src = _kernel_source(records[idx[0]], sources, torch_rows)
        launch(ops.misclass_scores, idx, src.shape[-1], src[None] if src.dim() == 1 else src,
               [(records[i].kind, records[i].const) for i in idx])
    if wim:
        if wim_status is None:
            raise NotImplementedError(f'{records[wim[0]].name}: OOD method outside this build')
        y_est = losses['y_est_already']
        status = wim_status(records[wim[0]].name, y_est.device)
        keys = list(dict.fromkeys(records[i].source for i in wim))
        C, N = losses[keys[0]].shape
        if C <= ops.MISCLASS_MAX_CLASSES and y_est.is_cuda and y_est.dtype == torch.int64 and all(
                losses[k].dtype == torch.float32 and losses[k].is_cuda and losses[k].dim() == 2 for k in keys):
            at = {records[i].source for i in wim if records[i].kind.endswith('AT')}
            factor = {records[i].source: records[i].const for i in wim}
            launch(ops.wim_scores, wim, N, [(losses[k], -factor[k] if k == 'total' else factor[k],
                                             losses[k + '@'].float() if k in at else None) for k in keys], y_est,
                   [(keys.index(records[i].source), records[i].kind) for i in wim], status=status)
    for i, rec in enumerate(records):
        if res[i] is None:
            res[i] = rec.torch_row(sources)
            if out is not None:
                n = res[i].shape[0]
                out[rows[i], col:col + n] = res[i]
                res[i] = out[rows[i], col:col + n]
    return res
