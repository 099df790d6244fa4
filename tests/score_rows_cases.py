"""The score rows as they were before module/score_rows.py existed, frozen: the `if` chain of batch_dist_measures and the torch
expressions of the WIM rows, copied verbatim as plain functions of (name, logits, losses, traits), and (tests/golden/score_rows/
table.json) the (source, kind, const) and roc_mode every name mapped to, written once by the helpers those functions replaced.
tests/test_score_rows.py and tests/test_19_score_rows_gpu.py hold the catalogue to both.  A helper module, not a conftest."""
import json
import math
import os

import torch

from oracle.cases import get_case
from test_ood_rows_restatement import make_source

TABLE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'score_rows', 'table.json')
MODEL_CASES = {'cvae': 'c1_n16_mlp', 'vae': 'ea2_n8_vae_L3', 'jvae': 'j2_n8_jvae', 'xvae': 'x2_n8_xvae', 'vib': 'b2_n8_vib'}
CLASS_AXIS = ('sum', 'mean', 'std', 'nstd', 'mag', 'IYx')
WIM_FACTORS = {'kl': -1., 'zdist': -0.5, 'iws': 1., 'elbo': 1.}
WIM_NAMES = [n for k in WIM_FACTORS for n in (k + '~', 'soft' + k + '~', k + '@', k + '~@')]
MALFORMED = {'iws-a-0-1': ValueError, 'iws-a-1': ValueError, 'softmax': NotImplementedError, 'mse~': NotImplementedError,
             'fisher_rao': NotImplementedError}
_table = []


def build_model(type_):
    from cvae import ClassificationVariationalNetwork as Net
    kw = dict(get_case(MODEL_CASES[type_])['net'])
    return Net(**(dict(kw, gamma=0.) if type_ == 'cvae' else kw))


def all_names():
    """Every entry of the OOD and misclassification tables of the five types, starred names expanded through `methods_params`
    (its ODIN grid is the class's), then the names only tests reach; each as it is listed and, without the suffix it may carry,
    plain, with '-2s' and with '-a-4-1'."""
    from cvae import ClassificationVariationalNetwork as Net
    names = []
    for per_type in (Net.ood_methods_per_type, Net.misclass_methods_per_type):
        for type_ in MODEL_CASES:
            for m in per_type[type_]:
                names += Net.methods_params.get(m[:-1], []) if m.endswith('*') else [m]
    names += ['softiws-5', 'softzdist-1', 'softzdist-100', *CLASS_AXIS, *WIM_NAMES]
    bases = [m[:-3] if m.endswith('-2s') else m.split('-a-')[0] for m in names]
    return list(dict.fromkeys(names + [b + s for b in bases for s in ('', '-2s', '-a-4-1')]))


def table():
    """{name: {model type: [source, kind, const, roc_mode] or {'raises': exception name}}}; a quantile roc_mode is a list."""
    if not _table:
        with open(TABLE_FILE) as f:
            _table.append({name: {t: row for types, row in groups for t in types} for name, groups in json.load(f).items()})
    return _table[0]


def inputs(C, N, spread, seed, names, per_class=True):
    """(logits (N, C), losses): every class-axis source a (C, N) `make_source` (a NaN column, a tied column), `total` +0. in every
    class of sample 5 (its `elbo` is -0.), the single-prior losses (N,), the `odin-*` rows of `names` (N,), labels in [0, C).
    Without `per_class`: the class-axis sources as (N,) rows, what a model without per-class losses computes."""
    g = torch.Generator().manual_seed(100 + seed)
    losses = {k: make_source(C, N, spread, seed + i) for i, k in enumerate(('total', 'iws', 'kl', 'zdist'))}
    losses['total'][:, 5] = 0.
    for k in ('cross_x', 'wmse', 'total@', 'iws@', 'kl@', 'zdist@'):
        losses[k] = spread * torch.randn(N, generator=g)
    losses.update({m: torch.randn(N, generator=g) for m in names if m.startswith('odin')})
    losses['y_est_already'] = torch.randint(0, C, (N,), generator=g)
    if not per_class:
        losses = {k: v[0].contiguous() if v.dim() == 2 else v for k, v in losses.items()}
    return spread * torch.randn(N, C, generator=g), losses


def frozen_base(name):
    """_base_method as it stood."""
    m = name[:-3] if name.endswith('-2s') else name
    return m.split('-')[0] if '-a-' in m else m


def frozen_plain(name, logits, losses, traits):
    """ClassificationVariationalNetwork.batch_dist_measures without `out`, one name, as it stood."""
    C = traits.num_labels
    m = frozen_base(name)
    per_class = traits.losses_might_be_computed_for_each_class
    if m.startswith('odin'):
        v = losses[m]
    elif m in ('elbo', 'max'):
        v = (-losses['total']).max(0)[0] if (per_class or m == 'max') else -losses['total']
    elif m == 'iws' and not per_class:
        v = losses['iws']
    elif m == 'iws':
        top = losses['iws'].max(0)[0]
        v = (losses['iws'] - top).exp().sum(0).log() + top
        if not traits.is_jvae:
            v = v + math.log(C)
    elif m == 'softiws':
        v = losses['iws'].softmax(0).max(0)[0]
    elif m.startswith('softiws-'):
        v = (-losses['iws'] / float(m[8:])).softmax(0).max(0)[0]
    elif m in ('soft', 'softkl'):
        v = (-losses['kl']).softmax(0).max(0)[0]
    elif m.startswith('softkl-'):
        v = (-losses['kl'] / float(m[7:])).softmax(0).max(0)[0]
    elif m in ('zdist', 'kl'):
        v = (-losses[m]).max(0)[0] if not traits.is_vae else -losses[m]
    elif m.startswith('soft') and '-' in m:
        v = (-losses[m.split('-')[0][4:]] / float(m.split('-')[-1])).softmax(0).max(0)[0]
    elif m == 'mse':
        v = -losses['cross_x']
    elif m == 'wmse':
        v = -losses['wmse']
    elif m == 'logits':
        v = logits.max(-1)[0]
    elif m.startswith('baseline'):
        T = float(m.split('-')[-1]) if '-' in m else 1.
        v = (logits / T).softmax(-1).max(-1)[0]
    elif m == 'hyz':
        p_y_z = logits.softmax(-1)
        v = (p_y_z * p_y_z.log()).sum(-1)
    elif m in CLASS_AXIS:
        logp = -losses['total']
        top = logp.max(0)[0]
        d = logp - top
        if m == 'sum':
            v = d.exp().sum(0).log() + top
        elif m == 'mean':
            v = d.exp().mean(0).log() + top
        elif m == 'std':
            v = logp.std(0)
        elif m == 'nstd':
            v = (d.exp().std(0).log() - d.exp().mean(0).log()).exp().pow(2)
        elif m == 'mag':
            v = top - logp.median(0)[0]
        else:
            d_x = d.exp().mean(0).log()
            v = (d * d.exp()).sum(0) / (C * d_x.exp()) - d_x
    else:
        raise NotImplementedError(f'{name}: OOD method outside this build')
    return v


def frozen_wim_row(m):
    """WIMJob._wim_row as it stood: name -> (family, kind of ops.wim_scores)."""
    if m.endswith('~@'):
        k, kind = m[:-2], 'Y_AT'
    elif m.endswith('@'):
        k, kind = m[:-1], 'LSE_AT'
    elif m.startswith('soft'):
        k, kind = m[4:-1], 'SOFT_Y'
    else:
        k, kind = m[:-1], 'Y'
    if k not in WIM_FACTORS:
        raise NotImplementedError(f'{m}: WIM score outside this build')
    return k, kind


def frozen_wim(name, losses):
    """WIMJob._wim_rows_torch as it stood, one name."""
    k, kind = frozen_wim_row(name)
    y = losses['y_est_already'].unsqueeze(0)
    f = WIM_FACTORS[k]
    v = -losses['total'] if k == 'elbo' else losses[k]
    if kind in ('LSE_AT', 'Y_AT'):
        alt = -losses['total@'] if k == 'elbo' else losses[k + '@']
    if kind == 'Y':
        r = f * v.gather(0, y).squeeze(0)
    elif kind == 'SOFT_Y':
        r = (v * f).softmax(0).gather(0, y).squeeze(0)
    elif kind == 'LSE_AT':
        r = (v * f).logsumexp(0) - f * alt
    else:
        r = f * v.gather(0, y).squeeze(0) - f * alt
    return r


def frozen_row(name, logits, losses, traits):
    """The plain batch_dist_measures call of a WIMJob, one name: names ending in `~` / `@` are WIM rows, the others the chain's."""
    return frozen_wim(name, losses) if name[-1] in '~@' else frozen_plain(name, logits, losses, traits)
