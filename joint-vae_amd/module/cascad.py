"""Chained models: model k + 1 evaluates the first sampled reconstruction of model k (reference: module/cascad.py).

The public names of the reference's module - CascadModels, iterate_with_prior - under its import path, with the same arguments
and the same returned tuples and dictionaries.  Underneath, csrc/cascad.hip: the M (M + 1) / 2 stage-pair mean squared errors
of a batch come from ONE pass over the stages (ops.cascade_mse: every stage element loaded once; the reference makes an
(L, N, D) temporary and two full reads per pair), `iterate_with_prior` is one launch (ops.iterate_prior).  The latent mutual
information of every pair of models is one ops.class_posterior launch per stage, for all temperatures, and
ops.latent_mutual_info per pair (csrc/aggregate.hip).  There is no CPU path: CPU tensors raise jvae_hip.JvaeHipError.

Kept from the reference: the order of the `mse` rows, `for i in 1..M: for j in 0..i-1` with the input image as stage 0, and of
the `Im-T` rows, `for i: for j < i`; the key 'Im-{}'.format(T); `predict_methods == ['iter']` and 'iter' returning
`logits[-1].max(0)` (values and classes, logits (M, C, N) as the recorder keeps them); the files of save() / load():
params.json {index: the model's saved_dir}, test.json, ood.json.

Deliberate differences:
  * CascadModels is an nn.Module that HOLDS the models as children '0' .. 'M-1' (parameters(), to(), eval() and train() work)
    and exposes input_shape, input_dim, num_labels, training_parameters and latent_sampling of the last one.  The reference
    copies the last model through save() / load(), swaps the copy's class, and its eval() raises, so that each model has to be
    put into eval mode itself.
  * Models whose input_shape, latent_sampling or num_labels differ are refused by name at construction (the reference's
    torch.stack fails on them during evaluate()), and so are models with coded labels (their label-free evaluate() does not
    exist, in the reference either), a categorical output distribution (its reconstruction is a (256, ...) level tensor, not
    an image the next stage could read) and models without a decoder (type 'vib').
  * evaluate(x, y) with y other than None raises NotImplementedError.  The reference itself fails there: it tests `if y` on a
    tensor, which is ambiguous for more than one label.
  * evaluate() takes `epsilon`, an optional list of one (L + 1, N, K_i) reparameterisation noise per stage (the test hook
    module.aggregation.latent_mutual_info has).
  * With z_output=True every prior has to be a conditional Gaussian; the tilted and uniform priors raise NotImplementedError by
    name, as in module.aggregation.  Temperatures have to be proper ones (none of NAN_TEMPS).
  * A cascade of ONE model returns an empty (0, N) tensor per `Im-T` (the reference's torch.stack of no rows raises).
  * predict_after_evaluate() with another method than 'iter' goes to the last model with the last stage's logits (back in the
    model's own (N, C) layout) and the last stage's row of every per-model loss; the reference raises a NameError there.
  * load() takes `model_class` (default: cvae.ClassificationVariationalNetwork), whose load() rebuilds each model.
  * record_sets() is the loop of the reference's `__main__` block over a dictionary {name: dataset object}; named datasets, the
    model registry, rsync file lists and argparse stay in the reference.
  * At most 8 models; at most 128 classes for iterate_with_prior and the mutual information (the kernels' limits).
"""
import json
import os

import torch
from torch import nn

from jvae_hip import ops
from module import aggregation


def _save_json(d, dir_name, name):
    os.makedirs(dir_name, exist_ok=True)
    with open(os.path.join(dir_name, name), 'w') as f:
        json.dump(d, f)


def _load_json(dir_name, name, int_keys=False):
    """utils/save_load/misc.py::load_json; int_keys: its presumed_type=int, applied to the keys of every level."""
    with open(os.path.join(dir_name, name)) as f:
        d = json.load(f)

    def keys(o):
        if not isinstance(o, dict):
            return o
        return {(int(k) if k.lstrip('-').isdigit() else k): keys(v) for k, v in o.items()}
    return keys(d) if int_keys else d


def _refuse(models):
    if not 1 <= len(models) <= ops.CASCADE_MAX_MODELS:
        raise ValueError('a cascade holds 1 .. {} models, got {}'.format(ops.CASCADE_MAX_MODELS, len(models)))
    for i, m in enumerate(models):
        if getattr(m, 'is_vib', False) or not getattr(m, 'x_is_generated', True):
            raise ValueError('model {} has no decoder: the next stage would have nothing to read'.format(i))
        if getattr(m, 'y_is_coded', False):
            raise NotImplementedError('model {} has coded labels: its evaluation without labels does not exist'.format(i))
        if getattr(m, 'output_distribution', 'gaussian') == 'categorical':
            raise NotImplementedError('model {} has a categorical output distribution: its reconstruction is not an image '
                                      'the next stage could read'.format(i))
        for attr in ('input_shape', 'latent_sampling', 'num_labels'):
            mine, first = getattr(m, attr), getattr(models[0], attr)
            if (tuple(mine) != tuple(first)) if attr == 'input_shape' else (mine != first):
                raise ValueError('the models of a cascade share their {}: model {} has {}, model 0 {}'.format(attr, i, mine, first))


class CascadModels(nn.Module):

    def __init__(self, *models):
        super().__init__()
        _refuse(models)
        for i, m in enumerate(models):
            self.add_module(str(i), m)
        self._models = tuple(models)
        self.predict_methods = ['iter']
        self.ood_results = {}
        self.testing = {}
        self.saved_dir = None

    def __len__(self):
        return len(self._models)

    input_shape = property(lambda self: self._models[-1].input_shape)
    input_dim = property(lambda self: self._models[-1].input_dim)
    num_labels = property(lambda self: self._models[-1].num_labels)
    latent_sampling = property(lambda self: self._models[-1].latent_sampling)
    training_parameters = property(lambda self: self._models[-1].training_parameters)

    # ---- files -------------------------------------------------------------------------------------
    def save(self, job_dir='cascad-jobs', dir_name=None):
        if dir_name is None:
            trainset = self.training_parameters['set']
            dir_name = os.path.join(job_dir, str(trainset), '-'.join(str(m.job_number) for m in self._models))
        architecture = {i: getattr(m, 'saved_dir', None) for i, m in enumerate(self._models)}
        _save_json(architecture, dir_name, 'params.json')
        _save_json(self.testing, dir_name, 'test.json')
        _save_json(self.ood_results, dir_name, 'ood.json')
        self.saved_dir = dir_name
        return dir_name

    @classmethod
    def load(cls, dir_name, *a, model_class=None, **kw):
        if model_class is None:
            from cvae import ClassificationVariationalNetwork as model_class
        architecture = _load_json(dir_name, 'params.json')
        m = cls(*[model_class.load(architecture[str(i)], *a, **kw) for i in range(len(architecture))])
        for attr, name in (('testing', 'test.json'), ('ood_results', 'ood.json')):
            try:
                setattr(m, attr, _load_json(dir_name, name, int_keys=True))
            except FileNotFoundError:
                pass
        m.saved_dir = dir_name
        return m

    # ---- evaluation ----------------------------------------------------------------------------------
    def evaluate(self, x, y=None, z_output=False, temps=[1, 2, 5, 10], epsilon=None, **kw):
        """-> (x_ (M, L + 1, N, ...), y_ (M, N, C), losses, measures): model k + 1 evaluates x_reco[1] of model k, read in place.
        losses[k] is the stack of the models' own (C, N) or (N,) losses, losses['mse'] (M (M + 1) / 2, N) the mean squared
        error between every pair of stages over the L draws (stage 0: x), and with z_output=True losses['Im-T']
        (M (M - 1) / 2, N) the latent mutual information of every pair of models at every temperature; measures[k] (M,).
        epsilon: a list of one (L + 1, N, K_i) noise per stage.  y other than None raises NotImplementedError (the
        reference's own code fails there: `if y` on a tensor of labels is ambiguous)."""
        if y is not None:
            raise NotImplementedError('a cascade is evaluated without labels (the reference fails on `if y` with a tensor)')
        temps = list(temps)
        if z_output and any(aggregation._is_nan_temp(t) for t in temps):
            raise ValueError('the latent mutual information needs proper temperatures, got {}'.format(temps))
        if epsilon is not None and len(epsilon) != len(self):
            raise ValueError('one noise per stage expected: {} for {} models'.format(len(epsilon), len(self)))
        if z_output:                               # before any stage runs
            for i, m in enumerate(self._models):
                prior = m.encoder.prior
                kind = getattr(prior, 'distribution', type(prior).__name__)
                if kind != 'gaussian' or not prior.conditional:
                    raise NotImplementedError('the latent mutual information is built for conditional gaussian priors, model {} '
                                              'has a {}{} prior'.format(i, '' if prior.conditional else 'non-conditional ', kind))
        outs, pyz, x_in = [], [], x
        for i, m in enumerate(self._models):
            out = m.evaluate(x_in, None, z_output=z_output, epsilon=None if epsilon is None else epsilon[i], **kw)
            outs.append(out)
            x_in = out[0][1]                       # a view: nothing is copied between two stages
            if z_output:
                z = out[-1][1:]
                _, P = aggregation.class_posteriors(m.encoder.prior, z.reshape(z.shape[0], -1, z.shape[-1]), temps, logp=False)
                pyz.append(P)
        first = outs[0][0]
        x0 = x if x.dim() == first.dim() - 1 else x.reshape(first.shape[1:])
        losses = {k: torch.stack([o[2][k] for o in outs]) for k in outs[0][2]}
        measures = {k: torch.tensor([o[3][k] for o in outs]) for k in outs[0][3]}
        losses['mse'] = ops.cascade_mse(x0, [o[0][1:] for o in outs])
        if z_output:
            rows = [ops.latent_mutual_info(pyz[i], pyz[j]) for i in range(len(self)) for j in range(i)]      # (nT, N) each
            for t, T in enumerate(temps):
                losses['Im-{}'.format(T)] = torch.stack([r[t] for r in rows]) if rows else first.new_empty((0, x0.shape[0]))
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), losses, measures

    def predict_after_evaluate(self, logits, losses, method='iter'):
        if method == 'iter':
            return logits[-1].max(dim=0)
        M = len(self)
        per_model = {k: v[-1] for k, v in losses.items() if k != 'mse' and not k.startswith('Im-') and len(v) == M}
        return self._models[-1].predict_after_evaluate(logits[-1].transpose(0, 1), per_model, method=method)


def iterate_with_prior(logp_x_y):
    """p (M, C, N) - M the number of models, C of labels, N of samples - -> the posteriors (M, C, N) of a sequential Bayesian
    update: prior_0 = 1 / C, posterior[i] = p[i] prior / sum_c p[i] prior, prior = posterior[i]."""
    return ops.iterate_prior(logp_x_y)


def record_sets(model, sets, batch_size=32, num_batch=int(1e6), temps=[1], saved_samples_per_batch=2, job_dir='cascad-jobs'):
    """The loop of the reference's command-line block over sets = {name: dataset object of (x, y) items}: per set every batch is
    evaluated under no_grad with z_output=True, its losses, `y_true` and `logits` = y_.permute(0, 2, 1) go to a LossRecorder,
    and the first `saved_samples_per_batch` images of every batch with their two first reconstruction rows are kept.  Written
    into model.saved_dir (model.save(job_dir=job_dir)): record-<set>.pth and sample-<set>.pth, a dictionary {'x': (n, ...),
    'x_': (M, 2, n, ...), 'y': (n,)} on the CPU.  -> model.saved_dir"""
    from jvae_compat.recorders import LossRecorder
    device = next(model.parameters()).device
    for name, dset in sets.items():
        loader = torch.utils.data.DataLoader(dset, batch_size=batch_size, shuffle=False)
        recorder = LossRecorder(batch_size)
        samples = {'x': [], 'x_': [], 'y': []}
        for i, (x, y) in enumerate(loader):
            if i >= num_batch:
                break
            x, y = x.to(device), y.to(device)
            with torch.no_grad():
                x_, y_, losses, _ = model.evaluate(x, z_output=True, temps=temps)
            losses.update(y_true=y, logits=y_.permute(0, 2, 1))
            recorder.append_batch(**losses)
            n = saved_samples_per_batch
            samples['x'].append(x[:n].to('cpu'))
            samples['x_'].append(x_[:, :2, :n].to('cpu'))
            samples['y'].append(y[:n].to('cpu'))
        for k, dim in (('x', 0), ('x_', 2), ('y', 0)):
            samples[k] = torch.cat(samples[k], dim=dim)
        model.save(job_dir=job_dir)
        recorder.save(os.path.join(model.saved_dir, 'record-{}.pth'.format(name)))
        torch.save(samples, os.path.join(model.saved_dir, 'sample-{}.pth'.format(name)))
    return model.saved_dir
