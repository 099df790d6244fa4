"""`WIMJob`: the reference's fine-tuned model with two priors (ft/wim.py + the model half of ft/job.py) on the drop-in.

A WIM job keeps the class-conditional prior the model was trained with (the *original* prior) and a second, single prior (the
*alternate* one) that the fine-tuning pulls unknown samples towards.  What the reference runs the fine-tuning for is the
evaluation under BOTH priors and the scores read from it (`k~`, `softk~`, `k@`, `k~@` for k in kl, zdist, iws, elbo).  Here

  * `evaluate_on_both_priors()` costs ONE pass through features, encoder and decoder (`WIM_SHARED_PASS`): only the
    prior-dependent tail (KL, distances, log p(z|y), importance weights, total) runs once per prior - the reference runs the
    whole evaluation twice;
  * every WIM score row of a batch comes from ONE launch of csrc/wim.hip (`ops.wim_scores`) instead of about ten small torch
    launches per method.

Data sets yield `((x, y_est), y)` items, as the reference's `EstimatedLabelsDataset` does (`EstimatedLabelsDataset` below).
The `finetune()` loop itself (mixture / moving sets of named data sets), POSCOD and job arrays stay in the reference's `ft/`
package: see DESIGN.md.
"""
import json
import logging
import os
from contextlib import contextmanager

import torch

from cvae import ClassificationVariationalNetwork, _mean_over_draws
from jvae_hip import ops
from module.priors import build_prior


class EstimatedLabelsDataset(torch.utils.data.Dataset):
    """`dataset` with an estimated label per item: item i is ((x_i, y_est_i), y_i)."""

    def __init__(self, dataset, y_est):
        if len(y_est) != len(dataset):
            raise ValueError(f'{len(y_est)} estimated labels for {len(dataset)} items')
        self.dataset = dataset
        self.y_est = torch.as_tensor(y_est, dtype=torch.int64).cpu()
        self.name = getattr(dataset, 'name', 'set')

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, i):
        x, y = self.dataset[i][:2]
        return (x, self.y_est[i]), y


class WIMJob(ClassificationVariationalNetwork):

    predict_methods_per_type = {'vae': [], 'cvae': ['already'], 'vib': ['already']}
    added_loss_components_per_type = {'cvae': ('y_est_already',), 'vae': (), 'vib': ('y_est_already',)}
    ood_methods_per_type = {'vae': ['zdist', 'elbo', 'kl'],
                            'cvae': ['zdist', 'zdist~', 'zdist@', 'zdist~@', 'elbo', 'elbo~', 'elbo@', 'elbo~@']}
    misclass_methods_per_type = {'cvae': ['softzdist~', 'zdist~'], 'vae': []}
    printed_loss = ('zdist',)
    ft_param_file = 'wim.json'
    # keys of wim.json that describe the fine-tuning run, not the alternate prior (ft/wim.py:208-213)
    FT_RUN_KEYS = ('sets', 'alpha', 'train_size', 'moving_size', 'padding', 'mix_padding', 'padding_sets', 'from', 'mix', 'hash',
                   'array_size')

    # evaluate_on_both_priors(): one pass through features / encoder / decoder and the prior-dependent tail once per prior
    # (True), or two full evaluations as the reference runs them (False).  Same bits for every loss with the same epsilon.
    WIM_SHARED_PASS = True

    # the factor of each score family on its loss (ft/wim.py:145); `elbo` is -total
    WIM_FACTORS = {'kl': -1., 'zdist': -0.5, 'iws': 1., 'elbo': 1.}

    def __init__(self, *a, alternate_prior=None, **kw):
        super().__init__(*a, **kw)
        self.update_loss_components()
        self._original_num_labels = self.num_labels
        self._with_estimated_labels = self.is_cvae or self.is_vib
        self.ood_methods = list(self.ood_methods_per_type[self.type])
        self._original_prior = self.encoder.prior
        for p in self._original_prior.parameters():
            p.requires_grad_(False)
        self._alternate_prior = None
        if alternate_prior is not None:
            self.set_alternate_prior(**alternate_prior)
        self._is_alternate_prior = False
        self._evaluate_on_both_priors = False
        self._wim_status = None

    def update_loss_components(self):
        self.loss_components += tuple(k + '@' for k in self.loss_components)
        self.loss_components += self.added_loss_components_per_type.get(self.type, ())

    # ------------------------------------------------------------------------------------ the two priors
    @classmethod
    def is_wim(cls, d):
        return os.path.exists(os.path.join(d, cls.ft_param_file))

    is_one = is_wim

    @property
    def is_alternate_prior(self):
        return self._is_alternate_prior

    @property
    def is_original_prior(self):
        return not self._is_alternate_prior

    def _switch_to_alternate_prior(self, b):
        if b:
            if self._alternate_prior is None:
                raise AttributeError('this model has no alternate prior yet (set_alternate_prior)')
            self.encoder.prior, self.num_labels = self._alternate_prior, 1
        else:
            self.encoder.prior, self.num_labels = self._original_prior, self._original_num_labels
        self._is_alternate_prior = bool(b)
        logging.debug('Switched to %s prior: %s', 'alternate' if b else 'original', self.encoder.prior)
        return self.encoder.prior

    @contextmanager
    def _prior_span(self, alternate):
        back = self._is_alternate_prior
        try:
            yield self._switch_to_alternate_prior(alternate)
        finally:
            self._switch_to_alternate_prior(back)

    @property
    def original_prior(self):
        """`with job.original_prior as prior:` evaluates under the original prior and restores the one in place before;
        `job.original_prior = True / False` switches for good."""
        return self._prior_span(False)

    @original_prior.setter
    def original_prior(self, b):
        self._switch_to_alternate_prior(not b)

    @property
    def alternate_prior(self):
        return self._prior_span(True)

    @alternate_prior.setter
    def alternate_prior(self, b):
        self._switch_to_alternate_prior(b)

    def set_alternate_prior(self, **p):
        """Build the alternate prior from the keywords of `build_prior` (dim, num_priors, distribution, ...); it is frozen."""
        assert self._alternate_prior is None, 'the alternate prior is already set'
        self._alternate_prior = build_prior(**p).to(self.device)
        if not hasattr(self, 'ft_params'):
            self.ft_params = dict(p)
        for q in self._alternate_prior.parameters():
            q.requires_grad_(False)

    @contextmanager
    def evaluate_on_both_priors(self):
        state = self._evaluate_on_both_priors
        self._evaluate_on_both_priors = True
        try:
            yield
        finally:
            self._evaluate_on_both_priors = state

    @contextmanager
    def no_estimated_labels(self):
        """evaluate(x) takes a plain x again and `ood_methods` keeps the names that need neither y_est nor the alternate prior."""
        state = self._with_estimated_labels
        try:
            self.ood_methods = [m for m in self.ood_methods_per_type[self.type] if m[-1] not in '@~']
            self._with_estimated_labels = False
            yield
        finally:
            self.ood_methods = list(self.ood_methods_per_type[self.type])
            self._with_estimated_labels = state

    # ------------------------------------------------------------------------------------ module state
    def train(self, *a, **kw):
        """Every BatchNorm stays on its running statistics while the rest trains (ft/job.py:97-111)."""
        super().train(*a, **kw)
        if self.training:
            kept = 0
            for m in self.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.eval()
                    kept += 1
            logging.debug('Kept %d bn layers in eval mode', kept)
        return self

    # ------------------------------------------------------------------------------------ evaluate
    def evaluate(self, x, *a, **kw):
        """The base class's evaluate(); with estimated labels on, `x` is the pair (x, y_est) and losses['y_est_already'] = y_est.
        Inside `evaluate_on_both_priors()`: the output under the original prior plus losses[k + '@'] for every loss k under the
        alternate prior (ft/wim.py:114-130)."""
        y_est = None
        if self._with_estimated_labels:
            x, y_est = x
        if not self._evaluate_on_both_priors:
            o = super().evaluate(x, *a, **kw)
            if y_est is not None:
                o[2]['y_est_already'] = y_est
            return o
        self._evaluate_on_both_priors = False
        try:
            o = self._evaluate_both(x, *a, **kw)
        finally:
            self._evaluate_on_both_priors = True
        if y_est is not None:
            o[2].update({'y_est_already': y_est, 'y_est_already@': y_est})
        return o

    def _evaluate_both(self, x, y=None, batch=0, current_measures=None, with_beta=False, kl_var_weighting=1., gamma_weighting=1,
                       z_output=False, epsilon=None, **kw):
        base = super()
        if not self.WIM_SHARED_PASS or y is not None or self.is_vib:
            def run():
                return base.evaluate(x, y, batch=batch, current_measures=current_measures, with_beta=with_beta,
                                     kl_var_weighting=kl_var_weighting, gamma_weighting=gamma_weighting, z_output=z_output,
                                     epsilon=epsilon, **kw)
            with self.alternate_prior:
                alternate = run()[2]
            with self.original_prior:
                o = run()
        else:
            with self._constant_weights(x):
                with self.original_prior:
                    fwd = self._all_classes_forward(x, epsilon)
                    losses, measures = self._all_classes_tail(fwd, self._original_prior, self._original_num_labels, batch,
                                                              current_measures, with_beta)
                if self._alternate_prior is None:
                    raise AttributeError('this model has no alternate prior yet (set_alternate_prior)')
                alternate, _ = self._all_classes_tail(fwd, self._alternate_prior, 1, batch, None, with_beta, with_measures=False)
            o = (fwd['x_reco'], _mean_over_draws(fwd['logits']), losses, measures)
            if z_output:
                o += (fwd['mu'], fwd['log_var'], fwd['z'])
        o[2].update({k + '@': v for k, v in alternate.items() if not k.endswith('~')})
        return o

    # ------------------------------------------------------------------------------------ scores
    @classmethod
    def _wim_row(cls, m):
        """Method name -> (family, kind of ops.wim_scores): 'zdist~' -> ('zdist', 'Y'), 'softkl~' -> ('kl', 'SOFT_Y'),
        'elbo@' -> ('elbo', 'LSE_AT'), 'iws~@' -> ('iws', 'Y_AT')."""
        if m.endswith('~@'):
            k, kind = m[:-2], 'Y_AT'
        elif m.endswith('@'):
            k, kind = m[:-1], 'LSE_AT'
        elif m.startswith('soft'):
            k, kind = m[4:-1], 'SOFT_Y'
        else:
            k, kind = m[:-1], 'Y'
        if k not in cls.WIM_FACTORS:
            raise NotImplementedError(f'{m}: WIM score outside this build')
        return k, kind

    def _wim_rows_torch(self, losses, rows_of):
        """The torch expressions of ft/wim.py:145-192 for the (family, kind) pairs of `rows_of` -> {(family, kind): (N,)}."""
        y = losses['y_est_already'].unsqueeze(0)
        out = {}
        for k, kind in rows_of:
            f = self.WIM_FACTORS[k]
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
            out[k, kind] = r
        return out

    def batch_dist_measures(self, logits, losses, methods, to_cpu=False, out=None, rows=None, col=0):
        """The base class's scores for names without a trailing `~` / `@`; the WIM names (ft/wim.py:132-201) from ONE
        `ops.wim_scores` launch over the sources kl, zdist, iws and total (f = -1 on total stands for elbo), written into
        out[row, col:col + N] when `out` is given, else into a fresh (R, N) buffer.  The torch expressions remain for more
        than ops.MISCLASS_MAX_CLASSES classes or a source that is not fp32 on the device.  `losses` is left as found."""
        methods = list(methods)
        rows = list(range(len(methods))) if rows is None else [int(r) for r in rows]
        if len(rows) != len(methods):
            raise ValueError(f'batch_dist_measures: {len(methods)} methods and {len(rows)} rows')
        wim = [(m, r) for m, r in zip(methods, rows) if m[-1] in '~@']
        plain = [(m, r) for m, r in zip(methods, rows) if m[-1] not in '~@']
        if out is not None and plain:
            res = super().batch_dist_measures(logits, losses, [m for m, _ in plain], to_cpu=to_cpu, out=out,
                                              rows=[r for _, r in plain], col=col)
        else:
            res = super().batch_dist_measures(logits, losses, [m for m, _ in plain], to_cpu=to_cpu)
        if not wim:
            return res
        if not self.is_cvae:
            raise NotImplementedError('the `~` / `@` scores need the class-conditional model (type cvae)')
        specs = [self._wim_row(m) for m, _ in wim]
        families = list(dict.fromkeys(k for k, _ in specs))
        src = {k: losses['total' if k == 'elbo' else k] for k in families}
        y_est = losses['y_est_already']
        C, N = src[families[0]].shape
        fused = C <= ops.MISCLASS_MAX_CLASSES and y_est.is_cuda and y_est.dtype == torch.int64 and all(
            v.dtype == torch.float32 and v.is_cuda and v.dim() == 2 for v in src.values())
        if fused:
            at = {k for k, kind in specs if kind.endswith('AT')}
            sources = [(src[k], -1. if k == 'elbo' else self.WIM_FACTORS[k],
                        losses[('total' if k == 'elbo' else k) + '@'].float() if k in at else None) for k in families]
            if self._wim_status is None or self._wim_status.device != y_est.device:
                self._wim_status = torch.zeros(1, dtype=torch.int32, device=y_est.device)
            buf, where = (out, [r for _, r in wim]) if out is not None else (None, None)
            buf = ops.wim_scores(sources, y_est, [(families.index(k), kind) for k, kind in specs], out=buf, rows=where, col=col,
                                 status=self._wim_status)
            where = where if out is not None else list(range(len(wim)))
            got = {m: buf[r, col:col + N] if out is not None else buf[r] for (m, _), r in zip(wim, where)}
        else:
            by_torch = self._wim_rows_torch(losses, specs)
            got = {}
            for (m, r), spec in zip(wim, specs):
                got[m] = by_torch[spec]
                if out is not None:
                    out[r, col:col + N] = got[m]
                    got[m] = out[r, col:col + N]
        res.update({m: v.cpu() if to_cpu else v for m, v in got.items()})
        return {m: res[m] for m in methods}

    def _score_row_by_torch(self, m):
        return m[-1] not in '~@' and super()._score_row_by_torch(m)

    def _evaluate_for_scores(self, x, batch, measures):
        """Scoring pass of ood_detection_rates: with estimated labels on, the loader's item is the pair (x, y_est) and the
        evaluation runs under both priors."""
        if not self._with_estimated_labels:
            return super()._evaluate_for_scores(x, batch, measures)
        x, y_est = x
        x = self._device_batch(x.to(self.device))
        with self.evaluate_on_both_priors():
            _, logits, losses, measures = self.evaluate((x, y_est.to(self.device)), batch=batch, current_measures=measures)
        return x, logits, losses, measures

    def ood_detection_rates(self, *a, **kw):
        """The base class's method over `((x, y_est), y)` items; a label outside [0, C) met by the score kernel raises here,
        after the pass (the launches themselves do not synchronise)."""
        res = super().ood_detection_rates(*a, **kw)
        if self._wim_status is not None:
            ops.wim_check_status(self._wim_status)
        return res

    # ------------------------------------------------------------------------------------ fine-tuning step
    def finetune_batch(self, epoch, batch, x_in, y_in, x_mix, alpha=0.1):
        """One WIM step's loss (ft/wim.py:215-259): the labelled batch under the original prior plus alpha x the mixture batch
        under the alternate prior, every sample of it with label 0 -> (L to back-propagate, in losses, mix losses).  Leaves the
        alternate prior in place, as the reference does."""
        self._evaluate_on_both_priors = False
        self.original_prior = True
        self.train()
        with self.no_estimated_labels():
            _, _, in_loss, _ = self.evaluate(x_in, y_in, batch=batch, with_beta=True)
        L = in_loss['total'].mean()
        self.alternate_prior = True
        y_mix = torch.zeros(len(x_mix), device=x_mix.device, dtype=torch.int64)
        self.train()
        with self.no_estimated_labels():
            _, _, mix_loss, _ = self.evaluate(x_mix, y_mix, batch=batch, with_beta=True)
        L = L + alpha * mix_loss['total'].mean()
        self._evaluate_on_both_priors = True
        return L, in_loss, mix_loss

    # ------------------------------------------------------------------------------------ persistence
    def save(self, *a, except_state=True, **kw):
        """The base class's files written under the original prior, never the optimiser, the tensors only on request, plus
        wim.json (ft/job.py:154-161)."""
        kw['except_optimizer'] = True
        with self.original_prior:
            dir_name = super().save(*a, except_state=except_state, **kw)
        with open(os.path.join(dir_name, self.ft_param_file), 'w') as f:
            json.dump(getattr(self, 'ft_params', {}), f, default=str)
        return dir_name

    @classmethod
    def transfer_from_model(cls, state):
        """A plain model's state dict gets the keys a WIM job adds: the original prior is the model's own."""
        state['_original_prior.mean'] = torch.clone(state['encoder.prior.mean'])
        state['_original_prior._var_parameter'] = torch.clone(state['encoder.prior._var_parameter'])

    def load_post_hook(self, **ft_params):
        for k in self.FT_RUN_KEYS:
            ft_params.pop(k, None)
        self.set_alternate_prior(**ft_params)

    @classmethod
    def load(cls, dir_name, build_module=True, load_state=True, **kw):
        """A WIM directory (wim.json: the alternate prior is rebuilt from it) or a plain job directory (its prior becomes the
        original prior; earlier OOD results are dropped): ft/job.py:121-152."""
        kw.pop('strict', None)
        model = super().load(dir_name, build_module=build_module, load_state=False, **kw)
        state_file = os.path.join(dir_name, 'state.pth')
        if load_state and build_module and os.path.exists(state_file):
            state = torch.load(state_file, map_location=model.device)
            if any(k.startswith('_original_prior.') and k not in state for k in model.state_dict()):
                logging.debug('%s: not a WIM state, its prior becomes the original prior', dir_name)
                cls.transfer_from_model(state)
                model.ood_results = {}
            model.load_state_dict(state, strict=False)
            opt = os.path.join(dir_name, 'optimizer.pth')
            if os.path.exists(opt):
                model.optimizer.load_state_dict(torch.load(opt, map_location=model.device))
            model.optimizer.update_scheduler_from_epoch(model.trained)
        if cls.is_wim(dir_name):
            with open(os.path.join(dir_name, cls.ft_param_file)) as f:
                model.ft_params = json.load(f)
            if build_module:
                model.load_post_hook(**model.ft_params)
        else:
            model.ood_results = {}
        return model
