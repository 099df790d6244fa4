"""`WIMJob`: the reference's fine-tuned model with two priors (ft/wim.py + the model half of ft/job.py) on the drop-in.

A WIM job keeps the class-conditional prior the model was trained with (the *original* prior) and a second, single prior (the
*alternate* one) that the fine-tuning pulls unknown samples towards.  What the reference runs the fine-tuning for is the
evaluation under BOTH priors and the scores read from it (`k~`, `softk~`, `k@`, `k~@` for k in kl, zdist, iws, elbo).  Here

  * `evaluate_on_both_priors()` costs ONE pass through features, encoder and decoder (`WIM_SHARED_PASS`): only the
    prior-dependent tail (KL, distances, log p(z|y), importance weights, total) runs once per prior - the reference runs the
    whole evaluation twice;
  * every WIM score row of a batch comes from ONE launch of csrc/wim.hip (`ops.wim_scores`) instead of about ten small torch
    launches per method.

  * `finetune()` is the reference's fine-tuning loop (ft/job.py:170-478) over data-set objects, and `finetune_step()` its step
    in ONE pass: `finetune_batch()` evaluates the labelled batch under the original prior and the mixture batch under the
    alternate one, two passes through the network; every BatchNorm being on its running statistics, the two batches differ
    only in the prior of their KL, so they are concatenated and `ops.latent_mixed` (csrc/latent.hip) measures each part against
    its prior in one launch (`WIM_FUSED_STEP`).  Same per-sample losses bit for bit; measured on config 2
    (tools/wim_finetune_bench.py, profiles/wim_finetune_bench.json, median of 20 steps): 4.01 ms against 6.89 ms at 64 + 64
    images, 6.52 ms against 8.01 ms at 512 + 512.  The printed losses are tallied per group on the device (`ops.group_tally`).

Data sets yield `((x, y_est), y)` items, as the reference's `EstimatedLabelsDataset` does (`EstimatedLabelsDataset` below).
`finetune(moving_size=...)` builds the reference's seeded, padded moving set (jvae_compat/ft_datasets.py) and reads its mixed
batches with one launch each (`torch_load.mixed_loader`).  The `_generalize` switch, POSCOD and job arrays
stay in the reference's `ft/` package: see DESIGN.md section 7d.
"""
import json
import logging
import os
import time
from contextlib import contextmanager

import torch

from cvae import ClassificationVariationalNetwork, _mean_over_draws
from jvae_compat.ft_datasets import MovingSet, create_moving_set, finetune_schedule
from jvae_compat.recorders import LossRecorder
from jvae_hip import ops
from module.priors import build_prior
from module.vae_layers.layers import draw_epsilon


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

    # finetune_step(): the two halves of a fine-tuning step in ONE pass over the concatenated batch with a two-prior latent
    # kernel (True, where `_fused_step_applies()`), or always the two evaluations of finetune_batch() (False).  The same
    # per-sample losses bit for bit; the gradients are the same per-sample terms summed in another order.
    WIM_FUSED_STEP = True
    last_finetune_route = None          # 'fused' / 'two_pass': what the last finetune_step() ran

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
    def _wim_status_word(self, name, device):
        """What score_rows.write_rows asks before the `~` / `@` rows of a batch (ft/wim.py:132-201; ONE `ops.wim_scores` launch
        over the sources kl, zdist, iws and total): the word that launch flags a label outside [0, C) in."""
        if not self.is_cvae:
            raise NotImplementedError('the `~` / `@` scores need the class-conditional model (type cvae)')
        if self._wim_status is None or self._wim_status.device != device:
            self._wim_status = torch.zeros(1, dtype=torch.int32, device=device)
        return self._wim_status

    def _evaluate_for_scores(self, x, batch, measures, with_mu=False, with_reco=False):
        """Scoring pass of ood_detection_rates: with estimated labels on, the loader's item is the pair (x, y_est) and the
        evaluation runs under both priors.  `with_mu`: the posterior means of that same pass come back as a fifth item;
        `with_reco`: its reconstructions as the last one."""
        if not self._with_estimated_labels:
            return super()._evaluate_for_scores(x, batch, measures, with_mu=with_mu, with_reco=with_reco)
        x, y_est = x
        x = self._device_batch(x.to(self.device))
        with self.evaluate_on_both_priors():
            out = self.evaluate((x, y_est.to(self.device)), batch=batch, current_measures=measures, z_output=with_mu)
        return (x,) + tuple(out[1:4]) + ((out[4],) if with_mu else ()) + ((out[0],) if with_reco else ())

    def ood_detection_rates(self, *a, **kw):
        """The base class's method over `((x, y_est), y)` items; a label outside [0, C) met by the score kernel raises here,
        after the pass (the launches themselves do not synchronise)."""
        res = super().ood_detection_rates(*a, **kw)
        if self._wim_status is not None:
            ops.wim_check_status(self._wim_status)
        return res

    # ------------------------------------------------------------------------------------ fine-tuning step
    def finetune_batch(self, epoch, batch, x_in, y_in, x_mix, alpha=0.1, epsilon=None):
        """One WIM step's loss (ft/wim.py:215-259): the labelled batch under the original prior plus alpha x the mixture batch
        under the alternate prior, every sample of it with label 0 -> (L to back-propagate, in losses, mix losses).  Leaves the
        alternate prior in place, as the reference does.  `epsilon` (L+1, N_in + N_mix, K), optional: the noise of both halves."""
        eps_in, eps_mix = (None, None) if epsilon is None else (epsilon[:, :len(x_in)], epsilon[:, len(x_in):])
        self._evaluate_on_both_priors = False
        self.original_prior = True
        self.train()
        with self.no_estimated_labels():
            _, _, in_loss, _ = self.evaluate(x_in, y_in, batch=batch, with_beta=True, epsilon=eps_in)
        L = in_loss['total'].mean()
        self.alternate_prior = True
        y_mix = torch.zeros(len(x_mix), device=x_mix.device, dtype=torch.int64)
        self.train()
        with self.no_estimated_labels():
            _, _, mix_loss, _ = self.evaluate(x_mix, y_mix, batch=batch, with_beta=True, epsilon=eps_mix)
        L = L + alpha * mix_loss['total'].mean()
        self._evaluate_on_both_priors = True
        return L, in_loss, mix_loss

    def _fused_step_applies(self):
        """Host decision of finetune_step(): may the two halves of a step share one pass?  No sample's result may depend on
        its batch (every BatchNorm on running statistics, no active dropout, a sigma that does not follow the batch rmse), the
        prior may reach the loss through the latent kernel only (cvae, labels not coded, no classifier term), fp32 compute."""
        from module.vae_layers.layers import HipDropout
        if not (self.WIM_FUSED_STEP and self.is_cvae and not self.y_is_coded and not self.y_is_decoded):
            return False
        if getattr(self, 'compute_dtype', 'fp32') != 'fp32' or self.sigma.kind not in ('fixed', 'learned'):
            return False
        if self._alternate_prior is None or not self._original_prior.conditional:
            return False
        for m in self.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.training:
                return False
            if isinstance(m, HipDropout) and m.p and m.training:
                return False
        return True

    @contextmanager
    def _mixed_prior(self, split):
        """Inside: the encoder measures rows [split, N) of its batch against the alternate prior (the original one is in place
        for the rows before) - the seam of finetune_step() in Encoder.encode."""
        self.encoder.mixed_prior = (self._alternate_prior, int(split))
        try:
            yield
        finally:
            self.encoder.mixed_prior = None

    def finetune_step(self, epoch, batch, x_in, y_in, x_mix, alpha=0.1, epsilon=None):
        """finetune_batch() in ONE pass through the network: cat(x_in, x_mix) is evaluated once, the latent kernel measures
        the first len(x_in) rows against the original prior and the others against the alternate one (`ops.latent_mixed`), and
        the per-sample losses are sliced at the seam -> (L, in losses, mix losses), the same keys and the same state left behind
        as finetune_batch().  Without `epsilon` the noise is drawn as finetune_batch() draws it (the in part, then the mix part),
        so the two forms see the same noise under one torch seed.  Applies when `_fused_step_applies()`; else, and with
        `WIM_FUSED_STEP = False`, this IS finetune_batch().  `last_finetune_route` tells which ran: 'fused' or 'two_pass'."""
        self._evaluate_on_both_priors = False
        self.original_prior = True
        self.train()
        if not self._fused_step_applies():
            self.last_finetune_route = 'two_pass'
            return self.finetune_batch(epoch, batch, x_in, y_in, x_mix, alpha=alpha, epsilon=epsilon)
        self.last_finetune_route = 'fused'
        split, n_mix = len(x_in), len(x_mix)
        x = torch.cat((x_in, x_mix))
        y = torch.cat((y_in.reshape(-1), torch.zeros(n_mix, device=y_in.device, dtype=torch.int64)))
        if epsilon is None:
            shape = (self.encoder.sampling_size, self.latent_dim, self.encoder.sampling.distribution)
            epsilon = torch.cat([draw_epsilon(shape[0], (n, shape[1]), x.device, shape[2]) for n in (split, n_mix)], 1)
        with self.no_estimated_labels(), self._mixed_prior(split):
            _, _, losses, _ = self.evaluate(x, y, batch=batch, with_beta=True, epsilon=epsilon)
        in_loss = {k: v[..., :split] for k, v in losses.items()}
        mix_loss = {k: v[..., split:] for k, v in losses.items() if k != 'dzdist'}
        L = in_loss['total'].mean() + alpha * mix_loss['total'].mean()
        self.alternate_prior = True
        self._evaluate_on_both_priors = True
        return L, in_loss, mix_loss

    # ------------------------------------------------------------------------------------ fine-tuning loop
    TALLY_GROUPS = ('ind', 'ood', 'in')          # groups of the printed losses: moving set's two classes, then the labelled batch

    def finetune(self, trainset, ind_set, ood_sets, *, train_size=100000, epochs=None, batch_size=None, test_batch_size=8192,
                 optimizer=None, outputs=None, alpha=0.1, report_every=10, testset_name=None, on_batch=None,
                 sample_recorders=None, moving_size=None, ood_mix=0.5, padding=0., padding_sets=None, mix_padding=0., seed=0,
                 task=0):
        """The WIM fine-tuning loop (ft/job.py:170-478) over data-set objects: `trainset` yields the labelled (x, y) batches,
        `ind_set` and the sets of `ood_sets` (name -> data set) make the `MovingSet` the alternate prior pulls on.

          before   ood_detection_rates under the original prior, recorders filled per set, then `ood_results` cleared;
          epochs   ceil(train_size / len(moving set)) of them (`finetune_schedule`); per batch zero_grad, finetune_step(),
                   backward, optimizer.step() and then optimizer.clip() - the reference's order; the printed losses
                   (`printed_loss`) are tallied per group on the device (`ops.group_tally`) and read back every
                   `report_every` batches and at the last one, for outputs.results(losses={'ind_zdist', 'ood_zdist',
                   'in_zdist'});
          after    y_est = argmin over the classes of the recorded kl, per set, and ood_detection_rates under both priors.

        The scoring passes re-seed torch for their recorders; the generator states found at the call are put back before the
        first epoch, so `torch.manual_seed(s)` in front of finetune() fixes the loaders' order and the noise of the epochs.
        `on_batch(epoch, batch, in_loss, mix_loss, tags)` is called after each step with that step's loss dictionaries.
        `trained` is left as found, as in the reference.  Named data sets (names, or None for the recorded set) are opened from
        `DATA_ROOT` when it is set and raise NotImplementedError when it is None; see DESIGN.md for what
        else of the reference's loop is outside this build.

        `moving_size` given: the moving set is the reference's seeded one, `create_moving_set(ind_set, ood_sets, padding_sets,
        moving_size, ood_mix, padding, mix_padding, seed, task)` (jvae_compat/ft_datasets.py) with classes 'ood', 'ind', 'pad'
        (padding > 0) and 'padmix' (mix_padding > 0).  `padding_sets`: a dict name -> data set or name, or a list of them (names
        are opened from `DATA_ROOT`; 'uniform' / 'const' = that sibling of the model's set); empty with padding > 0 = the
        `uniform*` and `const*` siblings of the model's set, as in ft/job.py:225-231.  `ft_params`
        records moving_size - reduced to len(moving set) // (1 + padding + mix_padding) when that is smaller (ft/job.py:264-267)
        - padding, padding_sets, mix_padding and mix = the share of class 'ood'.  A sample's tally group is 'ind' for class
        'ind' and 'ood' for every other class (ft/job.py:374-375).  When every set of the moving set is resident on the device
        its batches come from `torch_load.mixed_loader`, one launch per batch, else from a DataLoader: the same batches either
        way (`tags` is then on the device).  `moving_size=None` is the plain `MovingSet` of everything, in order.

        `sample_recorders` ({set name: SampleRecorder}, see `make_sample_recorders`): the latent records of the reference's
        `--inspection` switch (ft/job.py:282-300, 451-470).  They are filled by the scoring pass before tuning and, with `saved_dir`
        set, written as `saved_dir/samples/<trained:04d>/init/samples-<set>.pth`; then reset(), filled again by the pass after
        tuning and written into `saved_dir/samples/<trained:04d>`.  Without `saved_dir` no file is written and the recorders
        hold the records of the pass after tuning.  They change nothing else: the same launches of the loop, the same parameters."""
        named = [s for s in (trainset, ind_set) if isinstance(s, str) or s is None]
        if named or not isinstance(ood_sets, dict) or any(isinstance(s, str) for s in ood_sets.values()):
            if self.DATA_ROOT is None:
                raise NotImplementedError('named torchvision datasets are outside this build: pass torch.utils.data.Datasets '
                                          '(ood_sets: a dict of name -> Dataset)')
            if trainset is None or isinstance(trainset, str):
                trainset = self._open_named(trainset, 'train')
            if ind_set is None or isinstance(ind_set, str):
                ind_set = self._open_named(ind_set)
            if not isinstance(ood_sets, dict):   # names (ft/job.py hands over a list of them)
                ood_sets = {str(getattr(s, 'name', s)): s for s in ood_sets}
            ood_sets = {n: self._open_named(s, transformer=ind_set.transformer) if isinstance(s, str) else s
                        for n, s in ood_sets.items()}
        optimizer = self.optimizer if optimizer is None else optimizer
        batch_size = int(batch_size or self.training_parameters['batch_size'])
        testset_name = testset_name or getattr(ind_set, 'name', None) or self.training_parameters.get('set') or 'ind'
        device = self.device
        if moving_size is None:
            moving_set, group_of_tag = MovingSet(ind_set, ood_sets), None
        else:
            padding_sets = self._padding_sets(padding_sets, padding, ind_set)
            moving_set = create_moving_set(ind_set, ood_sets, padding_sets, moving_size, ood_mix, padding=padding,
                                           mix_padding=mix_padding, seed=seed, task=task)
            group_of_tag = torch.tensor([0 if c == 'ind' else 1 for c in moving_set.classes], dtype=torch.int32, device=device)
        if not hasattr(self, 'ft_params'):
            self.ft_params = {}
        if moving_size is None:
            self.ft_params.update(sets=list(ood_sets), train_size=train_size, moving_size=len(moving_set), mix=moving_set.mix[1],
                                  padding=0, padding_sets=[], mix_padding=0, alpha=alpha)
        else:
            actual = int(len(moving_set) // (1 + padding + mix_padding))
            if actual < moving_size:
                logging.warning('Moving size reduced to %d (instead of %d)', actual, moving_size)
            self.ft_params.update(sets=list(ood_sets), train_size=train_size, moving_size=min(actual, int(moving_size)),
                                  mix=moving_set.mix[moving_set.classes.index('ood')], padding=padding,
                                  padding_sets=list(padding_sets), mix_padding=mix_padding, alpha=alpha)
        test_batch_size = min(self.max_batch_sizes['test'], test_batch_size)
        logging.info('Moving set of length %d, with mixture %s', len(moving_set),
                     ', '.join('{}:{:.1%}'.format(n, m) for n, m in zip(moving_set.classes, moving_set.mix)))

        def sample_dirs(*sub):
            saved = getattr(self, 'saved_dir', None)
            if not sample_recorders or not saved:
                return []
            return [os.path.join(saved, 'samples', '{:04d}'.format(self.trained), *sub)]

        # ---- before tuning: the original prior's rates, and the recorders the estimated labels are read from
        rng = (torch.get_rng_state(), torch.cuda.get_rng_state(device) if device.type == 'cuda' else None)
        self.eval()
        self.original_prior = True
        self._evaluate_on_both_priors = False
        recorders = {n: LossRecorder(test_batch_size) for n in list(ood_sets) + [testset_name]}
        ood_ = moving_set.extract_subdataset('ood')
        with self.no_estimated_labels(), torch.no_grad():
            self.ood_detection_rates(batch_size=test_batch_size,
                                     testset=moving_set.extract_subdataset('ind', new_name=testset_name),
                                     oodsets=[ood_.extract_subdataset(n, new_name=n) for n in ood_sets],
                                     outputs=outputs, recorders=recorders, print_result='*',
                                     sample_recorders=sample_recorders, sample_dirs=sample_dirs('init'))
            self.ood_results = {}
        for r in (sample_recorders or {}).values():
            r.reset()
        torch.set_rng_state(rng[0])
        if rng[1] is not None:
            torch.cuda.set_rng_state(rng[1], device)

        # ---- the epochs
        train_loader = torch.utils.data.DataLoader(trainset, batch_size=batch_size, shuffle=True, num_workers=0)
        moving_loader = None
        if moving_size is not None:
            from jvae_compat import torch_load
            moving_loader = torch_load.mixed_loader(moving_set, batch_size, True, True)
        if moving_loader is None:
            moving_loader = torch.utils.data.DataLoader(moving_set, drop_last=True, batch_size=batch_size, shuffle=True, num_workers=0)
        self.ft_params['train_size'], schedule = finetune_schedule(train_size, len(moving_set), batch_size, epochs)
        epochs = len(schedule)
        logging.info('Epochs: %d of %s batches of size %d', epochs, schedule, batch_size)
        printed = [k for k in self.printed_loss]
        G = len(self.TALLY_GROUPS)
        sums = torch.zeros((len(printed), G), dtype=torch.float64, device=device)
        counts = torch.zeros(G, dtype=torch.int64, device=device)
        sink = outputs if outputs is not None and hasattr(outputs, 'results') else None
        for epoch, per_epoch in enumerate(schedule):
            self.eval()
            sums.zero_()
            counts.zero_()
            t0 = time.time()
            shown = {f'{g}_{k}': float('nan') for g in self.TALLY_GROUPS for k in printed}
            train_iter, moving_iter = iter(train_loader), iter(moving_loader)
            for batch in range(per_epoch):
                x_u, tags = next(moving_iter)
                try:
                    x_a, y_a = next(train_iter)[:2]
                except StopIteration:
                    train_iter = iter(train_loader)
                    x_a, y_a = next(train_iter)[:2]
                optimizer.zero_grad()
                L, in_loss, mix_loss = self.finetune_step(epoch, batch, x_a.to(device), y_a.to(device), x_u.to(device), alpha=alpha)
                L.backward()
                optimizer.step()
                optimizer.clip(self.parameters())          # after the step, as the reference has it (ft/job.py:397-399)
                # the printed losses: this batch's rows [mix | in] and their groups, one launch, nothing read back
                if group_of_tag is None:
                    group = torch.cat((tags.to(torch.int32), torch.full((len(x_a),), G - 1, dtype=torch.int32))).to(device)
                else:                                      # class -> tally group, one small lookup on the device
                    group = torch.cat((group_of_tag[tags.to(device)],
                                       torch.full((len(x_a),), G - 1, dtype=torch.int32, device=device)))
                rows = torch.stack([torch.cat((mix_loss[k].detach(), in_loss[k].detach())) for k in printed])
                ops.group_tally(rows, group, sums, counts)
                if on_batch is not None:
                    on_batch(epoch, batch, in_loss, mix_loss, tags)
                if batch % report_every == 0 or batch + 1 == per_epoch:
                    host = (sums / counts).tolist()          # the only read-back of the loop; an empty group shows nan
                    shown = {f'{g}_{k}': host[r][j] for r, k in enumerate(printed) for j, g in enumerate(self.TALLY_GROUPS)}
                if sink is not None:
                    sink.results(batch, per_epoch, epoch + 1, epochs, preambule='finetune', losses=dict(shown),
                                 batch_size=2 * batch_size, time_per_i=(time.time() - t0) / (batch + 1), end_of_epoch='\n')

        # ---- after tuning: estimated labels from the recorded kl, rates under both priors
        logging.info('Computing ood fprs')
        self.eval()
        self.original_prior = True
        self._evaluate_on_both_priors = False

        def with_estimated(dset):
            kl = recorders[dset.name]['kl']
            y_est = kl.argmin(0) if kl.dim() > 1 else torch.zeros(kl.shape[-1], dtype=torch.int64)
            return EstimatedLabelsDataset(dset, y_est[:len(dset)])

        testset = with_estimated(moving_set.extract_subdataset('ind', new_name=testset_name))
        oodsets = [with_estimated(ood_.extract_subdataset(n, new_name=n)) for n in ood_sets]
        with torch.no_grad():
            res = self.ood_detection_rates(batch_size=test_batch_size, testset=testset, oodsets=oodsets, num_batch='all',
                                           outputs=outputs, recorders={}, print_result='*',
                                           sample_recorders=sample_recorders, sample_dirs=sample_dirs())
        logging.info('misclassification_detection_rates with the `~` scores is outside this build: skipped')
        return res

    def _padding_sets(self, padding_sets, padding, ind_set):
        """The padding sets of a moving set as a dict name -> data set.  Given: a dict name -> data set or name, or a list of
        data sets and names; a name is opened from `DATA_ROOT`, and the short names 'uniform' / 'const' stand for the uniform* /
        const* sibling of the model's set; none given = ['uniform', 'const'] (ft/job.py:225-231).  No padding, no sets."""
        if not padding:
            return {}
        if not padding_sets:
            padding_sets = ['uniform', 'const']
        if not isinstance(padding_sets, dict):
            padding_sets = {str(getattr(p, 'name', p)): p for p in padding_sets}
        if not any(isinstance(p, str) for p in padding_sets.values()):
            return dict(padding_sets)
        if self.DATA_ROOT is None:
            raise NotImplementedError('named torchvision datasets are outside this build: pass padding_sets as a dict of '
                                      'name -> Dataset')
        from jvae_compat import torch_load
        set_name = self.training_parameters.get('set') or getattr(ind_set, 'name', None)
        transformer = getattr(ind_set, 'transformer', None)
        opened = {}
        for name, p in padding_sets.items():
            if p in ('uniform', 'const'):
                found = [n for n in (torch_load.get_same_size_by_name(set_name) if set_name else []) if n.startswith(p)]
                if not found:
                    raise ValueError('no {}* sibling of {} to pad the moving set with'.format(p, set_name))
                name = p = found[0]
            opened[name] = self._open_named(p, transformer=transformer) if isinstance(p, str) else p
        return opened

    def make_sample_recorders(self, names, batch_size):
        """The sample recorders of the reference's `--inspection` switch (ft/__main__.py:208-221), one per name: `mu` and `y`,
        plus `y_nearest` for a cvae, `batch_size` slots to begin with, with the auxiliary tensors `centroids` (the original
        prior's means) and `alternate` (the first mean of the alternate prior)."""
        from jvae_compat.recorders import SampleRecorder
        fakes = dict(mu=torch.zeros(batch_size, self.latent_dim, device=self.device),
                     y=torch.zeros(batch_size, dtype=torch.int64, device=self.device))
        if self.is_cvae:
            fakes['y_nearest'] = fakes['y']
        if self._alternate_prior is None:
            raise AttributeError('this model has no alternate prior yet (set_alternate_prior)')
        out = {}
        for n in names:
            out[n] = r = SampleRecorder(batch_size, **fakes)
            r.add_auxiliary(centroids=self._original_prior.mean.detach().clone(),
                            alternate=self._alternate_prior.mean[0].detach().clone())
        return out

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
