"""The scoring and detection methods of the model (reference cvae.py:972-1085,1187-2079) as a mixin of
ClassificationVariationalNetwork: per-sample OOD scores, accuracy, OOD and misclassification detection rates.  What a method name
means, and the one writer of score rows, are in module/score_rows.py; the model itself (evaluate, predict_after_evaluate,
odin_scores, the tables of method names) is in cvae.py."""
import contextlib
import logging
import math
import os
import time

import numpy as np
import torch

from jvae_hip import ops
from jvae_hip import lib as _lib
from module import score_rows


class ScoringMixin:
    # Rows (by the start of their name) that ood_detection_rates leaves on the torch expressions although a kernel row exists:
    # existing ROC checks hold their thresholds to the bits of exactly these expressions, and a softmax or log-sum-exp summed in
    # another order moves a last bit (measured on the MI355X: up to 2 fp32 ulp between the kernel's softmax rows and torch's).
    SCORE_SET_TORCH_ROWS = ('iws', 'elbo', 'soft', 'baseline', 'hyz')
    MISCLASS_TORCH_ROWS = ('iws', score_rows.ODIN.prefix)     # misclassification_detection_rates: `iws`, the recorded `odin-*`
    _wim_status_word = None                   # jvae_compat.wim.WIMJob: (name, device) -> the status word of its `~` / `@` rows

    def batch_dist_measures(self, logits, losses, methods, to_cpu=False, out=None, rows=None, col=0):
        """OOD scores per sample (higher = more in-distribution) for the reference's methods (cvae.py:972-1085), the class-axis
        scores `sum`, `mean`, `std`, `nstd`, `mag`, `IYx` of the all-class total loss among them; the '-2s' / '-a-x-y' suffixes
        only name the thresholding done downstream.  -> {method: (N,) scores}.

        Plain call: the reference's torch expressions.  With `out` (a dense (M, n) fp32 device buffer), `rows` (the row of each
        method, default 0 .. len(methods) - 1) and `col` (first column): the scores are WRITTEN into out[row, col:col + N] and
        the returned tensors are those views.  Every row with a kernel form goes through `ops.misclass_scores`
        (csrc/misclass.hip), ONE launch per source tensor (`total`, `iws`, `kl`, `zdist`, `logits`, `cross_x`, `wmse`), grouped
        as misclassification_detection_rates groups them; the torch expression is kept for a source with more than
        ops.MISCLASS_MAX_CLASSES classes or that is not fp32, and for the recorded `odin-*` rows.  Against the plain call the
        pure max / negation rows (`max`, `elbo`, `kl`, `zdist`, `logits`, `mse`, `wmse`, a single-prior `iws`) and `mag` are
        bit-identical; the softmax and log-sum-exp rows agree within the fp32 error of either
        (tests/test_13_ood_phase_gpu.py).  What each name means: module/score_rows.py."""
        methods = list(methods)
        records = [score_rows.parse(m, score_rows.traits_of(self)) for m in methods]
        rows = list(range(len(methods))) if rows is None else [int(r) for r in rows]
        if len(rows) != len(methods):
            raise ValueError(f'batch_dist_measures: {len(methods)} methods and {len(rows)} rows')
        got = score_rows.write_rows(records, rows, logits, losses, out, col, torch_rows=('',) if out is None else (),
                                    wim_status=self._wim_status_word)
        return {m: v.cpu() if to_cpu else v for m, v in zip(methods, got)}

    # Named data sets ('cifar10-3', 'mnist32r', ...; jvae_compat/torch_load.py) are an opt-in: the torchvision-style directory
    # their raw files are read from.  None (the default): a name, or a set left out, raises NotImplementedError as it always did.
    DATA_ROOT = None

    def _open_named(self, name=None, split='test', transformer=None, data_augmentation=()):
        """One split of the named set (None: the recorded training set, with its recorded transformer) from `DATA_ROOT`, on the
        model's device (cvae.py:1208-1212,1473-1477)."""
        from jvae_compat import torch_load
        if transformer is None:
            transformer = self.training_parameters.get('transformer')
        if transformer is None:
            transformer = 'default'
        return torch_load.open_named(name or self.training_parameters['set'], transformer, self.DATA_ROOT, self.device, split,
                                     data_augmentation)

    def _open_named_sets(self, testset, oodsets):
        """ood_detection_rates' sets by name: the test set as in accuracy(); `oodsets=None` = the same-size siblings of the test
        set that can be opened (cvae.py:1486-1488), a name in the list = that set (FileNotFoundError when it is not there)."""
        from jvae_compat import torch_load
        if testset is None or isinstance(testset, str):
            testset = self._open_named(testset)
        if oodsets is None:
            oodsets = torch_load.open_siblings(testset, self.DATA_ROOT, self.device)
        else:
            transformer = getattr(testset, 'transformer', None)
            oodsets = [self._open_named(o, transformer=transformer) if isinstance(o, str) else o for o in oodsets]
        return testset, oodsets

    def _batch_source(self, dset, batch_size, shuffle):
        """The batches of an evaluation pass: device batches straight from a device-resident set (jvae_compat.torch_load
        .device_loader: float32, on the device, same sample order and generator use), else the DataLoader of cvae.py:1245."""
        from jvae_compat import torch_load
        batches = torch_load.device_loader(dset, batch_size, shuffle)
        if batches is not None:
            return batches
        return torch.utils.data.DataLoader(dset, batch_size=batch_size, num_workers=0, shuffle=shuffle)

    @contextlib.contextmanager
    def _recorded_pass(self, dset, name, batch_size, num_batch, shuffle, recorder, sample_dirs):
        """One pass over `dset` with a `LossRecorder` (or None), around the caller's loop: -> (recorded, recording, num_batch,
        batch_size, iterator over the batches).  recorded: the recorder holds the batches already, their number and size are its
        own and nothing is loaded (iterator None); recording: it is reset, the caller appends every batch and `record-<name>.pth`
        is written into `sample_dirs` afterwards.  The loader is made and read between init_seed_for_dataloader() and
        restore_seed(): every pass with the recorder sees the same samples in the same order."""
        recorded = recorder is not None and len(recorder) >= num_batch
        recording = recorder is not None and not recorded
        if recorded:
            num_batch, batch_size = len(recorder), recorder.batch_size
        if recording:
            recorder.reset()
            recorder.num_batch = num_batch
        if recorder is not None:
            recorder.init_seed_for_dataloader()
        try:
            yield recorded, recording, num_batch, batch_size, None if recorded else iter(self._batch_source(dset, batch_size, shuffle))
        finally:
            if recorder is not None:
                recorder.restore_seed()
        if recording:
            for d in sample_dirs:
                os.makedirs(d, exist_ok=True)
                recorder.save(os.path.join(d, 'record-{}.pth'.format(name)))

    def accuracy(self, testset=None, batch_size=100, num_batch='all', method='all', print_result=False,
                 update_self_testing=True, outputs=None, sample_dirs=[], recorder=None, epoch='last', from_where='all',
                 epoch_tolerance=0, log=True):
        """Classification accuracy of `testset` (any map-style dataset of (x, label)) per prediction method, with the
        reference's signature and bookkeeping (cvae.py:1187-1452): every batch goes through the label-free evaluation
        (all-class losses, `iws`: SURVEY.md §8f-1); with a `LossRecorder` the per-sample losses, `logits.T` and the labels are
        recorded batch by batch and written as `record-<set>.pth` into `sample_dirs` (the files test.py / results/ of the
        reference read, §8f-3) - or, if the recorder already holds the batches, the losses are RECOVERED from it instead of
        being computed.  `testset=None` (the recorded training set's test split) or a name is resolved from `DATA_ROOT` when that
        is set (jvae_compat/torch_load.py), else refused; a device-resident set is read through `device_loader`, one launch per
        batch.  The registry lookup of earlier results (`from_where`) is host-side plumbing outside this build."""
        if testset is None or isinstance(testset, str):
            if self.DATA_ROOT is None:
                raise NotImplementedError('named torchvision datasets are outside this build: pass a torch.utils.data.Dataset')
            testset = self._open_named(testset)
        name = getattr(testset, 'name', 'testset')
        only_one = isinstance(method, str) and method != 'all'
        methods = list(self.predict_methods) if method == 'all' else ([method] if only_one else list(method))
        full = int(np.ceil(len(testset) / batch_size))
        shuffle = not (num_batch == 'all' or num_batch >= full)
        num_batch = full if not shuffle else int(num_batch)
        if epoch == 'last':
            epoch = self.trained
        device = self.device
        was_training = self.training
        self.eval()
        errors = torch.zeros(len(methods), device=device)
        sums, n, measures, t0 = {}, 0, None, time.time()
        with torch.no_grad(), self._recorded_pass(testset, name, batch_size, num_batch, shuffle, recorder, sample_dirs) as (
                recorded, recording, num_batch, batch_size, loader):
            for i in range(num_batch):
                if recorded:
                    keys = [k for k in recorder.keys() if k in self.loss_components]
                    losses = recorder.get_batch(i, *keys, force_dict=True)
                    logits = recorder.get_batch(i, 'logits').T
                    y = recorder.get_batch(i, 'y_true')
                else:
                    x, y = next(loader)[:2]
                    x, y = self._device_batch(x.to(device)), y.to(device)      # raw uint8 images: ToTensor on the device
                    _, logits, losses, measures = self.evaluate(x, batch=i, current_measures=measures)
                preds = [self.predict_after_evaluate(logits, losses, method=m) for m in methods]
                if recording:
                    recorder.append_batch(**losses, y_true=y, logits=logits.T)
                if getattr(self, 'SEMI_SUPERVISED', False):
                    # a set with unlabelled samples (validation cut out of a HiddenLabels set, train_accuracy): a negative label
                    # is no class - such a row counts neither as a prediction nor as an error, it is never an index of the
                    # gather, and the losses that are per class are averaged over the labelled rows (losses without a class
                    # axis over all rows, as ever).  n = the labelled rows.
                    lab = y >= 0
                    n_lab = int(lab.sum())
                    errors += torch.stack([((p != y) & lab).sum() for p in preds]).float()
                    for k, v in losses.items():
                        if v.dim() == 2:
                            v = (v.gather(0, y.clamp_min(0).unsqueeze(0))[0].float() * lab).sum() / max(n_lab, 1)
                        else:
                            v = v.float().mean()
                        sums[k] = sums.get(k, 0.) + v
                    n += n_lab
                else:
                    errors += torch.stack([(p != y).sum() for p in preds]).float()
                    for k, v in losses.items():                     # loss of the TRUE class where a loss is per class (C, N)
                        v = v.gather(0, y.unsqueeze(0))[0] if v.dim() == 2 else v
                        sums[k] = sums.get(k, 0.) + v.float().mean()
                    n += y.numel()
                if print_result and outputs is not None and hasattr(outputs, 'results'):
                    acc_now = (1 - errors / n).tolist()
                    outputs.results(i, num_batch, 0, 0, losses={k: float(sums[k]) / (i + 1) for k in self.loss_components if k in sums},
                                    metrics={k: (measures or {}).get(k, np.nan) for k in self.metrics},
                                    accuracy=dict(zip(methods, acc_now)), time_per_i=(time.time() - t0) / (i + 1),
                                    batch_size=batch_size, preambule=print_result)
        acc = dict(zip(methods, (1 - errors / max(n, 1)).tolist()))
        self.test_losses = {k: float(v) / max(num_batch, 1) for k, v in sums.items()}
        if measures:
            self.test_measures = dict(measures)
        if update_self_testing:
            for m in methods:
                if n > self.testing.get(epoch, {}).get(m, {'n': 0})['n']:
                    self.testing.setdefault(epoch, {})[m] = {'n': n, 'epochs': epoch,
                                                             'sampling': self._latent_samplings['eval'], 'accuracy': acc[m]}
        if was_training:
            self.train()
        return acc[methods[0]] if only_one else acc

    OOD_KEPT_TPR = [pc / 100 for pc in range(90, 100)]                        # cvae.py:1736
    OOD_ROC_EVERY = 100                                                       # batches between two progress ROCs (cvae.py:1843)
    # The '-a-x-y' methods (cvae.py:1852-1854): two-sided test on every x-th / y-th sorted in-score (ops.roc_curve, mode
    # ('quantile', x, y)).  Off by default: the reference reads these thresholds off a spline whose rounding noise decides
    # its kept rates, so the numbers here are close to the reference's, not equal to them.
    OOD_QUANTILE_METHODS = False
    # The precision-recall side of the detection rates (ops.pr_metrics, csrc/prc.hip).  Off by default:
    # every dictionary and file is the reference's.  On: ood_detection_rates() adds 'aupr_in', 'aupr_out', 'aucpr_in',
    # 'aucpr_out' and 'dete' to every per-method dictionary of an OOD set (not to the '-a-x-y' methods, which have no scalar
    # score) and misclassification_detection_rates() adds 'aupr_correct', 'aupr_error', 'aucpr_correct', 'aucpr_error' and
    # 'dete' to every entry.  Whether the reference's loaders accept the extra keys in ood.json / test.json is not claimed.
    DETECTION_PR_METRICS = False
    MISCLASS_PR_KEYS = ('aupr_correct', 'aupr_error', 'aucpr_correct', 'aucpr_error', 'dete')

    # The likelihood-regret rows `regret-<steps>-<lr>` (Xiao, Yan, Amit 2020; cvae.likelihood_regret): T
    # decoder forward and input-gradient passes per batch and pair of `REGRET_PARAMS`.  Off by default: every name raises, 'all'
    # is the reference's table.  On (class or instance): 'all' and 'regret*' expand to the pairs on the types of REGRET_TYPES.
    OOD_REGRET_METHODS = False
    REGRET_TYPES = ('cvae', 'vae', 'xvae')
    REGRET_PARAMS = [(5, 0.05), (20, 0.02)]                                   # (steps, lr): a starting point nobody has tuned

    def _regret_names(self):
        """The `regret-<steps>-<lr:.4f>` method names of this instance's `REGRET_PARAMS`, in their order."""
        return ['regret-{:d}-{:.4f}'.format(int(s), float(lr)) for s, lr in self.REGRET_PARAMS]

    def regret_scores(self, x, y=None, logits=None, losses=None, epsilon=None):
        """The likelihood-regret rows of a batch for every (steps, lr) pair of `REGRET_PARAMS`: {'regret-<steps>-<lr>': (N,) fp32
        device tensor}, higher = more in-distribution (the row is MINUS the regret).  `logits`, `losses`: what a label-free
        evaluate(x) of the batch returned, if the caller has it (the class is predicted from them instead of from a pass of its
        own).  `epsilon`: {name: (steps + 1, L, N, K)} noise per row.  One `likelihood_regret` call per pair."""
        seen = None if losses is None else (logits, losses)
        out = {}
        for name, (steps, lr) in zip(self._regret_names(), self.REGRET_PARAMS):
            regret = self.likelihood_regret(x, y, steps=int(steps), lr=float(lr), evaluated=seen,
                                            epsilon=None if epsilon is None else epsilon[name])[0]
            out[name] = -regret
        return out

    # The nearest-neighbour rows `knn-<k>` (Sun, Ming, Zhu, Li 2022): minus the distance from a sample's
    # posterior mean to its k-th nearest neighbour among the means of a training set, the bank of `fit_latent_bank`.  Off by
    # default: every name raises, 'all' is the reference's table.  On (class or instance): 'all' and 'knn*' expand to `KNN_K`.
    # A set scored against a bank fitted on itself meets itself: `knn-1` is then about 0 (there is no leave-one-out).
    OOD_KNN_METHODS = False
    KNN_K = (1, 10, 50)
    KNN_NORMALIZE = True                                                      # distances between the F.normalize()d means
    latent_bank = None                                                        # {'bank' (M, K), 'sq' (M,), 'labels' (M,), 'set'}
    LATENT_BANK_FILE = 'latent-bank.pth'

    def _knn_names(self):
        """The `knn-<k>` method names of this instance's `KNN_K`, in their order."""
        return ['knn-{:d}'.format(int(k)) for k in self.KNN_K]

    @staticmethod
    def _seeded_subset(n, ratio, seed, who):
        """The seeded random subset of the fitted stores -> (keep, M): a host bool mask of n samples with round(ratio * n) (at
        least one) set, from a torch.Generator permutation, or None for ratio = 1 (all n); M: how many are kept."""
        if not 0 < ratio <= 1:
            raise ValueError(f'{who}: a ratio in (0, 1] expected, got {ratio}')
        if ratio == 1:
            return None, n
        keep = torch.zeros(n, dtype=torch.bool)
        keep[torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))[:max(1, int(round(ratio * n)))]] = True
        return keep, int(keep.sum())

    def _save_store(self, attr, file_name, dir_name, nothing):
        """Write the fitted store `attr` as `file_name` into `dir_name`, its tensors on the host -> the path."""
        store = getattr(self, attr)
        if store is None:
            raise ValueError(nothing)
        os.makedirs(dir_name, exist_ok=True)
        path = os.path.join(dir_name, file_name)
        torch.save({k: v.cpu() if torch.is_tensor(v) else v for k, v in store.items()}, path)
        return path

    def _load_store(self, attr, file_name, dir_name, check):
        """Read `file_name` of `dir_name` on the host, have `check(d)` raise for what is not this store, and set `attr` to it with
        its tensors on the model's device -> the store."""
        d = torch.load(os.path.join(dir_name, file_name), map_location='cpu')
        check(d)
        setattr(self, attr, {k: v.to(self.device).contiguous() if torch.is_tensor(v) else v for k, v in d.items()})
        return getattr(self, attr)

    def _refuse_types(self, who, types, more='', why=None):
        """NotImplementedError for a model of another type than `types` or with coded labels, or for the caller's own reason `why`."""
        if self.type not in types or self.y_is_coded:
            why = f'not type {self.type}' + (' with coded labels' if self.y_is_coded else '')
        if why:
            raise NotImplementedError(f'{who}: built for models without coded labels of the types {", ".join(types)}{more}, {why}')

    def _posterior_rows(self, dataset, batch_size, ratio, seed, who):
        """The pass of the fitted latent stores: one latent_posterior() pass over `dataset` in eval mode, each batch's mu and
        log sigma^2 written straight into preallocated (M, K) fp32 device tensors, the labels beside them -> (mu, log_var,
        labels).  ratio < 1: a seeded random subset of round(ratio * len) samples (a torch.Generator permutation on the host,
        chosen before the pass; only the kept rows are stored, in the order of the set; a batch that keeps any row is encoded
        whole).  Models with coded labels are refused, as latent_posterior(x) refuses them."""
        if self.y_is_coded:
            raise NotImplementedError(f'{who}: latent_posterior(x) without labels is not possible for models with coded '
                                      'labels (their encoder reads y)')
        keep, M = self._seeded_subset(len(dataset), ratio, seed, who)
        device = self.device
        was_training = self.training
        self.eval()
        mus, lvs, labels, seen, pos = None, None, torch.empty(M, dtype=torch.int64, device=device), 0, 0
        with torch.no_grad():
            for batch in self._batch_source(dataset, batch_size, False):
                x, y = batch[:2]
                sel = None if keep is None else keep[seen:seen + x.shape[0]]
                seen += x.shape[0]
                if sel is not None and not bool(sel.any()):
                    continue
                mu, lv = self.latent_posterior(self._device_batch(x.to(device)))
                y = y.to(device)
                if sel is not None and not bool(sel.all()):       # the whole batch is encoded: the rows are those of a full pass
                    rows = sel.nonzero()[:, 0].to(device)
                    mu, lv, y = mu[rows], lv[rows], y[rows]
                if mus is None:
                    mus, lvs = (torch.empty((M, mu.shape[1]), dtype=torch.float32, device=device) for _ in range(2))
                mus[pos:pos + mu.shape[0]] = mu
                lvs[pos:pos + mu.shape[0]] = lv
                labels[pos:pos + mu.shape[0]] = y
                pos += mu.shape[0]
        if was_training:
            self.train()
        if mus is None or pos != M:
            raise ValueError(f'{who}: the set yielded {pos} of the {M} rows expected')
        return mus, lvs, labels

    def fit_latent_bank(self, dataset, batch_size=100, ratio=1.0, seed=0):
        """Fill `latent_bank` with the posterior means of `dataset` (any map-style dataset of (x, label)): one latent_posterior()
        pass in eval mode, each batch's `mu` written straight into a preallocated (M, K) fp32 device tensor, the labels beside
        it, then the rows' norms (ops.knn_bank).  ratio < 1: a seeded random subset of round(ratio * len) samples (a
        torch.Generator permutation on the host, chosen before the pass; only the kept rows are stored, in the order of the
        set).  -> the bank's dictionary.  Models with coded labels are refused, as latent_posterior(x) refuses them."""
        mu, _, labels = self._posterior_rows(dataset, batch_size, ratio, seed, 'fit_latent_bank')
        bank, sq = ops.knn_bank(mu)
        self.latent_bank = {'bank': bank, 'sq': sq, 'labels': labels, 'set': getattr(dataset, 'name', 'set')}
        return self.latent_bank

    def save_latent_bank(self, dir_name):
        """Write the fitted bank as `latent-bank.pth` into `dir_name` (a file of its own: save() / load() do not know it)."""
        return self._save_store('latent_bank', self.LATENT_BANK_FILE, dir_name, 'save_latent_bank: no bank is fitted (fit_latent_bank)')

    def load_latent_bank(self, dir_name):
        """Read `latent-bank.pth` of `dir_name` onto the model's device -> the bank's dictionary, bit for bit what was saved."""
        def check(d):
            if set(d) != {'bank', 'sq', 'labels', 'set'} or d['bank'].dtype != torch.float32 or d['bank'].dim() != 2 \
                    or tuple(d['sq'].shape) != (d['bank'].shape[0],) or tuple(d['labels'].shape) != (d['bank'].shape[0],):
                raise ValueError(f'load_latent_bank: {dir_name} does not hold a latent bank')
        return self._load_store('latent_bank', self.LATENT_BANK_FILE, dir_name, check)

    def knn_scores(self, mu):
        """The nearest-neighbour rows of a batch of posterior means mu (N, K) for every k of `KNN_K`: {'knn-<k>': (N,) fp32 device
        tensor} = -sqrt(d2 to the k-th nearest row of the bank), higher = more in-distribution.  ONE `ops.knn` call with
        k = max(KNN_K); `KNN_NORMALIZE`: distances between the normalised rows.  ValueError without a bank, or with a bank of
        fewer rows than max(KNN_K).  A non-finite row sets the device's `ops.knn_status` word (`ops.knn_check_status`)."""
        ks = [int(k) for k in self.KNN_K]
        if self.latent_bank is None:
            raise ValueError('knn_scores: no latent bank is fitted (fit_latent_bank or load_latent_bank)')
        bank = self.latent_bank
        if not ks or min(ks) < 1 or bank['bank'].shape[0] < max(ks):
            raise ValueError(f"knn_scores: the bank holds {bank['bank'].shape[0]} rows, KNN_K = {tuple(ks)} needs 1 <= k <= rows")
        d2, _ = ops.knn(mu.float(), bank['bank'], bank['sq'], max(ks), normalized=bool(self.KNN_NORMALIZE))
        return {name: -d2[:, k - 1].sqrt() for name, k in zip(self._knn_names(), ks)}

    # The aggregate posterior q(z) = 1/N sum_n q(z | x_n) of a set and the decomposition of the KL term it gives (Hoffman & Johnson
    # 2016; Chen et al. 2018): the bank of `fit_posterior_bank` holds the posteriors (mu, log sigma^2) of a
    # training set, `aggregate_logdensity` evaluates log q(z) (log q(z | y) given classes) of any codes under it in HIP
    # (ops.aggpost_logdensity), `elbo_decomposition` splits the mean KL(q(z|x) || p(z|y)) into mutual information, the KL of the
    # aggregate posterior to the prior, total correlation and dimension-wise KL.  No OOD row family: nothing here is a score row.
    posterior_bank = None                     # {'mu', 'log_var' (N, K), 'labels' (N,), 'set'} and the operands of ops.aggpost_bank
    POSTERIOR_BANK_FILE = 'posterior-bank.pth'
    ELBO_TYPES = ('cvae', 'xvae', 'vae', 'vib', 'jvae')

    def fit_posterior_bank(self, dataset, batch_size=100, ratio=1.0, seed=0):
        """Fill `posterior_bank` with the posteriors of `dataset` (any map-style dataset of (x, label)): the pass of
        `fit_latent_bank` (one latent_posterior() pass in eval mode into preallocated device tensors, its seeded subset and
        whole-batch rule) keeping mu AND log sigma^2, then the stored operands of the density kernel (ops.aggpost_bank; the labels
        are its groups).  -> the bank's dictionary.  Models with coded labels are refused, as latent_posterior(x) refuses them."""
        mu, lv, labels = self._posterior_rows(dataset, batch_size, ratio, seed, 'fit_posterior_bank')
        self.posterior_bank = dict(ops.aggpost_bank(mu, lv, labels), labels=labels, set=getattr(dataset, 'name', 'set'))
        return self.posterior_bank

    def save_posterior_bank(self, dir_name):
        """Write the fitted bank as `posterior-bank.pth` into `dir_name` (a file of its own: save() / load() do not know it)."""
        return self._save_store('posterior_bank', self.POSTERIOR_BANK_FILE, dir_name,
                                'save_posterior_bank: no bank is fitted (fit_posterior_bank)')

    def load_posterior_bank(self, dir_name):
        """Read `posterior-bank.pth` of `dir_name` onto the model's device -> the bank's dictionary, bit for bit what was saved."""
        def check(d):
            try:
                ok = isinstance(d, dict) and set(d) == set(ops.AGGPOST_BANK_KEYS) | {'labels', 'set'}
                N, _ = ops.aggpost_check_bank(d, 'load_posterior_bank') if ok else (0, 0)
                ok = ok and torch.is_tensor(d['labels']) and d['labels'].dtype == torch.int64 and tuple(d['labels'].shape) == (N,)
            except ValueError:
                ok = False
            if not ok:
                raise ValueError(f'load_posterior_bank: {dir_name} does not hold a posterior bank')
        return self._load_store('posterior_bank', self.POSTERIOR_BANK_FILE, dir_name, check)

    def _posterior_bank_for(self, who):
        self._refuse_types(who, self.ELBO_TYPES)
        if self.posterior_bank is None:
            raise ValueError(f'{who}: no posterior bank is fitted (fit_posterior_bank or load_posterior_bank)')
        return self.posterior_bank

    def aggregate_logdensity(self, z, y=None, dims=False):
        """log q(z) of codes z (M, K) under the aggregate posterior of the bank -> (logq (M,), logq_dims (M, K) or None), fp32
        device tensors; with y (M,) labels: log q(z | y), the mixture of the bank rows of that class.  dims: the same for every
        coordinate alone.  ValueError without a bank.  What the kernel flags (a class without bank rows, a non-finite code) is in
        `ops.aggpost_status(device)` (`ops.aggpost_check_status`)."""
        bank = self._posterior_bank_for('aggregate_logdensity')
        z = z.to(device=bank['mu'].device, dtype=torch.float32)
        if y is not None:
            y = y.reshape(-1).to(z.device)
        return ops.aggpost_logdensity(z, bank, zgroup=y, conditional=y is not None, dims=dims)

    def elbo_decomposition(self, samples=None, seed=0, epsilon=None, dims=True):
        """The mean KL term of the bank's set taken apart, from ONE draw z_m = mu_m + sigma_m eps_m of `samples` rows of the bank
        (None: all of them in their order; else the first `samples` of a seeded host permutation); eps: `epsilon` (M, K) or a
        seeded draw on the device.  Per query: log q(z|x) = -1/2 sum_k (eps^2 + log sigma^2 + log 2 pi) in fp64, log q(z) and the
        per-coordinate log q(z_k) from the density kernel over the WHOLE bank, log p from the prior's log_density.  -> a dictionary
        of host values (means in fp64 on the device, one read-back):
          'kl' the mean analytic KL of the queried rows (the prior's kl()), 'kl_mc' mean[log q(z|x) - log p], 'mi' mean[log q(z|x) -
          log q(z)], 'kl_marginal' mean[log q(z) - log p], 'tc' mean[log q(z) - sum_k log q(z_k)], 'dwkl' mean[sum_k log q(z_k) -
          log p] and 'dwkl_per_dim' (K,) (None unless the prior is Gaussian with scalar or diagonal variance; tc and both None
          without `dims`), 'mi_bound' log N, 'n', 'm'; kl_mc = mi + kl_marginal and kl_marginal = tc + dwkl by construction.
        With a conditional prior (cvae, xvae) q(z) is q(z | y) of the row's class and p is p(z | y): mi is I(x; z | y), kl_marginal
        the mean KL(q(z|y) || p(z|y)); 'per_class' holds (C,) 'mi', 'kl_marginal' and 'count' (NaN where a class has no query) and
        'mi_unconditional' comes from a second launch against the bank as a whole.  'rows' (the queried rows, None for all) and 'z'
        (M, K, on the device) are the queries themselves.  ValueError without a bank; coded labels are refused."""
        bank = self._posterior_bank_for('elbo_decomposition')
        prior = self.encoder.prior
        N, K = bank['mu'].shape
        dev = bank['mu'].device
        if samples is None:
            rows, mu, lv, y = None, bank['mu'], bank['log_var'], bank['labels']
        else:
            if not 1 <= int(samples) <= N:
                raise ValueError(f'elbo_decomposition: 1 <= samples <= {N} (the rows of the bank) expected, got {samples}')
            rows = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:int(samples)]
            at = rows.to(dev)
            mu, lv, y = bank['mu'][at], bank['log_var'][at], bank['labels'][at]
        M = mu.shape[0]
        if epsilon is None:
            epsilon = torch.randn((M, K), generator=torch.Generator(device=dev).manual_seed(int(seed)), device=dev)
        elif not torch.is_tensor(epsilon) or tuple(epsilon.shape) != (M, K):
            raise ValueError(f'elbo_decomposition: epsilon ({M}, {K}) expected')
        eps = epsilon.to(device=dev, dtype=torch.float32)
        cond = bool(prior.conditional)
        with torch.no_grad():
            z = (mu + (0.5 * lv).exp() * eps).contiguous()
            lqzx = -0.5 * (eps.double().square() + lv.double() + math.log(2 * math.pi)).sum(1)
            logq, logq_dims = ops.aggpost_logdensity(z, bank, zgroup=y if cond else None, conditional=cond, dims=bool(dims))
            logq = logq.double()
            logp = prior.log_density(z, y if cond else None).double()
            fields = {'kl': prior.kl(mu, lv, y if cond else None, output_dict=False).double().mean(), 'kl_mc': (lqzx - logp).mean(),
                      'mi': (lqzx - logq).mean(), 'kl_marginal': (logq - logp).mean()}
            factorised = prior.distribution == 'gaussian' and prior.var_dim in ('scalar', 'diag')
            if dims:
                qsum = logq_dims.double().sum(1)
                fields['tc'] = (logq - qsum).mean()
                if factorised:
                    t = prior.inv_trans.detach().double()
                    t = (t.reshape(-1, 1) if prior.var_dim == 'scalar' else t.reshape(-1, K)).expand(prior.num_priors if cond else 1, K)
                    means = prior.mean.detach().double().reshape(-1, K)
                    at = y if cond else torch.zeros(M, dtype=torch.int64, device=dev)
                    logp_k = -0.5 * math.log(2 * math.pi) - 0.5 * ((z.double() - means[at]) * t[at]).square() + t[at].abs().log()
                    fields['dwkl'] = (qsum - logp).mean()
                    fields['dwkl_per_dim'] = (logq_dims.double() - logp_k).mean(0)
            if cond:
                C = prior.num_priors
                count = torch.bincount(y, minlength=C).double()
                fields['count'] = count
                for name, v in (('mi_c', lqzx - logq), ('kl_marginal_c', logq - logp)):
                    fields[name] = torch.zeros(C, dtype=torch.float64, device=dev).index_add_(0, y, v) / count
                fields['mi_unconditional'] = (lqzx - ops.aggpost_logdensity(z, bank)[0].double()).mean()
            host = ops.read_back(fields)
        out = {k: float(host[k]) for k in ('kl', 'kl_mc', 'mi', 'kl_marginal')}
        out['tc'] = float(host['tc']) if dims else None
        out['dwkl'] = float(host['dwkl']) if 'dwkl' in host else None
        out['dwkl_per_dim'] = host.get('dwkl_per_dim')
        out.update(mi_bound=math.log(N), n=N, m=M)
        if cond:
            out['per_class'] = {'mi': host['mi_c'], 'kl_marginal': host['kl_marginal_c'], 'count': host['count'].astype(np.int64)}
            out['mi_unconditional'] = float(host['mi_unconditional'])
        out.update(rows=rows, z=z)
        return out

    # The Mahalanobis rows `maha` and `maha-rel` (Lee et al. 2018; Ren et al. 2021): minus the squared
    # Mahalanobis distance from a sample's posterior mean to the nearest of the class Gaussians - one per class of the bank, with
    # one shared covariance - that `fit_latent_gaussians` fits on the latent bank, and the same minus the distance under ONE
    # Gaussian for the whole bank.  `zdist` is the distance to the centroids the prior learned; this is the distance to the
    # Gaussians the encoder produces on the training set.  Off by default: every name raises, 'all' is the reference's table.
    # On (class or instance): 'all' and 'maha*' expand to `_maha_names()`.  Fitting is the caller's job.
    OOD_MAHA_METHODS = False
    latent_gaussians = None                                                   # ops.maha_fit's dictionary and 'set'
    LATENT_GAUSSIANS_FILE = 'latent-gaussians.pth'

    def _maha_names(self):
        """`maha` and `maha-rel`; `maha` alone once Gaussians with a single non-empty class are fitted (`maha-rel` is then 0)."""
        g = self.latent_gaussians
        return ['maha'] if g is not None and g['cmap'].shape[0] < 2 else ['maha', 'maha-rel']

    def fit_latent_gaussians(self, shrinkage=0.0):
        """Fit `latent_gaussians` on `latent_bank`: the moments of the bank by class on the device in fp64 (ops.maha_moments),
        then the two factorisations on the host (ops.maha_fit; `shrinkage` * the mean variance is added to both diagonals,
        ValueError naming it when a matrix is not positive definite).  -> the dictionary: ops.maha_fit's - counts, means, mean0,
        the fp64 factors W and W0, the fp32 operands, the class map, the shrinkage - and 'set', the bank's set name.  ValueError
        without a bank, with a bank of fewer than two rows, and for a bank row with a label outside the model's classes or a
        non-finite element.  This call synchronises; scoring does not."""
        bank = self.latent_bank
        if bank is None:
            raise ValueError('fit_latent_gaussians: no latent bank is fitted (fit_latent_bank or load_latent_bank)')
        if bank['bank'].shape[0] < 2:
            raise ValueError(f"fit_latent_gaussians: the bank holds {bank['bank'].shape[0]} rows, at least two are needed")
        status = torch.zeros(1, dtype=torch.int32, device=bank['bank'].device)
        moments = ops.maha_moments(bank['bank'], bank['labels'], self.num_labels, status=status)
        ops.maha_check_status(status)
        self.latent_gaussians = dict(ops.maha_fit(moments, shrinkage), set=bank['set'])
        return self.latent_gaussians

    def save_latent_gaussians(self, dir_name):
        """Write the fitted Gaussians as `latent-gaussians.pth` into `dir_name` (a file of its own: save() / load() do not know it)."""
        return self._save_store('latent_gaussians', self.LATENT_GAUSSIANS_FILE, dir_name,
                                'save_latent_gaussians: no Gaussians are fitted (fit_latent_gaussians)')

    def load_latent_gaussians(self, dir_name):
        """Read `latent-gaussians.pth` of `dir_name` onto the model's device -> the dictionary, bit for bit what was saved."""
        def check(d):
            if not isinstance(d, dict) or set(d) != set(ops.MAHA_FIT_KEYS) | {'set'}:
                raise ValueError(f'load_latent_gaussians: {dir_name} does not hold latent Gaussians')
            ops.maha_check_fit(d, 'load_latent_gaussians')
        return self._load_store('latent_gaussians', self.LATENT_GAUSSIANS_FILE, dir_name, check)

    def maha_scores(self, mu):
        """The Mahalanobis rows of a batch of posterior means mu (N, K): {'maha': -d, 'maha-rel': -rel}, (N,) fp32 device tensors,
        higher = more in-distribution, from ONE `ops.maha_scores` call (d: the squared distance to the nearest class Gaussian,
        rel: d minus the squared distance under the Gaussian of the whole bank); `maha` alone when a single class is fitted.
        ValueError without fitted Gaussians.  A non-finite row sets the device's `ops.maha_status` word (`ops.maha_check_status`)."""
        if self.latent_gaussians is None:
            raise ValueError('maha_scores: no latent Gaussians are fitted (fit_latent_gaussians or load_latent_gaussians)')
        d, _, rel = ops.maha_scores(mu.float(), self.latent_gaussians)
        return {name: -v for name, v in zip(self._maha_names(), (d, rel))}

    # The input-complexity rows `ic-bits`, `ic-elbo` and `ic-iws` (Serra et al. 2020): a VAE's likelihood is
    # high on a simple image whatever set it comes from, and S(x) = -log2 p(x) - L(x) takes the length L(x) of the image under a
    # lossless coder out of it.  `ic-bits` is -L alone, `ic-elbo` / `ic-iws` are log2 of the model's `elbo` / `iws` row as the
    # probability of the pixel's 8-bit bin, plus L: higher = more in-distribution, as every row here.  L comes from ONE launch
    # of csrc/ic.hip per batch (ops.image_code_length).  Off by default: every name raises, 'all' is the reference's table.
    # On (class or instance): 'all' and 'ic*' expand to `_ic_names()` on the types of IC_TYPES (`vib` has no decoder).
    OOD_IC_METHODS = False
    IC_TYPES = ('cvae', 'vae', 'xvae')

    def _ic_names(self):
        """`ic-bits`, `ic-elbo`, `ic-iws`."""
        return ['ic-bits', 'ic-elbo', 'ic-iws']

    def input_complexity(self, x):
        """The code length of a batch of images x (N, *input_shape) fp32 on the device, values in [0, 1]: {'bits': (N,) fp64, the
        length L(x) in bits of the image quantised to 8 bits, 'bits_per_dim': bits / (C H W), 'choice': (N,) int32, the coder's
        colour space and modes (`ops.ic_choice`)}.  ONE `ops.image_code_length` call; nothing is synchronised.  A pixel off the
        8-bit grid or a non-finite one sets the device's `ops.ic_status` word (`ops.ic_check_status`)."""
        shape = tuple(self.input_shape)
        if len(shape) != 3:
            raise NotImplementedError(f'input_complexity: images (C, H, W) expected, the model reads {shape}')
        bits, _, choice = ops.image_code_length(x.reshape(-1, *shape))
        return {'bits': bits, 'bits_per_dim': bits / float(np.prod(shape)), 'choice': choice}

    def ic_scores(self, x, losses):
        """The input-complexity rows of a batch: x as `input_complexity` takes it, `losses` what a label-free evaluate(x) of the
        batch returned -> {'ic-bits': -L, 'ic-elbo': e / ln 2 - D log2 255 + L, 'ic-iws': the same on the `iws` row}, (N,) fp32
        device tensors computed in fp64 and rounded once.  e: the model's own `elbo` row (score_rows.parse('elbo'): the max over
        the classes for a cvae), in nats; D = C H W; D log2 255 turns the density of x = q / 255 into the probability of its bin
        and is left out for output_distribution='categorical', whose likelihood is discrete already.  Models of another type
        than IC_TYPES or with coded labels are refused, as latent_posterior(x) refuses the latter."""
        self._refuse_types('ic_scores', self.IC_TYPES)
        L = self.input_complexity(x)['bits']
        D = float(np.prod(tuple(self.input_shape)))
        traits = score_rows.traits_of(self)
        # both rows through one chain of elementwise launches: the same operations in the same order as row by row
        log2p = torch.stack([score_rows.parse(base, traits).torch_row(losses) for base in ('elbo', 'iws')]).double() / math.log(2)
        if self.output_distribution != 'categorical':
            log2p = log2p - D * math.log2(255)
        elbo, iws = (log2p + L).float()
        return {'ic-bits': (-L).float(), 'ic-elbo': elbo, 'ic-iws': iws}

    # The SSIM rows `ssim`, `ssim-mu` and `ssim-cs` (Wang et al. 2004; Bergmann et al. 2018): every other row
    # judges a reconstruction by its squared error, which a blurred reconstruction of the right brightness keeps small whatever
    # it lost of edges and texture.  These rows score the reconstruction as an image: the structural similarity of x to x_reco
    # under an 11-tap Gaussian window - local means, variances and the covariance.  `ssim` is the mean over the sampled draws
    # (rows 1 .. L of x_reco, the rows `mse` averages), `ssim-mu` the row decoded from the posterior mean (row 0: no noise, the
    # same bits under any seed), `ssim-cs` the mean over the draws of the contrast-structure term alone (the luminance term
    # taken out).  Higher = more in-distribution.  ONE launch of csrc/ssim.hip per batch (ops.ssim), on the x_reco the label-free
    # evaluation of the batch has made anyway.  Off by default: every name raises, 'all' is the reference's table.  On (class or
    # instance): 'all' and 'ssim*' expand to `_ssim_names()` on the types of SSIM_TYPES (`vib` has no decoder).
    OOD_SSIM_METHODS = False
    SSIM_TYPES = ('cvae', 'vae', 'xvae')

    def _ssim_names(self):
        """`ssim`, `ssim-mu`, `ssim-cs`."""
        return ['ssim', 'ssim-mu', 'ssim-cs']

    def _ssim_refuse(self, who):
        shape = tuple(self.input_shape)
        why = None
        if self.output_distribution == 'categorical':
            why = "not output_distribution='categorical' (its x_reco holds 256 levels per pixel)"
        elif len(shape) != 3 or min(shape[1:]) < ops.SSIM_WINDOW:
            why = f'the model reads {shape}'
        self._refuse_types(who, self.SSIM_TYPES, f' that decode images (C, H, W) with min(H, W) >= {ops.SSIM_WINDOW}', why)

    def ssim_scores(self, x, x_reco):
        """The SSIM rows of a batch: x (N, *input_shape) and x_reco (L + 1, N, *input_shape), what a label-free evaluate(x)
        returned first -> {'ssim': the mean over rows 1 .. L of ssim[r, n], 'ssim-mu': ssim[0, n], 'ssim-cs': the mean over rows
        1 .. L of cs[r, n]}, (N,) fp32 device tensors from ONE `ops.ssim` call, the means taken in fp64 and rounded once.
        Refused (NotImplementedError) for another type than SSIM_TYPES, coded labels, a categorical decoder and inputs that are
        not images with min(H, W) >= 11.  A non-finite pixel sets the device's `ops.ssim_status` word (`ops.ssim_check_status`)."""
        self._ssim_refuse('ssim_scores')
        shape = tuple(self.input_shape)
        x = x.reshape(-1, *shape)
        s, cs = ops.ssim(x, x_reco.reshape(-1, x.shape[0], *shape))
        if s.shape[0] < 2:
            raise ValueError('ssim_scores: x_reco with the mean row and at least one sampled draw expected')
        mean, mean_cs = torch.stack([s[1:], cs[1:]]).double().mean(1).float()
        return {'ssim': mean, 'ssim-mu': s[0], 'ssim-cs': mean_cs}

    def ssim_map(self, x):
        """The per-pixel similarity map of a batch x (N, *input_shape) against its reconstruction from the posterior mean:
        (N, H - 10, W - 10) fp32, the channel mean of l * cs, for localisation.  One label-free evaluate in eval mode under
        no_grad and ONE `ops.ssim(maps=True)` call; the training flag is restored."""
        self._ssim_refuse('ssim_map')
        shape = tuple(self.input_shape)
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                x = x.reshape(-1, *shape)
                x_reco = self.evaluate(x)[0]
                return ops.ssim(x, x_reco.reshape(-1, x.shape[0], *shape), maps=True)[2][0]
        finally:
            if was_training:
                self.train()

    # The density-of-states rows (Morningstar et al. 2021; for one statistic the typicality test of Nalisnick et al. 2019;
    # DESIGN.md section 7s).  Every other row is monotone in a statistic, and a VAE's known failure is the sample whose statistic
    # is TOO good; these rows ask how typical a sample's statistics `DOSE_STATS` are of a training set, the score bank of
    # `fit_score_bank`: `dose-<stat>` is the log-density of the statistic under a Gaussian kernel density estimate of the bank's
    # (bandwidth DOSE_BANDWIDTH x Scott's), `dose` their sum (the paper's score), `dose-joint` the log-density of all of them
    # under a product kernel, `dose-typ-<stat>` minus the distance to the bank's mean in its standard deviations.  Higher = more
    # in-distribution, as every row here.  ONE `ops.kde_logdensity` call per batch (csrc/dose.hip).  Off by default: every name
    # raises, 'all' is the reference's table.  On (class or instance): 'all' and 'dose*' expand to `_dose_names()` on the types
    # of DOSE_TYPES.  Fitting is the caller's job.  A set scored against a bank fitted on itself meets itself: each of its
    # samples is one of the kernels it is scored under (there is no leave-one-out).
    OOD_DOSE_METHODS = False
    DOSE_BANDWIDTH = 1.0
    DOSE_TYPES = ('cvae', 'vae', 'xvae', 'vib')
    _DOSE_STATS = {'vib': ('kl', 'zdist', 'logits')}
    score_bank = None                                                         # ops.kde_fit's dictionary, 'stats' and 'set'
    SCORE_BANK_FILE = 'score-bank.pth'

    @property
    def DOSE_STATS(self):
        """The statistics of the density-of-states rows: an instance's own tuple once it sets one, else its type's default."""
        own = self.__dict__.get('_dose_stats')
        return own if own is not None else self._DOSE_STATS.get(self.type, ('elbo', 'iws', 'kl', 'zdist', 'mse'))

    @DOSE_STATS.setter
    def DOSE_STATS(self, names):
        self.__dict__['_dose_stats'] = None if names is None else tuple(names)

    def _dose_stat_rows(self):
        """DOSE_STATS -> their Rows.  ValueError for an entry that is not a plain score name of this model: a name with a `-`,
        a row of a recorded family, `joint` or `typ`, or a name score_rows.parse does not accept."""
        stats = tuple(self.DOSE_STATS)
        traits = score_rows.traits_of(self)
        if not traits.losses_might_be_computed_for_each_class:
            # a vib's `kl` and `zdist` have no class axis, as a vae's: the statistic is minus the loss (the reference's rows
            # take a maximum over the first axis for every type but vae, cvae.py:1035-1039 - over the SAMPLES here)
            traits = traits._replace(is_vae=True)
        rows = []
        for name in stats:
            bad = None
            if not isinstance(name, str) or not name or '-' in name or name[-1] in '~@' or name in ('joint', 'typ'):
                bad = 'a plain score name expected'
            elif score_rows.claimed_by(name) is not None or score_rows.recorded_by(name) is not None:
                bad = 'a row of a recorded family'
            else:
                try:
                    rows.append(score_rows.parse(name, traits))
                except NotImplementedError:
                    bad = f'not a score of a {self.type}'
            if bad:
                raise ValueError(f'DOSE_STATS: {name!r}: {bad}')
        if not 1 <= len(stats) <= ops.DOSE_MAX_STATS or len(set(stats)) != len(stats):
            raise ValueError(f'DOSE_STATS: 1 to {ops.DOSE_MAX_STATS} different statistics expected, got {stats}')
        return rows

    def _dose_names(self):
        """`dose`, `dose-joint` (not for a single statistic: it is `dose` then), `dose-<stat>` and `dose-typ-<stat>` for the
        statistics of `DOSE_STATS`, in their order."""
        stats = tuple(self.DOSE_STATS)
        return (['dose'] + ['dose-joint'] * (len(stats) > 1) + ['dose-' + s for s in stats] + ['dose-typ-' + s for s in stats])

    def _dose_refuse(self, who):
        self._refuse_types(who, self.DOSE_TYPES)

    def _dose_stat_values(self, rows, logits, losses, out=None, col=0):
        """The statistics of a batch by their torch expressions, stacked: (S, N) fp32 (into out[:, col:col + N] with `out`)."""
        got = score_rows.write_rows(rows, range(len(rows)), logits, losses, out, col, torch_rows=('',))
        return torch.stack([v.float() for v in got]) if out is None else out[:, col:col + got[0].shape[0]]

    def fit_score_bank(self, dataset, batch_size=100, ratio=1.0, seed=0):
        """Fill `score_bank` with the statistics `DOSE_STATS` of `dataset` (any map-style dataset of (x, label)): ONE label-free
        evaluation pass in eval mode, the rows of each batch written through score_rows.write_rows (their torch expressions)
        straight into a preallocated (S, M) fp32 device buffer, then `ops.kde_fit` (bandwidth DOSE_BANDWIDTH).  ratio < 1: a
        seeded random subset of round(ratio * len) samples, by the rule of `fit_latent_bank`; every batch is evaluated whole,
        also one that keeps no sample, so under one seed of the latent noise the kept columns are those of a full pass.  -> the bank's dictionary: ops.kde_fit's, 'stats' (the names) and 'set'.
        ValueError for a `DOSE_STATS` entry that is not a plain score name of the model, for a statistic that is constant or not
        finite on the set and for fewer than two samples.  Models of another type than DOSE_TYPES or with coded labels are
        refused, as the other families refuse the latter.  This call synchronises."""
        self._dose_refuse('fit_score_bank')
        rows = self._dose_stat_rows()
        keep, M = self._seeded_subset(len(dataset), ratio, seed, 'fit_score_bank')
        device = self.device
        was_training = self.training
        self.eval()
        bank, seen, pos, measures = torch.empty((len(rows), M), dtype=torch.float32, device=device), 0, 0, None
        with torch.no_grad():
            for i, batch in enumerate(self._batch_source(dataset, batch_size, False)):
                x = batch[0]
                sel = None if keep is None else keep[seen:seen + x.shape[0]]
                seen += x.shape[0]
                # EVERY batch is evaluated, one without a kept sample too: the statistics draw latent noise, and a batch left
                # out would shift the draws of every batch behind it (the posterior means of fit_latent_bank draw none)
                _, logits, losses, measures = self._evaluate_for_scores(x, i, measures)[:4]
                if sel is not None and not bool(sel.any()):
                    continue
                if sel is None or bool(sel.all()):
                    pos += self._dose_stat_values(rows, logits, losses, bank, pos).shape[1]
                else:
                    cols = sel.nonzero()[:, 0].to(device)
                    bank[:, pos:pos + cols.shape[0]] = self._dose_stat_values(rows, logits, losses)[:, cols]
                    pos += cols.shape[0]
        if was_training:
            self.train()
        if pos != M:
            raise ValueError(f'fit_score_bank: the set yielded {pos} of the {M} samples expected')
        fit = ops.kde_fit(bank, float(self.DOSE_BANDWIDTH))
        self.score_bank = dict(fit, stats=tuple(self.DOSE_STATS), set=getattr(dataset, 'name', 'set'))
        return self.score_bank

    def save_score_bank(self, dir_name):
        """Write the fitted bank as `score-bank.pth` into `dir_name` (a file of its own: save() / load() do not know it)."""
        return self._save_store('score_bank', self.SCORE_BANK_FILE, dir_name, 'save_score_bank: no bank is fitted (fit_score_bank)')

    def load_score_bank(self, dir_name):
        """Read `score-bank.pth` of `dir_name` onto the model's device -> the bank's dictionary, bit for bit what was saved.
        ValueError for a file that does not hold a score bank, and for one whose 'stats' are not this model's `DOSE_STATS`."""
        def check(d):
            if not isinstance(d, dict) or set(d) != set(ops.DOSE_FIT_KEYS) | {'stats', 'set'} or not isinstance(d['stats'], tuple):
                raise ValueError(f'load_score_bank: {dir_name} does not hold a score bank')
            ops.kde_check_fit(d, 'load_score_bank')
            if len(d['stats']) != d['S']:
                raise ValueError(f'load_score_bank: {dir_name} does not hold a score bank')
            if d['stats'] != tuple(self.DOSE_STATS):
                raise ValueError(f"load_score_bank: the bank was fitted on the statistics {d['stats']}, this model's DOSE_STATS are "
                                 f'{tuple(self.DOSE_STATS)}')
        return self._load_store('score_bank', self.SCORE_BANK_FILE, dir_name, check)

    def dose_scores(self, logits, losses):
        """The density-of-states rows of a batch, `logits` and `losses` what a label-free evaluate(x) of it returned:
        {name: (N,) fp32 device tensor} for the names of `_dose_names()`, higher = more in-distribution.  The statistics come by
        their torch expressions, stacked (S, N), and go through ONE `ops.kde_logdensity` call.  ValueError without a bank, or
        with a bank of other statistics than `DOSE_STATS`.  A non-finite statistic sets the device's `ops.kde_status` word
        (`ops.kde_check_status`)."""
        self._dose_refuse('dose_scores')
        if self.score_bank is None:
            raise ValueError('dose_scores: no score bank is fitted (fit_score_bank or load_score_bank)')
        if tuple(self.score_bank['stats']) != tuple(self.DOSE_STATS):
            raise ValueError(f"dose_scores: the bank was fitted on the statistics {self.score_bank['stats']}, this model's "
                             f'DOSE_STATS are {tuple(self.DOSE_STATS)}')
        rows = self._dose_stat_rows()
        out = ops.kde_logdensity(self._dose_stat_values(rows, logits, losses).contiguous(), self.score_bank)
        by_name = dict(zip(['dose-' + s for s in self.DOSE_STATS] + ['dose', 'dose-joint']
                           + ['dose-typ-' + s for s in self.DOSE_STATS], out))
        return {name: by_name[name] for name in self._dose_names()}

    def _odin_names(self):
        """The `odin-T-eps` method names of this instance's grid, temperature-major (cvae.py:124-127)."""
        return [score_rows.odin_name(T, e) for T in self.ODIN_TEMPS for e in self.ODIN_EPS]

    def _ood_methods(self, method):
        """The score rows of ood_detection_rates: `method` = 'all' (this type's table minus what is not built, said in ONE log
        line), a name or a list of names.  The recorded families (score_rows.FAMILIES: `odin*` on a type whose table lists
        it, i.e. vib; the opt-ins `regret*`, `knn*`, `maha*`, `ic*`, `dose*` and `ssim*`): off, their names raise and 'all' does not hold them; on, 'all' and the starred
        name expand to the model's own list (the plain names first, the expansions behind them in the table's order, as the
        reference's develop_starred_methods orders them) and a single name has to be on that list.  The spline-threshold
        ('-a-x-y') methods raise unless `OOD_QUANTILE_METHODS` is set, with which they are rows like the others."""
        families = score_rows.FAMILIES
        on = {f: f.on(self) for f in families}

        def refusal(m):                                         # why m is outside this build, or None
            spline = '-a-' in m and not self.OOD_QUANTILE_METHODS      # the spline thresholds share ODIN's sentence
            f = score_rows.ODIN if spline else score_rows.claimed_by(m)
            return f.off.format(m=m, types=', '.join(self.REGRET_TYPES)) if spline or not on.get(f, True) else None

        def expand(names):
            plain = [m for m in names if m not in [f.starred for f in families]]
            return plain + [e for f in families if f.starred in names for e in getattr(self, f.names)()]
        if method == 'all':
            skipped = [m for m in self.ood_methods if refusal(m)]
            if skipped:
                logging.warning('ood_detection_rates: methods outside this build are left out: %s', ', '.join(skipped))
            built = [m for m in self.ood_methods if not refusal(m)]
            return expand(built + [f.starred for f in families if on[f] and f.starred not in built])
        methods = [method] if isinstance(method, str) else list(method)
        for m in methods:
            if refusal(m):
                raise NotImplementedError(refusal(m))
        methods = expand(methods)
        listed = {f: getattr(self, f.names)() for f in families if on[f]}
        for m in methods:
            f = score_rows.claimed_by(m)
            if f is not None and m not in listed[f]:
                raise ValueError(f.unlisted.format(m=m))
            if '-a-' in m:
                score_rows.roc_mode(m)
        return methods

    def _score_set(self, dset, methods, batch_size, num_batch, shuffle, recorder, sample_dirs, on_batch=None, keep_test=False,
                   sample_recorder=None):
        """One pass over `dset` for ood_detection_rates: per batch the label-free evaluation (or the batch read back from a full
        recorder), then `score_rows.write_rows`: the score rows go straight into ONE preallocated (M, n) device buffer, one
        kernel launch per source tensor (the `SCORE_SET_TORCH_ROWS` by their torch expressions) - no value comes to the host
        here.  on_batch(i, num_batch, scores_so_far) is called after each batch.  -> (M, n) fp32 device scores.

        `sample_recorder` (a jvae_compat.recorders.SampleRecorder, or None): every EVALUATED batch appends, of the keys the recorder
        holds, `mu` (the posterior means of the same pass: no second one), `y` (the loader's labels) and `y_nearest` (argmin over
        the classes of this batch's zdist); a set read back from a full LossRecorder appends nothing (cvae.py:1634-1642,1793-1795).
        It is saved as samples-<set>.pth beside the loss record."""
        device = self.device
        name = getattr(dset, 'name', 'set')
        records = [score_rows.parse(m, score_rows.traits_of(self)) for m in methods]
        families = [f for f in score_rows.FAMILIES if any(f.is_row(r.base) for r in records)]      # what this pass computes per batch
        with_mu = sample_recorder is not None or any('mu' in f.args for f in families)
        with_reco = any('x_reco' in f.args for f in families)   # the reconstructions of the same pass: no second decode
        filled, sums, measures = 0, {}, None
        with torch.no_grad(), self._recorded_pass(dset, name, batch_size, num_batch, shuffle, recorder, sample_dirs) as (
                recorded, recording, num_batch, batch_size, loader):
            buf = torch.empty((len(methods), num_batch * batch_size), dtype=torch.float32, device=device)
            for i in range(num_batch):
                if recorded:
                    keys = [k for k in recorder.keys() if k in self.loss_components or score_rows.recorded_by(k)]     # cvae.py:1665-1667
                    losses = recorder.get_batch(i, *keys, force_dict=True)
                    logits = recorder.get_batch(i, 'logits').T if 'logits' in recorder.keys() else None
                else:
                    x, y = next(loader)[:2]
                    more = {'with_reco': True} if with_reco else {}           # no family reads x_reco: the call as it always was
                    x, logits, losses, measures, *mu = self._evaluate_for_scores(x, i, measures, with_mu=with_mu, **more)
                    x_reco = mu.pop() if with_reco else None
                    y = y.to(device)
                    if sample_recorder is not None:
                        sample_recorder.append_batch(**self._sample_record(sample_recorder, mu[0], y, losses))
                    have = {'x': x, 'logits': logits, 'losses': losses, 'mu': mu[0] if mu else None, 'x_reco': x_reco}
                    for f in families:
                        # all rows of the family per batch (it is what the recorder holds), from the pass above, on the device
                        have['losses'] = losses = dict(losses, **getattr(self, f.scores)(**{a: have[a] for a in f.args}))
                    if recording:
                        extra = {} if logits is None else {'logits': logits.T}
                        recorder.append_batch(**losses, y_true=y, **extra)
                n = score_rows.write_rows(records, range(len(records)), logits, losses, buf, filled, self.SCORE_SET_TORCH_ROWS,
                                          self._wim_status_word)[0].shape[0]
                if families:
                    losses = {k: v for k, v in losses.items() if not score_rows.recorded_by(k)}     # test_losses: the loss components
                filled += n
                if keep_test:
                    for k, v in losses.items():                                      # cvae.py:1671, summed on the device
                        sums[k] = sums.get(k, 0.) + v.float().mean()
                if on_batch is not None:
                    on_batch(i, num_batch, buf[:, :filled])
        if keep_test:
            self.test_losses = {k: float(v) / max(num_batch, 1) for k, v in
                                zip(sums, torch.stack(list(sums.values())).tolist())} if sums else {}
            if measures:
                self.test_measures = dict(measures)
        if sample_recorder is not None:
            for d in sample_dirs:
                os.makedirs(d, exist_ok=True)
                sample_recorder.save(os.path.join(d, 'samples-{}.pth'.format(name)))
        return buf[:, :filled].contiguous()

    @staticmethod
    def _sample_record(recorder, mu, y, losses):
        """What one evaluated batch appends to a sample recorder: the keys it holds among mu, y, y_nearest."""
        keys = set(recorder.keys()) if len(recorder.keys()) else {'mu', 'y'}
        unknown = keys - {'mu', 'y', 'y_nearest'}
        if unknown:
            raise KeyError('sample recorders hold mu, y and y_nearest, not ' + ', '.join(sorted(unknown)))
        out = {}
        if 'mu' in keys:
            out['mu'] = mu
        if 'y' in keys:
            out['y'] = y
        if 'y_nearest' in keys:
            zdist = losses['zdist']
            if zdist.dim() < 2:
                raise ValueError('y_nearest needs a zdist with a class axis (a class-conditional prior evaluated without labels)')
            out['y_nearest'] = zdist.argmin(0)
        return out

    @staticmethod
    def _row_mean_std(scores):
        """fp64 mean and population standard deviation (np.std, ddof = 0) of each score row, on the device -> (M, 2)."""
        x = scores.double()
        mean = x.mean(1)
        return torch.stack([mean, ((x - mean[:, None]).abs() ** 2).mean(1).sqrt()], 1)

    def ood_detection_rates(self, oodsets=None, testset=None, batch_size=100, num_batch='all', method='all', print_result=False,
                            update_self_ood=True, epoch='last', outputs=None, recorders=None, from_where='all', sample_dirs=[],
                            sample_recorders=None, log=True):
        """OOD detection rates of `oodsets` against the in-distribution `testset` per OOD method, with the reference's signature
        and result dictionary (cvae.py:1455-1911): -> {set: {method: {'epochs', 'n', 'mean', 'std', 'auc', 'tpr', 'fpr',
        'thresholds'}}}, `self.ood_results[epoch]` updated when `update_self_ood` (with the in-distribution set's
        {'n', 'epochs', 'mean', 'std:'} entry - the reference's key has that colon), `test_losses` / `test_measures` set from
        the in-distribution pass, `record-<set>.pth` written into `sample_dirs` through the `LossRecorder`s of `recorders`
        ({} = make one per set, filled in place), and a full recorder read back instead of evaluating, as in accuracy().

        train_model() makes this call in its test phase when `TRAIN_OOD_PHASE` is set.

        Underneath, the scores never leave the device: every batch's `batch_dist_measures(out=...)` rows are written into one
        (M, n) buffer per set by csrc/misclass.hip, one launch per source tensor (`SCORE_SET_TORCH_ROWS` - `iws`, `elbo` and
        the softmax rows - by their torch expressions, whose bits the ROC thresholds are held to), the ROC of all M methods of a set is ONE `ops.roc_curve` call (csrc/roc.hip) made every 100 batches for the
        progress line and at the last batch, as the reference does with its Python loop (utils/roc_curves.py:38-210), and only
        its (M, K) results and the fp64 row means / deviations come to the host.  'thresholds' holds the K [low, up] pairs
        (the reference stores list(dict), i.e. the two key names).  Methods: what `batch_dist_measures` computes, one-sided,
        with the '-2s' suffix (two-sided around the mean) or, with `OOD_QUANTILE_METHODS`, the '-a-x-y' suffix (two-sided on
        in-score quantiles; ValueError below 4 in-distribution samples); see `_ood_methods` for the rest.  Named datasets
        (`testset=None` or a string, `oodsets=None` = the same-size siblings of the test set that can be opened, or names) are
        resolved from `DATA_ROOT` when that is set, else refused, as for accuracy(); the registry lookup of earlier results
        (`from_where`) is host plumbing outside this build.

        `sample_recorders` ({set name: SampleRecorder}): a set named there has the posterior means `mu`, the labels `y` and the
        nearest class `y_nearest` of every evaluated batch appended (the keys the recorder holds; `_score_set`) and
        `samples-<set>.pth` written into every `sample_dirs` entry.  The OOD sets get `y` and `y_nearest` as well when their
        recorder holds them - the reference leaves zeros there (cvae.py:1793-1795 appends `mu` alone) and its ft/inspection.py
        recomputes `y_nearest` from `mu`.  Empty or None: nothing changes, the same launches and the same results.

        With `DETECTION_PR_METRICS` every per-method dictionary of an OOD set also holds 'aupr_in', 'aupr_out', 'aucpr_in',
        'aucpr_out' and 'dete' (ONE `ops.pr_metrics` call beside each ROC, its figures in the ROC's host copy); the '-a-x-y'
        methods gain nothing."""
        if testset is None or isinstance(testset, str) or oodsets is None or any(isinstance(o, str) for o in oodsets):
            if self.DATA_ROOT is None:
                raise NotImplementedError('named torchvision datasets are outside this build: pass torch.utils.data.Datasets')
            testset, oodsets = self._open_named_sets(testset, oodsets)
        if not method:
            return
        if epoch == 'last':
            epoch = self.trained
        methods = self._ood_methods(method)
        names = [getattr(s, 'name', 'set') for s in [testset] + list(oodsets)]
        if recorders is not None and not recorders:
            from jvae_compat.recorders import LossRecorder
            recorders.update({n: LossRecorder(batch_size) for n in names})
        recorders = recorders or {}
        sample_recorders = sample_recorders or {}
        ood_results = {n: {} for n in names[1:]}
        if not oodsets:
            return ood_results
        was_training = self.training
        self.eval()
        modes = [score_rows.roc_mode(m) for m in methods]

        def plan(dset):
            full = int(np.ceil(len(dset) / batch_size))
            limited = isinstance(num_batch, int) and num_batch < full
            return (num_batch if limited else full), limited

        sink = outputs if outputs is not None and hasattr(outputs, 'results') else None

        def progress_line(name, row_means, fpr):
            """on_batch callback of a pass: the progress line of cvae.py:1709-1715,1870-1875, written at the reference's ROC
            points (every 100 batches and the last one); None without a sink, and the pass then brings nothing to the host."""
            if sink is None:
                return None
            t0 = time.time()

            def on_batch(i, nb, scores):
                if i % self.OOD_ROC_EVERY and i != nb - 1:
                    return
                sink.results(i, nb, 0, 1, metrics=dict(zip(methods, row_means(scores))), fpr=fpr(),
                             time_per_i=(time.time() - t0) / (i + 1), batch_size=batch_size, preambule=name)
            return on_batch

        nb, shuffle = plan(testset)
        ind = self._score_set(testset, methods, batch_size, nb, shuffle, recorders.get(names[0]), sample_dirs, keep_test=True,
                              sample_recorder=sample_recorders.get(names[0]), on_batch=progress_line(names[0], lambda s: self._row_mean_std(s)[:, 0].tolist(),
                                                     lambda: {m: np.nan for m in methods}))
        for m in methods:
            if '-a-' in m and ind.shape[1] < 4:
                raise ValueError(f'{m}: {ind.shape[1]} in-distribution samples, the cubic spline of the reference needs 4 '
                                 '(utils/roc_curves.py:79)')
        if update_self_ood:
            entry = self.ood_results.setdefault(epoch, {}).setdefault(names[0], {})
            for m, (mean, std) in zip(methods, self._row_mean_std(ind).tolist()):
                entry[m] = {'n': ind.shape[1], 'epochs': epoch, 'mean': mean, 'std:': std}

        kept = torch.tensor(self.OOD_KEPT_TPR, dtype=torch.float64, device=ind.device)
        with_pr = bool(self.DETECTION_PR_METRICS)
        for oodset, name in zip(oodsets, names[1:]):
            last = {}

            def roc(scores):
                """ONE device ROC for all methods, ONE copy of its results to the host."""
                fields = dict(ops.roc_curve(ind, scores.contiguous(), kept, modes), mean_std=self._row_mean_std(scores))
                if with_pr:        # ONE ops.pr_metrics call, its (M, 5) figures in the same copy (the ROC's status word flags the same rows)
                    p = ops.pr_metrics(ind, scores.contiguous(), modes)
                    fields['pr'] = torch.stack([p[k] for k in ops.PR_FIGURES], 1)
                host = last['host'] = ops.read_back(fields)
                ops.roc_check_status(host['status'].astype(np.int64))
                return host['mean_std'][:, 0].tolist()

            def fpr95():
                return {m: float(f[5]) for m, f in zip(methods, last['host']['fpr'])}      # fpr_at_tpr(..., 0.95): slot 5 of the kept TPRs

            nb, shuffle = plan(oodset)
            scores = self._score_set(oodset, methods, batch_size, nb, shuffle, recorders.get(name), sample_dirs,
                                     sample_recorder=sample_recorders.get(name), on_batch=progress_line(name, roc, fpr95))
            if sink is None:                                  # with a sink the last batch's progress ROC is the final one
                roc(scores)
            keys = ('auc', 'fpr', 'low', 'up', 'mean_std') + ('pr',) * with_pr
            for m, auc, fpr, low, up, (mean, std), *pr in zip(methods, *(last['host'][k] for k in keys)):
                ood_results[name][m] = {'epochs': epoch, 'n': scores.shape[1], 'mean': float(mean), 'std': float(std),
                                        'auc': float(auc), 'tpr': list(self.OOD_KEPT_TPR), 'fpr': [float(f) for f in fpr],
                                        'thresholds': [[float(a), float(b)] for a, b in zip(low, up)]}
                if with_pr and '-a-' not in m:                # a quantile row has no scalar score: no figures
                    ood_results[name][m].update(zip(ops.PR_FIGURES, (float(f) for f in pr[0])))
                if update_self_ood:
                    self.ood_results.setdefault(epoch, {}).setdefault(name, {})[m] = ood_results[name][m]
        if was_training:
            self.train()
        return ood_results

    # ------------------------------------------------------------------------------------ misclassification detection
    def _starred(self, names):
        """develop_starred_methods (utils/save_load/dictify.py:198-212) on a copy: the plain names in their order, then what
        each starred name expands to; a starred name without an entry in `methods_params` (softiws*) expands to nothing."""
        grids = dict(self.methods_params, **{score_rows.ODIN.prefix: self._odin_names()})
        plain = [m for m in names if not m.endswith('*')]
        return plain + [e for m in names if m.endswith('*') for e in grids.get(m[:-1], [])]

    def scod_rates(self, sample_dir=None, epoch='last', **kw):
        """SCOD figures of this saved job - selective classification in the presence of OOD data (reference tests/scod.py):
        {'fpr95', 'sr95', 'auroc', 'aust', 'auscodt'} from the `record-*.pth` files of `sample_dir` (default: the job's sample
        directory of `epoch`), with the job's training set as the in-distribution set and its type ('wim' for a WIMJob) as the
        model type.  Keywords (`r`, `g`, `weight`, lists of them, `curves`) and everything else: jvae_compat.scod.scod_rates."""
        from jvae_compat import scod
        return scod.job_scod_rates(self, sample_dir=sample_dir, epoch=epoch, **kw)

    def misclassification_detection_rates(self, predict_methods='all', misclass_methods='all', epoch='last', shown_tpr=0.95,
                                          from_where=('json', 'recorders'), print_result=False, update_self_results=True,
                                          outputs=None, recorder=None):
        """How well each misclassification score separates the correctly from the wrongly classified samples of the recorded test
        set, per prediction method (cvae.py:1913-2079): the ROC of score[correct] against score[missed] - AUC, FPR at the kept
        TPRs 0.90 .. 0.99 - and the precision tp / (tp + fp) at each kept threshold.  Stored, as the reference stores it, in
        `self.testing[epoch][predict_method][m] = {'n', 'epochs', 'sampling', 'tpr', 'fpr', 'auc', 'precision'}` (plain floats and
        lists, `save()` writes them to test.json) and, unlike the reference (which returns None), returned as
        {predict_method: {m: entry}}.

        The scores come from a `LossRecorder` (the all-class losses, `logits` as (C, N), `y_true`): the one passed as `recorder`,
        or `saved_dir/samples/<epoch:04d>/record-<training_parameters['set']>.pth` (`epoch='last'`: the largest epoch directory
        holding that file).  Nothing to do (None, said at debug level) without that file, without 'recorders' in `from_where`, or
        for a model type without misclassification methods.  The registry lookup of earlier results (`available_results`) is host
        plumbing outside this build, as for accuracy().  Starred names expand through `methods_params` (`odin*`: this model's
        grid); `softiws*` has no entry there and expands to nothing, as in the reference.  A name outside the model's table is an
        error; a method whose loss the recorder does not hold is skipped.

        Underneath, per prediction method: the score rows are computed on the device into ONE (M, N) buffer (csrc/misclass.hip,
        one launch per source tensor; `batch_dist_measures` for `iws` and the recorded `odin-*` rows), then ONE split by
        correctness, ONE ROC of all M rows (csrc/roc.hip), ONE confusion count, and ONE copy of the (M, 6K + 2) results to the
        host; n_correct is the only other value read back.  No (M, N) or (C, N) tensor goes to the host.

        Decided where the reference fails: a prediction method that gets every sample right - or none - is skipped with a
        warning (the reference dies in roc_curve); a row with a NaN score (`hyz` on a saturated softmax) is skipped with a warning
        naming it.  The reference's "n already there" guard reads `self.testing[epoch][predict_methods][m]` - the ARGUMENT, a
        list or 'all', so it never finds anything (cvae.py:2064); here it looks under the prediction method being processed.
        The P / R / FPR at `shown_tpr` are logged at debug level (and sent to `outputs` with `print_result`); NaN when no kept slot
        reaches `shown_tpr`.  Nothing stored depends on them.

        With `DETECTION_PR_METRICS` every entry also holds `MISCLASS_PR_KEYS`: 'aupr_correct' / 'aucpr_correct' (correct =
        positive), 'aupr_error' / 'aucpr_error' (missed = positive, score negated) and 'dete', from ONE `ops.pr_metrics` call on
        the two row sets of the split, in the same host copy."""
        def nothing(why):
            logging.debug('misclassification_detection_rates: nothing to do (%s)', why)

        if not self.misclass_methods:
            return nothing(f'no misclassification methods for type {self.type}')
        if not (from_where == 'all' or 'recorders' in from_where):
            return nothing("'recorders' is not in from_where")
        if recorder is None:
            from jvae_compat.recorders import LossRecorder
            fname = 'record-{}.pth'.format(self.training_parameters['set'])
            root = os.path.join(getattr(self, 'saved_dir', None) or '', 'samples')
            if epoch == 'last':
                found = [int(d) for d in (os.listdir(root) if os.path.isdir(root) else [])
                         if d.isdigit() and os.path.exists(os.path.join(root, d, fname))]
                if not found:
                    return nothing(f'no {fname} under {root}')
                epoch = max(found)
            path = os.path.join(root, '{:04d}'.format(int(epoch)), fname)
            if not os.path.exists(path):
                return nothing(f'no {path}')
            recorder = LossRecorder.load(path, map_location=self.device)
        elif epoch == 'last':
            epoch = self.trained
        epoch = int(epoch)

        chosen = {}
        for which, arg, table in (('predict', predict_methods, self.predict_methods), ('miss', misclass_methods, self.misclass_methods)):
            everything = self._starred(table)
            names = [arg] if isinstance(arg, str) else list(arg or [])
            names = everything if names and names[0] in ('all', 'default') else self._starred(names)
            for m in names:
                if m not in everything:
                    raise ValueError(f'{m}: not a {which} method of a {self.type} ({", ".join(table)})')
            chosen[which] = names

        tensors = {k: recorder[k].to(self.device) for k in recorder.keys()}
        _lib.ptr(tensors['y_true'])                                          # there is no CPU path
        logits_cn, y = tensors.pop('logits', None), tensors.pop('y_true')
        logits = None if logits_cn is None else logits_cn.T
        sources = dict(tensors, logits=logits)
        n = y.shape[0]
        rows_of = {m: score_rows.parse(m, score_rows.traits_of(self), misclass=True) for m in chosen['miss']}
        methods = [m for m in chosen['miss'] if sources.get(rows_of[m].source) is not None]
        skipped = [m for m in chosen['miss'] if m not in methods]
        if skipped:
            logging.debug('misclassification_detection_rates: not in the recorder: %s', ', '.join(skipped))
        sampling = self._latent_samplings['eval']
        with_pr = bool(self.DETECTION_PR_METRICS)
        results = {}
        if not methods:
            return results

        # the score rows do not depend on the prediction method: ONE (M, N) buffer, one launch per source tensor
        scores = torch.empty((len(methods), n), dtype=torch.float32, device=y.device)
        with torch.no_grad():
            score_rows.write_rows([rows_of[m] for m in methods], range(len(methods)), logits, tensors, scores,
                                  torch_rows=self.MISCLASS_TORCH_ROWS)
            kept = torch.tensor(self.OOD_KEPT_TPR, dtype=torch.float64, device=y.device)
            sink = outputs if print_result and outputs is not None and hasattr(outputs, 'write') else None
            for pm in chosen['predict']:
                correct = self.predict_after_evaluate(logits, tensors, method=pm) == y
                try:
                    r = ops.misclass_rates(scores, correct, kept, pr=True) if with_pr else ops.misclass_rates(scores, correct, kept)
                except ValueError as err:
                    logging.warning('misclassification_detection_rates: prediction method %s skipped: %s', pm, err)
                    continue
                n_correct = r['n_correct']
                acc = n_correct / n
                host = ops.read_back({k: r[k] for k in ('auc', 'fpr', 'tpr', 'tp', 'fp', 'status') + ('pr',) * with_pr})
                logging.debug('Acc. for method %s: (%5.2f) ****', pm, 100 * acc)
                results[pm] = {}
                best = (None, 0.)
                for m, auc, fpr, tpr, tp, fp, status, *pr in zip(methods, *host.values()):
                    if int(status):
                        logging.warning('misclassification_detection_rates: %s-%s skipped: NaN score', pm, m)
                        continue
                    with np.errstate(invalid='ignore', divide='ignore'):
                        precision = tp / (tp + fp)                          # 0 / 0 = NaN, as numpy gives the reference
                    at = np.where(tpr >= shown_tpr)[0]                      # fpr_at_tpr (utils/roc_curves.py:8-27)
                    p95, r95, f95 = ((precision[at.min()], tp[at.min()] / n_correct, fp[at.min()] / (n - n_correct))
                                     if len(at) else (np.nan, np.nan, np.nan))
                    if p95 > best[1]:
                        best = (m, p95)
                    line = '{:16}: \tP={:5.2f} ({:+4.1f}) R={:5.2f} FPR={:5.2f}'.format(m, 100 * p95, 100 * (p95 - acc), 100 * r95,
                                                                                       100 * f95)
                    logging.debug(line)
                    if sink is not None:
                        sink.write(line + '\n')
                    entry = {'n': n, 'epochs': epoch, 'sampling': sampling, 'tpr': [float(t) for t in tpr],
                             'fpr': [float(f) for f in fpr], 'auc': float(auc), 'precision': [float(p) for p in precision]}
                    if with_pr:
                        entry.update(zip(self.MISCLASS_PR_KEYS, (float(f) for f in pr[0])))
                    results[pm][m] = entry
                    n_already = self.testing.get(epoch, {}).get(pm, {}).get(m, {'n': 0})['n']
                    if update_self_results and n >= n_already:
                        slot = self.testing.setdefault(epoch, {})
                        if pm not in slot:
                            slot[pm] = {'n': n, 'epochs': epoch, 'sampling': sampling, 'accuracy': float(acc)}
                        slot[pm][m] = entry
                logging.debug('best method for %s: %s (P=%.2f)', pm, best[0], 100 * best[1])
        return results
