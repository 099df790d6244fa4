"""MI355X-native joint / class-conditional VAE: drop-in for the reference's `cvae.ClassificationVariationalNetwork`.

Scope: the per-batch training step of the reference (cvae.py:2424-2479) —
features -> encoder -> (mu, log sigma^2) -> reparameterised z -> decoder / imager -> ELBO terms -> backward ->
clip -> Adam — executed by hand-written gfx950 HIP kernels (libjvae_hip.so) behind the same Python API:

    ClassificationVariationalNetwork(input_shape, num_labels, type, ..., sigma, optimizer, ...)   cvae.py:135-167
    .forward(x, y=None, x_features=None, z_output=True, sampling_epsilon_norm_out=False, sigma_out=False)  :426-521
    .evaluate(x, y, batch, current_measures, with_beta, kl_var_weighting, gamma_weighting, z_output)       :523-917
    .train_model(...)   (hot loop :2424-2479, test phase; the OOD phase is an opt-in: TRAIN_OOD_PHASE)       :2081-2547
    .train() / .to() / .save() / .load() / .latent_sampling / .device / .nparams

What is NOT rebuilt here (raises NotImplementedError when asked for): (cvae / xvae / vae / vib are complete, jvae: training and labelled evaluation only); resnet
feature stacks (torchvision); a per-dimension sigma (the reference fails on it too).  A categorical (256-level) decoder,
its label-free evaluation included, pooling / up-sampling layer tokens, SGD,
the `y=None` all-class evaluation with its OOD scores, the WIM fine-tuning step and the evaluation methods accuracy(),
ood_detection_rates() and misclassification_detection_rates() are built (module/scoring.py), and so is generate():
images decoded from draws of the prior (module/sample.py builds the reference's grids of them).
latent_posterior(x, y) is the encode-only pass (mu, log_var bit for bit evaluate()'s, nothing decoded) under module.sample.zsample();
the sample recorders of ood_detection_rates() write the reference's samples-<set>.pth.
fit_latent_bank() keeps the posterior means of a training set on the device and knn_scores() / the `knn-<k>` OOD rows (an opt-in,
OOD_KNN_METHODS; module/scoring.py, csrc/knn.hip) score a sample by its distance to them: no counterpart in the reference (section 7p).
fit_latent_gaussians() fits class Gaussians with one shared covariance on that bank and maha_scores() / the `maha`, `maha-rel` OOD
rows (an opt-in, OOD_MAHA_METHODS; module/scoring.py, csrc/maha.hip) are the Mahalanobis distances to them (section 7q).
fit_score_bank() keeps the statistics DOSE_STATS of a training set and dose_scores() / the `dose*` OOD rows (an opt-in,
OOD_DOSE_METHODS; module/scoring.py, csrc/dose.hip) are their kernel density estimates: how TYPICAL a sample's scores are (section 7s).
input_complexity() is the length of a batch's images under a lossless coder, one launch of csrc/ic.hip, and the `ic-bits`, `ic-elbo`,
`ic-iws` OOD rows (an opt-in, OOD_IC_METHODS; module/scoring.py) take it out of the likelihood (Serra et al. 2020; section 7r).
ssim_scores() / ssim_map() and the `ssim`, `ssim-mu`, `ssim-cs` OOD rows (an opt-in, OOD_SSIM_METHODS; module/scoring.py) are the
structural similarity of a batch to its reconstructions, one launch of csrc/ssim.hip on the x_reco of the scoring pass (section 7t).
Named data sets ('cifar10-3', 'mnist32r', 'svhn', ...: jvae_compat/torch_load.py, device-resident sets whose batches are one
launch of csrc/imageset.hip) are an opt-in, `DATA_ROOT` (class attribute, settable per instance: the torchvision-style directory
of the raw files); None, the default, keeps every refusal of a name as it was.
TRAIN_OBJECTIVE = 'iwae' (class attribute, settable per instance; default 'elbo') trains on the importance-weighted bound of Burda et
al. instead of the ELBO: the labelled training-mode evaluate() forms total = -bound from the draws, reconstruction rows and prior it
already holds (ops.iw_bound, csrc/iwae.hip: weights, bound, effective sample size and every direct gradient fused), reports `iwae` and
`ess` beside the usual losses, and refuses by name what it does not cover; iw_bound(x, y, samples) is the matching evaluation entry,
the proper log (1/L) sum_l w_l over slabs of draws - not the reference's `iws`.
TRAIN_OBJECTIVE = 'tcvae' trains on the beta-TCVAE split of Chen et al.: total = cross_x + b (alpha mi + beta_tc tc + gamma dwkl), the
three terms elbo_decomposition() measures, here estimated over the batch's own posteriors with their gradients (ops.tc_objective,
csrc/tcvae.hip); TC_WEIGHTS = (alpha, beta_tc, gamma), default (1, 6, 1), TC_DATASET_SIZE the training samples behind the batch
(train_model() fills it); `mi`, `tc` and `dwkl` are reported beside the usual losses.
SEMI_SUPERVISED = True (class attribute, settable per instance; default False) lets a training batch carry unlabelled rows: a
negative label gives that row the class-marginal KL U = -log sum_c pi_c exp(-KL_c) (ops.class_marginal_kl, csrc/semisup.hip),
labelled rows are untouched; UNLABELLED_CLASS_WEIGHTS sets pi, class_marginal(x) returns (U, q(y|x)) in evaluation, and what
is not covered is refused by name.
TRAIN_OBJECTIVE = 'mmd' trains on an MMD-regularised bound (InfoVAE, Zhao et al.; WAE-MMD, Tolstikhin et al.): total = cross_x +
b kl_weight kl + mmd_weight m, m the per-row terms of the unbiased MMD^2 between the step's draws and draws of the sample's own
class prior (ops.mmd_objective, csrc/mmd.hip); MMD_WEIGHTS = (kl_weight, mmd_weight), default (1, 1000), MMD_KERNEL = (kind,
scales), MMD_JOINT; `mmd` is reported beside the usual losses and prior_mmd(codes, y) is the evaluation entry.
There is no CPU path: calling forward/evaluate with CPU tensors raises.
"""
import contextlib
import json
import logging
import math
import os
import sys
import time

import numpy as np
import torch
from torch import nn

from jvae_hip import ops
from jvae_hip import lib as _lib
from module import score_rows
from module.scoring import ScoringMixin
from module.optimizers import Optimizer
from module.losses import x_loss, mse_loss, categorical_loss  # noqa: F401  (import surface of the reference)
from module.vae_layers import Encoder, Classifier, Sigma, build_de_conv_layers, find_input_shape
from module.vae_layers import onehot_encoding, activation_layers
from module.vae_layers.layers import HipLinear, HipDropout, DenseStack, draw_epsilon

DEFAULT_ACTIVATION = 'relu'
DEFAULT_OUTPUT_ACTIVATION = 'linear'
DEFAULT_LATENT_SAMPLING = 100
VERSION = 2.
LOG2PI = math.log(2 * math.pi)


class _LazyDict(dict):
    """A dict whose content is produced by `_fill()` the first time anything reads it."""

    def _fill(self):
        raise NotImplementedError

    def copy(self):
        self._fill()
        return dict(self)


def _lazy(name):
    def method(self, *a, **k):
        self._fill()
        return getattr(dict, name)(self, *a, **k)
    method.__name__ = name
    return method


for _n in ('__getitem__', 'get', '__contains__', '__iter__', '__len__', 'keys', 'values', 'items', '__repr__', '__eq__'):
    setattr(_LazyDict, _n, _lazy(_n))


# The 16-float block ops.measures writes (csrc/loss.hip): name -> index, the ONLY Python copy of that layout.  A captured
# loop keeps the block at the head of a 40-float state block that one copy reads back (_capture_buffers).
MEASURE_INDEX = {'sigma': 0, 'xpow': 10, 'mse': 11, 'rmse': 12, 'dB': 13, 'zdist': 14, 'var_kl': 15}
DICTIONARY_MEASURE_INDEX = {'ld-norm': 6, 'imut-zy': 7, 'd-mind': 8}     # conditional priors only
MEASURES_NONFINITE = 9                          # non-zero: the optimiser's flag was up when the block was written
MEASURES_LEN, STATE_LEN = 16, 40
STATE_RUN, STATE_SUMS = slice(0, 16), slice(16, 32)     # the measures; the epoch sums of the batch-mean losses
STATE_FLAG = 32                                 # the optimiser's non-finite flag itself (an int32 in place)


def decode_measures(h, has_dictionary, only=None):
    """The measures dict of a block read back as a list of floats; `only`: the names to keep."""
    m = {k: h[i] for k, i in MEASURE_INDEX.items()}
    if has_dictionary:
        m.update((k, h[i]) for k, i in DICTIONARY_MEASURE_INDEX.items())
    return m if only is None else {k: v for k, v in m.items() if k in only}


def measures_nonfinite(h):
    """Did a parameter become NaN / Inf?  `h`: a measures block or a captured loop's whole state block, read back."""
    return h[MEASURES_NONFINITE] != 0 or (len(h) > STATE_FLAG and h[STATE_FLAG] != 0)


class Measures(_LazyDict):
    """`total_measures` of evaluate(): a dict of Python floats (rmse, dB, sigma, ...) exactly as in the reference, but
    materialised LAZILY: the 16 scalars sit in one device buffer (running means included, continued on the device from
    batch to batch) that is copied to pinned host memory asynchronously; the first time any entry is read the dict
    waits for that copy.  A training loop that only threads `measures` into the next evaluate() never synchronises."""

    def __init__(self, dev, has_dictionary, on_nan, from_main=False, only=None):
        super().__init__()
        self._only = only                                # type 'vib': ('sigma', 'zdist', 'var_kl') - nothing is reconstructed
        self._dev = dev
        self._host = torch.empty(MEASURES_LEN, dtype=torch.float32, pin_memory=True)
        side = _lib.side_stream(dev.device)          # `dev` was produced on the side stream (logging is off the critical path)
        if from_main:                                # ... or by a graph replay on the current stream
            side.wait_stream(torch.cuda.current_stream(dev.device))
        with torch.cuda.stream(side):
            self._host.copy_(dev, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record(side)
        self._has_dictionary = has_dictionary
        self._on_nan = on_nan
        self._ready = False

    def _fill(self):
        if self._ready:
            return
        self._ready = True
        self._event.synchronize()
        h = self._host.tolist()
        if measures_nonfinite(h):
            self._on_nan()
        dict.update(self, decode_measures(h, self._has_dictionary, self._only))


class _LazySigmaParams(_LazyDict):
    """training_parameters['sigma'] (Sigma.params with the current rms value) without a device read-back per batch."""

    def __init__(self, sigma, measures):
        super().__init__()
        self._s, self._m, self._done = sigma, measures, False

    def _fill(self):
        if not self._done:
            self._done = True
            dict.update(self, self._s.host_params(self._m['sigma']))


def _mean_over_draws(logits):
    """y_est = logits[1:].mean(0) (cvae.py:910-917): with ONE latent draw (training: L = 1) that mean is the row itself -
    returned as a view, bit-identical, without a reduction kernel on the step's main stream."""
    return logits[1] if logits.shape[0] == 2 else logits[1:].mean(0)


def _restores_tc_dataset_size(train_model):
    """train_model() fills TC_DATASET_SIZE from the set it trains on when the attribute is None: whatever way the call ends, the
    instance gets back what it had (an instance value, or none of its own)."""
    import functools

    @functools.wraps(train_model)
    def wrapper(self, *a, **kw):
        own = 'TC_DATASET_SIZE' in self.__dict__
        before = self.__dict__.get('TC_DATASET_SIZE')
        try:
            return train_model(self, *a, **kw)
        finally:
            if own:
                self.TC_DATASET_SIZE = before
            else:
                self.__dict__.pop('TC_DATASET_SIZE', None)
    return wrapper


def _grad_nan_exit():
    print('GRAD NAN')              # cvae.py:2454-2457; detected by the Adam kernel: train_step() checks the flag of the previous update
                                   # before every backward (as the reference's scan does), lazily-read measures check it as well
    sys.exit(1)


class CapturedStep:
    """A training step captured into HIP graphs: what graph_train_step() and capture_train_step() return.  `step(x, y)` copies
    the batch into the static buffers `x` / `y`, replays `graphs` in order - with `between()` in front of every graph after
    the first (data parallel: the eager gradient all-reduce) - and notes the optimiser step on the host.  A graph is any
    object with `.replay()`; `graph` is the graph, or the tuple of them when there is more than one.  `losses`: the graphs'
    own loss rows, overwritten by the next replay.  `constants`: what the graphs read that nothing else is bound to keep.
    `measures`: the 16-float device block the graphs write, which a call wraps into a fresh Measures and returns beside the
    losses (graph_train_step); None: a call returns the losses alone and the measures continue on the device, in `buffers`
    (capture_train_step, which also fills in `epsilon` and `key`; see there)."""

    def __init__(self, net, x, y, graphs, between=None, losses=None, measures=None, has_dictionary=False, buffers=None,
                 constants=()):
        self.net, self.x, self.y, self.graphs, self.between = net, x, y, list(graphs), between
        self.graph = self.graphs[0] if len(self.graphs) == 1 else tuple(self.graphs)
        self.losses, self.keys, self.measures, self.has_dictionary = losses, list(losses or ()), measures, has_dictionary
        self.buffers, self.constants, self.epsilon, self.key = buffers, constants, None, None

    def __call__(self, xb, yb):
        self.x.copy_(xb, non_blocking=True)
        self.y.copy_(yb, non_blocking=True)
        self.graphs[0].replay()
        for g in self.graphs[1:]:
            self.between()
            g.replay()
        self.net.optimizer.note_replayed_step()
        if self.measures is None:
            return self.losses
        return self.losses, Measures(self.measures, self.has_dictionary, _grad_nan_exit, from_main=True)

    def set_weights(self, kl_w, gamma_w):
        """The two warm-up weights the captured kernels read from the device: kl_var_weighting and the cross_y weight."""
        cw = gamma_w * self.net.gamma if self.net.y_is_decoded else 0.
        self.buffers['weights'].copy_(torch.tensor([float(kl_w), float(cw or 0.)], dtype=torch.float32))

    def seed_measures(self, prev, batch):
        """Continue after `batch` eager batches whose last measures buffer (16 device floats) is `prev`."""
        self.buffers['run'].copy_(prev)
        self.buffers['counter'].fill_(int(batch))

    def reset_epoch(self):
        self.buffers['counter'].zero_()
        self.buffers['sums'].zero_()


class ClassificationVariationalNetwork(ScoringMixin, nn.Module):
    r"""X -- features -- encoder -- Z -- decoder -- imager -- X^   with a class-conditional prior p(z|y)
    (and a classifier head on z when gamma > 0)."""

    # the tables of cvae.py:82-112 for the two types built here
    loss_components_per_type = {'cvae': ('cross_x', 'kl', 'total', 'zdist', 'var_kl', 'dzdist', 'iws',
                                         'sigma', 'wmse', 'z_logdet', 'z_tr_inv_cov'),
                                'vae': ('cross_x', 'kl', 'zdist', 'var_kl', 'total', 'iws'),
                                'jvae': ('cross_x', 'kl', 'cross_y', 'total'),
                                'xvae': ('cross_x', 'kl', 'total', 'zdist', 'iws'),
                                'vib': ('cross_y', 'kl', 'total')}
    predict_methods_per_type = {'cvae': ['iws', 'closest'], 'vae': [], 'jvae': ['loss', 'esty'], 'xvae': ['loss', 'closest'],
                                'vib': ['esty']}
    metrics_per_type = {'cvae': ['rmse', 'dB', 'd-mind', 'ld-norm', 'sigma'], 'vae': ['rmse', 'dB', 'sigma'],
                        'jvae': ['rmse', 'dB', 'sigma'], 'xvae': ['rmse', 'dB', 'zdist', 'd-mind', 'ld-norm', 'sigma'],
                        'vib': ['sigma']}
    ood_methods_per_type = {'cvae': ['iws-2s', 'iws-a-1-1', 'iws-a-4-1', 'iws', 'mse', 'elbo', 'soft',
                                     'elbo-2s', 'elbo-a-1-1', 'elbo-a-4-1', 'zdist'],
                            'vae': ['iws', 'iws-2s', 'iws-a-1-1', 'iws-a-4-1', 'elbo', 'elbo-2s', 'elbo-a-1-1',
                                    'elbo-a-4-1', 'zdist'],
                            'jvae': ['max', 'sum', 'std'], 'xvae': ['max', 'mean', 'std'],
                            'vib': ['odin*', 'baseline', 'logits']}
    misclass_methods_per_type = {'cvae': ['softkl*', 'iws', 'softiws*', 'kl', 'max', 'zdist', 'softzdist*',
                                          'baseline*', 'hyz'],
                                 'vae': [], 'jvae': [], 'xvae': [], 'vib': ['odin*', 'baseline', 'logits', 'hyz']}

    # cvae.py:120-133: the ODIN grid (10 temperatures x 21 perturbation sizes) and what a starred method name expands to; an
    # instance may override the two lists (its `odin*` rows then follow its own lists)
    ODIN_TEMPS = [m * 10 ** i for i in (0, 1, 2) for m in (1, 2, 5)] + [1000]
    ODIN_EPS = [k / 20 * 0.004 for k in range(21)]
    methods_params = {'softkl': [], 'softzdist': [], 'baseline': [], score_rows.ODIN.prefix: []}
    for _T in ODIN_TEMPS:
        for _k in ('softkl', 'softzdist', 'baseline'):
            methods_params[_k].append('{}-{:.0f}'.format(_k, _T))
        for _e in ODIN_EPS:
            methods_params[score_rows.ODIN.prefix].append(score_rows.odin_name(_T, _e))
    del _T, _k, _e

    # train_model(): run every full-size batch of the train phase as a replay of ONE captured HIP graph (zero_grad ... Adam,
    # the epoch's loss sums and running measures included) instead of the eager train_step().  Opt-in; an instance may set
    # it.  What stays eager, and the late NaN exit: INTEGRATION.md ("The captured training loop").
    TRAIN_CAPTURED = False
    # the objective of the labelled training-mode evaluate(): 'elbo' (the reference's, with the analytic KL) or 'iwae' (the
    # importance-weighted bound over the step's L draws, ops.iw_bound).  Opt-in; an instance may set it.  Evaluation mode is
    # never affected.  What 'iwae' refuses: _check_iwae_objective().
    TRAIN_OBJECTIVE = 'elbo'
    # 'tcvae' (Chen et al. 2018): the KL of the loss is replaced by alpha mi + beta_tc tc + gamma dwkl, the three terms of
    # elbo_decomposition() estimated over the batch's own posteriors (ops.tc_objective).  TC_WEIGHTS = (alpha, beta_tc, gamma).
    # TC_DATASET_SIZE: the training samples behind the batch's sets - None: the batch is the set (train_model() fills it from
    # the set it trains on and restores it), an int for a single prior, C class counts for a conditional one.  It moves the
    # three reported terms by constants and enters no gradient.  What 'tcvae' refuses: _check_tc_objective().
    TC_WEIGHTS = (1., 6., 1.)
    TC_DATASET_SIZE = None
    # 'mmd' (InfoVAE / WAE-MMD): total = cross_x + b kl_weight kl + mmd_weight m (+ cw cross_y), m the per-row terms of the unbiased
    # MMD^2 between the step's draws and as many draws of each sample's own class prior (ops.mmd_objective).  MMD_WEIGHTS =
    # (kl_weight, mmd_weight): (1, 1000) is InfoVAE's alpha = 0, lambda = 1000 (not tuned on this model), (0, lambda) is WAE-MMD.
    # MMD_KERNEL = (kind, scales): 'imq' or 'rbf', scales a tuple of at most 8 positive floats or None (2 K s for WAE's seven s).
    # MMD_JOINT: pairs are counted inside a class only (the MMD of the joint laws of (z, y)); False matches the two mixtures.
    # What 'mmd' refuses: _check_mmd_objective().
    MMD_WEIGHTS = (1., 1000.)
    MMD_KERNEL = ('imq', None)
    MMD_JOINT = True
    # semi-supervised training: a NEGATIVE label of the labelled training-mode evaluate() means "no label".  Such a row's KL is
    # the class-marginal bound U = -log sum_c pi_c exp(-KL_c) (ops.class_marginal_kl) instead of the KL to
    # ONE class; labelled rows are untouched.  Opt-in; an instance may set it.  UNLABELLED_CLASS_WEIGHTS: None (uniform pi) or C
    # positive numbers, normalised once.  What it refuses: _check_semi_supervised().
    SEMI_SUPERVISED = False
    UNLABELLED_CLASS_WEIGHTS = None
    # train_model(): run the reference's OOD phase (ood_detection_rates on `oodsets` every `ood_detection_every` epochs and once
    # after the loop, cvae.py:2309-2336,2513-2526).  Opt-in; an instance may set it.  Off: one warning, the phase is skipped.
    TRAIN_OOD_PHASE = False
    # full-size eager batches in front of every capture (allocations, the optimiser's flat buffers, lazy initialisations):
    # they are real batches of the epoch run through train_step() - a capture costs no extra optimiser step
    CAPTURE_WARMUP_BATCHES = 2
    # test hook: when set, train_model() calls it after every batch, on both paths, as hook(epoch, i, x, y, eps, losses) with
    # the loop's own tensors (captured path: the graph's buffers, overwritten by the next replay - clone what you keep;
    # eps: the (L, N, K) noise encode() returned).  It exists so that tests can replay the very batches of a run through
    # train_step(); it is not part of the reference's interface.
    _train_batch_hook = None
    _captures_built = 0             # how many captured steps this model has built (capture_train_step)

    def __init__(self, input_shape, num_labels, type='cvae', y_is_coded=False, output_distribution='gaussian',
                 job_number=0, features=None, pretrained_features=None, batch_norm=False, dropout=False,
                 encoder=[36], latent_dim=32, prior={}, beta=1., gamma=0., decoder=[36], upsampler=None,
                 pretrained_upsampler=None, classifier=[36], name='joint-vae', activation=DEFAULT_ACTIVATION,
                 latent_sampling=DEFAULT_LATENT_SAMPLING, test_latent_sampling=None,
                 encoder_forced_variance=False, output_activation=DEFAULT_OUTPUT_ACTIVATION, sigma={'value': 1},
                 optimizer={}, shadow=False, representation='rgb', version=VERSION, *args, **kw):
        super().__init__(*args, **kw)
        assert type in ('jvae', 'cvae', 'xvae', 'vib', 'vae')
        assert not (y_is_coded and type in ('vib', 'vae'))
        assert output_distribution in ('gaussian', 'categorical')
        assert not upsampler or features, 'no upsampler without features'

        self.name = name
        self.job_number = job_number
        self.type = type
        self.is_cvae, self.is_jvae, self.is_vib, self.is_vae, self.is_xvae = (type == 'cvae', type == 'jvae', type == 'vib',
                                                                              type == 'vae', type == 'xvae')
        self.loss_components = self.loss_components_per_type[type]
        self.metrics = self.metrics_per_type[type]
        self.predict_methods = list(self.predict_methods_per_type[type])
        self.ood_methods = list(self.ood_methods_per_type[type])
        self.misclass_methods = list(self.misclass_methods_per_type[type])
        self.y_is_coded = y_is_coded
        self.y_is_decoded = gamma if (self.is_cvae or self.is_vae) else True      # cvae.py:196-199
        self.x_is_generated = not self.is_vib                               # cvae.py:201: 'vib' has no decoder / imager
        self.output_distribution = output_distribution if self.x_is_generated else None
        self.losses_might_be_computed_for_each_class = not self.is_vae and not self.is_vib      # cvae.py:205
        if not self.x_is_generated:
            decoder, upsampler = [], None                                   # cvae.py:222-224

        if self.y_is_decoded:
            self.classifier_type = 'linear'
            if classifier and isinstance(classifier[0], str):
                assert classifier[0] in ('softmax',)
                self.classifier_type = classifier[0]
            if 'esty' not in self.predict_methods:
                self.predict_methods.append('esty')
            if 'cross_y' not in self.loss_components:
                self.loss_components += ('cross_y',)
        else:
            self.classifier_type = None
            classifier = []

        bn_enc = bool(features) and batch_norm in ('encoder', 'both')
        bn_dec = bool(features) and batch_norm == 'both'
        if not features:
            batch_norm = False

        if features:
            self.features = build_de_conv_layers(input_shape, features, activation=activation, batch_norm=bn_enc,
                                                 pretrained_dict=pretrained_features)
            enc_in = self.features.output_shape
        else:
            self.features = None
            enc_in = input_shape

        self.trained = 0
        if isinstance(sigma, Sigma):
            self.sigma = sigma
        elif isinstance(sigma, dict):
            self.sigma = Sigma(**sigma)
        else:
            self.sigma = Sigma(value=sigma)
        if self.sigma.per_dim:
            # The reference itself cannot run one: cvae.py:649 divides (L,N,C,H,W) by a (C,H,W) sigma but cvae.py:789 adds
            # its (C,H,W) log to the (N,) wmse - `RuntimeError: The size of tensor a (N) must match ...` for a learned and for
            # a coded per-dimension sigma alike (probed on the reference in the build container).  Same outcome here, earlier.
            raise NotImplementedError('per-dimension sigma: the reference fails on it as well (shape mismatch at '
                                      'cvae.py:789); scalar fixed / decayed / learned / rmse / coded sigma are built')

        test_latent_sampling = test_latent_sampling or latent_sampling
        self.beta = beta
        self.gamma = gamma if self.y_is_decoded else None
        prior = dict(prior)
        if self.is_cvae or self.is_xvae:          # cvae.py:274-275: one prior component per class; 'vae' / 'jvae': a single one
            prior['num_priors'] = num_labels
        self.encoder = Encoder(enc_in, num_labels, intermediate_dims=encoder, latent_dim=latent_dim,
                               y_is_coded=self.y_is_coded, dropout=dropout,
                               sigma_output_dim=self.sigma.output_dim if self.sigma.coded else 0,        # cvae.py:283
                               forced_variance=encoder_forced_variance, sampling_size=latent_sampling, prior=prior,
                               activation=activation, sampling=latent_sampling > 1 or beta > 0)

        dense, width = [], latent_dim
        shared_act = activation_layers[activation]()
        for d in decoder:
            dense += [HipLinear(width, d), shared_act]
            if dropout:
                dense.append(HipDropout(p=dropout))
            width = d
        if not self.x_is_generated:
            pass                                  # cvae.py:291: no `decoder` / `imager` modules (nor state_dict keys) at all
        elif upsampler:
            self.decoder = DenseStack(*dense)
            hw = find_input_shape(upsampler, input_shape[1:])
            cells = hw[0] * hw[1]
            assert not width % cells, 'Could not go from {} to *, {} {}'.format(width, *hw)
            self.imager = build_de_conv_layers((width // cells, *hw), upsampler, batch_norm=bn_dec,
                                               activation=activation, output_activation=output_activation,
                                               output_distribution=self.output_distribution,
                                               pretrained_dict=pretrained_upsampler, where='output')
        else:
            self.decoder = DenseStack(*dense)
            upsampler = None
            self.imager = DenseStack(HipLinear(width, int(np.prod(input_shape))),
                                     activation_layers[output_activation]())
            self.imager.input_shape = (width,)

        if self.classifier_type in ('linear', None):
            self.classifier = Classifier(latent_dim, num_labels, classifier, activation=activation)

        self.input_shape = tuple(input_shape)
        self.num_labels = num_labels
        self.input_dim = len(input_shape)
        self.batch_norm = batch_norm
        self.dropout = dropout
        self._sizes_of_layers = [input_shape, num_labels, encoder, latent_dim, decoder, upsampler, classifier]
        self.architecture = {'input_shape': input_shape, 'num_labels': num_labels,
                             'output_distribution': self.output_distribution, 'type': type,
                             'representation': representation, 'encoder': encoder, 'batch_norm': batch_norm,
                             'dropout': dropout, 'activation': activation,
                             'encoder_forced_variance': self.encoder.forced_variance, 'latent_dim': latent_dim,
                             'test_latent_sampling': test_latent_sampling, 'prior': self.encoder.prior.params,
                             'decoder': decoder, 'upsampler': upsampler, 'classifier': classifier,
                             'output_activation': output_activation, 'version': VERSION}
        if features:
            self.architecture['features'] = self.features.name
        linear_clf = self.classifier_type == 'linear'
        self.depth = (len(encoder) + len(decoder) + len(classifier)) if linear_clf else 0
        self.width = (sum(encoder) + sum(decoder) + sum(classifier)) if linear_clf else 0

        self.training_parameters = {'sigma': self.sigma.params, 'beta': self.beta, 'gamma': self.gamma,
                                    'latent_sampling': latent_sampling, 'set': None, 'data_augmentation': [],
                                    'pretrained_features': getattr(pretrained_features, 'name', None),
                                    'pretrained_upsampler': getattr(pretrained_upsampler, 'name', None),
                                    'epochs': 0, 'batch_size': None, 'fine_tuning': []}
        self.testing = {0: {m: {'n': 0, 'epochs': 0, 'accuracy': 0} for m in self.predict_methods}}
        self.ood_results = {}
        self.optimizer = Optimizer(self.parameters(), **optimizer)
        if self.x_is_generated:
            self.optimizer.set_early_bucket(list(self.imager.parameters()) + list(self.decoder.parameters()))
        self.training_parameters['optimizer'] = self.optimizer.params
        self.train_history = {'epochs': 0}

        self.latent_dim = latent_dim
        self._latent_samplings = {'train': latent_sampling, 'eval': test_latent_sampling}
        self.latent_sampling = latent_sampling
        self.encoder_layer_sizes, self.decoder_layer_sizes, self.classifier_layer_sizes = encoder, decoder, classifier
        self.upsampler = upsampler
        self.activation = activation
        self.output_activation = output_activation
        self.z_output = False
        self._host_cache = {}
        self.eval()

    # ------------------------------------------------------------------------------------ module state
    def train(self, *a, **k):
        super().train(*a, **k)
        self.latent_sampling = self._latent_samplings['train' if self.training else 'eval']
        return self

    @property
    def latent_sampling(self):
        return self._latent_sampling

    @latent_sampling.setter
    def latent_sampling(self, v):
        self._latent_sampling = v
        self.encoder.sampling_size = v

    @property
    def device(self):
        return next(self.parameters()).device

    @device.setter
    def device(self, d):
        self.to(d)

    def to(self, d):
        super().to(d)
        self.optimizer.to(d)
        return self

    @property
    def nparams(self):
        return sum(p.nelement() for p in self.parameters())

    def set_distributed(self, world_size, process_group=None, seed_offset=True):
        """Data-parallel replica set-up (no counterpart in the single-process reference): rank 0's
        parameters, BatchNorm buffers and optimiser state are broadcast to every rank (replicas no longer rely on identical
        seeding), the gradient exchange is switched on, and - seed_offset - the device generator that draws the
        reparameterisation noise is re-seeded per rank so that ranks draw DIFFERENT epsilon (and dropout masks)."""
        import torch.distributed as dist
        world_size = int(world_size)
        if world_size > 1 and dist.is_available() and dist.is_initialized():
            with torch.no_grad():
                for t in self.state_dict().values():
                    if t.is_cuda and dist.get_backend(process_group) != 'nccl':
                        h = t.cpu()
                        dist.broadcast(h, 0, group=process_group)
                        t.copy_(h)
                    else:
                        dist.broadcast(t, 0, group=process_group)
            if seed_offset:
                rank = dist.get_rank(process_group)
                base = torch.initial_seed()
                if torch.cuda.is_available():
                    torch.cuda.manual_seed(base + 7919 * (rank + 1))
        self.optimizer.set_distributed(world_size, process_group)
        return self

    def set_sync_batchnorm(self, world_size, process_group=None):
        """Data-parallel option: BatchNorm statistics over ALL ranks, i.e. exactly what the single-process
        reference computes on the global batch (default: per-rank statistics, as DistributedDataParallel does)."""
        from module.vae_layers.conv import HipBatchNorm2d
        for m in self.modules():
            if isinstance(m, HipBatchNorm2d):
                m.sync_world, m.sync_group = int(world_size), process_group
        return self

    def set_compute_dtype(self, dtype):
        """'fp32' (the reference's arithmetic; default) or 'bf16' (config 5 of BASELINE.json): bf16 activations between the
        layers of the conv stacks and bf16 matrix-core convolutions from the fp32 master weights; BatchNorm statistics,
        the dense heads, the latent / loss math, gradients of parameters and Adam stay fp32.  Native bf16 layers: 5x5 and 3x3
        padding-1 convolutions on maps of 4x4 and larger (conv32*, deconv32*, vgg*, ivgg*) and the M / A / U tokens; the
        others (3x3 padding-0 / 7x7 / 8x8 heads, 3x3 layers on 2x2 / 1x1 maps) run on the fp32 kernels between two conversions."""
        from module.vae_layers.conv import HipConvStack
        if dtype not in ('fp32', 'bf16'):
            raise ValueError(dtype)
        if dtype == 'bf16' and self.activation == 'leaky':
            raise NotImplementedError("the bf16 mode has ReLU kernels only: activation='leaky' (config.ini:113) trains in fp32")
        for m in self.modules():
            if isinstance(m, HipConvStack):
                m.compute_dtype = dtype
        self.compute_dtype = dtype
        return self

    @property
    def max_batch_sizes(self):
        """The reference hard-wires {'train': 32, 'test': 32} (cvae.py:1145-1147) after a halving search
        (cvae.py:1087-1143).  Here the bounds follow from the tensors themselves (powers of two, as the search returns):
        train - the decoder batch (L+1)*N times the widest activation stays below 2^31 elements (one launch chain, every
        activation kept for backward: ~3 MB per image of config 2, 50 GB at the bound); test - the label-free evaluation
        decodes in slabs (`_decode`), so only the returned reconstruction (L_test+1, N, ...) and, for a class-conditional prior, the
        (L_test, C, N, K) latents scored under every class must stay below 2^31 elements."""
        def pow2_below(v):
            v = max(int(v), 1)
            return 1 << (v.bit_length() - 1)
        lim = (1 << 31) - 1
        if not self.x_is_generated:
            return {'train': 1 << 16, 'test': 1 << 16}
        wide = self._widest_decoder_activation()
        reco = int(np.prod(self._reco_shape()))
        train = pow2_below(lim // ((self._latent_samplings['train'] + 1) * wide))
        test = pow2_below(lim // ((self._latent_samplings['eval'] + 1) * reco))
        if self.encoder.prior.conditional:
            # the importance weights of the label-free evaluation score every draw under every class: (L, C, N, K) latents
            # go through the prior's Mahalanobis kernel as ONE tensor (cvae.py:793-873)
            test = min(test, pow2_below(lim // (max(self._latent_samplings['eval'], 1) * self.num_labels * self.latent_dim)))
        return {'train': min(train, 1 << 16), 'test': min(test, 1 << 16)}

    # ------------------------------------------------------------------------------------ forward
    def _features_of(self, x):
        if not self.features:
            return x
        lead = (1,) if x.dim() == self.input_dim else x.shape[:-self.input_dim]
        t = self.features(x.reshape(-1, *self.input_shape))
        return t.view(*lead, *self.encoder.input_shape)

    def forward(self, x, y=None, x_features=None, **kw):
        """x (N1..Ng, D1..Dt), y (N1..Ng) -> (x_reco (L+1, N.., D..), logits (L+1, N.., C)[, mu, log_var, z]...)."""
        if y is None and self.y_is_coded:
            raise ValueError('y is supposed to be an input of the net')
        lead = (1,) if x.dim() == self.input_dim else x.shape[:-self.input_dim]
        with self._constant_weights(x):          # a span of its own when called outside evaluate() (see _constant_weights)
            if x_features is None:
                x_features = self._features_of(x)
            return self.forward_from_features(x_features, None if y is None else y.view(*lead), x, **kw)

    def _dump_after_encoder_error(self, err, x, y):
        """cvae.py:476-488: a ValueError out of the encoder saves the model and the offending batch under
        log/dump-<job_number> and is re-raised.  (The reference's own NaN probe that used to raise it is commented out,
        layers.py:381-386; the contract is kept for encoders / priors that do raise.)"""
        where = os.path.join('log', 'dump-{}'.format(self.job_number))
        self.save(where)
        torch.save(x, os.path.join(where, 'x.pt'))
        torch.save(y, os.path.join(where, 'y.pt'))
        logging.error('Error %s, net dumped in %s', str(err), where)

    def _reco_shape(self):
        """Per-sample shape of the decoder output: the image, or (256, C, H, W) level logits for a categorical decoder."""
        return self.input_shape if self.output_distribution != 'categorical' else (256, *self.input_shape)

    # largest activation of one launch chain of the label-free evaluation, in elements: keeps every tensor on that path far
    # below 2^31 elements and the working set of the (L+1)*N decoder batch bounded (the reference bounds the same thing by
    # halving the evaluation batch until it fits, cvae.py:1087-1153)
    EVAL_SLAB_ELEMENTS = 1 << 28

    def _widest_decoder_activation(self):
        """Elements per image of the widest tensor between z and the reconstruction."""
        widths = [int(np.prod(self._reco_shape()))]
        for stack in (self.decoder, self.imager):
            for m in stack.modules():
                if isinstance(m, nn.Linear):
                    widths.append(m.out_features)
            for sh in getattr(stack, 'shapes', None) or []:
                widths.append(int(np.prod(sh)))
        return max(widths)

    def _eval_slab_rows(self):
        env = os.environ.get('JVAE_EVAL_SLAB_ROWS')                 # tests: force many small slabs
        if env:
            return max(int(env), 1)
        return max(self.EVAL_SLAB_ELEMENTS // self._widest_decoder_activation(), 1)

    def _decode_rows(self, z):
        u = self.decoder(z)
        return self.imager(u.reshape(-1, *self.imager.input_shape))

    def _decode(self, z):
        x_ = None
        if self.x_is_generated:
            rows = z.numel() // z.shape[-1]
            slab = self._eval_slab_rows()
            if rows > slab and not torch.is_grad_enabled() and not self.training:
                # evaluation (running-statistics BatchNorm: decoder rows are independent): slabs of rows through the
                # decoder, each written into its place of the one (rows, ...) reconstruction the caller returns
                zf = z.reshape(rows, z.shape[-1])
                x_ = torch.empty((rows, *self._reco_shape()), device=z.device, dtype=torch.float32)
                for r0 in range(0, rows, slab):
                    x_[r0:r0 + slab].copy_(self._decode_rows(zf[r0:r0 + slab]).view(-1, *self._reco_shape()))
            else:
                x_ = self._decode_rows(z)
        if self.classifier_type in ('linear', None):
            logits = self.classifier(z)
        else:                                   # 'softmax': logits from the dictionary itself (cvae.py:498-499)
            m = self.encoder.prior.mean
            logits = ops.linear(z, m, m.pow(2).sum(-1) / 2)
        return x_, logits

    def generate(self, y=None, L=1, epsilon=None, temperature=1., prior_variance=False, prior=None, z_output=False):
        """Images decoded from draws of the prior: z ~ p(z | y), x = imager(decoder(z)) -> (L, N, *input_shape) fp32 on the
        device (what the prior branch of the reference's module/sample.py:124-139 computes by hand).

        y (N,) labels: one draw set per label; default one per class for a class-conditional prior, and N = num_labels
        unconditioned items for a single prior (its y, if given, only sets N).  epsilon (L, N, K) injects the unit noise.
        prior_variance=False is the reference's draw, mean[y] + temperature * epsilon; True draws with the prior's own
        variance (GaussianPrior.sample).  prior: another prior than self.encoder.prior (the alternate one of a WIMJob).
        z_output=True returns (x, z).

        Runs under no_grad with the whole model in eval mode (running-statistics BatchNorm: decoded rows are independent), so
        the L * N rows go through the decoder in slabs of `_eval_slab_rows()` like the label-free evaluation; the training flag
        is restored.  fp32 compute mode only (bf16: NotImplementedError, as odin_scores)."""
        if not self.x_is_generated:
            raise ValueError('You try to generate images with a net which is {}'.format(self.type))     # module/sample.py:158-160
        if getattr(self, 'compute_dtype', 'fp32') != 'fp32':
            raise NotImplementedError('generate() is built for the fp32 compute mode (set_compute_dtype("fp32"))')
        pr = self.encoder.prior if prior is None else prior
        dev = self.device
        if y is None:
            n = epsilon.shape[1] if epsilon is not None and not pr.conditional else self.num_labels
            y = torch.arange(n, device=dev)
        y = y.reshape(-1).to(dev)
        N, K = y.shape[0], self.latent_dim
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                z = pr.sample(y=y if pr.conditional else None, n=N, L=L, epsilon=epsilon, temperature=temperature,
                              with_variance=prior_variance)
                rows, slab = z.shape[0] * N, self._eval_slab_rows()
                zf = z.reshape(rows, K)
                with self._constant_weights(zf):
                    if rows <= slab:
                        x_ = self._decode_rows(zf)
                    else:
                        x_ = torch.empty((rows, *self._reco_shape()), device=dev, dtype=torch.float32)
                        for r0 in range(0, rows, slab):
                            x_[r0:r0 + slab].copy_(self._decode_rows(zf[r0:r0 + slab]).view(-1, *self._reco_shape()))
        finally:
            if was_training:
                self.train()
        x_ = x_.view(z.shape[0], N, *self._reco_shape())
        return (x_, z) if z_output else x_

    def forward_from_features(self, x_features, y, x, z_output=True, sampling_epsilon_norm_out=False,
                              sigma_out=False, epsilon=None):
        lead = x_features.shape[:x_features.dim() - len(self.encoder.input_shape)]
        flat = x_features.reshape(*lead, -1)
        y1h = None if (y is None or not self.y_is_coded) else onehot_encoding(y, self.num_labels).float()
        try:
            mu, log_var, z, eps, sigma = self.encoder(flat, y1h, epsilon=epsilon)
        except ValueError as err:
            self._dump_after_encoder_error(err, x, y)
            raise
        x_, logits = self._decode(z)
        out = ((x,) if self.is_vib else (x_.view(self.latent_sampling + 1, *lead, *self._reco_shape()),)) + (logits,)   # cvae.py:504-508
        if z_output:
            out += (mu, log_var, z)
        if sampling_epsilon_norm_out:
            out += ((eps ** 2).sum(-1),)
        if sigma_out:
            out += (sigma,)
        return out

    # ------------------------------------------------------------------------------------ evaluate
    def evaluate(self, x, y=None, batch=0, current_measures=None, with_beta=False, kl_var_weighting=1.,
                 gamma_weighting=1, z_output=False, epsilon=None, **kw):
        """Forward + every per-sample loss term of one batch (training branch of cvae.py:523-917).

        Returns (x_reco (L+1,N,..), y_est (N,C), batch_losses {name: (N,) tensor}, total_measures {name: float}
        [, mu, log_var, z]).  `epsilon` (L+1,N,K) optionally injects the reparameterisation noise.
        All Python floats of `total_measures` come from ONE packed device read-back.

        The call opens a span in which the weights are constant (this forward and, in training, the backward that
        follows, until Optimizer.step()): the packed operand forms of all convolution weights are refreshed by ONE launch
        here instead of one launch in front of every convolution (jvae_hip/lib.py::pack_cache_begin)."""
        with self._constant_weights(x):
            return self._evaluate(x, y, batch, current_measures, with_beta, kl_var_weighting, gamma_weighting, z_output,
                                  epsilon, **kw)

    @contextlib.contextmanager
    def _constant_weights(self, x):
        """The span in which the convolution weights are vouched for (packed operand forms served from the step's cache).
        Opened by evaluate() and by a stand-alone forward(); closed when the call returns if no backward can follow (eval
        mode / no_grad), else by the backward pass itself (ops._close_span_after_backward), by Optimizer.zero_grad() /
        step(), and by everything that rewrites the weights wholesale (load_state_dict, load_weights, .to()/_apply).  A
        nested call (forward() inside evaluate()) belongs to the outer span.  A convolution FORWARD called outside any such call
        (a submodule invoked directly) disarms a cache left armed for a backward that has not come yet and packs per call
        (ops._Conv.forward): the weights may have changed through .data in between."""
        if getattr(self, '_span_open', False) or not x.is_cuda:     # CPU tensors: the ops raise their own "no CPU fallback" error
            yield
            return
        self._span_open = True
        _lib.span_depth += 1
        try:
            ws = getattr(self, '_conv_weights', None)
            if ws is None:
                from module.vae_layers.conv import HipConv2d, HipConvTranspose2d
                ws = self._conv_weights = [m.weight for m in self.modules() if isinstance(m, (HipConv2d, HipConvTranspose2d))]
            _lib.pack_cache_begin(ws, x.device)
            if torch.cuda.is_current_stream_capturing():
                _lib.pack_cache_pin()            # the graph bakes this owner's slot addresses in: never recycle its region
            yield
        finally:
            self._span_open = False
            _lib.span_depth -= 1
            if not (self.training and torch.is_grad_enabled()):
                _lib.pack_cache_end()            # no backward will follow: stop vouching for the weights now

    def _apply(self, fn, *a, **kw):
        _lib.pack_cache_end()                    # .to() / .float() / .cuda(): the weights move or change
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        _lib.pack_cache_end()
        if getattr(self, 'optimizer', None) is not None:
            self.optimizer._scan_pending = True          # loaded values: the next check_nonfinite() scans every parameter
        return super().load_state_dict(*a, **kw)

    def _evaluate(self, x, y=None, batch=0, current_measures=None, with_beta=False, kl_var_weighting=1.,
                  gamma_weighting=1, z_output=False, epsilon=None, **kw):
        # the labelled training-mode evaluation alone follows SEMI_SUPERVISED and TRAIN_OBJECTIVE (refusals are raised here, before
        # any work)
        mmd = self.training and y is not None and self._check_mmd_objective(kl_var_weighting, kw)      # first: it names SEMI_SUPERVISED
        semi = self.training and y is not None and self._check_semi_supervised(kl_var_weighting, kw)
        iwae = self.training and y is not None and self._check_iwae_objective(kl_var_weighting, kw)
        tcvae = self.training and y is not None and self._check_tc_objective(kl_var_weighting, kw)
        if y is None or self.is_vib:
            if self.is_vib:
                return self._evaluate_vib(x, y, batch, current_measures, with_beta, kl_var_weighting, gamma_weighting,
                                          z_output, epsilon, kw.get('_raw_measures'), kw.get('_dev_weights'),
                                          kw.get('_dev_state'))
            return self._evaluate_all_classes(x, batch, current_measures, with_beta, z_output, epsilon)
        if x.dim() != self.input_dim + 1:
            x = x.reshape(-1, *self.input_shape)
            y = y.reshape(-1)
        N = x.shape[0]
        L = self.latent_sampling
        D = int(np.prod(self.input_shape))
        cross_y_weight = False                                               # cvae.py:557-563
        if self.y_is_decoded:
            if self.is_cvae or self.is_vae:
                cross_y_weight = gamma_weighting * self.gamma if self.training else False
            else:
                cross_y_weight = gamma_weighting * self.gamma

        # captured step of train_model(): the two warm-up weights as device scalars ([kl_var_weighting, cross_y weight]; the
        # host values above only decide WHETHER cross_y is in the loss) and the running measures / batch counter on the device
        dev_weights, dev_state = kw.get('_dev_weights'), kw.get('_dev_state')
        cw = cross_y_weight
        if dev_weights is not None:
            kl_var_weighting = dev_weights[0:1]
            cw = dev_weights[1:2] if cross_y_weight else cross_y_weight

        y_given = y
        if semi:
            # the draws and the labelled rows are what they are without the switch.  An unlabelled row is measured against class
            # 0 by the latent op and that kl is then discarded: its backward meets g = 0 there.  0 x inf is not reachable: with
            # the log-variance clipped to +-20 and fp32 means the class-0 terms stay far below the fp32 range.
            y = y.clamp_min(0)
        feats = self._features_of(x).reshape(N, -1)
        y1h = onehot_encoding(y, self.num_labels).float() if self.y_is_coded else None
        try:
            mu, log_var, z, eps, sigma_coded, terms = self.encoder.encode(feats, y1h, y, kl_var_weighting, epsilon)
        except ValueError as err:
            self._dump_after_encoder_error(err, x, y)
            raise
        self._last_epsilon = eps
        if semi:
            # SEMI_SUPERVISED: the rows with a negative label take the class-marginal bound, its zdist and var_kl (ops.class_marginal_kl,
            # csrc/semisup.hip); the others pass through with their bits.  The op runs on every such step: the host never asks
            # whether a batch holds an unlabelled row.
            pr = self.encoder.prior
            s_kl, s_zd, s_vkl, _ = ops.class_marginal_kl(
                mu.reshape(N, -1).contiguous(), log_var.reshape(N, -1), y_given, pr.mean, pr._var_parameter, terms['kl'],
                terms['distance'], terms['var_kl'], log_pi=self._semi_log_pi(pr.mean.shape[0], x.device),
                w=float(kl_var_weighting), var_dim=pr.var_dim)
            terms = dict(terms, kl=s_kl, distance=s_zd, var_kl=s_vkl)
        if self.training and self.optimizer._world > 1 and z.requires_grad \
                and not getattr(self.optimizer, '_external_reduce', False):
            # data-parallel: the decoder's gradients are final once d(loss)/dz exists -> start their all-reduce there
            z.register_hook(self._early_reduce_hook)
        x_, logits = self._decode(z)
        x_reco = x_.view(L + 1, N, *self._reco_shape())

        s, s_kind, sigma_rms = self._sigma_operand(sigma_coded, N)
        ce = None
        if self.y_is_decoded:
            ce = x_loss(y, logits, batch_mean=False)                         # all L+1 rows, as cvae.py:738 does
            if semi:
                ce = ce * (y_given >= 0).to(ce.dtype)                        # no label: no cross_y, in value and in gradient
        if self.output_distribution == 'categorical':
            # cvae.py:654-660,752-753: -log p(x|z) is the 256-level cross entropy of every pixel, summed over the image (the
            # only term with a gradient); `wmse` is the plain mean-square error of the arg-max image (reported, sigma not
            # applied: the `catgorical` test at cvae.py:638 never matches), `mse` = wmse * sigma^2 as for a gaussian decoder
            ndim = len(self.input_shape)
            ce_x = categorical_loss(x_reco[1:], x, ndim=ndim, batch_mean=False)                       # (L, N)
            with torch.no_grad():
                levels = x_reco[1:].argmax(-ndim - 1).float() / 255
                wmse = mse_loss(levels, x, ndim=ndim, batch_mean=False).mean(0)
                mse = None
            cross_x = ce_x.mean(0)
            total = cross_x + (self.beta if with_beta else 1.) * terms['kl']
            if cross_y_weight:
                total = total + cw * ce
        elif iwae:
            # TRAIN_OBJECTIVE = 'iwae': total = -bound over the L draws of this very step (ops.iw_bound: weights, bound, ess and
            # the direct gradients in csrc/iwae.hip; autograd carries z and log_var on through the unchanged latent / decoder
            # ops).  wmse, cross_x and mse are reported as the ELBO reports them, outside the loss.
            wmse_s = ops.recon_wmse(x_reco, x, s, s_kind, snapshot=bool(self.sigma.decay))                      # (L, N)
            pr = self.encoder.prior
            lab, means, T = pr._kernel_operands(y if pr.conditional else None, N, x.device)
            bound, ess = ops.iw_bound(wmse_s, z, log_var, eps, lab, means, T, s, s_kind, D,
                                      beta=self.beta if with_beta else 1., var_dim=pr.var_dim)
            with torch.no_grad():
                wmse, cross_x, _, mse = ops.elbo(wmse_s, terms['kl'], None, s, s_kind, D, 1., 0., with_mse=True)
            total = -bound
            if cross_y_weight:
                total = total + cw * ce
        elif tcvae:
            # TRAIN_OBJECTIVE = 'tcvae': total = cross_x + b (alpha mi + beta_tc tc + gamma dwkl) (+ cw cross_y).  The
            # reconstruction term keeps the ELBO's own path (ops.elbo with a zero KL operand); the regulariser and its direct
            # gradients are ops.tc_objective (csrc/tcvae.hip), autograd carries z and log_var on through the unchanged latent op.
            # kl, zdist and var_kl are reported as before, outside the loss.
            wmse_s = ops.recon_wmse(x_reco, x, s, s_kind, snapshot=bool(self.sigma.decay))                      # (L, N)
            b = self.beta if with_beta else 1.
            wmse, cross_x, total, mse = ops.elbo(wmse_s, torch.zeros_like(terms['kl']), ce if cross_y_weight else None, s, s_kind,
                                                 D, b, float(cross_y_weight or 0.), with_mse=True)
            pr = self.encoder.prior
            lab, means, T = pr._kernel_operands(y if pr.conditional else None, N, x.device)
            reg, tc_mi, tc_tc, tc_dwkl = ops.tc_objective(z, mu.contiguous(), log_var, eps, lab, means, T, self.TC_WEIGHTS,
                                                          self._tc_log_n(means.shape[0], x.device), var_dim=pr.var_dim)
            total = total + b * reg
        elif mmd:
            # TRAIN_OBJECTIVE = 'mmd': total = cross_x + b kl_weight kl + mmd_weight m (+ cw cross_y).  The ELBO keeps its own path
            # (ops.elbo with the KL operand scaled by kl_weight); m and its direct gradients are ops.mmd_objective (csrc/mmd.hip) on
            # the step's own z and a second noise tensor, drawn here - after the encoder's draw and under this objective only, so
            # that every other run keeps its random stream.  kl, zdist and var_kl are reported as before.
            wmse_s = ops.recon_wmse(x_reco, x, s, s_kind, snapshot=bool(self.sigma.decay))                      # (L, N)
            kl_weight, mmd_weight = (float(w) for w in self.MMD_WEIGHTS)
            wmse, cross_x, total, mse = ops.elbo(wmse_s, terms['kl'] if kl_weight == 1. else terms['kl'] * kl_weight,
                                                 ce if cross_y_weight else None, s, s_kind, D, self.beta if with_beta else 1.,
                                                 float(cross_y_weight or 0.), with_mse=True)
            pr = self.encoder.prior
            lab, means, T = pr._kernel_operands(y if pr.conditional else None, N, x.device)
            eps_p = kw.get('prior_epsilon')
            if eps_p is None:
                eps_p = torch.randn(eps.shape, device=x.device, dtype=torch.float32)
            elif tuple(eps_p.shape) != tuple(eps.shape):
                raise ValueError('prior_epsilon must be {}, got {}'.format(tuple(eps.shape), tuple(eps_p.shape)))
            self._last_prior_epsilon = eps_p
            mmd_rows = ops.mmd_objective(z, eps_p, lab, means, T, kernel=self.MMD_KERNEL, joint=self.MMD_JOINT, var_dim=pr.var_dim)
            total = total + mmd_weight * mmd_rows
        else:
            wmse_s = ops.recon_wmse(x_reco, x, s, s_kind, snapshot=bool(self.training and self.sigma.decay))     # (L, N)
            wmse, cross_x, total, mse = ops.elbo(wmse_s, terms['kl'], ce if cross_y_weight else None, s, s_kind, D,
                                                 self.beta if with_beta else 1.,
                                                 cw if torch.is_tensor(cw) else float(cross_y_weight or 0.), with_mse=True)
        losses = {'kl': terms['kl'], 'zdist': terms['distance'], 'var_kl': terms['var_kl']}
        if iwae:
            losses['iwae'], losses['ess'] = bound, ess
        if tcvae:
            losses['mi'], losses['tc'], losses['dwkl'] = tc_mi, tc_tc, tc_dwkl
        if mmd:
            losses['mmd'] = mmd_rows
        dictionary = self.encoder.prior.mean if self.encoder.prior.conditional else None
        if dictionary is not None:
            losses['dzdist'] = terms['dzdist']
        losses['wmse'] = wmse
        losses['cross_x'] = cross_x
        if ce is not None:
            losses['cross_y'] = ce
        losses['total'] = total

        prev = self._prev_measures(current_measures, batch, x.device)
        packed = self._pack_measures(x, wmse, terms, dictionary, prev, batch, mse=mse, sigma_rms=sigma_rms, sigma_t=s,
                                     dev_state=dev_state)
        if self.training:
            if self.sigma.decay and not self.sigma.learned:                  # the decay rule computes with the rmse now
                torch.cuda.current_stream(x.device).wait_stream(_lib.side_stream(x.device))
            self.sigma.update(rmse=packed[3])                                # device scalar, as in the reference
        if kw.get('_raw_measures'):
            # graph capture (graph_train_step): the 16-float device buffer itself; the host copy is made after each replay
            measures = (packed, dictionary is not None)
        else:
            measures = Measures(packed, dictionary is not None, _grad_nan_exit)
            if self.training:
                self.training_parameters['sigma'] = _LazySigmaParams(self.sigma, measures)
        out = (x_reco, _mean_over_draws(logits), losses, measures)
        if z_output:
            out += (mu, log_var, z)
        return out

    # ------------------------------------------------------------------------------------ importance-weighted objective
    def _check_iwae_objective(self, kl_var_weighting, kw):
        """Is this training-mode evaluate() on the importance-weighted bound?  TRAIN_OBJECTIVE 'elbo': False.  'iwae': True, or
        NotImplementedError naming what the bound is not built for (DESIGN.md section 7v says why for each)."""
        objective = self.TRAIN_OBJECTIVE
        if objective == 'elbo':
            return False
        if objective in ('tcvae', 'mmd'):          # _check_tc_objective() / _check_mmd_objective() decide those branches and make
            return False                           # their own refusals
        if objective != 'iwae':
            raise ValueError("TRAIN_OBJECTIVE is 'elbo' or 'iwae' or 'tcvae' or 'mmd', got {!r}".format(objective))

        def refuse(what):
            raise NotImplementedError("TRAIN_OBJECTIVE = 'iwae': " + what)
        self._iw_model_refusals(refuse)
        if self.encoder.mixed_prior is not None:
            refuse('a mixed (two-prior) encode is not built')
        if not self.encoder.sampling.is_sampled:
            refuse('the encoder does not sample (latent_sampling <= 1 and beta = 0): there are no draws to weigh')
        if torch.is_tensor(kl_var_weighting) or kl_var_weighting != 1:
            refuse('kl_var_weighting != 1 (a warm-up on the variance part of the KL) has no meaning for sampled densities')
        if getattr(self.optimizer, '_world', 1) > 1:
            refuse('data-parallel training (optimizer._world > 1) is not built')
        if (self.TRAIN_CAPTURED or kw.get('_raw_measures') or kw.get('_dev_weights') is not None
                or kw.get('_dev_state') is not None or getattr(self.optimizer, '_external_reduce', False)
                or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())):
            refuse('graph_train_step / capture_train_step / TRAIN_CAPTURED are not built: the captured steps train on the ELBO')
        return True

    def _iw_model_refusals(self, refuse):
        """What the importance-weighted bound is not built for ABOUT THE MODEL, the same for the training objective and for
        iw_bound(): `refuse(what)` raises with the caller's own prefix."""
        pr = self.encoder.prior
        if not (self.is_cvae or self.is_vae or self.is_xvae):
            refuse("built for the types 'cvae', 'vae' and 'xvae', not '{}'".format(self.type))
        if self.y_is_coded:
            refuse('coded labels (y_is_coded) are not built')
        if self.output_distribution == 'categorical':
            refuse('the categorical decoder is not built')
        if self.sigma.is_rmse:
            refuse('the rmse sigma (is_rmse) is not built: sigma would depend on all draws of the sample')
        if pr.distribution != 'gaussian':
            refuse("the '{}' prior is not built: Gaussian priors only".format(pr.distribution))
        if pr.var_dim == 'full':
            refuse("the full-variance prior (var_dim='full') is not built: 'scalar' and 'diag' only")
        if getattr(self, 'compute_dtype', 'fp32') != 'fp32':
            refuse('the bf16 compute mode is not built (set_compute_dtype("fp32"))')

    # ------------------------------------------------------------------------------------ beta-TCVAE objective
    def _check_tc_objective(self, kl_var_weighting, kw):
        """Is this training-mode evaluate() on the beta-TCVAE split?  True for TRAIN_OBJECTIVE 'tcvae', or NotImplementedError
        naming what the split is not built for; False for every other value (_check_iwae_objective(),
        called first, has already refused an unknown one)."""
        if self.TRAIN_OBJECTIVE != 'tcvae':
            return False

        def refuse(what):
            raise NotImplementedError("TRAIN_OBJECTIVE = 'tcvae': " + what)
        self._iw_model_refusals(refuse)
        if self.encoder.mixed_prior is not None:
            refuse('a mixed (two-prior) encode is not built')
        if not self.encoder.sampling.is_sampled:
            refuse('the encoder does not sample (latent_sampling <= 1 and beta = 0): there are no draws to place in the mixture')
        if torch.is_tensor(kl_var_weighting) or kl_var_weighting != 1:
            refuse('kl_var_weighting != 1 (a warm-up on the variance part of the KL) has no meaning for sampled densities')
        if getattr(self.optimizer, '_world', 1) > 1:
            refuse('data-parallel training (optimizer._world > 1) is not built: the mixture spans the whole batch and a rank '
                   'sees only its shard')
        if (self.TRAIN_CAPTURED or kw.get('_raw_measures') or kw.get('_dev_weights') is not None
                or kw.get('_dev_state') is not None or getattr(self.optimizer, '_external_reduce', False)
                or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())):
            refuse('graph_train_step / capture_train_step / TRAIN_CAPTURED are not built: the captured steps train on the ELBO')
        weights = self.TC_WEIGHTS
        if len(weights) != 3 or not all(np.isfinite(float(w)) for w in weights):
            raise ValueError('TC_WEIGHTS is (alpha, beta_tc, gamma), three finite numbers, got {!r}'.format(weights))
        return True

    def _tc_log_n(self, C, device):
        """TC_DATASET_SIZE as the operand of ops.tc_objective: None, or (C,) fp64 on the device, log of the training samples behind
        each class (kept until the attribute or the device changes)."""
        size = self.TC_DATASET_SIZE
        if size is None:
            return None
        counts = (int(size),) if np.ndim(size) == 0 else tuple(int(v) for v in size)
        if len(counts) != C:
            raise ValueError('TC_DATASET_SIZE: {} expected, got {!r}'.format(
                'an int (a single prior)' if C == 1 else 'the {} class counts of the conditional prior'.format(C), size))
        if min(counts) < 1:
            raise ValueError('TC_DATASET_SIZE: counts >= 1 expected, got {!r}'.format(size))
        key = (counts, str(device))
        if getattr(self, '_tc_log_n_cache', (None,))[0] != key:
            self._tc_log_n_cache = (key, torch.tensor(counts, dtype=torch.float64).log().to(device))
        return self._tc_log_n_cache[1]

    @staticmethod
    def _tc_dataset_size_of(trainset, C):
        """What train_model() fills TC_DATASET_SIZE with: len(trainset) for a single prior (C == 1), else one bincount of its labels
        (`.targets` / `.labels` of the dataset behind random_split's Subsets where it carries them, else the samples' own)."""
        if C == 1:
            return len(trainset)
        base, indices = trainset, None
        while isinstance(base, torch.utils.data.Subset):
            idx = torch.as_tensor(base.indices, dtype=torch.int64)
            indices = idx if indices is None else idx[indices]
            base = base.dataset
        labels = getattr(base, 'targets', None)
        if labels is None:
            labels = getattr(base, 'labels', None)
        transform = getattr(base, 'target_transform', None)
        lut = getattr(base, 'lut', None)
        if labels is None or lut is not None:
            labels = [int(trainset[i][1]) for i in range(len(trainset))]
        else:
            labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to('cpu', torch.int64)
            labels = (labels if indices is None else labels[indices]).tolist()
            if transform is not None:
                labels = [int(transform(int(v))) for v in labels]
        labels = torch.as_tensor(labels, dtype=torch.int64)
        labels = labels[(labels >= 0) & (labels < C)]             # a label out of range is in nobody's set: not counted
        counts = torch.bincount(labels, minlength=C)
        return tuple(max(int(v), 1) for v in counts.tolist())          # a class without a sample is in no set: any count serves

    # ------------------------------------------------------------------------------------ MMD-regularised objective
    def _check_mmd_objective(self, kl_var_weighting, kw):
        """Is this training-mode evaluate() on the MMD-regularised bound?  True for TRAIN_OBJECTIVE 'mmd', or NotImplementedError
        naming what it is not built for; False for every other value (_check_iwae_objective() refuses an
        unknown one).  kl_var_weighting is free here, a device scalar included: the KL keeps its own path."""
        if self.TRAIN_OBJECTIVE != 'mmd':
            return False

        def refuse(what):
            raise NotImplementedError("TRAIN_OBJECTIVE = 'mmd': " + what)
        self._iw_model_refusals(refuse)
        if self.encoder.mixed_prior is not None:
            refuse('a mixed (two-prior) encode is not built')
        if not self.encoder.sampling.is_sampled:
            refuse('the encoder does not sample (latent_sampling <= 1 and beta = 0): there are no draws to compare with the prior')
        if self.SEMI_SUPERVISED:
            refuse('SEMI_SUPERVISED is not built: a row without a label has no class prior to draw from')
        if getattr(self.optimizer, '_world', 1) > 1:
            refuse('data-parallel training (optimizer._world > 1) is not built: the pairs span the whole batch and a rank '
                   'sees only its shard')
        if (self.TRAIN_CAPTURED or kw.get('_raw_measures') or kw.get('_dev_weights') is not None
                or kw.get('_dev_state') is not None or getattr(self.optimizer, '_external_reduce', False)
                or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())):
            refuse('graph_train_step / capture_train_step / TRAIN_CAPTURED are not built: the captured steps train on the ELBO')
        self._mmd_settings()
        return True

    def _mmd_settings(self):
        """(kl_weight, mmd_weight, kind, scales) of MMD_WEIGHTS and MMD_KERNEL, or ValueError naming the malformed attribute."""
        weights = self.MMD_WEIGHTS
        try:
            ok = len(weights) == 2 and all(np.isfinite(float(w)) for w in weights)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('MMD_WEIGHTS is (kl_weight, mmd_weight), two finite numbers, got {!r}'.format(weights))
        try:
            kind, scales = ops.mmd_scales(self.MMD_KERNEL, self.latent_dim)
        except _lib.JvaeHipError as err:
            raise ValueError("MMD_KERNEL is (kind, scales): 'imq' or 'rbf', and at most 8 positive finite scales or None, "
                             'got {!r} ({})'.format(self.MMD_KERNEL, err)) from None
        return float(weights[0]), float(weights[1]), kind, scales

    def prior_mmd(self, codes, y=None, epsilon=None):
        """How far a set of latent codes is from the prior, with no density estimate -> (mmd2, rows): the unbiased U-statistic of
        MMD^2 between codes (M, K) and as many draws of the prior, and its per-row terms (M,), fp32 on the device; the op of
        TRAIN_OBJECTIVE = 'mmd' (ops.mmd_objective with one draw) under no_grad, with MMD_KERNEL and MMD_JOINT.  y (M,): the
        labels of the codes, required for a class-conditional prior (each code is compared with draws of its own class) and
        None for a single prior.  epsilon (M, K): the noise of the prior draws (default: drawn here).  M up to the op's limit
        (8192).  Refuses what the objective refuses about the model."""
        def refuse(what):
            raise NotImplementedError('prior_mmd: ' + what)
        self._iw_model_refusals(refuse)
        pr = self.encoder.prior
        if pr.conditional and y is None:
            raise ValueError('prior_mmd: a class-conditional prior needs the labels y')
        if not pr.conditional and y is not None:
            raise ValueError('prior_mmd: y must be None for a model with a single prior')
        if codes.dim() != 2 or codes.shape[1] != self.latent_dim:
            raise ValueError('prior_mmd: codes must be (M, {}), got {}'.format(self.latent_dim, tuple(codes.shape)))
        M, K = codes.shape
        if epsilon is not None and tuple(epsilon.shape) != (M, K):
            raise ValueError('prior_mmd: epsilon must be ({}, {}), got {}'.format(M, K, tuple(epsilon.shape)))
        self._mmd_settings()
        with torch.no_grad():
            codes = codes.detach().to(torch.float32)
            z = torch.stack([codes, codes])                                       # row 0 takes no part
            e = (torch.randn((1, M, K), device=codes.device, dtype=torch.float32) if epsilon is None
                 else epsilon.detach().to(torch.float32).reshape(1, M, K).contiguous())
            lab, means, T = pr._kernel_operands(None if y is None else y.reshape(-1), M, codes.device)
            rows = ops.mmd_objective(z, e, lab, means.detach(), T.detach(), kernel=self.MMD_KERNEL, joint=self.MMD_JOINT,
                                     var_dim=pr.var_dim)
            return rows.mean(), rows

    # ------------------------------------------------------------------------------------ semi-supervised training
    def _check_semi_supervised(self, kl_var_weighting, kw):
        """Does this training-mode evaluate() read negative labels as "no label"?  False while SEMI_SUPERVISED is off; True, or
        NotImplementedError naming what the class-marginal KL is not built for (DESIGN.md section 7x says why for each)."""
        if not self.SEMI_SUPERVISED:
            return False

        def refuse(what):
            raise NotImplementedError('SEMI_SUPERVISED: ' + what)
        self._iw_model_refusals(refuse)
        if not self.encoder.prior.conditional:
            refuse('a non-conditional prior has no classes to marginalise over')
        if self.encoder.mixed_prior is not None:
            refuse('a mixed (two-prior) encode is not built')
        if self.TRAIN_OBJECTIVE != 'elbo':
            refuse("TRAIN_OBJECTIVE = {!r} is not built: the class-marginal KL enters the ELBO only".format(self.TRAIN_OBJECTIVE))
        if torch.is_tensor(kl_var_weighting):
            refuse('kl_var_weighting as a device scalar is not built: the kernel takes the weight from the host')
        if getattr(self.optimizer, '_world', 1) > 1:
            refuse('data-parallel training (optimizer._world > 1) is not built')
        if (self.TRAIN_CAPTURED or kw.get('_raw_measures') or kw.get('_dev_weights') is not None
                or kw.get('_dev_state') is not None or getattr(self.optimizer, '_external_reduce', False)
                or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())):
            refuse('graph_train_step / capture_train_step / TRAIN_CAPTURED are not built: the captured steps take a label on every row')
        self._semi_class_weights(self.encoder.prior.mean.shape[0])
        return True

    def _semi_class_weights(self, C):
        """UNLABELLED_CLASS_WEIGHTS as a tuple of C floats, or None for uniform weights; ValueError for anything else."""
        weights = self.UNLABELLED_CLASS_WEIGHTS
        if weights is None:
            return None
        weights = tuple(float(v) for v in (weights.tolist() if hasattr(weights, 'tolist') else weights))
        if len(weights) != C or not all(np.isfinite(v) and v > 0 for v in weights):
            raise ValueError('UNLABELLED_CLASS_WEIGHTS is None or {} positive finite numbers, got {!r}'.format(
                C, self.UNLABELLED_CLASS_WEIGHTS))
        return weights

    def _semi_log_pi(self, C, device):
        """UNLABELLED_CLASS_WEIGHTS as the operand of ops.class_marginal_kl: None, or (C,) fp64 on the device, the logarithms of the
        normalised weights (kept until the attribute or the device changes)."""
        weights = self._semi_class_weights(C)
        if weights is None:
            return None
        key = (weights, str(device))
        if getattr(self, '_semi_log_pi_cache', (None,))[0] != key:
            w = torch.tensor(weights, dtype=torch.float64)
            self._semi_log_pi_cache = (key, (w / w.sum()).log().to(device))
        return self._semi_log_pi_cache[1]

    def class_marginal(self, x):
        """q(y | x) under the class-marginal bound and the bound itself -> (U (N,), r (N, C)), fp32 on the device:

            U = -log sum_c pi_c exp(-KL_c),    r_c = pi_c exp(-KL_c) / sum_c' pi_c' exp(-KL_c'),    KL_c = KL(q(z | x) || p(z | c))

        U is the KL part of the ELBO of the class-marginal model (an upper bound of KL(q || sum_c pi_c p_c)), r the rule predict()
        applies, with the weights of UNLABELLED_CLASS_WEIGHTS.  The encode-only pass (latent_posterior) and ONE launch of
        ops.class_marginal_kl with every label -1: no (C, N, K) operand exists.  Runs in eval mode under no_grad (the training flag
        is restored); SEMI_SUPERVISED need not be set.  Refuses what SEMI_SUPERVISED refuses about the model."""
        def refuse(what):
            raise NotImplementedError('class_marginal: ' + what)
        self._iw_model_refusals(refuse)
        pr = self.encoder.prior
        if not pr.conditional:
            refuse('a non-conditional prior has no classes to marginalise over')
        was_training = self.training
        self.eval()
        try:
            mu, log_var = self.latent_posterior(x)
            N = mu.shape[0]
            with torch.no_grad():
                none = torch.full((N,), -1, dtype=torch.int64, device=mu.device)
                zero = torch.zeros(N, dtype=torch.float32, device=mu.device)
                U, _, _, r = ops.class_marginal_kl(mu.contiguous(), log_var.contiguous(), none, pr.mean.detach(),
                                                   pr._var_parameter.detach(), zero, zero, zero,
                                                   log_pi=self._semi_log_pi(pr.mean.shape[0], mu.device), w=1., var_dim=pr.var_dim)
            return U, r
        finally:
            if was_training:
                self.train()

    def _refuse_captured_semi(self, who):
        """The captured steps take a label on every row: asked for under SEMI_SUPERVISED they refuse before anything is captured."""
        if self.SEMI_SUPERVISED:
            raise NotImplementedError('SEMI_SUPERVISED: {} is not built for it (graph_train_step / capture_train_step / '
                                      'TRAIN_CAPTURED take a label on every row)'.format(who))

    def _refuse_captured_iwae(self, who):
        """The captured steps train on the ELBO: asked for with another objective they refuse before anything is captured."""
        if self.TRAIN_OBJECTIVE != 'elbo':
            raise NotImplementedError("TRAIN_OBJECTIVE = {!r}: {} is not built for it (graph_train_step / capture_train_step / "
                                      "TRAIN_CAPTURED train on the ELBO)".format(self.TRAIN_OBJECTIVE, who))

    def iw_bound(self, x, y=None, samples=None, epsilon=None):
        """log p(x | y) estimated with `samples` importance draws from the encoder -> (bound (N,), ess (N,)), fp32 on the device:

            bound_n = log (1/L) sum_l w_l,    w_l = p(x | z_l) p(z_l | y) / q(z_l | x),    ess_n = (sum_l w_l)^2 / sum_l w_l^2

        the importance-weighted bound of Burda et al. with beta = 1, a lower bound of log p(x | y) in expectation that tightens
        with L.  This is the PROPER estimate: not `losses['iws']` of evaluate(x), which reproduces the reference as written (the
        mean of exp(l_i - m) plus m, not its logarithm: csrc/loss.hip marks the sic) and bounds nothing.

        y (N,) is required for a class-conditional prior and must be None for type 'vae'.  samples: default latent_sampling of the
        evaluation mode.  epsilon (samples + 1, N, K) injects the noise (row 0 is not used).  Runs in eval mode under no_grad (the
        training flag is restored).  The draws are cut into slabs so that no decoder activation passes EVAL_SLAB_ELEMENTS - 5000
        draws of 100 images never exist as one (L, N, D) tensor - and the slabs are folded on the device by an exact merge of
        (max, shifted sum) pairs inside the kernel (ops.iw_bound with a state).  Refuses what TRAIN_OBJECTIVE = 'iwae' refuses
        about the model (type, coded labels, categorical decoder, rmse sigma, non-Gaussian or full-variance priors, bf16).
        The reconstruction rows wmse_s reach the kernel as fp32 (ops.recon_wmse): a weight is as good as those rows times D / 2."""
        was_training = self.training
        self.eval()
        try:
            pr = self.encoder.prior

            def refuse(what):
                raise NotImplementedError('iw_bound: ' + what)
            self._iw_model_refusals(refuse)
            if pr.conditional and y is None:
                raise ValueError('iw_bound: a class-conditional prior needs the labels y')
            if not pr.conditional and y is not None:
                raise ValueError('iw_bound: y must be None for a model with a single prior')
            if x.dim() != self.input_dim + 1:
                x = x.reshape(-1, *self.input_shape)
            y = None if y is None else y.reshape(-1)
            N, K = x.shape[0], self.latent_dim
            D = int(np.prod(self.input_shape))
            L = int(samples if samples is not None else (epsilon.shape[0] - 1 if epsilon is not None else self.latent_sampling))
            if L < 1:
                raise ValueError('iw_bound: at least one draw')
            if epsilon is not None and tuple(epsilon.shape) != (L + 1, N, K):
                raise ValueError('iw_bound: epsilon must be ({}, {}, {}), got {}'.format(L + 1, N, K, tuple(epsilon.shape)))
            per_slab = max(self._eval_slab_rows() // max(N, 1) - 1, 1)          # draws per slab; each slab decodes one more row
            enc = self.encoder
            with torch.no_grad(), self._constant_weights(x):
                feats = self._features_of(x).reshape(N, -1)
                u, mu, lv_raw = enc.heads(feats, None)
                lab, means, T = pr._kernel_operands(y if pr.conditional else None, N, x.device)
                forced = math.log(enc.forced_variance) if enc.forced_variance else None
                s, s_kind, _ = self._sigma_operand(enc.sigma(u) if enc.sigma_output_dim else None, N, store=False)
                s = s.detach().contiguous()
                state = torch.zeros((4, N), device=x.device, dtype=torch.float64)
                bound = ess = None
                for l0 in range(0, L, per_slab):
                    Ls = min(per_slab, L - l0)
                    e = torch.empty((Ls + 1, N, K), device=x.device, dtype=torch.float32)
                    e[0] = 0
                    if epsilon is None:
                        e[1:].normal_()
                    else:
                        e[1:].copy_(epsilon[1 + l0:1 + l0 + Ls])
                    log_var, z = ops.latent(mu, mu if lv_raw is None else lv_raw, e, lab, means, T, prior=pr.distribution,
                                            var_dim=pr.var_dim, sampled=True, forced_lv=forced)[:2]
                    x_reco = self._decode_rows(z.reshape(-1, K)).view(Ls + 1, N, *self._reco_shape())
                    wmse_s = ops.recon_wmse(x_reco, x, s, s_kind)
                    bound, ess = ops.iw_bound(wmse_s, z, log_var, e[1:], lab, means.detach(), T.detach(), s, s_kind, D,
                                              beta=1., var_dim=pr.var_dim, state=state)
            return bound, ess
        finally:
            if was_training:
                self.train()

    # ------------------------------------------------------------------------------------ type 'vib'
    def _evaluate_vib(self, x, y, batch, current_measures, with_beta, kl_var_weighting, gamma_weighting, z_output, epsilon,
                      raw_measures=False, dev_weights=None, dev_state=None):
        """evaluate() of a model WITHOUT decoder (type 'vib': cvae.py:189,201,490-505,891-896): the loss is the classifier's
        cross entropy on z plus beta x the KL to the single prior; the returned `reconstruction` is x itself.  With labels:
        every loss (N,); without (the evaluation path): cross_y and total are (C, N) - one row per candidate class
        (module/losses.py:47-86) - and the prediction is the classifier's ('esty')."""
        if x.dim() != self.input_dim + 1:
            x = x.reshape(-1, *self.input_shape)
            y = None if y is None else y.reshape(-1)
        N = x.shape[0]
        cross_y_weight = gamma_weighting * self.gamma                                   # cvae.py:557-563: always in the loss
        cw = cross_y_weight
        if dev_weights is not None:              # captured step of train_model(): the weights as device scalars (see _evaluate)
            kl_var_weighting, cw = dev_weights[0:1], dev_weights[1]
        with torch.set_grad_enabled(torch.is_grad_enabled() and y is not None):
            feats = self._features_of(x).reshape(N, -1)
            dummy = y if y is not None else torch.zeros(N, dtype=torch.int64, device=x.device)
            try:
                mu, log_var, z, eps, _, terms = self.encoder.encode(feats, None, dummy, kl_var_weighting, epsilon)
            except ValueError as err:
                self._dump_after_encoder_error(err, x, y)
                raise
            self._last_epsilon = eps
            _, logits = self._decode(z)
            ce = x_loss(y, logits, batch_mean=False)                                     # (N,) or (C, N); all L+1 rows
            beta = self.beta if with_beta else 1.
            losses = {'kl': terms['kl'], 'zdist': terms['distance'], 'var_kl': terms['var_kl']}
            total = beta * terms['kl']
            if cross_y_weight:
                total = total + cw * ce                                                 # broadcasts to (C, N) without labels
            elif y is None:
                total = total.unsqueeze(0).expand_as(ce)
            losses['total'] = total
            losses['cross_y'] = ce
        prev = self._prev_measures(current_measures, batch, x.device)
        with torch.no_grad():
            packed = self._pack_measures_raw(x, torch.zeros(N, device=x.device), terms, None, prev, batch, self.sigma.detach(),
                                             int(self.sigma.is_log), dev_state=dev_state)
        keys = ('sigma', 'zdist', 'var_kl')
        measures = (packed, False) if raw_measures else Measures(packed, False, _grad_nan_exit, only=keys)
        out = (x, _mean_over_draws(logits), losses, measures)
        if z_output:
            out += (mu, log_var, z)
        return out

    # ------------------------------------------------------------------------------------ evaluation
    def _evaluate_all_classes(self, x, batch, current_measures, with_beta, z_output, epsilon):
        """evaluate(x) without labels (cvae.py:548-600, 793-873): every class is tried as the prior component.
        Losses kl / zdist / var_kl / total / iws [/ cross_y] are (C, N); wmse / cross_x / dzdist stay (N,).
        The heavy parts (conv stacks on (L+1)N latents, BatchNorm, latent / KL kernel on C*N rows, reconstruction,
        Mahalanobis distances of the L*C*N sampled latents, the importance-weight assembly) run on the HIP kernels.

        Two halves: what does not depend on the prior (`_all_classes_forward`: features, encoder, the epsilon draw, decoder,
        reconstruction terms) and the tail that does (`_all_classes_tail`: KL, distances, log p(z|y), importance weights, total).
        A fine-tuned model with two priors (jvae_compat/wim.py) runs the first half once and the tail once per prior."""
        fwd = self._all_classes_forward(x, epsilon)
        losses, measures = self._all_classes_tail(fwd, self.encoder.prior, self.num_labels, batch, current_measures, with_beta)
        out = (fwd['x_reco'], _mean_over_draws(fwd['logits']), losses, measures)
        if z_output:
            out += (fwd['mu'], fwd['log_var'], fwd['z'])
        return out

    def _all_classes_forward(self, x, epsilon):
        """The prior-independent half of the label-free evaluation -> the tensors `_all_classes_tail` reads."""
        if self.y_is_coded or self.is_jvae:
            # The reference cannot do it either: cvae.py:593-600 builds the (C, N) label grid and forward() (cvae.py:451)
            # then calls y.view(N) on it - "RuntimeError: shape '[N]' is invalid for input of size C*N" for conv and MLP
            # models alike (probed on the reference in the build container).  Same outcome, clearer message.
            raise NotImplementedError('evaluate(x) without labels is not possible for models with coded labels (the '
                                      'reference fails on it: cvae.py:451): pass y')
        if x.dim() != self.input_dim + 1:
            x = x.reshape(-1, *self.input_shape)
        N = x.shape[0]
        L = self.latent_sampling
        D = int(np.prod(self.input_shape))
        with torch.no_grad():
            feats = self._features_of(x).reshape(N, -1)
            dummy = torch.zeros(N, dtype=torch.int64, device=x.device)
            mu, log_var, z, eps, sigma_coded, _ = self.encoder.encode(feats, None, dummy, 1., epsilon)
            x_, logits = self._decode(z)
            x_reco = x_.view(L + 1, N, *self._reco_shape())
            s, s_kind, sigma_rms = self._sigma_operand(sigma_coded, N)
            categorical = self.output_distribution == 'categorical'
            s_report = s
            if categorical:
                # cvae.py:654-660,672-676: log p(x|z_l) = -(256-level pixel cross entropy); the kernels below take it as the
                # equivalent "weighted mse" of a unit-sigma gaussian: -D/2 (w + log 2 pi) = -ce  <=>  w = 2 ce / D - log 2 pi
                ndim = len(self.input_shape)
                ce_x = categorical_loss(x_reco[1:], x, ndim=ndim, batch_mean=False)          # (L, N)
                levels = x_reco[1:].argmax(-ndim - 1).float() / 255
                wmse_cat = mse_loss(levels, x, ndim=ndim, batch_mean=False).mean(0)
                wmse_s = 2. * ce_x / D - LOG2PI
                s, s_kind = torch.ones(1, device=x.device), ops.SIGMA_VALUE
            else:
                wmse_s = ops.recon_wmse(x_reco, x, s, s_kind)                             # (L, N)
            zero_kl = torch.zeros(N, device=x.device)
            wmse, cross_x, _, mse = ops.elbo(wmse_s, zero_kl, None, s, s_kind, D, 1., 0., with_mse=True)
            if categorical:
                wmse, mse = wmse_cat, None             # what the reference reports: the arg-max image's mean-square error
            cross_y = x_loss(None, logits, batch_mean=False) if self.y_is_decoded else None       # (C, N)
        return dict(x=x, N=N, L=L, D=D, dummy=dummy, mu=mu, log_var=log_var, z=z, eps=eps, x_reco=x_reco, logits=logits, s=s,
                    s_kind=s_kind, s_report=s_report, sigma_rms=sigma_rms, wmse_s=wmse_s, wmse=wmse, cross_x=cross_x, mse=mse,
                    cross_y=cross_y)

    def _all_classes_tail(self, fwd, pr, C, batch, current_measures, with_beta, with_measures=True):
        """The prior-dependent half: the losses of `fwd` under the prior `pr` with `C` candidate classes (one per component of a
        conditional prior) -> (losses, measures); measures None without `with_measures`."""
        x, N, L, D = fwd['x'], fwd['N'], fwd['L'], fwd['D']
        K = self.latent_dim
        mu, log_var, z, cross_x, s, s_kind = fwd['mu'], fwd['log_var'], fwd['z'], fwd['cross_x'], fwd['s'], fwd['s_kind']
        with torch.no_grad():
            y_all = torch.arange(C, device=x.device).unsqueeze(1).expand(C, N)
            kd = pr.kl(mu, log_var, y=y_all if pr.conditional else None)                  # (C, N) each
            losses = {'kl': kd['kl'], 'zdist': kd['distance'], 'var_kl': kd['var_kl']}
            dictionary = pr.mean if pr.conditional else None
            terms = {'distance': kd['distance'].reshape(-1), 'var_kl': kd['var_kl'].reshape(-1)}
            if dictionary is not None:
                _, _, _, _, _, dz = ops.latent(mu, log_var, torch.zeros((1, N, K), device=x.device), fwd['dummy'],
                                               dictionary, pr._var_parameter, var_dim=pr.var_dim, sampled=False)
                losses['dzdist'] = dz
            losses['wmse'], losses['cross_x'] = fwd['wmse'], cross_x
            if self.y_is_decoded:
                losses['cross_y'] = fwd['cross_y']                                        # (C, N)
            beta = self.beta if with_beta else 1.
            # one prior component per class: (C, N); a single prior (type 'vae'): (N,)
            losses['total'] = (cross_x.unsqueeze(0) if pr.conditional else cross_x) + beta * kd['kl']
            if self.y_is_decoded and not (self.is_cvae or self.is_vae) and self.gamma:
                losses['total'] = losses['total'] + self.gamma * losses['cross_y']        # cvae.py:557-563,886-889
            # importance-weighted bound: log p(x|z_l) + log p(z_l|y) - log q(z_l|x), cvae.py:672-676,793-873
            z_s = z[1:]
            if pr.conditional:
                z_y = z_s.unsqueeze(1).expand(L, C, N, K)
                y_s = y_all.unsqueeze(0).expand(L, C, N)
                log_pz = pr.log_density(z_y, y_s)                                         # (L, C, N)
            else:
                log_pz = pr.log_density(z_s, None)                                        # (L, N)
            # rows + max / mean-exp fold over the L samples in one kernel pair (jvae_iws_f32)
            losses['iws'] = ops.iws(fwd['wmse_s'], fwd['eps'], log_var, log_pz, s, s_kind, D)
            if not with_measures:
                return losses, None
            prev = self._prev_measures(current_measures, batch, x.device, upload=False)
            packed = self._pack_measures(x, fwd['wmse'], terms, dictionary, prev, batch, mse=fwd['mse'],
                                         sigma_rms=fwd['sigma_rms'], sigma_t=fwd['s_report'])
        return losses, Measures(packed, dictionary is not None, _grad_nan_exit)

    def predict_after_evaluate(self, logits, losses, method='default'):
        """Class prediction from the all-class losses (cvae.py:938-970)."""
        if method == 'default':
            method = self.predict_methods[0]
        if method is None:
            return logits.softmax(-1)
        table = {'iws': lambda: losses['iws'].argmax(0), 'closest': lambda: losses['zdist'].argmin(0),
                 'loss': lambda: losses['total'].argmin(0), 'esty': lambda: logits.argmax(-1),
                 'mean': lambda: logits.softmax(-1).mean(0).argmax(-1), 'already': lambda: losses['y_est_already']}
        if method not in table:
            raise ValueError(f'Unknown method {method}')
        return table[method]()

    def predict(self, x, method=None, **kw):
        _, logits, losses, _ = self.evaluate(x)
        return self.predict_after_evaluate(logits, losses, method=method or 'default')

    # ------------------------------------------------------------------------------------ ODIN (type 'vib')
    def _odin_slab_rows(self):
        """Rows of the perturbed batch that go through `features` at once: no activation passes EVAL_SLAB_ELEMENTS."""
        env = os.environ.get('JVAE_EVAL_SLAB_ROWS')                 # tests: force many small slabs
        if env:
            return max(int(env), 1)
        widest = max([int(np.prod(self.input_shape))] + [int(np.prod(sh)) for sh in getattr(self.features, 'shapes', [])])
        return max(self.EVAL_SLAB_ELEMENTS // widest, 1)

    def _odin_logits(self, feats, epsilon):
        """Encoder features (R, D) -> logits (L+1, R, C): the part of forward() ODIN reads (cvae.py:1649-1651)."""
        _, _, z, _, _ = self.encoder(feats, None, epsilon=epsilon)
        if self.classifier_type in ('linear', None):
            return self.classifier(z)
        m = self.encoder.prior.mean
        return ops.linear(z, m, m.pow(2).sum(-1) / 2)

    def odin_scores(self, x, epsilon=None, acc_out=None):
        """The ODIN out-of-distribution scores of a batch (Liang et al.; cvae.py:1645-1663) for every temperature of
        `ODIN_TEMPS` and perturbation size of `ODIN_EPS`: {'odin-T-eps': (N,) fp32 device tensor}, in evaluation mode.

            acc = 0
            for T:   s = max softmax(logits(x)[1:].mean(0) / T);  acc += d(sum s)/dx;  dx = sign(acc)
                     for eps:  score = max softmax(logits(x + eps * dx)[1:].mean(0) / T)

        Reproduced from the reference as written: (1) the input gradient ACCUMULATES over the temperatures (x.grad is never
        zeroed there), the sign at temperature k is that of the sum of the gradients of temperatures 1..k; (2) every forward
        draws its own reparameterisation noise; (3) row 0 of the draws (the mean latent) is left out of the mean and gets no
        gradient from the score - the gradient reaches mu / log_var through rows 1..L.  The perturbed image is not clamped.
        One deliberate difference: the reference's backward() also fills every parameter's .grad, which it never uses; here
        the input gradient alone is computed - no weight-gradient kernel runs and every .grad stays as it was.

        Underneath: per temperature the E perturbed forwards are ONE batch of E*N rows, cut into slabs for the conv stack
        (`_odin_slab_rows`); the T gradient passes share one `features(x)` forward and differ from the encoder on; the head
        (csrc/odin.hip) turns the logits of all T*E forwards into scores in one launch; the call is one span of constant
        weights and brings no value to the host.  `epsilon` (T, 1+E, L+1, N, K) injects the noise: slot [t, 0] is the
        gradient pass of temperature t, slot [t, 1+e] perturbed forward e.  `acc_out`: a list that receives a copy of the
        accumulated input gradient after each temperature (tests, diagnostics).  fp32 only."""
        if getattr(self, 'compute_dtype', 'fp32') != 'fp32':
            raise NotImplementedError('ODIN scores are built for the fp32 compute mode (set_compute_dtype("fp32"))')
        if self.classifier_type is None or self.y_is_coded:
            raise NotImplementedError('ODIN needs a classifier on z of a model without coded labels (type vib)')
        x = x.detach().reshape(-1, *self.input_shape)
        dev, N = x.device, x.shape[0]
        temps, sizes = list(self.ODIN_TEMPS), list(self.ODIN_EPS)
        T, E, K, C = len(temps), len(sizes), self.latent_dim, self.num_labels
        if epsilon is not None and tuple(epsilon.shape[:2]) != (T, 1 + E):
            raise ValueError(f'epsilon: (T, 1 + E, L+1, N, K) = ({T}, {1 + E}, ...) expected, got {tuple(epsilon.shape)}')
        was_training = self.training
        self.eval()
        L = self.latent_sampling
        frozen = [p for p in self.parameters() if p.requires_grad]
        for p in frozen:                      # input gradients only: no node of the gradient pass asks for a weight gradient
            p.requires_grad_(False)
        _lib.span_hold += 1
        try:
            with self._constant_weights(x):
                t_dev = torch.tensor([float(t) for t in temps for _ in sizes], dtype=torch.float32, device=dev)
                e_dev = torch.tensor([float(e) for e in sizes], dtype=torch.float32, device=dev)
                with torch.enable_grad():
                    xg = x.detach().requires_grad_(True)
                    feats = self._features_of(xg).reshape(N, -1)        # shared by the T gradient passes
                acc = torch.zeros_like(x)
                logits_all = torch.empty((L + 1, T, E * N, C), dtype=torch.float32, device=dev)
                slab = self._odin_slab_rows()
                for t in range(T):
                    with torch.enable_grad():
                        logits = self._odin_logits(feats, None if epsilon is None else epsilon[t, 0])
                    with torch.no_grad():
                        _, dlogits = ops.odin_head(logits.detach().unsqueeze(0), t_dev[t * E:t * E + 1], want_grad=True)
                    g, = torch.autograd.grad(logits, xg, grad_outputs=dlogits[0], retain_graph=t + 1 < T)
                    with torch.no_grad():
                        xp = ops.odin_perturb(acc, g, x, e_dev)         # (E * N, ...): acc += g, x + eps_e * sign(acc)
                        if acc_out is not None:
                            acc_out.append(acc.clone())
                        if self.features:
                            fp = torch.empty((E * N, feats.shape[1]), dtype=torch.float32, device=dev)
                            for r0 in range(0, E * N, slab):
                                fp[r0:r0 + slab] = self.features(xp[r0:r0 + slab]).reshape(-1, feats.shape[1])
                        else:
                            fp = xp.reshape(E * N, -1)
                        noise = None if epsilon is None else epsilon[t, 1:].transpose(0, 1).reshape(L + 1, E * N, K)
                        logits_all[:, t] = self._odin_logits(fp, noise)
                with torch.no_grad():
                    scores = ops.odin_head(logits_all.view(L + 1, T * E, N, C), t_dev, forwards_first=False)      # (T * E, N)
        finally:
            _lib.span_hold -= 1
            for p in frozen:
                p.requires_grad_(True)
            if was_training:
                self.train()
        return dict(zip(self._odin_names(), scores))

    # ------------------------------------------------------------------------------------ likelihood regret
    def _regret_objective(self, z, kl, x, s, s_kind, want_grad):
        """J (N,) = cross_x + kl, the `total` of evaluate(..., with_beta=False), at the draws z (L+1, N, K) of a posterior whose
        KL terms are `kl`, and with `want_grad` the decoder's part of its gradient, d(sum_n cross_x_n)/dz (L+1, N, K): rows are
        independent in eval mode, so that is each sample's own.  Samples go through the decoder in slabs of `_eval_slab_rows()`
        rows ((L+1) rows per sample); nothing asks for a weight gradient (the caller froze the parameters)."""
        Lp1, N, K = z.shape
        D = int(np.prod(self.input_shape))
        per = max(self._eval_slab_rows() // Lp1, 1)
        J = dz = None
        for n0 in range(0, N, per):
            n1 = min(N, n0 + per)
            whole = n0 == 0 and n1 == N
            zs = z if whole else z[:, n0:n1].contiguous()
            sig = s[n0:n1] if s_kind == ops.SIGMA_CODED else s
            with torch.enable_grad() if want_grad else torch.no_grad():
                if want_grad:
                    zs = zs.detach().requires_grad_(True)
                x_reco = self._decode_rows(zs).view(Lp1, n1 - n0, *self._reco_shape())
                wmse_s = ops.recon_wmse(x_reco, x[n0:n1], sig, s_kind)
                _, cross_x, total = ops.elbo(wmse_s, kl[n0:n1], None, sig, s_kind, D, 1., 0.)
                g = torch.autograd.grad(cross_x, zs, grad_outputs=torch.ones_like(cross_x))[0] if want_grad else None
            if whole:
                J, dz = total.detach(), None if g is None else g.contiguous()
                break
            if J is None:
                J = torch.empty(N, dtype=torch.float32, device=z.device)
                dz = torch.empty_like(z) if want_grad else None
            J[n0:n1] = total.detach()
            if want_grad:
                dz[:, n0:n1] = g
        return J, dz

    def likelihood_regret(self, x, y=None, steps=5, lr=0.05, epsilon=None, trajectory=None, evaluated=None):
        """The likelihood regret of a batch (Xiao, Yan, Amit, NeurIPS 2020): how much a sample's ELBO improves when its own
        posterior is optimised for `steps` Adam steps of learning rate `lr` with every weight frozen, in evaluation mode
        -> (regret (N,), mu (N, K), log_var (N, K)): the refined posterior with it.  Larger regret = more out of distribution
        (the `regret-*` score rows record MINUS this value).

            (mu_0, lv_0) = the encoder's posterior, bit for bit latent_posterior()'s
            for t < steps:  z_t = mu_t + exp(lv_t / 2) eps_t;  J_t = mean_l(-log p(x | z_tl)) + KL(q_t || p(z | y))
                            (mu, lv)_{t+1} = Adam step t + 1 on d J_t / d (mu_t, lv_t)      [per sample: Adam is elementwise]
            regret = J(mu_0, lv_0; eps_T) - J(mu_T, lv_T; eps_T)

        J is `total` as evaluate(x, y, with_beta=False) reports it, the scale of the `elbo` score.  Deliberately not the
        paper's: only the posterior's parameters move, not the encoder's weights, and both ELBOs of the difference share
        their noise eps_T (common random numbers), so that zero steps give exactly zero.

        y: the class of each sample under a class-conditional prior; without it the prediction (first predict method) of one
        label-free evaluate(x), or of `evaluated` = (logits, losses) when the caller already has that pass.  `epsilon`
        (steps + 1, L, N, K) injects the noise, L = the evaluation `latent_sampling`; slot 0 also serves the label-free pass.
        `trajectory`: a list that receives (mu_t, log_var_t, J_t) copies for t = 0 .. steps (J_steps under eps_T).

        Underneath, one iteration is the decoder forward, `ops.recon_wmse`, `ops.elbo`, their input-gradient passes back to z
        (eval-mode BatchNorm backward, no weight-gradient kernel: every .grad stays as it was) and ONE `ops.latent_refine`
        launch for gradient, Adam step and the next draw; the call is one span of constant weights and brings nothing to the
        host.  Types cvae, vae and xvae with a gaussian decoder and a fixed, decayed, learned or coded sigma, fp32 only."""
        if getattr(self, 'compute_dtype', 'fp32') != 'fp32':
            raise NotImplementedError('the likelihood regret is built for the fp32 compute mode (set_compute_dtype("fp32"))')
        if self.type not in self.REGRET_TYPES or self.y_is_coded:
            raise NotImplementedError(f'the likelihood regret needs a decoder and a model without coded labels (types '
                                      f'{", ".join(self.REGRET_TYPES)}), not type {self.type}')
        if self.output_distribution != 'gaussian':
            raise NotImplementedError(f'the likelihood regret is built for the gaussian decoder, not {self.output_distribution}')
        if self.sigma.is_rmse:
            raise NotImplementedError('the likelihood regret with a sigma that follows the rmse (is_rmse) is not built: that '
                                      'sigma is no constant of the refinement')
        enc = self.encoder
        pr = enc.prior
        if enc.mixed_prior is not None:
            raise NotImplementedError('the likelihood regret under a mixed prior is not built')
        steps = int(steps)
        if steps < 0 or not lr > 0:
            raise ValueError(f'steps {steps} >= 0 and lr {lr} > 0 expected')
        x = x.detach().reshape(-1, *self.input_shape)
        dev, N, K = x.device, x.shape[0], self.latent_dim
        was_training = self.training
        self.eval()
        L = self.latent_sampling
        if epsilon is not None and tuple(epsilon.shape) != (steps + 1, L, N, K):
            raise ValueError(f'epsilon: (steps + 1, L, N, K) = {(steps + 1, L, N, K)} expected, got {tuple(epsilon.shape)}')
        frozen = [p for p in self.parameters() if p.requires_grad]
        for p in frozen:                      # input gradients only: no node of a gradient pass asks for a weight gradient
            p.requires_grad_(False)
        _lib.span_hold += 1
        try:
            with torch.no_grad(), self._constant_weights(x):
                if epsilon is None:
                    eps = draw_epsilon(L, (steps + 1, N, K), dev, enc.sampling.distribution).transpose(0, 1).contiguous()
                else:
                    eps = torch.cat((torch.zeros((steps + 1, 1, N, K), dtype=torch.float32, device=dev),
                                     epsilon.to(dev, torch.float32)), 1)
                feats = self._features_of(x).reshape(N, -1)
                u, mu0, raw0 = enc.heads(feats, None)
                if self.sigma.coded:          # taken once from the encoder pass; the Sigma parameter is not touched
                    s, s_kind = enc.sigma(u).reshape(N).contiguous(), ops.SIGMA_CODED
                else:
                    s, s_kind = self.sigma.detach(), (ops.SIGMA_LOG if self.sigma.is_log else ops.SIGMA_VALUE)
                if pr.conditional:
                    if y is None:
                        if evaluated is None:
                            evaluated = self.evaluate(x, epsilon=None if epsilon is None else eps[0])[1:3]
                        y = self.predict_after_evaluate(*evaluated)
                    y = y.reshape(-1).to(dev, torch.int64)
                lab, means, T = pr._kernel_operands(y if pr.conditional else None, N, dev)
                forced = math.log(enc.forced_variance) if enc.forced_variance else None
                kw = dict(prior=pr.distribution, var_dim=pr.var_dim, tau=pr._tau, alpha=pr._alpha_k,
                          sampled=bool(enc.sampling.is_sampled), forced_lv=forced)
                mu0, raw0 = mu0.contiguous(), None if raw0 is None else raw0.contiguous()
                mu, raw, lv = mu0.clone(), None if raw0 is None else raw0.clone(), torch.empty_like(mu0)
                z, kl = ops.latent_refine(mu, raw, lv, lab, means, T, eps_next=eps[0], **kw)[:2]
                state = ops.latent_refine_state(mu, forced is not None)
                for t in range(steps):
                    J, dz = self._regret_objective(z, kl, x, s, s_kind, True)
                    if trajectory is not None:
                        trajectory.append((mu.clone(), lv.clone(), J))
                    z, kl = ops.latent_refine(mu, raw, lv, lab, means, T, eps_cur=eps[t], dz=dz, state=state, step=t + 1, lr=lr,
                                              eps_next=eps[t + 1], **kw)[:2]
                J_end = self._regret_objective(z, kl, x, s, s_kind, False)[0]
                if trajectory is not None:
                    trajectory.append((mu.clone(), lv.clone(), J_end))
                # the encoder's posterior under the same last noise: a forward-only launch leaves mu0 / raw0 as they are
                z, kl = ops.latent_refine(mu0, raw0, torch.empty_like(mu0), lab, means, T, eps_next=eps[steps], **kw)[:2]
                regret = self._regret_objective(z, kl, x, s, s_kind, False)[0] - J_end
        finally:
            _lib.span_hold -= 1
            for p in frozen:
                p.requires_grad_(True)
            if was_training:
                self.train()
        return regret, mu, lv

    def latent_posterior(self, x, y=None):
        """The encoder's posterior of a batch and nothing else -> (mu, log_var), each (N, K): the feature stack, the two heads of
        the encoder, then the +-20 clip of the log-variance (or the forced variance) as the latent kernel applies it.  No noise is
        drawn, nothing is decoded and no prior is consulted beyond the operand the kernel wants: bit for bit the mu, log_var of
        evaluate(x, y, z_output=True) on the same batch, without the (L + 1) N decoded images and the C-class tail that call
        spends on them (reference module/sample.py::zsample keeps these two tensors of a whole evaluate()).  Models with coded
        labels need y.  Runs under no_grad in both compute dtypes; put the model in eval mode first, as for evaluate()."""
        if y is None and self.y_is_coded:
            raise NotImplementedError('latent_posterior(x) without labels is not possible for models with coded labels (their '
                                      'encoder reads y): pass y')
        if x.dim() != self.input_dim + 1:
            x = x.reshape(-1, *self.input_shape)
            y = None if y is None else y.reshape(-1)
        N = x.shape[0]
        enc = self.encoder
        with torch.no_grad(), self._constant_weights(x):
            feats = self._features_of(x).reshape(N, -1)
            y1h = onehot_encoding(y, self.num_labels).float() if self.y_is_coded else None
            _, mu, lv_raw = enc.heads(feats, y1h)
            K = mu.shape[-1]
            pr = enc.prior
            dummy = torch.zeros(N, dtype=torch.int64, device=x.device)
            lab, means, T = pr._kernel_operands(dummy if pr.conditional else None, N, mu.device)
            forced = math.log(enc.forced_variance) if enc.forced_variance else None
            log_var = ops.latent(mu, mu if lv_raw is None else lv_raw, torch.zeros((1, N, K), device=x.device), lab, means, T,
                                 prior=pr.distribution, var_dim=pr.var_dim, tau=pr._tau, alpha=pr._alpha_k, sampled=False,
                                 forced_lv=forced)[0]
        return mu, log_var

    def _evaluate_for_scores(self, x, batch, measures, with_mu=False, with_reco=False):
        """One batch of the scoring pass: `x` as the data loader yields it -> (x on the device, logits, losses, measures[, mu]
        [, x_reco]).  `with_mu`: the posterior means of the same pass, for the sample recorders.  `with_reco`: the reconstructions
        (L + 1, N, ...) of the same pass as the LAST item, for the families that score them (no second decode).  A subclass
        whose items carry more than the image (jvae_compat/wim.py: (x, y_est) pairs) overrides this."""
        x = self._device_batch(x.to(self.device))
        out = self.evaluate(x, batch=batch, current_measures=measures, z_output=with_mu)
        return (x,) + tuple(out[1:4]) + ((out[4],) if with_mu else ()) + ((out[0],) if with_reco else ())

    def _early_reduce_hook(self, grad):
        self.optimizer.reduce_early_bucket()
        return grad

    def _upload_measures(self, current, device):
        """Running means handed in as plain floats (first batch of a resumed loop, a caller's own dict)."""
        t = torch.zeros(MEASURES_LEN)
        for k in ('xpow', 'mse', 'zdist', 'var_kl'):
            t[MEASURE_INDEX[k]] = float(current.get(k, 0.))
        return t.to(device, non_blocking=True)

    def _prev_measures(self, current_measures, batch, device, upload=True):
        """The device block the running means continue from: a Measures' own, or (`upload`) a plain dict's values sent up."""
        if isinstance(current_measures, Measures):
            return current_measures._dev
        if upload and current_measures and batch:
            return self._upload_measures(current_measures, device)
        return None

    def _sigma_operand(self, sigma_coded, N, store=True):
        """What the loss kernels get as `sigma` (cvae.py:626-646): (tensor, kind, rms) - rms is the device scalar reported
        as the `sigma` measure for the coded / rmse kinds (the parameter's value BEFORE this batch updates it: cvae.py:624),
        None otherwise (the measures kernel derives it from the parameter).  A coded sigma is also stored into the
        parameter (batch mean of the coded log sigma: Sigma.update(v=...), cvae.py:631-634)."""
        sg = self.sigma
        if not (sg.coded or sg.is_rmse):
            return sg, (ops.SIGMA_LOG if sg.is_log else ops.SIGMA_VALUE), None
        with torch.no_grad():
            d = sg.data
            rms = ((2 * d).exp() if sg.is_log else d * d).mean().sqrt().reshape(1)
        if sg.is_rmse:
            return sg, ops.SIGMA_RMSE, rms
        per_sample = sigma_coded.reshape(-1, *sg.output_dim)
        if store:                                # store=False (net.iw_bound): a scoring call leaves the parameter alone
            sg.update(v=per_sample.detach())
        return per_sample.reshape(N), ops.SIGMA_CODED, rms

    def _pack_measures(self, x, wmse, terms, dictionary, prev, batch, mse=None, sigma_rms=None, sigma_t=None, dev_state=None):
        """Every scalar evaluate() reports, computed by one kernel into one 16-float device buffer."""
        if sigma_rms is not None:
            if self.sigma.coded:
                # sic (cvae.py:668): wmse (N,) times sigma^2 (N,1,1,1) broadcasts to (N,1,1,N) in the reference; the mean of
                # that - the only use of `mse` with a coded sigma - is mean(wmse) * mean(sigma^2), reproduced here
                with torch.no_grad():
                    mse = (wmse.detach().mean() * (2 * sigma_t.detach()).exp().mean()).expand(wmse.numel()).contiguous()
            return self._pack_measures_raw(x, mse.detach(), terms, dictionary, prev, batch, sigma_rms, 2, dev_state=dev_state)
        return self._pack_measures_raw(x, wmse.detach(), terms, dictionary, prev, batch, self.sigma.detach(),
                                       int(self.sigma.is_log), dev_state=dev_state)

    def _pack_measures_raw(self, x, wmse, terms, dictionary, prev, batch, sigma_t, sigma_kind, dev_state=None):
        with torch.no_grad():
            if getattr(self, '_scratch', None) is None or self._scratch.device != x.device:
                self._scratch = torch.zeros(1, device=x.device, dtype=torch.float32)
            # logging only: off the critical path -> side stream (the C x C dictionary diagnostics take ~0.2 ms at C = 100)
            main, side = torch.cuda.current_stream(x.device), _lib.side_stream(x.device)
            side.wait_stream(main)
            args = (x, wmse, terms['distance'].detach(), terms['var_kl'].detach(), sigma_t)
            with torch.cuda.stream(side):
                run, counter = dev_state if dev_state is not None else (None, None)      # captured step: see ops.measures
                packed = ops.measures(*args, sigma_kind, None if dictionary is None else dictionary.detach(),
                                      self.optimizer.nonfinite_flag(), self._scratch, prev, batch, run=run, counter=counter)
            for t in args:
                t.record_stream(side)
            return packed

    # ------------------------------------------------------------------------------------ training loop
    def _mean_backward(self, tot):
        """tot.mean().backward() without the reduction kernels of a mean nobody reads and the expand of its backward:
        d(mean)/d(tot_i) = 1/numel, handed to autograd as a cached constant (the same fp32 value as torch's own)."""
        key = (tot.shape, tot.device)
        if getattr(self, '_mean_grad_key', None) != key:
            self._mean_grad = torch.ones_like(tot.detach()) / tot.numel()
            self._mean_grad_key = key
        torch.autograd.backward(tot, grad_tensors=self._mean_grad)

    def train_step(self, x, y, batch=0, current_measures=None, kl_var_weighting=1., gamma_weighting=1., epsilon=None,
                   prior_epsilon=None):
        """One iteration of the reference's hot loop (cvae.py:2429-2461): zero_grad, evaluate, backward, clip, step.
        prior_epsilon: the noise of the prior draws of TRAIN_OBJECTIVE = 'mmd' (no other objective reads it)."""
        self.optimizer.zero_grad()
        extra = {} if prior_epsilon is None else {'prior_epsilon': prior_epsilon}
        _, y_est, losses, measures = self.evaluate(x, y, batch=batch, with_beta=True,
                                                   kl_var_weighting=kl_var_weighting,
                                                   gamma_weighting=gamma_weighting,
                                                   current_measures=current_measures, epsilon=epsilon, **extra)
        if self.optimizer.check_nonfinite():     # cvae.py:2454-2457: a NaN / Inf parameter ends the run BEFORE backward
            _grad_nan_exit()
        self._mean_backward(losses['total'])
        self.optimizer.clip(self.parameters())
        self.optimizer.step()
        return losses, measures

    def graph_train_step(self, x, y, kl_var_weighting=1., gamma_weighting=1., warmup=3):
        """Capture one whole training step (zero_grad, evaluate, backward, clip, Adam - ~250 kernel launches on two
        streams) for batches shaped like (x, y) into a HIP graph; returns `step(x, y) -> (losses, measures)` that copies
        the batch into the captured buffers and replays the graph: one host call per step instead of ~4 ms of Python
        enqueue work.  No counterpart in the reference (its loop is eager).  Differences from train_step(): epsilon is
        drawn inside the graph (the generator's offset advances per replay), `measures` are those of the current batch
        only (batch index 0), the `losses` tensors are the graph's own buffers (overwritten by the next replay), the
        warm-up weights are fixed (kl / gamma weights of the call).  Data parallel (optimizer.set_distributed): see below -
        two captured halves with the gradient all-reduce between them.  Drop every reference to the outputs of earlier EAGER
        steps (losses, measures) before calling this: a live eager autograd graph keeps its gradient-accumulation nodes bound
        to the default stream, which a capture must not touch."""
        self._refuse_captured_iwae('graph_train_step()')
        self._refuse_captured_semi('graph_train_step()')
        world = getattr(self.optimizer, '_world', 1)
        dev = x.device
        self.optimizer.enable_device_hyper(True)
        sx, sy = x.clone(), y.clone()
        forward_backward, update = self._captured_body(sx, sy, kl_var_weighting, gamma_weighting)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):                      # eager warm-up on a side stream (allocations, lazy initialisations)
            for _ in range(max(int(warmup), 1)):
                update(forward_backward())
        torch.cuda.current_stream(dev).wait_stream(s)
        if world > 1:
            # Data parallel: the step is captured in TWO graphs - [zero_grad, forward, backward] and [clip, Adam] - with the
            # gradient exchange (ONE all-reduce of the flat buffer, any backend) issued eagerly between them: three host
            # calls per step.  The early-bucket overlap of the eager path is given up (the exchange is ~0.1 ms of a ~4 ms step).
            def first_half():
                out = forward_backward()
                _lib.join_side_stream()                 # weight gradients of the side stream: inside the captured half
                return out

            with self.optimizer.external_reduce():      # evaluate() must not launch the early-bucket hook while capturing
                graphs, ((losses, (packed, has_dict)), _) = self._capture((first_half, update), dev)
        else:
            graphs, ((losses, (packed, has_dict)),) = self._capture((lambda: update(forward_backward()),), dev)
        return CapturedStep(self, sx, sy, graphs, self.optimizer.all_reduce_flat if world > 1 else None, losses=losses,
                            measures=packed, has_dictionary=has_dict,
                            constants=(self._mean_grad,))       # the graphs read it: alive as long as the step is

    def _captured_body(self, sx, sy, kl_w, gamma_w, bufs=None):
        """THE training step as the captures record it, on the static batch (sx, sy): -> (forward_backward, update), the whole
        step being update(forward_backward()); the two-graph data-parallel form records each half into a graph of its own.
        Without `bufs` (graph_train_step) the weights are host constants and the measures those of batch 0; with `bufs`
        (_capture_buffers; capture_train_step) they are device words, and the last launch adds the loss means to the epoch sums."""
        opt = self.optimizer
        on_device = {} if bufs is None else {'_dev_weights': bufs['weights'], '_dev_state': (bufs['run'], bufs['counter'])}

        def forward_backward():
            opt.zero_grad()
            _, _, losses, raw = self.evaluate(sx, sy, batch=0, with_beta=True, kl_var_weighting=kl_w, gamma_weighting=gamma_w,
                                              _raw_measures=True, **on_device)
            self._mean_backward(losses['total'])        # (its constant was created by the eager warm-up, not captured)
            return losses, raw

        def update(out=None):
            opt.clip(self.parameters())
            opt.step()
            if bufs is not None:
                ops.loss_sums(list(out[0].values()), bufs['sums'])      # the step's last launch
            return out

        return forward_backward, update

    def _capture(self, parts, device):
        """Record each callable of `parts` into a HIP graph of its own, all in the first one's memory pool: -> (graphs, what
        the callables returned).  Nothing executes, so the host step count the recorded step() advanced is taken back."""
        torch.cuda.synchronize(device)
        graphs, results = [], []
        for part in parts:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=graphs[0].pool() if graphs else None):
                results.append(part())
            graphs.append(graph)
        self.optimizer.forget_captured_step()
        return graphs, results

    # ---- the captured step of train_model() (TRAIN_CAPTURED) ----------------------------------------------------------
    def _capture_buffers(self, device):
        """The device words a captured step shares with the loop: ONE 40-float block that one copy reads back (STATE_RUN,
        STATE_SUMS, STATE_FLAG: the optimiser's non-finite flag moves into it), the batch counter and the two warm-up weights."""
        b = getattr(self, '_capt_bufs', None)
        if b is None or b['state'].device != device:
            state = torch.zeros(STATE_LEN, device=device, dtype=torch.float32)
            b = self._capt_bufs = {'state': state, 'run': state[STATE_RUN], 'sums': state[STATE_SUMS],
                                   'flag': state.view(torch.int32)[STATE_FLAG:STATE_FLAG + 1],
                                   'counter': torch.zeros(1, device=device, dtype=torch.int32),
                                   'weights': torch.ones(2, device=device, dtype=torch.float32)}
        opt = self.optimizer
        if opt._flag is None or opt._flag.data_ptr() != b['flag'].data_ptr():
            if opt._flag is not None and opt._flag.device == device:
                b['flag'].copy_(opt._flag)           # the update kernels raise the flag inside the block from now on
            else:
                b['flag'].zero_()
            opt._flag = b['flag']
        return b

    def _capture_key(self, x, y, cross_y_on):
        """What a captured step is valid for: the batch's shape, the set of trainable parameters and where they (and the
        optimiser's device words) live, the number of latent draws, whether cross_y is part of the loss.  The learning rate
        and the warm-up weights are NOT in it: they are device words the replay reads."""
        opt = self.optimizer
        return (tuple(x.shape), str(x.dtype), tuple(y.shape), str(x.device), self.latent_sampling, bool(cross_y_on),
                getattr(self, 'compute_dtype', 'fp32'),
                tuple((id(p), p.data_ptr()) for p in self.parameters() if p.requires_grad),
                tuple((g.p.data_ptr(), getattr(g, 'hyper', None) is not None and g.hyper.data_ptr()) for g in opt._groups),
                None if opt._flag is None else opt._flag.data_ptr())

    def _cross_y_on(self, gamma_weighting):
        if not self.y_is_decoded:
            return False
        return bool(gamma_weighting * self.gamma)

    def capture_train_step(self, x, y, kl_var_weighting=1., gamma_weighting=1.):
        """The captured step train_model() replays (TRAIN_CAPTURED): sibling of graph_train_step() that is fit for a loop.
        * NO optimiser step is taken here: the caller has run its eager warm-up (CAPTURE_WARMUP_BATCHES real batches through
          train_step(), with optimizer.enable_device_hyper(True)); capture executes nothing and the host step count is rolled
          back.
        * kl_var_weighting and the cross_y weight (gamma_weighting * gamma) are read by the latent and ELBO kernels from a
          device buffer (`step.set_weights()`); the values given here only seed it.
        * the running measures continue from replay to replay: the batch index is a device counter the measures kernel
          increments (`step.seed_measures(prev, batch)` / `step.reset_epoch()`).
        * the step's last launch adds the mean of every loss row to the running sums (ops.loss_sums).
        * `step.epsilon`: the (L, N, K) noise of the replay that has just run; `step.losses`: the graph's loss rows.
        step(x, y) copies the batch in, replays and returns `step.losses`.  Single process only."""
        self._refuse_captured_iwae('capture_train_step()')
        self._refuse_captured_semi('capture_train_step()')
        if getattr(self.optimizer, '_world', 1) > 1:
            raise NotImplementedError('capture_train_step() is single-process: data-parallel models use graph_train_step()')
        if self.optimizer.kind != 'adam':
            raise NotImplementedError('capture_train_step() needs the device-side hyper-parameters of the Adam kernel')
        if not getattr(self.optimizer, '_device_hyper', False) or not self.optimizer._groups \
                or any(getattr(g, 'hyper', None) is None for g in self.optimizer._groups):
            raise RuntimeError('capture_train_step(): run the eager warm-up steps with optimizer.enable_device_hyper(True) first')
        dev = x.device
        bufs = self._capture_buffers(dev)
        opt = self.optimizer
        sx, sy = x.clone(), y.clone()
        forward_backward, update = self._captured_body(sx, sy, kl_var_weighting, gamma_weighting, bufs)
        was_training = self.training
        self.train()
        try:
            graphs, ((losses, _),) = self._capture((lambda: update(forward_backward()),), dev)
        finally:
            self.train(was_training)
        self._captures_built = self._captures_built + 1
        step = CapturedStep(self, sx, sy, graphs, losses=losses, has_dictionary=self.encoder.prior.conditional, buffers=bufs,
                            constants=(self._mean_grad, [g.hyper for g in opt._groups], opt._sqnorm,
                                       getattr(self, '_scratch', None)))    # what the graph reads besides the model
        step.set_weights(kl_var_weighting, gamma_weighting)
        step.epsilon = self._last_epsilon
        step.key = self._capture_key(x, y, self._cross_y_on(gamma_weighting))
        return step

    def _read_captured_state(self, bufs):
        """THE read-back of the captured loop: measures, loss sums and the non-finite flag in one copy (it synchronises).
        A NaN / Inf parameter ends the run here, as _grad_nan_exit() does on the eager path."""
        h = bufs['state'].tolist()
        if measures_nonfinite(h):
            _grad_nan_exit()
        return h

    def _measures_from_host(self, h, has_dictionary):
        return decode_measures(h, has_dictionary, only=('sigma', 'zdist', 'var_kl') if self.is_vib else None)

    def _report_batch(self, outputs, i, per_epoch, epoch, epochs, batch_size, t0, report_every, shown, read, unheard=False):
        """The end of train batch `i`, both loops: the progress line of `outputs`.  Every `report_every` batches and at the
        epoch's last one `read() -> (mean losses, measures)`, the loop's read-back, refreshes `shown` - for a listening
        `outputs`, or (`unheard`) whether anybody listens; the batches between show the losses last read and NaN measures."""
        listening = outputs is not None and hasattr(outputs, 'results')
        fresh = i % report_every == 0 or i + 1 == per_epoch
        if fresh and (listening or unheard):
            shown['losses'], shown['metrics'] = read()
        if listening:
            outputs.results(i, per_epoch, epoch + 1, epochs, preambule='train',
                            losses={k: shown['losses'].get(k, float('nan')) for k in self.loss_components},
                            metrics={k: shown['metrics'][k] if fresh else float('nan') for k in self.metrics},
                            accuracy={k: np.nan for k in self.predict_methods},
                            time_per_i=(time.time() - t0) / (i + 1), batch_size=batch_size, end_of_epoch='\n')

    def _train_epoch_eager(self, batches, epoch, epochs, batch_size, w_kl, w_gamma, outputs, report_every):
        """The train phase of one epoch, one train_step() per batch (cvae.py:2424-2501): -> (mean_loss, measures dict)."""
        per_epoch = len(batches)
        hook = self._train_batch_hook
        t0 = time.time()
        measures, nb = None, 0
        keys, acc = None, None          # running sums of the batch means of every loss: ONE device vector
        shown = {'losses': {}, 'metrics': {}}

        def read():                     # the only read-back of the loop: every k batches, for a listening `outputs`
            return dict(zip(keys, (acc / nb).tolist())), {k: measures[k] for k in self.metrics}

        for i, (x, y) in enumerate(batches):
            losses, measures = self.train_step(x, y, batch=i, current_measures=measures,
                                               kl_var_weighting=w_kl, gamma_weighting=w_gamma)
            if hook is not None:
                hook(epoch, i, x, y, self._last_epsilon, losses)
            if keys is None:
                keys = list(losses)
                acc = torch.zeros(len(keys), device=x.device)
            # one small kernel per batch (stack of means) instead of the reference's .item() per loss (cvae.py:2463-2469)
            acc += torch.stack([losses[k].detach().mean() for k in keys])
            nb = i + 1
            self._report_batch(outputs, i, per_epoch, epoch, epochs, batch_size, t0, report_every, shown, read)
        mean_loss = dict(zip(keys or [], (acc / max(nb, 1)).tolist() if acc is not None else []))
        return mean_loss, dict(measures or {})

    def _train_epoch_captured(self, batches, epoch, epochs, batch_size, w_kl, w_gamma, outputs, report_every):
        """The train phase of one epoch with TRAIN_CAPTURED: -> (mean_loss, measures dict).  Full-size batches are replays of
        the captured step; the first CAPTURE_WARMUP_BATCHES of an epoch that has to (re-)capture and the ragged last batch
        go through train_step().  One read-back every `report_every` batches and at the last one; no other host
        synchronisation."""
        opt = self.optimizer
        per_epoch = len(batches)
        hook = self._train_batch_hook
        if not getattr(opt, '_device_hyper', False):
            opt.enable_device_hyper(True)
        step = getattr(self, '_captured_step', None)
        bufs, keys, measures, t0 = None, None, None, time.time()
        shown, warm, checked, nb = {'losses': {}, 'metrics': {}}, 0, False, 0
        has_dict = self.encoder.prior.conditional

        def read():
            h = self._read_captured_state(bufs)
            return {k: v / nb for k, v in zip(keys, h[STATE_SUMS])}, self._measures_from_host(h, has_dict)

        for i, (x, y) in enumerate(batches):
            if bufs is None:
                bufs = self._capture_buffers(x.device)
                bufs['sums'].zero_()
                bufs['counter'].zero_()
            full = x.shape[0] == batch_size
            if full and step is not None and not checked \
                    and step.key != self._capture_key(x, y, self._cross_y_on(w_gamma)):
                step = self._captured_step = None      # thawed prior means, .to(), a re-flattened optimiser, another batch shape
            checked = checked or full                  # once per epoch: nothing in the loop changes the key
            if full and step is None and warm >= self.CAPTURE_WARMUP_BATCHES:
                measures = None                        # no live eager autograd graph may reach into the capture
                step = self._captured_step = self.capture_train_step(x, y, w_kl, w_gamma)
            if full and step is not None:
                if i == 0 or warm:
                    step.set_weights(w_kl, w_gamma)    # once per epoch
                    warm = 0
                losses = step(x, y)
                eps = step.epsilon
                keys = step.keys
            else:
                if i and measures is None:             # eager after replays (the ragged batch): continue their running means
                    measures = Measures(bufs['run'].clone(), has_dict, _grad_nan_exit, from_main=True)
                losses, measures = self.train_step(x, y, batch=i, current_measures=measures,
                                                   kl_var_weighting=w_kl, gamma_weighting=w_gamma)
                eps = self._last_epsilon
                keys = list(losses)
                ops.loss_sums([losses[k] for k in keys], bufs['sums'])
                torch.cuda.current_stream(x.device).wait_stream(_lib.side_stream(x.device))
                bufs['run'].copy_(measures._dev)       # the block always holds the latest measures, whichever path ran
                bufs['counter'].fill_(i + 1)
                if full:
                    warm += 1
                else:
                    measures = None
            if hook is not None:
                hook(epoch, i, x, y, eps, losses)
            del losses
            nb = i + 1
            self._report_batch(outputs, i, per_epoch, epoch, epochs, batch_size, t0, report_every, shown, read, unheard=True)
        if not shown['metrics']:
            return {}, {}
        if not self.is_vib:
            self.training_parameters['sigma'] = self.sigma.host_params(shown['metrics']['sigma'])
        return dict(shown['losses']), dict(shown['metrics'])

    @_restores_tc_dataset_size
    def train_model(self, trainset=None, transformer=None, data_augmentation=None, optimizer=None, epochs=50,
                    batch_size=100, test_batch_size=100, validation=4096, device=None, testset=None, oodsets=None,
                    acc_methods=None, fine_tuning=False, warmup=[0, 0], warmup_gamma=[0, 0], latent_sampling=None,
                    validation_sample_size=1024, full_test_every=10, ood_detection_every=10, train_accuracy=False,
                    save_dir=None, outputs=None, signal_handler=None, report_every=10):
        """Training loop with the reference's signature, bookkeeping and phases (cvae.py:2081-2547).

        `trainset` is a map-style dataset of (image, int label) - what utils/torch_load.get_dataset() returns (train.py:236-243
        hands it over with `.name`, `.transformer` and, for the torchvision sets, the raw images in `.data` / `.targets`), or any
        torch Dataset: float tensors in [0,1] shaped like `input_shape`, or RAW uint8 images ((H,W,C) or (C,H,W)), which are
        converted - and augmented - on the device.  A name (a string; None on resume: the recorded set) is opened from
        `DATA_ROOT` as a device-resident set when that attribute is set (jvae_compat/torch_load.py; the test split too when no
        `testset` is given, cvae.py:2160-2162), and refused when it is None, the default.

        What the reference does and this does too (same order):
        * `training_parameters` gets `epochs`, and - for an untrained net only - `set` (trainset.name), `transformer`
          (trainset.transformer), `validation`, `full_test_every`, `batch_size`, `latent_sampling`, `data_augmentation`
          (cvae.py:2108-2145: train.py:224-229 reads them back on --resume), then `validation_split_seed`, `warmup`,
          `warmup_gamma` (element-wise max with the recorded ones, cvae.py:2196-2202);
        * a seeded `random_split` holds `validation` samples out; training runs on the remainder (cvae.py:2164-2167);
        * every epoch (and once more at epoch == epochs) starts with the test phase: `accuracy(testset)` every
          `full_test_every` epochs -> history `test_accuracy / test_measures / test_loss`, `accuracy(validationset)` every
          epoch -> `validation_accuracy / _measures / _loss`, with `record-<set>.pth` written under `save_dir/samples/{last,
          <epoch>}` (cvae.py:2293-2382); `train_accuracy=True` adds `accuracy(trainset)` -> `train_accuracy`;
        * the hot loop cvae.py:2424-2501 = train_step(); the final test pass of cvae.py:2528-2545.
        The OOD phase (`oodsets`, cvae.py:2309-2336,2513-2526) is an opt-in, `TRAIN_OOD_PHASE` (class attribute, settable per
        instance).  Off (the default): a warning says so once and the phase is skipped - call `ood_detection_rates()` after
        training.  On: every `ood_detection_every` epochs and at epoch == epochs the test phase starts with
        `ood_detection_rates(oodsets, testset, batch_size=test_batch_size, num_batch='all', recorders=..., sample_dirs=...)`
        over this model's `ood_methods` (rows outside the build are left out, said in that function's one log line) ->
        `ood_results[epoch]` (`ood.json` in `save()`), `record-<set>.pth` / `record-<oodset>.pth` under `save_dir/samples/{last,
        <epoch>}` (the directories are then made on OOD epochs too); the `accuracy(testset)` of the same epoch reads the test
        set's full recorder back instead of evaluating again.  The same call runs once more after the loop, before the final
        accuracy pass, unless a signal above 1 came in.  OOD sets given by name raise NotImplementedError unless `DATA_ROOT` is set, as elsewhere;
        `sample_recorders` stay outside this build.

        data_augmentation: the reference hands the list to its dataset factory, which prepends RandomHorizontalFlip ('flip')
        and RandomCrop(size, padding=size//8 [0 for imagenet sets], padding_mode='edge') ('crop') to the training transforms
        (utils/torch_load.py:405-426) - it re-opens the dataset BY NAME for that (cvae.py:2160-2162), so train.py passes the
        un-augmented float (ToTensor) dataset together with the list.  Here the two transforms run on the device, one launch
        per batch (ops.augment_batch: flip, edge-pad crop, /255, bit-exact against the torchvision chain), on the raw uint8
        images: those the dataset yields, or - for a float dataset - those it CARRIES (`.data` uint8 + `.targets` / `.labels`,
        as torchvision's CIFAR / SVHN objects do), once two samples have shown that `dataset[i]` is exactly `data[i] / 255`
        (i.e. its own transform is ToTensor and nothing else).  A float dataset without raw images, or a token other than
        'flip' / 'crop', raises instead of training silently un-augmented.  `outputs.results` gets the running batch-mean
        losses the reference prints (cvae.py:2463-2479), refreshed from the device every `report_every` batches (extra
        keyword) so that the loop does not synchronise per batch.  The batch size is clamped to `max_batch_sizes['train']`."""
        if isinstance(trainset, str):
            if self.DATA_ROOT is None:
                raise NotImplementedError('named torchvision datasets are host-side plumbing outside this build: '
                                          'pass a torch.utils.data.Dataset')
            opened = self._open_named(trainset, 'train', transformer or 'default')      # cvae.py:2160-2162
            if testset is None:
                testset = self._open_named(trainset, 'test', opened.transformer)
            trainset = opened
        if epochs:
            self.training_parameters['epochs'] = epochs
        set_name = None
        if trainset is not None:                 # cvae.py:2111-2118
            set_name = getattr(trainset, 'name', None)
            if not set_name:
                set_name = str(trainset).splitlines()[0].split()[-1].lower()
            transformer = getattr(trainset, 'transformer', transformer)
        if self.trained:                         # cvae.py:2120-2122: a partially trained net keeps its recorded parameters
            logging.info('Network partially trained (%d epochs)', self.trained)
        else:
            if trainset is not None:
                self.training_parameters.update({'set': set_name, 'transformer': transformer, 'validation': validation,
                                                 'full_test_every': full_test_every})
            if batch_size:
                self.training_parameters['batch_size'] = batch_size
            if latent_sampling:
                self._latent_samplings['train'] = latent_sampling
                self.training_parameters['latent_sampling'] = latent_sampling
            if data_augmentation:
                self.training_parameters['data_augmentation'] = list(data_augmentation)
        if not self.training_parameters.get('set'):
            if trainset is None:
                raise AssertionError("training_parameters['set'] is empty and no trainset was given (cvae.py:2147)")
            self.training_parameters['set'] = set_name        # a resumed job whose record lacks the key (written before round 5)
        set_name = str(self.training_parameters['set'])
        if trainset is None:
            if self.DATA_ROOT is None:
                raise NotImplementedError('re-opening the recorded set {!r} by name is torchvision plumbing outside this build: '
                                          'pass the dataset (train.py:224-226 does)'.format(set_name))
            trainset = self._open_named(set_name, 'train')
            if testset is None:
                testset = self._open_named(set_name, 'test')
        data_augmentation = list(self.training_parameters.get('data_augmentation') or [])
        full_test_every = self.training_parameters.get('full_test_every', 10)
        unknown = [t for t in data_augmentation if t not in ('flip', 'crop')]
        if unknown:
            raise ValueError('data_augmentation: only flip and crop exist (utils/torch_load.py:405-413), got {}'.format(unknown))
        # cvae.py:2155-2158 asks for the key 'validation_split_seed ' (trailing blank), which never exists: the reference draws
        # a new seed in EVERY call, a resumed one included.  Same here.
        np.random.seed()
        seed = int(np.random.randint(0, 2 ** 12))
        self.training_parameters['validation_split_seed'] = seed
        if validation >= len(trainset):          # the reference's random_split([v, n - v]) would leave an EMPTY training set
            raise ValueError('validation={} leaves nothing of the {} training samples to train on'.format(validation, len(trainset)))
        validationset, trainset = torch.utils.data.random_split(trainset, [validation, len(trainset) - validation],
                                                                generator=torch.Generator().manual_seed(seed))
        validationset.name = 'validation'
        validation_sample_size = min(validation, validation_sample_size)
        device = device or self.device
        optimizer = optimizer or self.optimizer
        max_batch_sizes = self.max_batch_sizes
        test_batch_size = min(max_batch_sizes['test'], test_batch_size)
        if batch_size:                           # cvae.py:2180-2194
            train_batch_size = min(batch_size, max_batch_sizes['train'])
        else:
            train_batch_size = max_batch_sizes['train']
        logging.info('Train batch size is {}'.format(train_batch_size))
        batch_size = train_batch_size
        self.training_parameters['batch_size'] = batch_size
        warmup, warmup_gamma = list(warmup), list(warmup_gamma)
        warmup_ = self.training_parameters.get('warmup', [0, 0])
        warmup_gamma_ = self.training_parameters.get('warmup_gamma', [0, 0])
        for _ in (0, 1):                         # cvae.py:2196-2202
            warmup[_] = max(warmup[_], warmup_[_])
            warmup_gamma[_] = max(warmup_gamma[_], warmup_gamma_[_])
        self.training_parameters['warmup'] = warmup
        self.training_parameters['warmup_gamma'] = warmup_gamma
        if self.TRAIN_OBJECTIVE != 'elbo':         # a default run writes the job directory it always wrote
            self.training_parameters['objective'] = self.TRAIN_OBJECTIVE
        if self.SEMI_SUPERVISED:
            self.training_parameters['semi_supervised'] = True
        if self.TRAIN_OBJECTIVE == 'tcvae':
            if self.TC_DATASET_SIZE is None:       # the set this call trains on (after the validation split); restored on return
                prior = self.encoder.prior
                self.TC_DATASET_SIZE = self._tc_dataset_size_of(trainset, prior.mean.shape[0] if prior.conditional else 1)
            size = self.TC_DATASET_SIZE
            self.training_parameters['tc_weights'] = [float(w) for w in self.TC_WEIGHTS]
            self.training_parameters['tc_dataset_size'] = int(size) if np.ndim(size) == 0 else [int(v) for v in size]
        if self.TRAIN_OBJECTIVE == 'mmd':
            kl_weight, mmd_weight, kind, scales = self._mmd_settings()
            self.training_parameters['mmd_weights'] = [kl_weight, mmd_weight]
            self.training_parameters['mmd_kernel'] = {'kind': kind, 'scales': list(scales), 'joint': bool(self.MMD_JOINT)}

        from jvae_compat.recorders import LossRecorder
        sets = [set_name] + (['validation'] if validation else [])
        recorders = {s: LossRecorder(test_batch_size) for s in sets}      # tensors allocated by the first recorded batch
        ood_phase = bool(self.TRAIN_OOD_PHASE) and bool(oodsets)
        if ood_phase:
            if testset is None or isinstance(testset, str) or any(isinstance(o, str) for o in oodsets):
                if self.DATA_ROOT is None:
                    raise NotImplementedError('named torchvision datasets are outside this build: pass torch.utils.data.Datasets')
                testset, oodsets = self._open_named_sets(testset, oodsets)
            for o in oodsets:                                             # cvae.py:2226-2232: one recorder per OOD set
                recorders[getattr(o, 'name', 'set')] = LossRecorder(test_batch_size)
        elif oodsets:
            logging.warning('OOD detection rates (%s) are outside this build (SURVEY.md 2a): phase skipped; the recorders of '
                            'accuracy() hold the losses the reference computes them from',
                            ','.join(str(getattr(s, 'name', s)) for s in oodsets))
        batches = self._train_batches(trainset, batch_size, data_augmentation, set_name, device)
        per_epoch = len(batches)
        done_epochs = self.train_history['epochs']
        if done_epochs == 0:
            self.train_history = {'epochs': 0}
        if not acc_methods:
            acc_methods = self.predict_methods
        if fine_tuning:
            for p in self.parameters():
                p.requires_grad_(True)
        sig = signal_handler

        def signalled(level):
            return sig is not None and getattr(sig, 'sig', 0) > level
        epoch = done_epochs
        for epoch in range(done_epochs, epochs + 1):
            self.train_history[epoch] = {}
            history_checkpoint = self.train_history[epoch]
            for s in recorders:
                recorders[s].reset()
            # ---- test phase (cvae.py:2302-2382)
            full_test = bool((epoch - done_epochs) and epoch % full_test_every == 0) or epoch == epochs
            ood_detection = ood_phase and (bool((epoch - done_epochs) and epoch % ood_detection_every == 0) or epoch == epochs)
            if (full_test or not epoch or ood_detection) and save_dir:
                sample_dirs = [os.path.join(save_dir, 'samples', d) for d in ('last', '{:04d}'.format(epoch))]
                for d in sample_dirs:
                    os.makedirs(d, exist_ok=True)
            else:
                sample_dirs = []
            with torch.no_grad():
                self.test_losses, self.test_measures = {}, {}
                if ood_detection:                # cvae.py:2328-2336; the accuracy pass below then reads the test recorder back
                    self.ood_detection_rates(oodsets=oodsets, testset=testset, batch_size=test_batch_size, num_batch='all',
                                             outputs=outputs, recorders=recorders, sample_dirs=sample_dirs, print_result='*')
                if full_test and testset is not None:
                    test_accuracy = self.accuracy(testset, batch_size=test_batch_size, num_batch='all', method=acc_methods,
                                                  outputs=outputs, sample_dirs=sample_dirs, update_self_testing=full_test,
                                                  recorder=recorders[set_name], print_result='TEST' if full_test else 'test')
                    history_checkpoint['test_accuracy'] = test_accuracy
                    history_checkpoint['test_measures'] = dict(self.test_measures)
                    history_checkpoint['test_loss'] = dict(self.test_losses)
                if validation:
                    validation_accuracy = self.accuracy(validationset, batch_size=test_batch_size, num_batch='all',
                                                        method=acc_methods, outputs=outputs, sample_dirs=sample_dirs,
                                                        update_self_testing=False, recorder=recorders['validation'],
                                                        print_result='VALID' if full_test else 'valid')
                    history_checkpoint['validation_accuracy'] = validation_accuracy
                    history_checkpoint['validation_measures'] = dict(self.test_measures)
                    history_checkpoint['validation_loss'] = dict(self.test_losses)
                if signalled(3):
                    logging.warning('Abruptly breaking training loop bc of %s', sig)
                    break
                if save_dir:
                    self.save(save_dir)
            if epoch == epochs:
                break
            # ---- train phase (cvae.py:2388-2501)
            if train_accuracy:
                with torch.no_grad():
                    train_accuracy = self.accuracy(trainset, batch_size=test_batch_size, num_batch='all', method=acc_methods,
                                                   update_self_testing=False, log=False, outputs=outputs, print_result='acc')
            if signalled(3):
                logging.warning('Abruptly breaking training loop bc of %s', sig)
                break
            if save_dir:
                self.save(save_dir)
            if signalled(2) or (full_test and signalled(1)):
                logging.warning('Breaking training loop bc of signal %s after %d epochs', sig, epoch)
                break
            self.encoder.prior.thaw_means(epoch)
            self.train()
            w_kl = max(0., min(1., (epoch + 1 - warmup[0]) / (warmup[1] + 1)))
            w_gamma = max(0., min(1., (epoch + 1 - warmup_gamma[0]) / (warmup_gamma[1] + 1)))
            captured = bool(self.TRAIN_CAPTURED)
            if captured and (optimizer._world > 1 or optimizer.kind != 'adam' or optimizer is not self.optimizer):
                logging.info('TRAIN_CAPTURED: %s - this epoch runs the eager train_step()',
                             'data-parallel model' if optimizer._world > 1 else 'the captured step needs the built-in Adam')
                captured = False
            run_epoch = self._train_epoch_captured if captured else self._train_epoch_eager
            mean_loss, measures = run_epoch(batches, epoch, epochs, batch_size, w_kl, w_gamma, outputs, report_every)
            self.eval()
            if train_accuracy:
                history_checkpoint['train_accuracy'] = train_accuracy
            history_checkpoint['train_loss'] = mean_loss
            history_checkpoint['train_measures'] = measures
            self.train_history['epochs'] += 1
            history_checkpoint['lr'] = self.optimizer.lr
            self.trained += 1
            if fine_tuning:
                self.training_parameters['fine_tuning'].append(epoch)
            optimizer.update_lr()
            if signalled(3):
                logging.warning('Abruptly breaking training loop bc of %s', sig)
                break
            if save_dir:
                self.save(save_dir)
        # ---- after the loop (cvae.py:2503-2545): a last test pass over the whole test set, then save
        for s in recorders:
            recorders[s].reset()
        sample_dirs = []
        if save_dir:
            sample_dirs = [os.path.join(save_dir, 'samples', d) for d in ('last', '{:04d}'.format(epoch + 1))]
            for d in sample_dirs:
                os.makedirs(d, exist_ok=True)
        if ood_phase and not signalled(1):       # cvae.py:2513-2526
            with torch.no_grad():
                self.ood_detection_rates(oodsets=oodsets, testset=testset, batch_size=test_batch_size, num_batch='all',
                                         outputs=outputs, recorders=recorders, sample_dirs=sample_dirs, print_result='*')
        if testset is not None and not signalled(1):
            with torch.no_grad():
                self.accuracy(testset, batch_size=test_batch_size, method=acc_methods, recorder=recorders[set_name],
                              sample_dirs=sample_dirs, outputs=outputs, print_result='TEST')
        if signalled(3):
            logging.warning('Skipping saving because of %s', sig)
        elif save_dir:
            self.save(save_dir)
        return self.train_history

    def _train_batches(self, trainset, batch_size, data_augmentation, set_name, device):
        """The training loader of cvae.py:2245-2249 (batch_size, shuffle=True, num_workers=0, no drop_last) as a re-iterable of
        DEVICE batches (x float32 (n, *input_shape), y int64).  Three sources:
        * a dataset that yields uint8 images: collated by the DataLoader, converted / augmented by the input-pipeline kernel;
        * a float dataset, no augmentation asked: collated by the DataLoader, passed through;
        * a float dataset + `data_augmentation`: the raw uint8 images the dataset object carries (`.data`, `.targets` or
          `.labels`; behind a `random_split` Subset: its `.dataset` and `.indices`) are gathered per batch by the SAME
          DataLoader machinery run over the sample indices - the shuffling consumes the global generator exactly as the
          reference's loader does - and augmented on the device.  Accepted only if the dataset's own transform is ToTensor and
          nothing else: its first and last samples must equal `data[i] / 255` bit for bit, and its target_transform (held-out
          classes: utils/torch_load.py:338-343) is applied to the gathered labels."""
        model = self

        class Batches:
            def __init__(self, loader, convert):
                self.loader, self.convert = loader, convert

            def __len__(self):
                return len(self.loader)

            def __iter__(self):
                for item in self.loader:
                    yield self.convert(item)
        from jvae_compat import torch_load
        from jvae_compat.semi import HiddenLabels
        wrapped = trainset                       # train_model() hands over the Subset its seeded random_split returned
        while isinstance(wrapped, torch.utils.data.Subset):
            wrapped = wrapped.dataset
        if isinstance(wrapped, HiddenLabels) and torch_load.device_loader(wrapped.dataset, batch_size, False) is not None:
            # the resident loader gathers labels (through the set's look-up table) inside its batch launch and hands no sample index
            # back: hiding labels behind it is not built, and -1 must never reach that table
            raise NotImplementedError('HiddenLabels over a device-resident image set is not built: wrap the host dataset, or hide the '
                                      'labels of the device batches yourself')
        resident = torch_load.device_loader(trainset, batch_size, True, data_augmentation,
                                            getattr(self, 'augmentation_generator', None))
        if resident is not None:                 # a device-resident set: gathered, transformed and augmented in one launch
            return Batches(resident, lambda b: (b[0].to(device), b[1].to(device)))
        probe = trainset[0][0] if len(trainset) else None
        is_raw = torch.is_tensor(probe) and probe.dtype == torch.uint8
        if is_raw or not data_augmentation or probe is None:
            loader = torch.utils.data.DataLoader(trainset, batch_size=batch_size, shuffle=True, num_workers=0)
            return Batches(loader, lambda b: (model._device_batch(b[0].to(device), data_augmentation, set_name), b[1].to(device)))
        base, indices = trainset, None
        while isinstance(base, torch.utils.data.Subset):
            idx = torch.as_tensor(base.indices, dtype=torch.int64)
            indices = idx if indices is None else idx[indices]
            base = base.dataset
        data = getattr(base, 'data', None)
        labels = getattr(base, 'targets', None)
        if labels is None:
            labels = getattr(base, 'labels', None)
        why = None
        if data is None or labels is None:
            why = 'the dataset carries no raw images (.data and .targets / .labels)'
        else:
            data = torch.as_tensor(np.asarray(data) if not torch.is_tensor(data) else data)
            labels = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(torch.int64)
            C, H, W = self.input_shape
            if data.dtype != torch.uint8:
                why = 'its .data is {} (uint8 expected)'.format(data.dtype)
            elif data.dim() == 3 and C == 1 and tuple(data.shape[1:]) == (H, W):
                data = data.unsqueeze(1)
            elif data.dim() != 4 or tuple(data.shape[1:]) not in ((H, W, C), (C, H, W)):
                why = 'its .data is shaped {} (input_shape {})'.format(tuple(data.shape), tuple(self.input_shape))
        if why is None:
            n_base = len(base)
            if len(data) != n_base or len(labels) != n_base:
                why = '.data / .targets hold {} / {} entries for {} samples'.format(len(data), len(labels), n_base)
        if why is None:
            nhwc = tuple(data.shape[1:]) == (H, W, C) and not (C == H == W)
            for i in {0, n_base - 1}:
                xi = base[i][0]
                raw = data[i].permute(2, 0, 1) if nhwc else data[i]
                if not torch.is_tensor(xi) or tuple(xi.shape) != (C, H, W) or not torch.equal(
                        xi.to(torch.float32), raw.to(torch.float32).div(255)):
                    why = 'sample {} of the dataset is not its raw image / 255: its own transform is more than ToTensor'.format(i)
                    break
        if why is not None:
            raise ValueError('data_augmentation={} needs the raw uint8 images (the reference augments PIL images before '
                             'ToTensor, utils/torch_load.py:405-426); this dataset yields {} and {}'.format(
                                 list(data_augmentation), getattr(probe, 'dtype', type(probe)), why))
        target_transform = getattr(base, 'target_transform', None)

        class Indices(torch.utils.data.Dataset):
            def __len__(self):
                return len(trainset)

            def __getitem__(self, i):
                return i

        def gather(idx):
            if indices is not None:
                idx = indices[idx]
            y = labels[idx]
            if target_transform is not None:
                y = torch.tensor([int(target_transform(int(v))) for v in y.tolist()], dtype=torch.int64)
            return (model._device_batch(data[idx].to(device), data_augmentation, set_name), y.to(device))
        loader = torch.utils.data.DataLoader(Indices(), batch_size=batch_size, shuffle=True, num_workers=0)
        return Batches(loader, gather)

    def _device_batch(self, x, data_augmentation=(), set_name=''):
        """Collated training batch -> the float32 (N, *input_shape) tensor the step takes.  Raw uint8 images go through the
        input-pipeline kernel (flip / edge-pad crop decided per image on the device, then /255: the ToTensor of
        utils/torch_load.py:415-426); float batches pass through and cannot be augmented."""
        if x.dtype != torch.uint8:
            if data_augmentation:
                raise ValueError('data_augmentation={} needs the raw uint8 images (the reference augments PIL images before '
                                 'ToTensor, utils/torch_load.py:405-426); this dataset yields {}'.format(list(data_augmentation), x.dtype))
            return x
        C, H, W = self.input_shape
        if tuple(x.shape[1:]) == (H, W, C):
            nhwc = True
        elif tuple(x.shape[1:]) == (C, H, W):
            nhwc = False
        else:
            raise ValueError('uint8 batch of shape {} matches neither (N,{},{},{}) nor (N,{},{},{})'.format(
                tuple(x.shape), H, W, C, C, H, W))
        pad = 0
        if 'crop' in data_augmentation:          # utils/torch_load.py:409-411
            pad = 0 if 'imagenet' in set_name else H // 8
        flip, dy, dx = ops.draw_augmentation(x.shape[0], pad, x.device, generator=getattr(self, 'augmentation_generator', None),
                                             flip='flip' in data_augmentation, crop=pad > 0)
        return ops.augment_batch(x, flip, dy, dx, pad=pad, nhwc=nhwc)

    # ------------------------------------------------------------------------------------ persistence
    def save(self, dir_name=None, except_optimizer=False, except_state=False):
        """params.json / train_params.json / test.json / ood.json / history.json, and - once the model is trained and
        unless `except_state` - state.pth plus, unless `except_optimizer`, optimizer.pth (cvae.py:2650-2675; the
        fine-tuning jobs save with except_optimizer=True and except_state=<bool>: ft/job.py:154-158)."""
        if dir_name is None:
            dir_name = getattr(self, 'saved_dir', None) or os.path.join('jobs', self.print_architecture(),
                                                                        str(self.job_number))
        os.makedirs(dir_name, exist_ok=True)
        tp = dict(self.training_parameters)
        tp['sigma'] = self.sigma.params

        def dump(obj, name):
            with open(os.path.join(dir_name, name), 'w') as f:
                json.dump(obj, f, default=str)
        dump(self.architecture, 'params.json')
        dump(tp, 'train_params.json')
        dump(self.testing, 'test.json')
        dump(self.ood_results, 'ood.json')
        dump(self.train_history, 'history.json')
        if self.trained and not except_state:
            torch.save(self.state_dict(), os.path.join(dir_name, 'state.pth'))
            if not except_optimizer:
                torch.save(self.optimizer.state_dict(), os.path.join(dir_name, 'optimizer.pth'))
        self.saved_dir = dir_name
        return dir_name

    @classmethod
    def load(cls, dir_name, build_module=True, load_state=True, load_train=True, load_test=True, strict=True,
             device=None, **kw):
        """Rebuild a model from a job directory written by save() of this class OR of the reference
        (cvae.py:2677-2857): params.json + train_params.json give the constructor arguments, state.pth /
        optimizer.pth the tensors; history.json / test.json / ood.json the training record (`trained` =
        history['epochs'], and the learning-rate schedule is fast-forwarded by that many epochs: cvae.py:2815-2851)."""
        def read(name, int_keys=False, default=None):
            path = os.path.join(dir_name, name)
            if default is not None and not os.path.exists(path):
                return default
            with open(path) as f:
                d = json.load(f)
            if int_keys:                         # utils/save_load/misc.py:58-66 (presumed_type=int)
                d = {(int(k) if k.lstrip('-').isdigit() else k): v for k, v in d.items()}
            return d
        arch = read('params.json')
        tp = read('train_params.json')
        ctor = {k: arch[k] for k in ('input_shape', 'num_labels', 'type', 'output_distribution', 'representation',
                                     'encoder', 'batch_norm', 'dropout', 'activation', 'encoder_forced_variance',
                                     'latent_dim', 'test_latent_sampling', 'decoder', 'upsampler', 'classifier',
                                     'output_activation') if k in arch}
        ctor['features'] = arch.get('features')
        prior = dict(arch.get('prior', {}))
        for drop in ('dim', 'num_priors'):
            prior.pop(drop, None)
        ctor['prior'] = prior
        sig = {k: v for k, v in dict(tp.get('sigma', {'value': 1})).items()
               if k in ('value', 'learned', 'is_rmse', 'sdim', 'input_dim', 'reach', 'decay', 'max_step', 'sigma0', 'is_log')}
        if sig.get('learned'):          # `value` in the json is the CURRENT rms; the state_dict restores the tensor anyway
            sig['value'] = sig.get('sigma0') or sig.get('value')
        if not sig.get('reach'):
            sig.pop('reach', None)
        ctor['sigma'] = sig
        ctor['beta'] = tp.get('beta', 1.)
        ctor['gamma'] = tp.get('gamma') or 0.
        ctor['latent_sampling'] = tp.get('latent_sampling', 1)
        ctor['optimizer'] = dict(tp.get('optimizer', {}))
        net = cls(**ctor)
        net.training_parameters.update({k: v for k, v in tp.items() if k not in ('sigma', 'optimizer')})
        net.saved_dir = dir_name
        history = read('history.json', int_keys=True, default={'epochs': 0})
        net.train_history = history
        net.trained = int(history.get('epochs', 0))
        if load_test:
            tested = read('test.json', int_keys=True, default={})
            if tested:
                net.testing.update(tested)
            net.ood_results = read('ood.json', int_keys=True, default={})
        if device is not None:
            net.to(device)
        if load_state and build_module and os.path.exists(os.path.join(dir_name, 'state.pth')):
            net.load_weights(dir_name, strict=strict)
            net.optimizer.update_scheduler_from_epoch(net.trained)
        return net

    def load_weights(self, dir_name, strict=True, with_optimizer=True):
        """Load state.pth (+ optimizer.pth) written by save() of this class or of the reference."""
        state = torch.load(os.path.join(dir_name, 'state.pth'), map_location=self.device)
        _lib.pack_cache_end()                    # the weights change below
        self.optimizer._scan_pending = True      # ... to values nobody has vouched for: scanned before the next backward
        with torch.no_grad():
            mine = self.state_dict()
            for k, v in state.items():
                if k in mine:
                    mine[k].copy_(v)
                elif strict:
                    raise KeyError(k)
        opt = os.path.join(dir_name, 'optimizer.pth')
        if with_optimizer and os.path.exists(opt):
            self.optimizer.load_state_dict(torch.load(opt, map_location=self.device))
        return self

    def print_architecture(self, *a, **kw):
        arch = self.architecture
        return '{type} K={latent_dim} features={f} upsampler={upsampler}'.format(f=arch.get('features'), **arch)

    def print_training(self, *a, **kw):
        return 'sigma={} optimizer={}'.format(self.sigma, self.optimizer)
