"""Looking at the latent space and at the recorded losses (reference: utils/inspection.py and the two tensor functions of
ft/inspection.py), with the reference's file layouts.

Three layers, kept apart so that the CPU tests can hold the text to the reference's files without a device:

  statistics -> text   `hist_text`, `scatter_text`, `loss_hist_text`, `quantile_text`, `predicted_classes_text`: plain host code on
                       numpy arrays; `per_dim_statistics` turns the fp64 sums of `ops.latent_moments` into the five per-dimension
                       columns of `mu_z_var_z.dat`, `per_dim_hist` the K mean variances into `hist_var_z.dat`'s counts.
  tensors -> statistics on the device: histograms over samples are `ops.histogram` launches (the edges, B + 1 numbers, come
                       from numpy on the host: `bin_edges`), quantiles a `torch.sort` whose two neighbouring order statistics per
                       quantile come to the host and are interpolated there in fp64 (`quantiles`), nearest centroids
                       `ops.nearest_centroid`.
  the reference's functions  `output_latent_distribution`, `losses_distribution_graphs`, `loss_comparisons`, `estimate_y`, `dmu`,
                       `proj2d`, `plot2d`.

`proj2d` draws the latent means of the recorded sets, the class centroids and the alternate prior in two dimensions.  The
reference takes the projection from scikit-learn; here `PCA` and `TSNE` (the exact method, two components) are this module's
own classes over the kernels of csrc/embed.hip - moments and projection for the PCA (the K x K eigen-decomposition is numpy's,
on the host), squared distances, perplexity search, joint probabilities, gradient and update for the t-SNE - and scikit-learn
is not needed.

Outputs are file paths (the directory is made) and `sys.stdout`; a matplotlib `Axes` is served when matplotlib imports.
`to_mat` (scipy) and the command-line blocks stay in the reference.
"""
import errno
import logging
import os
import sys

import numpy as np
import torch

from jvae_hip import ops

DEFAULT_RESULTS_DIR = 'jobs/results'            # utils/parameters.py:14
DEFAULT_QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)


# ----------------------------------------------------------------------------------------------- statistics -> text (host)
def hist_text(edges, counts):
    """`hist_var_z.dat`: the left edge and the count of every bin, then the closing edge with count 0."""
    rows = ['edge          num\n']
    rows += [f'{b:-13.6e} {v:-12g}\n' for b, v in zip(edges[:-1], counts)]
    rows.append(f'{edges[-1]:-13.6e} {0:-12g}\n')
    return ''.join(rows)


def scatter_text(columns):
    """`mu_z_var_z.dat`: one right-aligned column per entry of `columns` (name -> 1-D array), rows sorted by the FIRST column,
    descending."""
    names = list(columns)
    cols = [np.asarray(columns[n]).reshape(-1) for n in names]
    order = np.argsort(-cols[0], kind='stable')
    rows = [' '.join(map('{:>14}'.format, names)) + '\n']
    rows += [' '.join('{:-14g}'.format(c[i]) for c in cols) + '\n' for i in order]
    return ''.join(rows)


def loss_hist_text(hists, bins):
    """The histogram table of `losses_distribution_graphs`: per set an edge and a density column; `bins - 1` rows - the
    reference drops the last bin's density, and so does this - then the closing edges with 0.  hists: name -> (density, edges)."""
    rows = [' '.join(['edge-{k:<8} num-{k:<7}'.format(k=k) for k in hists]) + '\n']
    for b in range(bins - 1):
        rows.append(' '.join(['{e:-13.6e} {v:-12g}'.format(e=hists[k][1][b], v=hists[k][0][b]) for k in hists]) + '\n')
    rows.append(' '.join(['{e:-13.6e} {v:-12g}'.format(e=hists[k][1][-1], v=0) for k in hists]) + '\n')
    return ''.join(rows)


def quantile_text(alpha, table):
    """The quantile table of `losses_distribution_graphs`: table: name -> the quantiles at `alpha`."""
    rows = ['{:20} '.format('which') + ' '.join([f'{a:14}' for a in alpha]) + '\n']
    rows += [f'{k:20} ' + ' '.join([f'{q:-14.7e}' for q in table[k]]) + '\n' for k in table]
    return ''.join(rows)


def predicted_classes_text(n_pred, num_labels):
    """`predicted-classes-per-set.tab`: one column per set, one row per class.  n_pred: name -> the C counts."""
    rows = [' '.join([f'{s:6}' for s in n_pred]) + '\n']
    rows += [' '.join([f'{int(n_pred[s][c]):6}' for s in n_pred]) + '\n' for c in range(num_labels)]
    return ''.join(rows)


def elbo_decomposition_text(result):
    """The table of `net.elbo_decomposition()`: one row per figure it gave (a figure that is None is left out), then one row per
    class with queries (conditional priors) and one per coordinate (where the prior factorises)."""
    names = ('kl', 'kl_mc', 'mi', 'mi_unconditional', 'mi_bound', 'kl_marginal', 'tc', 'dwkl')
    rows = ['{:20} {:>14}\n'.format('which', 'nats')]
    rows += [f'{k:20} {result[k]:-14.7e}\n' for k in names if result.get(k) is not None]
    rows.append('{:20} {:14d}\n{:20} {:14d}\n'.format('n', int(result['n']), 'm', int(result['m'])))
    per_class = result.get('per_class')
    if per_class is not None:
        rows.append('{:>6} {:>8} {:>14} {:>14}\n'.format('class', 'count', 'mi', 'kl_marginal'))
        rows += [f'{c:6d} {int(n):8d} {per_class["mi"][c]:-14.7e} {per_class["kl_marginal"][c]:-14.7e}\n'
                 for c, n in enumerate(per_class['count']) if n]
    if result.get('dwkl_per_dim') is not None:
        rows.append('{:>6} {:>14}\n'.format('dim', 'dwkl'))
        rows += [f'{k:6d} {v:-14.7e}\n' for k, v in enumerate(result['dwkl_per_dim'])]
    return ''.join(rows)


def per_dim_statistics(sums, count):
    """sums (4, K) fp64 = the sums over `count` samples of mu, mu^2, v, v^2 (one group of `ops.latent_moments`) -> the columns
    of `mu_z_var_z.dat` in the reference's order: mean of mu^2, mean variance, their sum, mean of mu, unbiased std of the
    variance (nan for a single sample, as torch.std gives), all fp64."""
    s = np.asarray(sums, dtype=np.float64)
    n = float(count)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = {'mu2_mu_z': s[1] / n, 'mu_var_z': s[2] / n}
        out['mu2_z'] = out['mu2_mu_z'] + out['mu_var_z']
        out['mu_mu_z'] = s[0] / n
        out['std_var_z'] = np.sqrt(np.maximum((s[3] - s[2] * s[2] / n) / (n - 1.), 0.))
    return out


def bin_edges(bins, lo, hi):
    """The B + 1 edges np.histogram(a, bins=B, range=(lo, hi)) uses on fp32 data `a` (fp32 edges; lo == hi is widened by numpy)."""
    return np.histogram_bin_edges(np.empty(0, np.float32), bins=bins, range=(lo, hi))


def per_dim_hist(mean_var, bins=10):
    """The K per-dimension mean variances -> (edges, counts) of `hist_var_z.dat`: numpy on K numbers, range (0, max), fp32 as the
    reference's tensor."""
    data = np.asarray(mean_var, dtype=np.float32)
    counts, edges = np.histogram(data, bins=bins, range=(0, float(data.max())))
    return edges, counts


def lerp_quantiles(lower, upper, frac):
    """numpy's 'linear' interpolation between the two neighbouring order statistics, in fp64."""
    a, b, t = (np.asarray(_, dtype=np.float64) for _ in (lower, upper, frac))
    d = b - a
    return np.where(t >= 0.5, b - d * (1. - t), a + d * t)


# ------------------------------------------------------------------------------------------------- outputs (reference 14-74)
def _axes_type():
    try:
        from matplotlib import pyplot as plt
        return plt.Axes
    except Exception:                              # matplotlib is optional: without it only files and stdout are served
        return None


def _create_output_plot(*outputs, pltf='plot'):
    writers, closers, plotters = [], [], []
    axes = _axes_type()
    for o in outputs:
        if o is None:
            continue
        if o is sys.stdout or isinstance(o, type(sys.stdout)):
            writers.append(o.write)
        elif isinstance(o, str):
            d = os.path.dirname(o)
            if d and not os.path.exists(d):
                try:
                    os.makedirs(d)
                except OSError as exc:
                    if exc.errno != errno.EEXIST:
                        raise
            f = open(o, 'w')
            closers.append(f.close)
            writers.append(f.write)
        elif axes is not None and isinstance(o, axes):
            def _p(*a, _o=o, **kw):
                legend = kw.pop('legend', False)
                getattr(_o, pltf)(*a, **kw)
                if legend:
                    _o.legend()
            plotters.append(_p)
        else:
            raise TypeError(f'output {o!r}: a file path, sys.stdout or a matplotlib Axes expected')

    def plot(*a, **kw):
        for f in plotters:
            f(*a, **kw)

    def write(text):
        for f in writers:
            f(text)

    def close():
        for f in closers:
            f()
    plot.wanted = bool(plotters)
    return plot, write, close


# ------------------------------------------------------------------------------------------- tensors -> statistics (device)
def _on_device(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ops.L.JvaeHipError(f'{what}: a tensor resident on the GPU expected (no CPU fallback)')
    return t


def sample_histogram(values, bins=10, range=None):
    """np.histogram(values, bins=bins, range=range) of a device tensor -> (counts int64 (B,), edges (B + 1,)) on the host: the
    outer edges (two numbers) are read from the device when `range` is None, the edges come from numpy, the counting is ONE
    `ops.histogram` launch; non-finite values raise ValueError, as numpy's automatic range does."""
    v = _on_device(values, 'sample_histogram').detach().reshape(-1).float()
    if v.numel() == 0:
        lo, hi = (0., 1.) if range is None else range
    elif range is None:
        lo, hi = torch.stack((v.min(), v.max())).tolist()
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f'autodetected range of [{lo}, {hi}] is not finite')
        lo, hi = np.float32(lo), np.float32(hi)
    else:
        lo, hi = range
    edges = bin_edges(bins, lo, hi)
    if v.numel() == 0:
        return np.zeros(len(edges) - 1, dtype=np.int64), edges
    counts = ops.histogram(v, edges, check=range is None)
    return counts[0].cpu().numpy(), edges


def grouped_histogram(values, group, G, edges):
    """The histograms of G groups that share `edges` in ONE launch: values (n,), group (n,) int32 -> counts (G, B) on the host."""
    v = _on_device(values, 'grouped_histogram').detach().reshape(-1).float()
    return ops.histogram(v, edges, group=group.to(torch.int32), G=G).cpu().numpy()


def quantiles(values, alpha):
    """np.quantile(values, alpha) of a device tensor: torch.sort on the device, the two neighbouring order statistics of each
    quantile come to the host (2 len(alpha) numbers) and are interpolated there in fp64."""
    v = _on_device(values, 'quantiles').detach().reshape(-1).float()
    alpha = np.asarray(alpha, dtype=np.float64)
    n = v.numel()
    if n == 0:
        return np.full(alpha.shape, np.nan)
    pos = alpha * (n - 1)
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    s = torch.sort(v).values
    picked = s[torch.from_numpy(np.concatenate([lo, hi])).to(v.device)].double().cpu().numpy()
    return lerp_quantiles(picked[:len(alpha)], picked[len(alpha):], pos - lo)


def estimate_y(mu, centroids):
    """The class whose centroid is nearest to each row of mu (N, K); centroids (C, K) (ft/inspection.py:24-32, there through
    an (N, C, K) temporary): `ops.nearest_centroid`."""
    return ops.nearest_centroid(mu, centroids)[0]


def dmu(mu, centroids, y=None):
    """mu minus its class centroid (centroids (C, K) indexed by y), or minus the single centroid (K,) (ft/inspection.py:35-44)."""
    assert y is not None or centroids.ndim == 1
    if y is None:
        return mu - centroids.unsqueeze(0)
    return mu - centroids.index_select(0, y)


# ---------------------------------------------------------------------------------------------- the reference's functions
def output_latent_distribution(mu_z, var_z, *outputs, result_type='hist_of_var', **options):
    r"""utils/inspection.py:77-132.  result_type:

        -- hist_of_var: histogram of the variances (of their per-dimension means with per_dim); options: those of
           numpy.histogram (bins) and log_scale=bool (default False)
        -- scatter: the (mu, var) pairs of every sample and dimension or, with per_dim, the five per-dimension statistics
    """
    _on_device(mu_z, 'output_latent_distribution'), _on_device(var_z, 'output_latent_distribution')
    per_dim = options.pop('per_dim', False)
    if result_type == 'hist_of_var':
        log_scale = options.pop('log_scale', False)
        bins = options.pop('bins', 10)
        if options:
            raise TypeError('hist_of_var takes bins, log_scale and per_dim, not ' + ', '.join(options))
        data = var_z.log() if log_scale else var_z
        if per_dim:
            data = data.mean(0).cpu().numpy()                              # K numbers: numpy on the host
            hrange = (float(data.min()), float(data.max())) if log_scale else (0, float(data.max()))
            hist, edges = np.histogram(data, range=hrange, bins=bins)
        else:
            lo, hi = torch.stack((data.min(), data.max())).tolist()
            hist, edges = sample_histogram(data, bins=bins, range=(lo, hi) if log_scale else (0, hi))
        if log_scale:
            edges = np.exp(edges)
        plot, write, close = _create_output_plot(*outputs, pltf='bar')
        plot(edges[:-1], hist, align='edge')
        write(hist_text(edges, hist))
        close()

    if result_type == 'scatter':
        if per_dim:
            data_ = {'mu2_mu_z': mu_z.pow(2).mean(0), 'mu_var_z': var_z.mean(0)}
            data_['mu2_z'] = data_['mu2_mu_z'] + data_['mu_var_z']
            data_['mu_mu_z'] = mu_z.mean(0)
            data_['std_var_z'] = var_z.std(0)
        else:
            data_ = {'mu_z': mu_z.reshape(-1), 'var_z': var_z.reshape(-1)}
        host = dict(zip(data_, torch.stack(list(data_.values())).cpu().numpy()))
        plot, write, close = _create_output_plot(*outputs, pltf='scatter')
        x, y = list(host)[:2]
        plot(host[x], host[y])
        write(scatter_text(host))
        close()


def losses_distribution_graphs(dict_of_losses, *outputs, graph='histogram', **opt):
    """utils/inspection.py:221-265: `graph` 'hist...' - the density histogram of every entry, each over its own range, as one
    table; 'box...' - their quantiles (`quantiles`, default 5 / 25 / 50 / 75 / 95 %).  The entries are device tensors."""
    bins = opt.pop('bins', 10)
    opt.pop('whis', 1.5)
    alpha = list(opt.pop('quantiles', DEFAULT_QUANTILES))

    if graph.startswith('hist'):
        plot, write, close = _create_output_plot(*outputs, pltf='plot')
        hist = {}
        for k, v in dict_of_losses.items():              # every set has its own range: one launch per set
            counts, edges = sample_histogram(v, bins=bins)
            with np.errstate(invalid='ignore', divide='ignore'):
                hist[k] = (counts / np.diff(edges).astype(float) / counts.sum(), edges)
        write(loss_hist_text(hist, bins))
        for k in hist:
            plot(hist[k][1][:-1], hist[k][0], label=k, legend=True)
        close()

    if graph.startswith('box'):
        plot, write, close = _create_output_plot(*outputs, pltf='boxplot')
        table = {k: quantiles(v, alpha) for k, v in dict_of_losses.items()}
        write(quantile_text(alpha, table))
        if plot.wanted:
            plot([v.detach().cpu().numpy() for v in dict_of_losses.values()], labels=list(dict_of_losses.keys()))
        close()


def job_to_str(number, string, formats={int: '{:06d}'}):
    return string.replace('%j', formats.get(type(number), '{}').format(number))


def loss_comparisons(net, root=os.path.join(DEFAULT_RESULTS_DIR, '%j', 'losses'), plot=False, echo=True, **kw):
    """utils/inspection.py:135-218 on the records `saved_dir/samples/last/record-<set>.pth` of the model's test set and of the
    sets of `net.ood_results`: per loss (total, cross_x, kl) the histogram and quantile tables per set - with the test set split
    into correct / missed - and per predicted class, and `predicted-classes-per-set.tab`.  The file names are the reference's,
    its `losses-<k>-per-class.tab-<graph>.tab` included.  `echo`: the tables go to sys.stdout as well, as in the reference."""
    from jvae_compat.recorders import LossRecorder
    if plot is True:
        plot = 'all'
    sample_directory = os.path.join(net.saved_dir, 'samples', 'last')
    root = job_to_str(net.job_number, root)
    if not os.path.exists(sample_directory):
        logging.warning(f'Net #{net.job_number} has no recorded loss')
        return
    if not os.path.exists(root):
        os.makedirs(root)

    testset = net.training_parameters['set']
    datasets = [testset] + list(net.ood_results.keys())
    losses, y_pred = {}, {}
    recorders = LossRecorder.loadall(sample_directory, *datasets, map_location=net.device)
    for s, r in recorders.items():
        losses[s] = {k: r[k].to(net.device) for k in r.keys()}
        logits = losses[s].pop('logits').T
        y_pred[s] = net.predict_after_evaluate(logits, losses[s])

    y_true = losses[testset].pop('y_true')
    hit = y_true == y_pred[testset]
    for s in losses:
        for k in losses[s]:
            if losses[s][k].dim() == 2:
                losses[s][k] = losses[s][k].gather(0, y_pred[s].unsqueeze(0)).squeeze(0)
    for w, i in zip(('correct', 'missed'), (hit, ~hit)):
        losses[w] = {k: losses[testset][k][i] for k in losses[testset]}

    def axes(name, graph):
        if plot and (plot == 'all' or plot.startswith(graph)):
            from matplotlib import pyplot as plt
            return plt.figure(name + str(net.job_number)).subplots(1)
        return None

    out = sys.stdout if echo else None
    for k in ('total', 'cross_x', 'kl'):
        logging.info('Distribution of %s', k)
        for graph in ('hist', 'boxp'):
            f_ = f'losses-{k}-per-set'
            losses_distribution_graphs({s: losses[s][k] for s in losses}, os.path.join(root, f_ + f'-{graph}.tab'), out,
                                       axes(f_, graph), graph=graph, **kw)
    for k in ('total', 'cross_x', 'kl'):
        logging.info('Distribution of %s per class', k)
        per_class = {f'{c}': losses[testset][k][y_pred[testset] == c] for c in range(net.num_labels)}
        for graph in ('hist', 'boxp'):
            f_ = f'losses-{k}-per-class.tab'
            losses_distribution_graphs(per_class, os.path.join(root, f_ + f'-{graph}.tab'), out, axes(f_, graph), graph=graph, **kw)

    n_pred = {s: torch.bincount(y_pred[s], minlength=net.num_labels).cpu().numpy() for s in y_pred}
    with open(os.path.join(root, 'predicted-classes-per-set.tab'), 'w') as f:
        f.write(predicted_classes_text(n_pred, net.num_labels))


# ------------------------------------------------------------------- 2-D pictures of the latent means (ft/inspection.py:100-206)
def _as_device_rows(X, device, what):
    """A numpy array or a tensor (N, K) -> a dense fp32 tensor on the device (the kernels have no CPU path)."""
    if not torch.is_tensor(X):
        X = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float32)))
    if X.dim() != 2:
        raise ValueError(f'{what}: a (N, K) array expected, got {tuple(X.shape)}')
    if device is None:
        device = X.device if X.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return X.detach().to(device=device, dtype=torch.float32).contiguous()


def principal_axes(cov, n_components):
    """The host part of the PCA, fp64: cov (K, K) symmetric -> (components (n_components, K), their eigenvalues), largest
    eigenvalue first, the sign of each component such that its largest-magnitude entry is positive (scikit-learn's svd_flip on
    the components)."""
    w, v = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = np.argsort(-w, kind='stable')[:n_components]
    comp = v[:, order].T.copy()
    big = np.abs(comp).argmax(axis=1)
    comp *= np.where(comp[np.arange(len(comp)), big] < 0, -1., 1.)[:, None]
    return comp, w[order]


class PCA:
    """sklearn.decomposition.PCA(n_components) as far as `proj2d` uses it: `fit_transform` and the attributes `mean_`,
    `components_`, `explained_variance_`.  Means and the centred covariance are summed on the device in fp64
    (`ops.pca_moments`), the K x K eigen-decomposition is numpy's on the host in fp64, the projection is `ops.project`."""
    MAX_COMPONENTS = ops.EMBED_MAX_COMPONENTS

    def __init__(self, n_components=2, device=None):
        self.n_components = int(n_components)
        self.device = device

    def fit_transform(self, X):
        x = _as_device_rows(X, self.device, 'PCA')
        N, K = x.shape
        if not 1 <= self.n_components <= min(N, K, self.MAX_COMPONENTS):
            raise ValueError(f'PCA: n_components = {self.n_components} must be between 1 and min(N, K, {self.MAX_COMPONENTS}) = '
                             f'{min(N, K, self.MAX_COMPONENTS)}')
        mean, cov = ops.pca_moments(x)
        self.mean_ = mean.cpu().numpy()
        self.components_, self.explained_variance_ = principal_axes(cov.cpu().numpy(), self.n_components)
        return self.transform(x)

    def transform(self, X):
        x = _as_device_rows(X, self.device, 'PCA')
        dev = x.device
        return ops.project(x, torch.from_numpy(self.mean_).to(dev), torch.from_numpy(self.components_).to(dev)).cpu().numpy()


class TSNE:
    """sklearn.manifold.TSNE(method='exact') in two dimensions, on the device: squared distances, the perplexity search and the
    joint probabilities once (`ops.pairwise_sqdist`, `ops.tsne_affinities`), then scikit-learn's gradient descent - 250
    iterations at momentum 0.5 with the early exaggeration, the rest at momentum 0.8, gains and update restarted in between -
    with one gradient and one update launch group per iteration.  Every 50th iteration two fp64 words (the KL divergence, the
    norm of the scaled gradient) are read back for scikit-learn's two stopping rules.  `kl_divergence_` is the KL kernel's
    value AT `embedding_` (scikit-learn keeps the value one update earlier).  The reference's default, Barnes-Hut, is an
    approximation of this method; it is not built.  N <= ops.EMBED_MAX_N points."""
    _EXPLORATION_MAX_ITER = 250
    _N_ITER_CHECK = 50

    def __init__(self, n_components=2, *, perplexity=30., early_exaggeration=12., learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, init='pca', random_state=None, device=None):
        if n_components != 2:
            raise NotImplementedError('TSNE: two components only')
        self.n_components = 2
        self.perplexity, self.early_exaggeration, self.learning_rate = perplexity, early_exaggeration, learning_rate
        self.max_iter, self.n_iter_without_progress, self.min_grad_norm = max_iter, n_iter_without_progress, min_grad_norm
        self.init, self.random_state, self.device = init, random_state, device

    def _initial(self, x):
        N = x.shape[0]
        if isinstance(self.init, str) and self.init == 'pca':
            y = PCA(2, device=x.device).fit_transform(x)
            return (y / np.std(y[:, 0]) * 1e-4).astype(np.float32)
        if isinstance(self.init, str) and self.init == 'random':
            rs = self.random_state
            rs = rs if isinstance(rs, np.random.RandomState) else (np.random.mtrand._rand if rs is None else np.random.RandomState(rs))
            return 1e-4 * rs.standard_normal(size=(N, 2)).astype(np.float32)
        if isinstance(self.init, str):
            raise ValueError(f"TSNE: init must be 'pca', 'random' or an array, not {self.init!r}")
        y = self.init.detach().cpu().numpy() if torch.is_tensor(self.init) else np.asarray(self.init)
        if y.shape != (N, 2):
            raise ValueError(f'TSNE: init of shape {(N, 2)} expected, got {y.shape}')
        return y.astype(np.float32)

    def _descend(self, P, state, it, max_iter, momentum, n_iter_without_progress, exaggeration):
        y, update, gains, g, words = state
        update.zero_()
        gains.fill_(1.)
        best_error, best_iter, i = np.finfo(float).max, it, it
        for i in range(it, max_iter):
            check = (i + 1) % self._N_ITER_CHECK == 0
            ops.tsne_gradient(P, y, exaggeration, g=g, stats=words[:2] if check else None)
            ops.tsne_update(y, update, gains, g, momentum, self.learning_rate_, norm=words[2:] if check else None)
            if check:
                error, _, grad_norm = words.tolist()          # the one read of this check: three fp64 words
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > n_iter_without_progress:
                    break
                if grad_norm <= self.min_grad_norm:
                    break
        return i

    def fit_transform(self, X):
        x = _as_device_rows(X, self.device, 'TSNE')
        N = x.shape[0]
        if self.perplexity >= N:
            raise ValueError(f'perplexity ({self.perplexity}) must be less than n_samples ({N})')
        if self.learning_rate == 'auto':
            self.learning_rate_ = max(N / self.early_exaggeration / 4, 50)
        else:
            self.learning_rate_ = float(self.learning_rate)
        y0 = self._initial(x)
        d = ops.pairwise_sqdist(x)
        P = ops.tsne_affinities(d, self.perplexity)[0]
        del d
        y = torch.from_numpy(np.ascontiguousarray(y0)).to(x.device)
        words = torch.zeros(3, dtype=torch.float64, device=x.device)
        state = (y, torch.empty_like(y), torch.empty_like(y), torch.empty_like(y), words)
        it = self._descend(P, state, 0, self._EXPLORATION_MAX_ITER, 0.5, self._EXPLORATION_MAX_ITER, self.early_exaggeration)
        if it < self._EXPLORATION_MAX_ITER or self.max_iter - self._EXPLORATION_MAX_ITER > 0:
            it = self._descend(P, state, it + 1, self.max_iter, 0.8, self.n_iter_without_progress, 1.)
        self.n_iter_ = it
        self.kl_divergence_ = self.kl_divergence(P, y)
        self.embedding_ = y.cpu().numpy()
        return self.embedding_

    @staticmethod
    def kl_divergence(P, y, exaggeration=1.):
        """KL(exaggeration P || Q(y)) through the KL kernel: P (N, N) and y (N, 2) on the device -> a Python float."""
        words = torch.zeros(2, dtype=torch.float64, device=y.device)
        ops.tsne_gradient(P, y, exaggeration, stats=words)
        return float(words[0])


def _split_key(k):
    """'<set>-<pre|ft>' -> (set, suffix), split at the LAST '-' (held-out names such as cifar10-3 keep theirs); a key without one
    -> (k, None)."""
    head, sep, tail = k.rpartition('-')
    return (head, tail) if sep else (k, None)


def proj2d_csv_text(mu_, y_, tset):
    """The rows `x1,x2,y,set,dist,ft` of proj2d's csv file: set rows (set, 'ind' for the training set else 'ood', 'pre' | 'ft'),
    centroids ('centroids', 'ind', 'both'), the alternate prior ('alt', 'ood', 'both')."""
    rows = [','.join(['x1', 'x2', 'y', 'set', 'dist', 'ft']) + '\n']
    for k in mu_:
        if k == 'centroids':
            dset, dist, ft = 'centroids', 'ind', 'both'
        elif k == 'alternate':
            dset, dist, ft = 'alt', 'ood', 'both'
        else:
            dset, ft = _split_key(k)
            dist = 'ind' if dset == tset else 'ood'
        for (x1, x2), y in zip(mu_[k], y_[k]):
            rows.append('{x1},{x2},{y},{s},{d},{ft}\n'.format(x1=x1, x2=x2, y=y, s=dset, d=dist, ft=ft))
    return ''.join(rows)


def proj2d(sample_recorders_pre, sample_recorders_ft, tset, include_alternate=False, N=60, N_=10, Model=TSNE, csv_file=None):
    """ft/inspection.py:100-179: ONE 2-D projection (`Model(2).fit_transform`) of the stack, over the recorders before and after
    fine-tuning and over their sets in recorder order, of N_ copies of the class centroids (and of the alternate prior with
    include_alternate) followed by the first N latent means of the sets whose name starts with `tset`, N // 10 of the others;
    the result is cut apart with the same slices -> (mu_, y_): 'centroids' (the C centroids; the reference hard-codes 10),
    'alternate', '<set>-pre', '<set>-ft' -> (n, 2) arrays and their labels, the class names for `tset` and the set name for the
    others.  The class names come from the registry of `torch_load`: no data set is opened.  The reference's function cannot
    run (a `np.zeros()` without a shape) and its csv block labels every set row `alt,ood,both`: this is the evident intent."""
    from jvae_compat.torch_load import get_classes_by_name

    def numpy(t):
        return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)

    centroids = numpy(sample_recorders_pre[tset]._aux['centroids'])
    C = centroids.shape[0]
    classes = list(get_classes_by_name(tset))
    if len(classes) != C:
        raise ValueError(f'proj2d: {C} centroids recorded for {tset}, which has {len(classes)} classes')
    centroids_labels = np.expand_dims(np.array(classes, dtype=object), 1)
    if include_alternate:
        centroids = np.vstack([centroids, numpy(sample_recorders_pre[tset]._aux['alternate']).reshape(1, -1)])
        centroids_labels = np.vstack([centroids_labels, np.array([['ood']], dtype=object)])

    mu = np.ndarray((0, centroids.shape[-1]))
    y = np.ndarray((0, 1), dtype=object)
    for sample_recorders in (sample_recorders_pre, sample_recorders_ft):
        for s in sample_recorders:
            _N = N if s.startswith(tset) else N // 10
            batch = numpy(sample_recorders[s]['mu'])[:_N]
            mu = np.vstack([mu, *([centroids] * N_), batch])
            if s == tset:
                c_batch = np.expand_dims(centroids_labels.take(numpy(sample_recorders[s]['y'])[:_N]), 1)
            else:
                c_batch = np.zeros((len(batch), 1), object)
                c_batch[:] = s
            y = np.vstack([y, *([centroids_labels] * N_), c_batch])

    logging.info('Mu of shape %s', mu.shape)
    mu = Model(2).fit_transform(mu)

    mu_, y_ = {}, {}
    start = 0
    for sample_recorders, suffix in zip((sample_recorders_pre, sample_recorders_ft), ('pre', 'ft')):
        for s in sample_recorders:
            _N = min(N if s.startswith(tset) else N // 10, len(numpy(sample_recorders[s]['mu'])))
            mu_['centroids'] = mu[start:start + C]
            y_['centroids'] = classes
            if include_alternate:
                mu_['alternate'] = mu[start + C:start + C + 1]
                y_['alternate'] = ['ood']
            start += N_ * len(centroids)
            k = '{}-{}'.format(s, suffix)
            mu_[k] = mu[start:start + _N]
            y_[k] = y[start:start + _N].squeeze(1)
            start += _N

    if csv_file:
        with open(csv_file, 'w') as f:
            f.write(proj2d_csv_text(mu_, y_, tset))
    return mu_, y_


def plot2d(mu2d, dset, ax=None):
    """ft/inspection.py:182-206: the scatter plot of proj2d's `mu_` - the sets of `dset` and the centroids in blue, the other
    sets and the alternate prior in red, crosses for the centroids and the prior.  Served when matplotlib imports."""
    if _axes_type() is None:
        raise ImportError('plot2d needs matplotlib')
    from matplotlib import pyplot as plt
    marker = {k: ',' for k in mu2d}
    marker['centroids'] = 'x'
    color = {'centroids': 'b'}
    for k in mu2d:
        if k.startswith(dset):
            color[k] = 'b'
    if 'alternate' in marker:
        marker['alternate'] = 'x'
        color['alternate'] = 'r'
    color.update({k: 'r' for k in mu2d if k not in color})
    ax = ax or plt.gca()
    for k in mu2d:
        facecolor = color[k] if marker[k] == 'x' else 'none'
        ax.scatter(mu2d[k][:, 0], mu2d[k][:, 1], marker=marker[k], edgecolors=color[k], facecolors=facecolor)
    return ax
