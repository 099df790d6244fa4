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
  the reference's functions  `output_latent_distribution`, `losses_distribution_graphs`, `loss_comparisons`, `estimate_y`, `dmu`.

Outputs are file paths (the directory is made) and `sys.stdout`; a matplotlib `Axes` is served when matplotlib imports.
`proj2d`, `plot2d`, `to_mat` (sklearn, pandas, scipy) and the command-line blocks stay in the reference.
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
