"""Latent-space inspection on the host: fp64 restatements of the three kernels of csrc/inspect.hip and of the statistics behind
the reference's files, held to tests/golden/inspection (written by tools/gen_inspection_golden.py from the reference), and the
host formatters of jvae_compat/inspection.py held to the reference's texts.

A text meets its golden when (`assert_text`): the same lines in the same order, the header character for character, every row
the same number of fields, an integer field (a count) equal, a float field within 1e-4 of the largest magnitude of its column
(the project's parity bar).  The GPU tests (test_20_inspection_gpu.py) import the restatements and this comparison.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'inspection')
RTOL = 1e-4
MARGIN = 1e-3
ZSAMPLE_CASES = ('c1_n16_mlp', 'e2_n8_L3', 'ea2_n8_vae_L3')


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ the kernels in fp64
def moments64(mu, log_var, group=None, G=1):
    """jvae_latent_moments_f32: mu, log_var (N, K) fp32 -> sums (G, 4, K) fp64, counts (G,) int64; v = exp taken in fp32."""
    mu = np.asarray(mu, np.float32)
    v = np.exp(np.asarray(log_var, np.float32)).astype(np.float64)
    m = mu.astype(np.float64)
    group = np.zeros(len(mu), np.int64) if group is None else np.asarray(group)
    sums, counts = np.zeros((G, 4, mu.shape[1])), np.zeros(G, np.int64)
    for g in range(G):
        i = group == g
        counts[g] = i.sum()
        sums[g] = [m[i].sum(0), (m[i] ** 2).sum(0), v[i].sum(0), (v[i] ** 2).sum(0)]
    return sums, counts


def dist64(mu, centroids):
    return ((np.asarray(mu, np.float64)[:, None] - np.asarray(centroids, np.float64)[None]) ** 2).sum(-1)


def nearest64(mu, centroids):
    """jvae_nearest_centroid_f32 -> (argmin (lowest index on ties), its squared distance)."""
    d = dist64(mu, centroids)
    return d.argmin(1), d.min(1)


def hist64(values, edges, group=None, G=1):
    """jvae_histogram_f32 -> (counts (G, B), number of non-finite values): the comparison rule itself, value by value."""
    values, edges = np.asarray(values, np.float64), np.asarray(edges, np.float64)
    B = len(edges) - 1
    group = np.zeros(len(values), np.int64) if group is None else np.asarray(group)
    counts, bad = np.zeros((G, B), np.int64), 0
    for x, g in zip(values, group):
        if not 0 <= g < G:
            continue
        if not np.isfinite(x):
            bad += 1
            continue
        if not edges[0] <= x <= edges[B]:
            continue
        b = int(np.searchsorted(edges, x, side='right')) - 1
        counts[g, min(b, B - 1)] += 1
    return counts, bad


def clear_margin(d):
    """rows of (N, C) distances whose two smallest values differ by more than MARGIN, relative"""
    if d.shape[1] < 2:
        return np.ones(len(d), bool)
    two = np.sort(d, 1)[:, :2]
    return two[:, 1] - two[:, 0] > MARGIN * two[:, 1]


def centroid_inputs(N, C, K, seed):
    """Seeded normal draws with a clear winner in every row (the rows without one are redrawn); asserted."""
    g = np.random.default_rng(seed)
    cent = g.standard_normal((C, K)).astype(np.float32)
    mu = g.standard_normal((N, K)).astype(np.float32)
    for _ in range(200):
        bad = np.where(~clear_margin(dist64(mu, cent)))[0]
        if not len(bad):
            break
        mu[bad] = g.standard_normal((len(bad), K)).astype(np.float32)
    assert clear_margin(dist64(mu, cent)).all()
    return mu, cent


# ------------------------------------------------------------------------------------------------------ text comparison
INTEGER = re.compile(r'^-?\d+$')


def assert_text(got, want, what=''):
    got, want = str(got), str(want)
    gl, wl = got.split('\n'), want.split('\n')
    assert len(gl) == len(wl), (what, len(gl), len(wl))
    assert gl[0] == wl[0], (what, gl[0], wl[0])
    assert got.endswith('\n') == want.endswith('\n')
    rows_g = [l.split() for l in gl[1:] if l.strip()]
    rows_w = [l.split() for l in wl[1:] if l.strip()]
    assert len(rows_g) == len(rows_w), what
    ncol = {len(r) for r in rows_w}
    assert len(ncol) <= 1 and all(len(a) == len(b) for a, b in zip(rows_g, rows_w)), what

    def num(t):
        try:
            return float(t)
        except ValueError:
            return None
    for c in range(ncol.pop() if ncol else 0):
        col_w = [r[c] for r in rows_w]
        col_g = [r[c] for r in rows_g]
        vals = [num(t) for t in col_w]
        if any(v is None for v in vals):                                   # a column of names
            assert col_g == col_w, (what, c)
            continue
        finite = [abs(v) for v in vals if np.isfinite(v)]
        top = max(finite) if finite else 0.
        for i, (g, w) in enumerate(zip(col_g, col_w)):
            if INTEGER.match(w):
                assert g == w, (what, 'row', i, 'column', c, g, w)
                continue
            gv, wv = float(g), float(w)
            if np.isnan(wv) or np.isinf(wv):
                assert (np.isnan(gv) and np.isnan(wv)) or gv == wv, (what, i, c, g, w)
            else:
                assert abs(gv - wv) <= RTOL * top, (what, 'row', i, 'column', c, g, w, top)


def test_assert_text_is_not_lenient():
    want = 'a b\n 1.0e+00  3\n 2.0e+00  4\n'
    assert_text(want, want)
    for bad in ('a c\n 1.0e+00  3\n 2.0e+00  4\n', 'a b\n 1.0e+00  4\n 2.0e+00  4\n', 'a b\n 1.1e+00  3\n 2.0e+00  4\n',
                'a b\n 2.0e+00  4\n 1.0e+00  3\n', 'a b\n 1.0e+00  3\n'):
        with pytest.raises(AssertionError):
            assert_text(bad, want)


# ----------------------------------------------------------------------------------------- statistics and formatters
def test_interfaces_exist():
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat import inspection
    from jvae_compat.wim import WIMJob
    from jvae_hip import ops
    from module import sample
    assert callable(Net.latent_posterior) and list(inspect.signature(Net.latent_posterior).parameters) == ['self', 'x', 'y']
    z = inspect.signature(sample.zsample).parameters
    assert list(z)[:4] == ['x', 'net', 'y', 'batch_size'] and z['batch_size'].default == 128 and z['bins'].default == 10 \
        and z['directory'].default == 'test'
    c = inspect.signature(sample.comparison).parameters
    assert list(c)[:2] == ['x', 'nets'] and c['batch_size'].default == 128
    assert 'sample_recorders' in inspect.signature(WIMJob.finetune).parameters
    assert 'sample_recorders' in inspect.signature(Net.ood_detection_rates).parameters
    assert 'with_mu' in inspect.signature(Net._evaluate_for_scores).parameters
    assert 'with_mu' in inspect.signature(WIMJob._evaluate_for_scores).parameters
    assert callable(WIMJob.make_sample_recorders)
    for f in ('latent_moments', 'nearest_centroid', 'histogram', 'histogram_check'):
        assert callable(getattr(ops, f))
    for f in ('estimate_y', 'dmu', 'output_latent_distribution', 'losses_distribution_graphs', 'loss_comparisons'):
        assert callable(getattr(inspection, f))


NEW_SYMBOLS = ('jvae_latent_moments_f32', 'jvae_nearest_centroid_f32', 'jvae_histogram_f32')


@pytest.mark.parametrize('name', NEW_SYMBOLS)
def test_new_symbols_are_declared_and_bound(name):
    from jvae_hip import lib
    with open(os.path.join(REPO, 'include', 'jvae_hip.h')) as f:
        header = f.read()
    decl = re.search(r'^int ' + name + r'\(([^;]*)\);', header, re.M | re.S)
    assert decl, name + ' is not declared in include/jvae_hip.h'
    assert name in lib._SIGS, name + ' is not bound in jvae_hip/lib.py'
    restype, argtypes = lib._SIGS[name]
    assert len(argtypes) == len(decl.group(1).split(',')), (name, len(argtypes))
    assert argtypes[-1] is lib.P                                            # the stream comes last


def test_ops_refuse_host_tensors():
    from jvae_hip import lib, ops
    mu = torch.zeros(4, 3)
    for call in (lambda: ops.latent_moments(mu, mu, None, torch.zeros(1, 4, 3, dtype=torch.float64), torch.zeros(1, dtype=torch.int64)),
                 lambda: ops.nearest_centroid(mu, mu), lambda: ops.histogram(mu.reshape(-1), np.linspace(0, 1, 4)),
                 lambda: ops.latent_moments(mu.double(), mu.double(), None, None, None)):
        with pytest.raises(lib.JvaeHipError):
            call()


@pytest.mark.parametrize('name', ZSAMPLE_CASES)
def test_the_moments_give_the_files_of_zsample(name):
    from jvae_compat import inspection
    g = load_golden('zsample_' + name)
    sums, counts = moments64(g['mu'], g['log_var'])
    assert counts[0] == len(g['mu'])
    stats = inspection.per_dim_statistics(sums[0], counts[0])
    assert list(stats) == ['mu2_mu_z', 'mu_var_z', 'mu2_z', 'mu_mu_z', 'std_var_z']
    assert_text(inspection.scatter_text(stats), g['mu_z_var_z'], name + ' mu_z_var_z')
    assert_text(inspection.hist_text(*inspection.per_dim_hist(stats['mu_var_z'], bins=int(g['bins']))), g['hist_var_z'],
                name + ' hist_var_z')
    # grouped by the labels: the groups add up to the whole, and a group of one sample has no deviation
    C = int(g['y'].max()) + 1
    gs, gc = moments64(g['mu'], g['log_var'], g['y'], C)
    assert gc.sum() == len(g['mu']) and np.allclose(gs.sum(0), sums[0], rtol=1e-12, atol=0)
    one = inspection.per_dim_statistics(moments64(g['mu'][:1], g['log_var'][:1])[0][0], 1)
    assert np.isnan(one['std_var_z']).all() and np.isfinite(one['mu2_z']).all()


def test_per_dim_statistics_against_torch():
    from jvae_compat import inspection
    g = load_golden('texts')
    mu, var = torch.from_numpy(g['mu_z']).double(), torch.from_numpy(g['var_z']).double()
    sums = np.stack([mu.sum(0).numpy(), (mu ** 2).sum(0).numpy(), var.sum(0).numpy(), (var ** 2).sum(0).numpy()])
    stats = inspection.per_dim_statistics(sums, len(mu))
    want = {'mu2_mu_z': mu.pow(2).mean(0), 'mu_var_z': var.mean(0), 'mu_mu_z': mu.mean(0), 'std_var_z': var.std(0)}
    for k, v in want.items():
        assert np.allclose(stats[k], v.numpy(), rtol=1e-10, atol=0), k
    assert_text(inspection.scatter_text(stats), g['lat.scatter_per_dim'], 'scatter per_dim')
    assert_text(inspection.hist_text(*inspection.per_dim_hist(stats['mu_var_z'], bins=int(g['bins']))), g['lat.hist_per_dim'],
                'hist per_dim')


def parse_hist(text):
    rows = [l.split() for l in str(text).split('\n')[1:] if l.strip()]
    return np.array([float(r[0]) for r in rows]), np.array([int(float(r[1])) for r in rows[:-1]])


def test_the_histogram_rule_is_numpys():
    from jvae_compat import inspection
    g = load_golden('texts')
    B = int(g['bins'])
    var = g['var_z'].reshape(-1)
    edges = inspection.bin_edges(B, 0, float(var.max()))
    counts, bad = hist64(var, edges)
    assert bad == 0 and (counts[0] == np.histogram(var, bins=B, range=(0, float(var.max())))[0]).all()
    assert_text(inspection.hist_text(edges, counts[0]), g['lat.hist'], 'hist')
    lv = np.log(var)
    edges = inspection.bin_edges(B, float(lv.min()), float(lv.max()))
    counts, _ = hist64(lv, edges)
    assert_text(inspection.hist_text(np.exp(edges), counts[0]), g['lat.hist_log'], 'hist log')
    # values on every edge and on both ends, outside, non-finite, groups
    edges = inspection.bin_edges(10, -1., 3.)
    rng = np.random.default_rng(3)
    v = np.concatenate([edges.astype(np.float32), rng.uniform(-2, 4, 500).astype(np.float32), [np.nan, np.inf, -np.inf]]).astype(np.float32)
    group = rng.integers(-1, 4, len(v))
    counts, bad = hist64(v, edges, group, 3)
    for k in range(3):
        sel = v[(group == k) & np.isfinite(v)]
        assert (counts[k] == np.histogram(sel, bins=10, range=(-1., 3.))[0]).all()
    assert bad == int((~np.isfinite(v[(group >= 0) & (group < 3)])).sum())


def test_scatter_text_of_all_pairs():
    from jvae_compat import inspection
    g = load_golden('texts')
    text = inspection.scatter_text({'mu_z': g['mu_z'].reshape(-1), 'var_z': g['var_z'].reshape(-1)})
    assert_text(text, g['lat.scatter'], 'scatter')


def test_loss_tables_against_the_reference():
    from jvae_compat import inspection
    g = load_golden('texts')
    bins = int(g['graph_bins'])
    losses = {k[5:]: g[k] for k in g if k.startswith('loss.')}
    assert list(losses) == ['cifar10', 'svhn', 'missed']
    hists = {}
    for k, v in losses.items():
        edges = inspection.bin_edges(bins, v.min(), v.max())
        counts, _ = hist64(v, edges)
        hists[k] = (counts[0] / np.diff(edges).astype(float) / counts[0].sum(), edges)
    assert_text(inspection.loss_hist_text(hists, bins), g['graph.hist'], 'graph hist')
    alpha = list(inspection.DEFAULT_QUANTILES)
    table = {}
    for k, v in losses.items():
        s = np.sort(v)
        pos = np.array(alpha) * (len(s) - 1)
        lo = np.floor(pos).astype(int)
        hi = np.minimum(lo + 1, len(s) - 1)
        table[k] = inspection.lerp_quantiles(s[lo], s[hi], pos - lo)
        assert np.array_equal(table[k], np.quantile(v, alpha))            # np.quantile on fp32 data: exactly that, in fp64
    assert_text(inspection.quantile_text(alpha, table), g['graph.boxp'], 'graph boxp')


def test_nearest_centroid_restatement_against_the_reference():
    from jvae_compat import inspection
    g = load_golden('centroids')
    assert clear_margin(dist64(g['mu'], g['centroids'])).all()
    y, d2 = nearest64(g['mu'], g['centroids'])
    assert (y == g['y_nearest']).all() and (d2 >= 0).all()
    mu, cent = torch.from_numpy(g['mu']), torch.from_numpy(g['centroids'])
    assert np.array_equal(inspection.dmu(mu, cent, y=torch.from_numpy(g['y'])).numpy(), g['dmu_y'])
    assert np.array_equal(inspection.dmu(mu, cent[3]).numpy(), g['dmu_single'])
    twice = np.concatenate([g['centroids'][:2], g['centroids'][:2]])
    assert nearest64(g['mu'], twice)[0].max() <= 1                           # two identical centroids: the lower index


def test_predicted_classes_table():
    from jvae_compat import inspection
    g = load_golden('tables')
    C = int(g['num_labels'])
    n_pred = {s: np.bincount(g[f'record.{s}.logits'].argmax(0), minlength=C) for s in ('ind', 'ood')}
    assert inspection.predicted_classes_text(n_pred, C) == str(g['table.predicted-classes-per-set.tab'])
    names = sorted(k[6:] for k in g if k.startswith('table.'))
    want = ['predicted-classes-per-set.tab'] + [f'losses-{k}-per-{w}-{gr}.tab' for k in ('total', 'cross_x', 'kl')
                                                  for w in ('set', 'class.tab') for gr in ('hist', 'boxp')]
    assert names == sorted(want)


def test_the_job_golden_meets_the_conditions_the_gpu_test_relies_on():
    g = load_golden('job_e2_n8_L3')
    for s in ('ind', 'ood'):
        n = len(g['x.' + s])
        assert g[f'samples.{s}.mu'].shape[0] == n and n % int(g['batch_size'])           # two batches, the last one ragged
    assert (g['samples.ind.y'] == g['y.ind']).all()
    zd = g['record.ind.zdist'].astype(np.float64)
    assert clear_margin(zd.T).mean() >= 0.9
    assert (g['samples.ind.y_nearest'] == zd.argmin(0)).all()
    assert not g['samples.ood.y'].any() and not g['samples.ood.y_nearest'].any()      # the reference leaves zeros there
