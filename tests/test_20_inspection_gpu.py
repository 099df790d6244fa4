"""Latent-space inspection on the device: the three kernels of csrc/inspect.hip (ops.latent_moments, ops.nearest_centroid,
ops.histogram) against the fp64 restatements of tests/test_inspection_restatement.py, the encode-only pass
`latent_posterior`, `zsample` / `comparison` of module/sample.py, the sample recorders of `ood_detection_rates` and
`WIMJob.finetune`, and jvae_compat/inspection.py on device tensors, against tests/golden/inspection (the reference's outputs).

Floats follow the rule of tests/test_17_aggregation_gpu.py (`Worst`): the error against the fp64 restatement, relative to the
tensor's largest magnitude, is finite and at most 4 x max(the error of the reference's fp32 torch expression on the same inputs,
one ulp).  Counts, labels and arg-mins are exact.  Texts meet the goldens under `assert_text` (test_inspection_restatement.py).

Measured on an MI355X (kernel error, in brackets the fp32 torch expression's), worst statistic of each shape:
    latent_moments (N, K, G)    (1, 1, 1) 1.42e-07 (1.62e-07)       (7, 3, 2) 6.00e-08 (8.58e-08)       (65, 64, 10) 5.68e-08 (9.04e-08)
                                (300, 16, 3) 2.40e-08 (1.39e-07)    (513, 130, 1) 5.47e-08 (1.03e-07)   (4099, 32, 100) 1.70e-07 (1.60e-07)
    nearest_centroid d2 (N, C, K)   (1, 1, 1) 1.65e-08 (5.14e-08)   (5, 2, 3) 3.59e-08 (7.47e-08)       (64, 10, 64) 3.39e-08 (1.11e-07)
                                (257, 100, 16) 3.96e-08 (1.08e-07)  (1000, 1000, 2) 1.89e-08 (2.42e-08)
The moments' error is that of expf against numpy's fp32 exp (the sums themselves are fp64); histogram counts, arg-mins and labels
are exact.

One case is not as the issue states it: `latent_posterior` of ex2_n8_xvae_L2 without labels does not raise, because that model
does not code its labels (see test_latent_posterior_is_the_posterior_of_evaluate); the refusal is shown on j2_n8_jvae.
"""
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state
from test_inspection_restatement import (MARGIN, RTOL, ZSAMPLE_CASES, assert_text, centroid_inputs, clear_margin, dist64, hist64,
                                         load_golden, moments64, nearest64)
from test_17_aggregation_gpu import Worst, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build(name, seed=0, job=4217, **over):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case(name)['net'], **over))
    load_det_state(net, seed=seed)
    net.to(DEV)
    net.eval()
    net.job_number = job
    return net


# ------------------------------------------------------------------------------------------------------ 1. latent_moments
def moment_inputs(N, K, G, seed=0):
    g = np.random.default_rng(seed + N)
    mu = (g.standard_normal((N, K)) * 2).astype(np.float32)
    lv = (g.standard_normal((N, K)) - 1).astype(np.float32)
    group = g.integers(0, G, N).astype(np.int32) if G > 1 else None
    if (N, K, G) == (300, 16, 3):                       # one empty group, ids of -1 and G
        group = g.integers(0, 2, N).astype(np.int32)
        group[::17], group[5::23] = -1, G
    return mu, lv, group


def torch_moments(mu, lv, group, G):
    """the fp32 torch expressions: masked sums per group"""
    m, v = torch.from_numpy(mu), torch.from_numpy(lv).exp()
    grp = torch.zeros(len(mu), dtype=torch.int64) if group is None else torch.from_numpy(group).long()
    out = np.zeros((G, 4, mu.shape[1]))
    for g in range(G):
        i = grp == g
        out[g] = torch.stack([m[i].sum(0), m[i].pow(2).sum(0), v[i].sum(0), v[i].pow(2).sum(0)]).double().numpy()
    return out


@pytest.mark.parametrize('shape', [(1, 1, 1), (7, 3, 2), (65, 64, 10), (300, 16, 3), (513, 130, 1), (4099, 32, 100)])
def test_latent_moments_against_the_fp64_restatement(shape):
    from jvae_hip import lib, ops
    N, K, G = shape
    mu, lv, group = moment_inputs(N, K, G)
    d = [dev(mu), dev(lv), None if group is None else dev(group)]

    def run(parts=((0, N),)):
        sums = torch.zeros((G, 4, K), dtype=torch.float64, device=DEV)
        counts = torch.zeros(G, dtype=torch.int64, device=DEV)
        for a, b in parts:
            ops.latent_moments(d[0][a:b], d[1][a:b], None if d[2] is None else d[2][a:b], sums, counts)
        return sums, counts

    sums, counts = run()
    exact, n = moments64(mu, lv, group, G)
    assert (counts.cpu().numpy() == n).all()
    again = run()
    assert same_bits(sums, again[0]) and same_bits(counts, again[1])
    ref = torch_moments(mu, lv, group, G)
    w = Worst(f'latent_moments {shape}')
    for s in range(4):
        w.check(sums[:, s], ref[:, s], exact[:, s], (shape, s))
    w.report()
    if N > 1:                                             # two calls on the halves: the same sums up to fp64 rounding
        halves, hc = run(((0, N // 2), (N // 2, N)))
        assert same_bits(hc, counts)
        absum = moments64(np.abs(mu), lv, group, G)[0]
        bound = N * 2. ** -52 * absum
        assert (np.abs(halves.cpu().numpy() - sums.cpu().numpy()) <= bound).all()
    if shape == (7, 3, 2):
        zeros = torch.zeros((G, 4, K), dtype=torch.float64, device=DEV), torch.zeros(G, dtype=torch.int64, device=DEV)
        for bad in (lambda: ops.latent_moments(d[0].double(), d[1].double(), d[2], *zeros),
                    lambda: ops.latent_moments(d[0], d[1], d[2].long(), *zeros),
                    lambda: ops.latent_moments(d[0], d[1], d[2], zeros[0].float(), zeros[1]),
                    lambda: ops.latent_moments(d[0], d[1], None, *zeros),
                    lambda: ops.latent_moments(d[0], d[1][:, :2], d[2], *zeros)):
            with pytest.raises(lib.JvaeHipError):
                bad()
        assert not zeros[0].any() and not zeros[1].any()


# ---------------------------------------------------------------------------------------------------- 2. nearest_centroid
@pytest.mark.parametrize('shape', [(1, 1, 1), (5, 2, 3), (64, 10, 64), (257, 100, 16), (1000, 1000, 2)])
def test_nearest_centroid_against_the_fp64_restatement(shape):
    from jvae_hip import ops
    N, C, K = shape
    mu, cent = centroid_inputs(N, C, K, seed=11)
    y, d2 = ops.nearest_centroid(dev(mu), dev(cent))
    assert y.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(y.shape) == (N,) == tuple(d2.shape)
    ey, ed = nearest64(mu, cent)
    assert (y.cpu().numpy() == ey).all()                                   # every row: none is left out
    tm, tc = torch.from_numpy(mu), torch.from_numpy(cent)
    ref = (tm.unsqueeze(1) - tc.unsqueeze(0)).pow(2).sum(-1).min(1).values
    w = Worst(f'nearest_centroid {shape}')
    w.check(d2, ref, ed, shape)
    w.report()
    again = ops.nearest_centroid(dev(mu), dev(cent))
    assert same_bits(y, again[0]) and same_bits(d2, again[1])
    twice = np.concatenate([cent, cent])                                   # two identical centroids: the lower index wins
    assert (ops.nearest_centroid(dev(mu), dev(twice))[0].cpu().numpy() == ey).all()


def test_estimate_y_and_dmu_against_the_reference():
    from jvae_compat import inspection
    g = load_golden('centroids')
    mu, cent = dev(g['mu']), dev(g['centroids'])
    assert (inspection.estimate_y(mu, cent).cpu().numpy() == g['y_nearest']).all()
    assert same_bits(inspection.dmu(mu, cent, y=dev(g['y'])), g['dmu_y'])
    assert same_bits(inspection.dmu(mu, cent[3]), g['dmu_single'])


# ------------------------------------------------------------------------------------------------------------ 3. histogram
def hist_inputs(n, B, G):
    from jvae_compat.inspection import bin_edges
    g = np.random.default_rng(n + B)
    lo, hi = -1.5, 2.25
    edges = bin_edges(B, lo, hi)
    v = g.uniform(lo - 0.5, hi + 0.5, n).astype(np.float32)
    if n == 1:
        v[:] = 0.5
    if (n, B) == (1000, 10):                                               # values on every edge and on both ends
        v[:B + 1] = edges.astype(np.float32)
        v[B + 1:B + 3] = [np.nextafter(np.float32(lo), np.float32(-9)), np.nextafter(np.float32(hi), np.float32(9))]
    group = None
    if G > 1:
        group = g.integers(-1, G + 1, n).astype(np.int32)                  # skipped ids: -1 and G
    return v, edges, group


@pytest.mark.parametrize('shape', [(1, 1, 1), (7, 3, 1), (1000, 10, 1), (4099, 20, 3), (100000, 64, 1), (5000, 4096, 1),
                                   (5000, 300, 20)])
def test_histogram_is_numpys(shape):
    from jvae_hip import ops
    n, B, G = shape                                                        # (5000, 300, 20): G B = 6000 does not fit the LDS path
    v, edges, group = hist_inputs(n, B, G)
    counts = ops.histogram(dev(v), edges, group=None if group is None else dev(group), G=G, check=True)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (G, B)
    got = counts.cpu().numpy()
    for k in range(G):
        sel = v if group is None else v[group == k]
        want = np.histogram(sel, bins=B, range=(float(edges[0]), float(edges[-1])))[0]
        assert (got[k] == want).all(), (shape, k)
    inside = (v >= edges[0]) & (v <= edges[-1]) & (True if group is None else (group >= 0) & (group < G))
    assert got.sum() == inside.sum() < n or n <= 7                          # values outside the range are not counted
    assert (got == hist64(v, edges, group, G)[0]).all()
    ops.histogram(dev(v), edges, group=None if group is None else dev(group), counts=counts)       # accumulation: exact
    assert (counts.cpu().numpy() == 2 * got).all()


@pytest.mark.parametrize('B,G', [(10, 1), (300, 20)])
def test_histogram_counts_the_non_finite_values_apart(B, G):
    from jvae_hip import ops
    v, edges, group = hist_inputs(4099, B, G)
    v[[3, 77, 4000]] = [np.nan, np.inf, -np.inf]
    if group is not None:
        group[[3, 77, 4000]] = 0
    gd = None if group is None else dev(group)
    counts = ops.histogram(dev(v), edges, group=gd, G=G)
    assert (counts.cpu().numpy() == hist64(v, edges, group, G)[0]).all()
    with pytest.raises(ValueError, match='3 non-finite'):
        ops.histogram_check()
    ops.histogram_check()                                                   # the word was cleared
    with pytest.raises(ValueError):
        ops.histogram(dev(v), edges, group=gd, G=G, check=True)
    with pytest.raises(ValueError):
        ops.histogram(dev(v), [0., 2., 1.])


# ----------------------------------------------------------------------------------------------------- 4. latent_posterior
@pytest.mark.parametrize('name,with_y', [('e2_n8_L3', False), ('c1_n16_mlp', False), ('ea2_n8_vae_L3', False), ('eb2_n8_vib_L2', False),
                                         ('ex2_n8_xvae_L2', True), ('ex2_n8_xvae_L2', False), ('j2_n8_jvae', True)])
def test_latent_posterior_is_the_posterior_of_evaluate(name, with_y, monkeypatch):
    """ex2_n8_xvae_L2 is evaluated with its labels, as for a model that needs them.  It does not: the case's y_is_coded is off
    and its label-free evaluate() runs (tests/golden/ex2_n8_xvae_L2.npz is that run), so latent_posterior(x) serves it too and
    is held to that run; the refusal without labels is shown on the coded model j2_n8_jvae."""
    net = build(name)
    kw = get_case(name)['net']
    x, y, _ = det_inputs(8, kw['input_shape'], kw['num_labels'], net.latent_sampling, kw['latent_dim'])
    x, y = x.to(DEV), y.to(DEV)
    assert net.y_is_coded == (name == 'j2_n8_jvae')
    with torch.no_grad():
        out = net.evaluate(x, y if with_y else None, z_output=True)
    if net.y_is_coded:
        with pytest.raises(NotImplementedError):
            net.latent_posterior(x)
    monkeypatch.setattr(net, '_decode', lambda z: (_ for _ in ()).throw(AssertionError('the decoder was called')))
    mu, log_var = net.latent_posterior(x, y if with_y else None)
    assert same_bits(mu, out[4]) and same_bits(log_var, out[5])
    assert not mu.requires_grad and tuple(mu.shape) == (8, kw['latent_dim'])


def test_latent_posterior_in_the_bf16_mode():
    net = build('c5_n4')
    net.set_compute_dtype('bf16')
    kw = get_case('c5_n4')['net']
    x, y, _ = det_inputs(4, kw['input_shape'], kw['num_labels'], net.latent_sampling, kw['latent_dim'])
    x, y = x.to(DEV), y.to(DEV)
    with torch.no_grad():
        out = net.evaluate(x, y if net.y_is_coded else None, z_output=True)
    mu, log_var = net.latent_posterior(x, y if net.y_is_coded else None)
    assert same_bits(mu, out[4]) and same_bits(log_var, out[5])


# -------------------------------------------------------------------------------------------------------------- 5. zsample
@pytest.mark.parametrize('name', ZSAMPLE_CASES)
def test_zsample_against_the_reference(name, tmp_path, monkeypatch):
    from jvae_compat import inspection
    from module.sample import zsample
    g = load_golden('zsample_' + name)
    net = build(name, job=int(g['job_number']))
    kw = get_case(name)['net']
    bs, bins, N = int(g['batch_size']), int(g['bins']), len(g['mu'])
    x, y, _ = det_inputs(N + 1, kw['input_shape'], kw['num_labels'], net.latent_sampling, kw['latent_dim'])
    x0, y0, _ = det_inputs(N, kw['input_shape'], kw['num_labels'], net.latent_sampling, kw['latent_dim'])
    x[:N], y[:N] = x0, y0                                                  # one more sample than a multiple of the batch: cut
    assert (y0.numpy() == g['y']).all()
    monkeypatch.setattr(net, '_decode', lambda z: (_ for _ in ()).throw(AssertionError('the decoder was called')))
    out = zsample(x, net, y=y, batch_size=bs, root=str(tmp_path / '%j'), bins=bins)
    d = tmp_path / ('%06d' % net.job_number) / 'test'
    assert out['dir'] == str(d) and out['counts'].sum() == N
    assert_text((d / 'mu_z_var_z.dat').read_text(), g['mu_z_var_z'], name)
    assert_text((d / 'hist_var_z.dat').read_text(), g['hist_var_z'], name)
    mu, lv = net.latent_posterior(x0.to(DEV), y0.to(DEV) if net.y_is_coded else None)
    assert float((mu.cpu() - torch.from_numpy(g['mu'])).abs().max()) <= RTOL * np.abs(g['mu']).max()
    mu, lv = mu.cpu().numpy(), lv.cpu().numpy()
    C = kw['num_labels']
    present = set(int(c) for c in g['y'])
    assert len(present) < C                                                 # the case has absent classes
    files = sorted(os.listdir(d))
    assert files == sorted(['hist_var_z.dat', 'mu_z_var_z.dat'] + [f'{s}{c}.dat' for s in ('hist_var_z', 'mu_z_var_z') for c in present])
    for c in present:                                                       # the class's own statistics, not the whole set's
        sums, n = moments64(mu[g['y'] == c], lv[g['y'] == c])
        stats = inspection.per_dim_statistics(sums[0], n[0])
        assert_text((d / f'mu_z_var_z{c}.dat').read_text(), inspection.scatter_text(stats), (name, c))
        assert_text((d / f'hist_var_z{c}.dat').read_text(), inspection.hist_text(*inspection.per_dim_hist(stats['mu_var_z'], bins=bins)),
                    (name, c))


# ------------------------------------------------------------------------------------------------- 6. sample recorders
class Named(torch.utils.data.TensorDataset):
    def __init__(self, name, *t):
        super().__init__(*t)
        self.name = name


def test_ood_detection_rates_fills_and_writes_the_sample_recorders(tmp_path):
    from jvae_compat.recorders import SampleRecorder
    g = load_golden('job_e2_n8_L3')
    bs = int(g['batch_size'])
    sets = {s: Named(s, torch.from_numpy(g['x.' + s]), torch.from_numpy(g['y.' + s])) for s in ('ind', 'ood')}

    def rates(**kw):
        net = build('e2_n8_L3')
        net.training_parameters['set'] = 'ind'
        torch.manual_seed(5)
        with torch.no_grad():
            return net, net.ood_detection_rates(oodsets=[sets['ood']], testset=sets['ind'], batch_size=bs, method=['iws', 'kl'], **kw)

    net, plain = rates()
    K = net.latent_dim
    fakes = dict(mu=torch.zeros(bs, K, device=DEV), y=torch.zeros(bs, dtype=torch.int64, device=DEV))
    fakes['y_nearest'] = fakes['y']
    recs = {s: SampleRecorder(bs, **fakes) for s in sets}
    dirs = [str(tmp_path / 'a'), str(tmp_path / 'b' / 'c')]
    _, with_recs = rates(sample_recorders=recs, sample_dirs=dirs)
    assert repr(with_recs) == repr(plain)                                   # the same bits: every float prints in full
    zd = g['record.ind.zdist'].astype(np.float64)
    clear = clear_margin(zd.T)
    assert clear.mean() >= 0.9
    for s in sets:
        for d in dirs:
            r = SampleRecorder.load(os.path.join(d, f'samples-{s}.pth'))
            assert sorted(r.keys()) == ['mu', 'y', 'y_nearest'] and r.recorded_samples == len(sets[s])
            assert same_bits(r['mu'].cpu(), recs[s]['mu'].cpu())
        mu = recs[s]['mu'].cpu().numpy()
        want = g[f'samples.{s}.mu']
        assert mu.shape == want.shape and np.abs(mu - want).max() <= RTOL * np.abs(want).max()
        assert (recs[s]['y'].cpu().numpy() == g['y.' + s]).all()             # the OOD sets get their labels too
    yn = recs['ind']['y_nearest'].cpu().numpy()
    assert (yn[clear] == g['samples.ind.y_nearest'][clear]).all()
    assert recs['ood']['y_nearest'].cpu().numpy().shape == (len(sets['ood']),)

    # a recorder with mu alone takes mu alone; a model without class axis in zdist cannot give y_nearest
    only_mu = {'ind': SampleRecorder(bs, mu=fakes['mu'])}
    rates(sample_recorders=only_mu)
    assert list(only_mu['ind'].keys()) == ['mu'] and same_bits(only_mu['ind']['mu'].cpu(), recs['ind']['mu'].cpu())
    vae = build('ea2_n8_vae_L3')
    vae.training_parameters['set'] = 'ind'
    with pytest.raises(ValueError, match='y_nearest'), torch.no_grad():
        vae.ood_detection_rates(oodsets=[sets['ood']], testset=sets['ind'], batch_size=bs, method=['iws'],
                                sample_recorders={'ind': SampleRecorder(bs, **fakes)})


def test_finetune_writes_the_latent_records_before_and_after(tmp_path):
    from jvae_compat.recorders import SampleRecorder
    from test_15_wim_finetune_gpu import loop_sets, wim_job

    def run(with_recorders):
        job, case = wim_job(fused=False)
        trainset, ind, oods = loop_sets()
        recs = None
        if with_recorders:
            job.saved_dir = str(tmp_path / 'job')
            recs = job.make_sample_recorders(['cifar', 'svhn'], 8)
        torch.manual_seed(21)
        job.finetune(trainset, ind, oods, batch_size=8, epochs=1, test_batch_size=8, alpha=case['alpha'], sample_recorders=recs)
        torch.cuda.synchronize()
        return job, recs

    job, recs = run(True)
    plain, _ = run(False)
    for (k, a), b in zip(job.state_dict().items(), plain.state_dict().values()):
        assert same_bits(a, b), k                                           # the recorders change nothing in the loop
    root = os.path.join(job.saved_dir, 'samples', '{:04d}'.format(job.trained))
    for s in ('cifar', 'svhn'):
        before = SampleRecorder.load(os.path.join(root, 'init', f'samples-{s}.pth'))
        after = SampleRecorder.load(os.path.join(root, f'samples-{s}.pth'))
        for r in (before, after):
            assert sorted(r.keys()) == ['mu', 'y', 'y_nearest'] and r.recorded_samples == 8
            assert tuple(r._aux['centroids'].shape) == (10, job.latent_dim) and tuple(r._aux['alternate'].shape) == (job.latent_dim,)
        assert not same_bits(before['mu'].cpu(), after['mu'].cpu())
        assert same_bits(after['mu'].cpu(), recs[s]['mu'].cpu()) and same_bits(before['y'].cpu(), after['y'].cpu())


# ------------------------------------------------------------------------------------------------------- 7. the host layer
def test_comparison_against_the_reference():
    from jvae_hip import ops
    from module.sample import comparison
    g = load_golden('comparison')
    jobs = [int(j) for j in g['jobs']]
    nets = [build('e2_n8_L3', seed=s, job=j) for s, j in enumerate(jobs)]
    x, eps = dev(g['x']), dev(g['eps'])
    for n in nets:                                                          # the golden's noise in every evaluate() of the run
        n.evaluate = (lambda own: lambda x_, **k: own(x_, epsilon=eps, **k))(n.evaluate)
    div, y_pred = comparison(x, *nets, batch_size=4)
    assert list(div) == jobs and list(div[jobs[0]]) == [jobs[1]] and div[jobs[1]] == {}
    got = div[jobs[0]][jobs[1]]
    assert float((got.double() - torch.from_numpy(g['div']).double()).abs().max()) <= RTOL * np.abs(g['div']).max()
    for j in jobs:
        assert (y_pred[j].numpy() == g[f'y_pred.{j}']).all()
    with torch.no_grad():
        reco = [torch.cat([n.evaluate(x[a:a + 4])[0][0] for a in (0, 4)]).unsqueeze(0) for n in nets]
    assert same_bits(got, ops.cascade_mse(x, reco)[2].cpu())                 # row p = 2 (2 - 1) / 2 + 1: stage 2 against stage 1


def test_output_latent_distribution_on_device_tensors(tmp_path, capsys):
    import sys
    from jvae_compat import inspection
    g = load_golden('texts')
    mu, var, bins = dev(g['mu_z']), dev(g['var_z']), int(g['bins'])
    modes = {'hist': dict(result_type='hist_of_var', bins=bins), 'hist_per_dim': dict(result_type='hist_of_var', bins=bins, per_dim=True),
             'hist_log': dict(result_type='hist_of_var', bins=bins, log_scale=True),
             'hist_log_per_dim': dict(result_type='hist_of_var', bins=bins, log_scale=True, per_dim=True),
             'scatter': dict(result_type='scatter'), 'scatter_per_dim': dict(result_type='scatter', per_dim=True)}
    for mode, kw in modes.items():
        f = tmp_path / 'sub' / (mode + '.dat')
        inspection.output_latent_distribution(mu, var, str(f), sys.stdout, **kw)
        assert_text(f.read_text(), g['lat.' + mode], mode)
        assert capsys.readouterr().out == f.read_text()


def test_loss_graphs_and_comparisons_on_device_tensors(tmp_path):
    import types
    from jvae_compat import inspection
    from jvae_compat.recorders import LossRecorder
    g = load_golden('texts')
    losses = {k[5:]: dev(g[k]) for k in g if k.startswith('loss.')}
    for graph in ('hist', 'boxp'):
        f = tmp_path / 'graphs' / (graph + '.tab')
        inspection.losses_distribution_graphs(losses, str(f), graph=graph, bins=int(g['graph_bins']))
        assert_text(f.read_text(), g['graph.' + graph], graph)

    t = load_golden('tables')
    net = types.SimpleNamespace(saved_dir=str(tmp_path / 'job'), job_number=int(t['job_number']), num_labels=int(t['num_labels']),
                                training_parameters={'set': 'ind'}, ood_results={'ood': {}}, device=torch.device(DEV),
                                predict_after_evaluate=lambda logits, losses: logits.argmax(-1))
    last = os.path.join(net.saved_dir, 'samples', 'last')
    os.makedirs(last)
    bs = int(t['batch_size'])
    for s in ('ind', 'ood'):
        keys = [k.split('.', 2)[2] for k in t if k.startswith(f'record.{s}.')]
        r = LossRecorder(bs)
        n = len(t[f'record.{s}.y_true'])
        for a in range(0, n, bs):
            r.append_batch(**{k: torch.from_numpy(t[f'record.{s}.{k}'][..., a:a + bs]) for k in keys})
        r.save(os.path.join(last, f'record-{s}.pth'))
    root = tmp_path / 'tables'
    inspection.loss_comparisons(net, root=str(root), bins=int(t['bins']), echo=False)
    names = sorted(k[6:] for k in t if k.startswith('table.'))
    assert sorted(os.listdir(root)) == names
    for f in names:
        assert_text((root / f).read_text(), t['table.' + f], f)
