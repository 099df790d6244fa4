#!/usr/bin/env python3
"""Write tests/golden/inspection/*.npz: what the REFERENCE's latent-space inspection computes and writes, on seeded inputs.

    python tools/gen_inspection_golden.py --reference <checkout of moxime/joint-vae>

Runs on the CPU.  The reference is imported under the placeholder modules of oracle/gen_golden.py::import_reference(); only
data is written (tensors, texts of the files the reference wrote, names):

  texts.npz          utils/inspection.py on synthetic tensors: `mu_z`, `var_z` (N, K) and the text output_latent_distribution
                     writes for hist_of_var / scatter, per_dim or not, and hist_of_var with log_scale (`lat.<mode>`);
                     three loss vectors of different lengths (`loss.<name>`) and the text of losses_distribution_graphs for
                     graph='hist' and 'boxp' (`graph.hist`, `graph.boxp`), with `bins`.
  zsample_<case>.npz module/sample.py::zsample on det-state models (c1_n16_mlp, e2_n8_L3, ea2_n8_vae_L3) and det_inputs: the
                     two all-sample files (`hist_var_z`, `mu_z_var_z`), the `mu` / `log_var` the reference's evaluate() returned,
                     `y`, `batch_size`, `bins`.  (For a cvae the reference reads `encoder.latent_dictionary`, which its encoder no
                     longer has: the prior's means are put there, they are only printed.)  ASSERTED: every per-class file the
                     reference writes is byte-identical to the all-sample file (it never applies its class mask).
  centroids.npz      ft/inspection.py::estimate_y / dmu on seeded `mu` (N, K), `centroids` (C, K), `y`: `y_nearest`, `dmu_y`,
                     `dmu_single`.  ASSERTED: the two smallest squared distances of every row differ by more than 1e-3 relative
                     in fp64 (rows that do not are redrawn).
  job_e2_n8_L3.npz   cvae.py::ood_detection_rates(sample_recorders=..., recorders={}) for e2_n8_L3 on an in-distribution and an
                     OOD TensorDataset of two batches each, the last one ragged: the inputs (`x.<set>`, `y.<set>`), the tensors
                     of the sample recorders (`samples.<set>.<key>`) and of the loss recorders (`record.<set>.<key>`).
                     ASSERTED: at least 90 % of the in-distribution samples have their two smallest zdist more than 1e-3
                     (relative) apart.
  tables.npz         utils/inspection.py::loss_comparisons on a synthetic job directory (see tables()): the recorded tensors
                     (`record.<set>.<key>`) and every table it writes (`table.<file name>`).
  comparison.npz     module/sample.py::comparison on two det-state models (seeds 0 and 1 of e2_n8_L3): `x`, `jobs`, `div`,
                     `y_pred.<job>`, and `eps` (L + 1, 4, K), the noise injected into every evaluate() of the run (the predictions
                     read sampled losses).
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'inspection')
sys.path.insert(0, REPO)

JOB_NUMBER = 4217
ZSAMPLE = {'c1_n16_mlp': dict(N=16, batch_size=8), 'e2_n8_L3': dict(N=8, batch_size=4), 'ea2_n8_vae_L3': dict(N=8, batch_size=4)}
BINS = 7
SETS = {'ind': 7, 'ood': 6}          # samples per set of the job fixture; batch size 4: two batches, the last one ragged
BATCH = 4
MARGIN = 1e-3


def det_net(Net, name, seed=0, job=JOB_NUMBER):
    from oracle.cases import get_case
    from oracle.det_init import load_det_state
    kw = get_case(name)['net']
    torch.manual_seed(0)
    net = Net(**kw)
    load_det_state(net, seed=seed)
    net.eval()
    net.job_number = job
    return net, kw


def read(path):
    with open(path) as f:
        return f.read()


def save(name, **data):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **data)
    print(f'{name}: {len(data)} entries, {os.path.getsize(path)} bytes')


def texts(ref_insp):
    g = torch.Generator().manual_seed(99)
    N, K = 37, 6
    mu_z = torch.randn(N, K, generator=g) * torch.linspace(0.2, 2., K)
    var_z = (torch.randn(N, K, generator=g) * 0.5 - torch.linspace(0., 3., K)).exp()
    data = dict(mu_z=mu_z.numpy(), var_z=var_z.numpy(), bins=np.int64(BINS))
    with tempfile.TemporaryDirectory() as tmp:
        modes = {'hist': dict(result_type='hist_of_var', bins=BINS), 'hist_per_dim': dict(result_type='hist_of_var', bins=BINS, per_dim=True),
                 'hist_log': dict(result_type='hist_of_var', bins=BINS, log_scale=True),
                 'hist_log_per_dim': dict(result_type='hist_of_var', bins=BINS, log_scale=True, per_dim=True),
                 'scatter': dict(result_type='scatter'), 'scatter_per_dim': dict(result_type='scatter', per_dim=True)}
        for mode, kw in modes.items():
            f = os.path.join(tmp, 'sub', mode + '.dat')
            ref_insp.output_latent_distribution(mu_z, var_z, f, **kw)
            data['lat.' + mode] = np.array(read(f))
        losses = {'cifar10': torch.randn(53, generator=g) * 3 + 100, 'svhn': torch.randn(41, generator=g) * 8 + 120,
                  'missed': torch.rand(17, generator=g) * 5 + 90}
        for k, v in losses.items():
            data['loss.' + k] = v.numpy()
        for graph in ('hist', 'boxp'):
            f = os.path.join(tmp, 'graphs', graph + '.tab')
            ref_insp.losses_distribution_graphs(losses, f, graph=graph, bins=BINS + 1)
            data['graph.' + graph] = np.array(read(f))
        data['graph_bins'] = np.int64(BINS + 1)
    save('texts', **data)


def zsample(Net, ref_sample):
    from oracle.det_init import det_inputs
    for name, p in ZSAMPLE.items():
        net, kw = det_net(Net, name)
        x, y, _ = det_inputs(p['N'], kw['input_shape'], kw['num_labels'], net.latent_sampling, kw['latent_dim'])
        kept = []
        evaluate = net.evaluate

        def spy(*a, **k):
            out = evaluate(*a, **k)
            kept.append((out[4].clone(), out[5].clone()))
            return out
        net.evaluate = spy
        if net.is_cvae:               # zsample reads an attribute the reference's encoder no longer has (module/sample.py:208)
            net.encoder.latent_dictionary = net.encoder.prior.mean.detach()
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            ref_sample.zsample(x, net, y=y, batch_size=p['batch_size'], root=os.path.join(tmp, '%j'), bins=BINS, directory='test')
            d = os.path.join(tmp, '%06d' % JOB_NUMBER, 'test')
            files = {f: read(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        C = kw['num_labels']
        assert set(files) == {'hist_var_z.dat', 'mu_z_var_z.dat'} | {f'{s}{c}.dat' for s in ('hist_var_z', 'mu_z_var_z') for c in range(C)}
        for c in range(C):            # the class mask is built and never applied: every per-class file repeats the all-sample one
            assert files[f'hist_var_z{c}.dat'] == files['hist_var_z.dat'] and files[f'mu_z_var_z{c}.dat'] == files['mu_z_var_z.dat']
        save('zsample_' + name, hist_var_z=np.array(files['hist_var_z.dat']), mu_z_var_z=np.array(files['mu_z_var_z.dat']),
             mu=torch.cat([m for m, _ in kept]).numpy(), log_var=torch.cat([v for _, v in kept]).numpy(), y=y.numpy(),
             batch_size=np.int64(p['batch_size']), bins=np.int64(BINS), job_number=np.int64(JOB_NUMBER))


def centroid_inputs(N, C, K, seed):
    """Seeded normal draws whose best and second-best squared distance differ by more than MARGIN (relative, fp64); the few rows
    that do not are redrawn."""
    g = np.random.default_rng(seed)
    cent = g.standard_normal((C, K)).astype(np.float32)
    mu = g.standard_normal((N, K)).astype(np.float32)
    for _ in range(100):
        d = ((mu[:, None].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1)
        if C < 2:
            break
        two = np.sort(d, 1)[:, :2]
        bad = np.where(two[:, 1] - two[:, 0] <= MARGIN * two[:, 1])[0]
        if not len(bad):
            break
        mu[bad] = g.standard_normal((len(bad), K)).astype(np.float32)
    else:
        raise AssertionError('no draw with the margin')
    return mu, cent


def centroids(ref_ft):
    mu, cent = centroid_inputs(61, 10, 16, 7)
    y = np.random.default_rng(8).integers(0, 10, 61)
    tm, tc, ty = torch.from_numpy(mu), torch.from_numpy(cent), torch.from_numpy(y)
    save('centroids', mu=mu, centroids=cent, y=y, y_nearest=ref_ft.estimate_y(tm, tc).numpy(),
         dmu_y=ref_ft.dmu(tm, tc, y=ty).numpy(), dmu_single=ref_ft.dmu(tm, tc[3]).numpy())


class NamedSet(torch.utils.data.TensorDataset):
    def __init__(self, name, *t):
        super().__init__(*t)
        self.name = name


def job(Net):
    from utils.save_load import LossRecorder, SampleRecorder
    net, kw = det_net(Net, 'e2_n8_L3')
    C, K = kw['num_labels'], kw['latent_dim']
    net.training_parameters['set'] = 'ind'
    g = torch.Generator().manual_seed(2024)
    sets, data = {}, {}
    for s, n in SETS.items():
        x = torch.rand((n, *kw['input_shape']), generator=g)
        y = torch.randint(0, C, (n,), generator=g)
        sets[s] = NamedSet(s, x, y)
        data['x.' + s], data['y.' + s] = x.numpy(), y.numpy()
    fakes = dict(mu=torch.zeros(BATCH, K), y=torch.zeros(BATCH, dtype=int))
    fakes['y_nearest'] = fakes['y']
    recs = {s: SampleRecorder(BATCH, **fakes) for s in sets}
    loss_recs = {s: LossRecorder(BATCH) for s in sets}
    with tempfile.TemporaryDirectory() as tmp:
        net.saved_dir = os.path.join(tmp, 'job')
        last = os.path.join(net.saved_dir, 'samples', 'last')
        os.makedirs(last)
        torch.manual_seed(5)
        with torch.no_grad():
            net.ood_detection_rates(oodsets=[sets['ood']], testset=sets['ind'], batch_size=BATCH, num_batch='all',
                                    method=['iws', 'kl'], recorders=loss_recs, sample_dirs=[last], sample_recorders=recs,
                                    from_where='compute', print_result=False)
        for s in sets:
            assert os.path.exists(os.path.join(last, f'samples-{s}.pth')) and os.path.exists(os.path.join(last, f'record-{s}.pth'))
            for k in recs[s].keys():
                data[f'samples.{s}.{k}'] = recs[s][k].numpy()
            for k in loss_recs[s].keys():
                data[f'record.{s}.{k}'] = loss_recs[s][k].numpy()
        zd = np.sort(data['record.ind.zdist'].astype(np.float64), 0)
        clear = (zd[1] - zd[0]) > MARGIN * zd[1]
        assert clear.mean() >= 0.9, clear.mean()
        assert (data['samples.ind.y'] == data['y.ind']).all()
    data.update(batch_size=np.int64(BATCH), job_number=np.int64(JOB_NUMBER))
    save('job_e2_n8_L3', **data)


def tables(ref_insp):
    """loss_comparisons on a synthetic job directory: three classes, a test set and one OOD set of 40 and 30 recorded samples whose
    logits predict every class and miss some labels (the reference fails on an empty group).  The net is a stand-in object:
    loss_comparisons reads saved_dir, job_number, training_parameters['set'], ood_results, num_labels and calls
    predict_after_evaluate(logits, losses), here the arg-max of the logits."""
    import types
    from utils.save_load import LossRecorder
    C, g = 3, torch.Generator().manual_seed(31)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        net = types.SimpleNamespace(saved_dir=os.path.join(tmp, 'job'), job_number=JOB_NUMBER, num_labels=C,
                                    training_parameters={'set': 'ind'}, ood_results={'ood': {}},
                                    predict_after_evaluate=lambda logits, losses: logits.argmax(-1))
        last = os.path.join(net.saved_dir, 'samples', 'last')
        os.makedirs(last)
        for s, n in (('ind', 40), ('ood', 30)):
            r = LossRecorder(10)
            for b in range(n // 10):
                y = torch.randint(0, C, (10,), generator=g)
                logits = torch.randn(C, 10, generator=g) + 1.5 * torch.nn.functional.one_hot(y, C).T
                r.append_batch(total=torch.randn(C, 10, generator=g) * 4 + 200, cross_x=torch.randn(10, generator=g) * 3 + 180,
                               kl=torch.rand(C, 10, generator=g) * 20, logits=logits, y_true=y)
            r.save(os.path.join(last, f'record-{s}.pth'))
            for k in r.keys():
                data[f'record.{s}.{k}'] = r[k].numpy()
        pred = data['record.ind.logits'].argmax(0)
        hit = pred == data['record.ind.y_true']
        assert hit.any() and (~hit).any() and set(pred) == set(range(C))
        root = os.path.join(tmp, 'tables')
        with contextlib.redirect_stdout(io.StringIO()):
            ref_insp.loss_comparisons(net, root=root, bins=BINS)
        for f in sorted(os.listdir(root)):
            data['table.' + f] = np.array(read(os.path.join(root, f)))
    data.update(batch_size=np.int64(10), bins=np.int64(BINS), job_number=np.int64(JOB_NUMBER), num_labels=np.int64(C))
    save('tables', **data)


def comparison(Net, ref_sample):
    nets = [det_net(Net, 'e2_n8_L3', seed=s, job=JOB_NUMBER + s)[0] for s in (0, 1)]
    kw = det_net(Net, 'e2_n8_L3')[1]
    x = torch.rand((8, *kw['input_shape']), generator=torch.Generator().manual_seed(77))
    for n in nets:
        n.compute_max_batch_size = lambda batch_size, which: batch_size       # the reference probes the device memory here
    from oracle import gen_golden
    jobs = [n.job_number for n in nets]
    # the predictions read sampled losses (iws): every evaluate() of the run gets the same injected noise, stored as `eps`
    eps = torch.randn((nets[0].latent_sampling + 1, 4, kw['latent_dim']), generator=torch.Generator().manual_seed(78))
    eps[0] = 0
    with gen_golden.inject_eps(eps):
        div, y_pred = ref_sample.comparison(x, *nets, batch_size=4)
    torch.manual_seed(3)              # the mean reconstructions do not hang on the draw
    assert torch.equal(ref_sample.comparison(x, *nets, batch_size=4)[0][jobs[0]][jobs[1]], div[jobs[0]][jobs[1]])
    save('comparison', x=x.numpy(), eps=eps.numpy(), jobs=np.array(jobs), div=div[jobs[0]][jobs[1]].numpy(),
         **{f'y_pred.{j}': y_pred[j].numpy() for j in jobs})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds cvae.py)')
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    from oracle import gen_golden
    gen_golden.REF = os.path.abspath(a.reference)
    Net = gen_golden.import_reference()
    import matplotlib
    matplotlib.use('Agg')
    import module.sample as ref_sample
    import utils.inspection as ref_insp
    import ft.inspection as ref_ft
    for m in (ref_sample, ref_insp, ref_ft):
        assert os.path.abspath(m.__file__).startswith(gen_golden.REF), m.__file__
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    parts = {'texts': lambda: texts(ref_insp), 'zsample': lambda: zsample(Net, ref_sample), 'centroids': lambda: centroids(ref_ft),
             'job': lambda: job(Net), 'tables': lambda: tables(ref_insp),
             'comparison': lambda: comparison(Net, ref_sample)}
    for k, f in parts.items():
        if a.only is None or k in a.only:
            f()


if __name__ == '__main__':
    main()
