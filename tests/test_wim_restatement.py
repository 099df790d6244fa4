"""WIMJob on the host (jvae_compat/wim.py; no GPU): the torch expressions `batch_dist_measures` keeps as its fallback reproduce the
rows the REFERENCE's WIMJob wrote (tools/gen_wim_golden.py -> tests/golden/wim), and the host logic of the two priors.

`~` and `~@` rows (a gather, one fp32 subtraction of exact products) are compared bit for bit; `soft*~` and `k@` rows within
4 x the reference's own fp32 error against the fp64 formulas, per family of row (`referr_*` of the golden; the factor
tests/test_7_mdr_gpu.py uses)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle.cases import WIM_CASES, get_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wim')
SCORE_CASES = [(1, 65), (2, 64), (10, 257), (100, 63), (128, 1500), (10, 1)]
NAMES = [f'scores_C{C}_N{N}' for C, N in SCORE_CASES] + ['model_e2_n8_L3']
FACTORS = {'kl': -1., 'zdist': -.5, 'iws': 1., 'elbo': 1.}
METHODS = [k + s for k in FACTORS for s in ('~', '@', '~@')] + ['soft' + k + '~' for k in FACTORS]
EXACT_FAMILIES = ('~', '~@')
MAX_SPREAD = 80.
_cache = {}


def family(m):
    if m.endswith('~@'):
        return '~@'
    if m.endswith('@'):
        return '@'
    return 'soft~' if m.startswith('soft') else '~'


def load_case(name):
    """-> dict: 'inputs' {loss name: numpy}, 'rows' {method: fp32 row}, 'referr' {family: float}, 'raw' the npz.  Read once."""
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        _cache[name] = {'inputs': {f[3:]: g[f] for f in g.files if f.startswith('in.')},
                        'rows': {f[4:]: g[f] for f in g.files if f.startswith('row.')},
                        'referr': dict(zip((str(n) for n in g['referr_names']), (float(v) for v in g['referr_values']))),
                        'route': str(g['route']), 'raw': g}
    return _cache[name]


def fp64_rows(inputs):
    """The table of ft/wim.py:171-192 in fp64 numpy on the fp32 inputs -> {method: (N,) fp64}."""
    y = inputs['y_est_already']
    n = np.arange(y.shape[0])
    out = {}
    for k, f in FACTORS.items():
        sign = -1. if k == 'elbo' else 1.
        x = f * sign * inputs['total' if k == 'elbo' else k].astype(np.float64)
        fa = f * sign * inputs[('total' if k == 'elbo' else k) + '@'].astype(np.float64)
        top = x.max(0)
        e = np.exp(x - top)
        out[k + '~'] = x[y, n]
        out['soft' + k + '~'] = (e / e.sum(0))[y, n]
        out[k + '@'] = np.log(e.sum(0)) + top - fa
        out[k + '~@'] = x[y, n] - fa
    return out


def check_rows(name, got, exact_too=True):
    """got {method: fp32 numpy row} against the golden of `name`: bits for the exact families, 4 x referr (against fp64) else.
    -> {family: worst error against fp64}."""
    c = load_case(name)
    exact = fp64_rows(c['inputs'])
    worst = {}
    for m in METHODS:
        row = np.asarray(got[m])
        assert row.dtype == np.float32 and row.shape == c['rows'][m].shape, m
        fam = family(m)
        if fam in EXACT_FAMILIES:
            assert row.tobytes() == c['rows'][m].tobytes(), (name, m)
        worst[fam] = max(worst.get(fam, 0.), float(np.abs(row.astype(np.float64) - exact[m]).max()))
    for fam in ('soft~', '@'):
        print(name, fam, 'error against fp64', worst[fam], 'reference error', c['referr'][fam])
        assert worst[fam] <= 4 * c['referr'][fam], (name, fam, worst[fam], c['referr'][fam])
    return worst


def tiny_job(**kw):
    from jvae_compat.wim import WIMJob
    net = dict(get_case('c1_n16_mlp')['net'], gamma=0.)
    alt = dict(WIM_CASES['w2_n8']['alternate_prior'], num_priors=1, dim=net['latent_dim'])
    return WIMJob(**net, alternate_prior=alt, **kw)


@pytest.mark.parametrize('name', NAMES)
def test_golden_input_conditions(name):
    c = load_case(name)
    t = c['inputs']
    C = t['kl'].shape[0]
    assert c['route'] == 'reference' and set(c['rows']) == set(METHODS) and set(c['referr']) == {'~', '~@', 'soft~', '@'}
    assert t['y_est_already'].dtype == np.int64 and ((0 <= t['y_est_already']) & (t['y_est_already'] < C)).all()
    for k in ('kl', 'zdist', 'iws', 'total'):
        assert t[k].dtype == np.float32 and t[k + '@'].shape == t[k].shape[1:]
        spread = np.abs(FACTORS.get(k, 1.)) * (t[k].astype(np.float64).max(0) - t[k].astype(np.float64).min(0))
        assert spread.max() < MAX_SPREAD, (k, spread.max())
    assert c['referr']['~'] == 0                        # a gather of an exact product
    if name.startswith('scores'):
        assert (C, t['kl'].shape[1]) in SCORE_CASES


@pytest.mark.parametrize('name', NAMES)
def test_fallback_expressions_reproduce_the_reference_rows(name):
    job = tiny_job()
    c = load_case(name)
    losses = {k: torch.from_numpy(v) for k, v in c['inputs'].items()}
    before = set(losses)
    got = job.batch_dist_measures(None, losses, METHODS)
    assert set(losses) == before                        # no elbo / elbo@ keys left behind
    assert list(got) == METHODS
    check_rows(name, {m: v.numpy() for m, v in got.items()})
    buf = torch.full((20, c['inputs']['kl'].shape[1] + 5), 7.)
    rows = list(range(19, 3, -1))
    into = job.batch_dist_measures(None, losses, METHODS, out=buf, rows=rows, col=2)
    for m, r in zip(METHODS, rows):
        assert torch.equal(into[m], got[m]) and torch.equal(buf[r, 2:-3], got[m]), m
    assert bool((buf[:4] == 7).all() and (buf[:, :2] == 7).all() and (buf[:, -3:] == 7).all())


def test_method_names_and_tables():
    from jvae_compat.wim import WIMJob
    job = tiny_job()
    from module import score_rows

    def wim_row(m):                                         # elbo reads `total`; the factor is the family's (ft/wim.py:145)
        row = score_rows.parse(m, score_rows.traits_of(job))
        return row.source, row.kind, row.const
    assert wim_row('zdist~') == ('zdist', 'Y', -.5) and wim_row('softkl~') == ('kl', 'SOFT_Y', -1.)
    assert wim_row('elbo@') == ('total', 'LSE_AT', 1.) and wim_row('iws~@') == ('iws', 'Y_AT', 1.)
    with pytest.raises(NotImplementedError):
        wim_row('mse~')
    assert job.ood_methods == ['zdist', 'zdist~', 'zdist@', 'zdist~@', 'elbo', 'elbo~', 'elbo@', 'elbo~@']
    assert job.misclass_methods == ['softzdist~', 'zdist~'] and job.predict_methods == ['already']
    base = type(job).__mro__[1].loss_components_per_type['cvae']
    assert job.loss_components == base + tuple(k + '@' for k in base) + ('y_est_already',)
    with job.no_estimated_labels():
        assert job.ood_methods == ['zdist', 'elbo'] and not job._with_estimated_labels
    assert job.ood_methods[1] == 'zdist~' and job._with_estimated_labels
    y = torch.tensor([3, 1])
    assert job.predict_after_evaluate(None, {'y_est_already': y}, method='already') is y


def test_prior_swap_restores_after_an_exception():
    job = tiny_job()
    original, alternate = job.encoder.prior, job._alternate_prior
    assert job.is_original_prior and original.conditional and not alternate.conditional
    assert not any(p.requires_grad for p in original.parameters()) and not any(p.requires_grad for p in alternate.parameters())
    with pytest.raises(RuntimeError, match='inside'):
        with job.alternate_prior as p:
            assert p is alternate and job.encoder.prior is alternate and job.num_labels == 1 and job.is_alternate_prior
            with job.original_prior as q:
                assert q is original and job.num_labels == 10
            assert job.encoder.prior is alternate and job.num_labels == 1
            raise RuntimeError('inside')
    assert job.encoder.prior is original and job.num_labels == 10 and job.is_original_prior
    job.alternate_prior = True
    assert job.encoder.prior is alternate and job.num_labels == 1
    with pytest.raises(RuntimeError):
        with job.original_prior:
            raise RuntimeError('inside')
    assert job.encoder.prior is alternate and job.is_alternate_prior
    job.original_prior = True
    assert job.encoder.prior is original and job.num_labels == 10
    with pytest.raises(RuntimeError):
        with job.evaluate_on_both_priors():
            assert job._evaluate_on_both_priors
            raise RuntimeError('inside')
    assert not job._evaluate_on_both_priors
    from jvae_compat.wim import WIMJob
    bare = WIMJob(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))
    with pytest.raises(AttributeError):
        bare.alternate_prior = True


def test_train_keeps_batchnorm_in_eval_mode():
    from jvae_compat.wim import WIMJob
    job = WIMJob(**get_case('w2_n8')['net'])
    job.train()
    bns = [m for m in job.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert bns and job.training and not any(m.training for m in bns) and job.encoder.training
    job.eval()
    assert not job.training


def test_save_and_load_of_a_wim_directory_and_of_a_plain_one(tmp_path):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.wim import WIMJob
    job = tiny_job()
    job.trained = 2
    job.ft_params.update(sets=['a', 'b'], alpha=.1, train_size=100, moving_size=10, padding=0., mix_padding=0., padding_sets=[],
                         mix=.5, hash=123, array_size=4)
    job.ft_params['from'] = 7
    job.alternate_prior = True
    d = job.save(str(tmp_path / 'wim'))                     # except_state defaults to True, never an optimiser
    assert job.is_alternate_prior                           # saved under the original prior, the state in place is restored
    assert set(os.listdir(d)) == {'params.json', 'train_params.json', 'test.json', 'ood.json', 'history.json', 'wim.json'}
    assert json.load(open(os.path.join(d, 'params.json')))['prior']['num_priors'] == 10
    assert WIMJob.is_wim(d) and json.load(open(os.path.join(d, 'wim.json')))['mean_shift'] == 1.5
    d = job.save(str(tmp_path / 'wim'), except_state=False)
    assert 'state.pth' in os.listdir(d) and 'optimizer.pth' not in os.listdir(d)
    again = WIMJob.load(d)
    assert again.ft_params == json.load(open(os.path.join(d, 'wim.json')))       # the data-set keys stay in ft_params ...
    assert again._alternate_prior is not None and again._alternate_prior.num_priors == 1   # ... and never reach build_prior
    assert float(again._alternate_prior.mean.mean()) == 1.5 and again.is_original_prior
    for (k, v), (k2, v2) in zip(job.state_dict().items(), again.state_dict().items()):
        if not k.startswith('encoder.prior.'):               # `job` is left under its alternate prior
            assert k == k2 and torch.equal(v, v2), k
    assert torch.equal(again.encoder.prior.mean, job._original_prior.mean)
    lazy = WIMJob.load(d, build_module=False)
    assert lazy.ft_params['alpha'] == .1 and lazy._alternate_prior is None
    plain = Net(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))
    plain.trained, plain.ood_results = 1, {1: {'set': {}}}
    p = plain.save(str(tmp_path / 'plain'))
    state = torch.load(os.path.join(p, 'state.pth'))
    assert '_original_prior.mean' not in state and not WIMJob.is_wim(p)
    WIMJob.transfer_from_model(state)
    assert torch.equal(state['_original_prior.mean'], state['encoder.prior.mean'])
    assert torch.equal(state['_original_prior._var_parameter'], state['encoder.prior._var_parameter'])
    moved = WIMJob.load(p)
    assert moved.ood_results == {} and moved._alternate_prior is None and not hasattr(moved, 'ft_params')
    assert torch.equal(moved._original_prior.mean, plain.encoder.prior.mean)
    assert torch.equal(moved.encoder.dense_mean.weight, plain.encoder.dense_mean.weight)


def test_estimated_labels_dataset_items():
    from jvae_compat.wim import EstimatedLabelsDataset
    base = torch.utils.data.TensorDataset(torch.arange(12.).view(6, 2), torch.arange(6))
    base.name = 'six'
    ds = EstimatedLabelsDataset(base, [5, 4, 3, 2, 1, 0])
    assert len(ds) == 6 and ds.name == 'six'
    (x, y_est), y = ds[2]
    assert x.tolist() == [4., 5.] and int(y_est) == 3 and int(y) == 2
    (xb, yb_est), yb = next(iter(torch.utils.data.DataLoader(ds, batch_size=4)))
    assert xb.shape == (4, 2) and yb_est.tolist() == [5, 4, 3, 2] and yb_est.dtype == torch.int64 and yb.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        EstimatedLabelsDataset(base, [0])
