"""WIMJob on the device: the fused score rows of csrc/wim.hip (ops.wim_scores), the both-prior evaluation in one pass and
ood_detection_rates over ((x, y_est), y) items, against the goldens the REFERENCE's WIMJob wrote (tools/gen_wim_golden.py ->
tests/golden/wim) and the fp64 restatement of tests/test_wim_restatement.py.

Bars: `~` and `~@` rows bit-identical to the reference's; `soft*~` and `k@` rows within 4 x the reference's own fp32 error against
the fp64 formulas (`referr_*`, per family of row); model losses within 1e-4 relative, the bar of the evaluation goldens.

Measured on the MI355X, maximum error of the kernel's rows against fp64 (and the reference's own):
    case            soft~                      @
    C1_N65          0         (0)              4.77e-07 (4.77e-07)
    C2_N64          7.84e-08  (7.84e-08)       3.80e-06 (3.80e-06)
    C10_N257        7.65e-08  (1.42e-07)       3.87e-06 (3.86e-06)
    C100_N63        1.37e-08  (7.96e-08)       3.89e-06 (3.89e-06)
    C128_N1500      2.51e-08  (1.90e-07)       4.02e-06 (3.98e-06)
    C10_N1          1.40e-08  (4.56e-08)       2.72e-06 (2.72e-06)
    model_e2_n8_L3  1.23e-08  (5.62e-08)       1.11e-04 (1.11e-04)"""
import numpy as np
import pytest
import torch

from oracle.cases import WIM_CASES, get_case
from oracle.det_init import det_inputs, det_tensor, load_det_state
from test_wim_restatement import FACTORS, METHODS, SCORE_CASES, check_rows, family, fp64_rows, load_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RTOL = 1e-4
FAMILIES = ['kl', 'zdist', 'iws', 'elbo']
KIND = {'~': 'Y', 'soft~': 'SOFT_Y', '@': 'LSE_AT', '~@': 'Y_AT'}


def rel(a, b, floor=1e-30):
    a = np.asarray(a.detach().double().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().double().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def as_dict(measures):
    return {k: measures[k] for k in measures.keys()}


def device_inputs(inputs):
    return {k: torch.from_numpy(v).to(DEV) for k, v in inputs.items()}


def sources_of(t):
    """The four sources of ops.wim_scores from a dict of losses: elbo is `total` with the factor -1."""
    return [(t['total' if k == 'elbo' else k], -1. if k == 'elbo' else FACTORS[k], t[('total' if k == 'elbo' else k) + '@'])
            for k in FAMILIES]


def specs_of(methods):
    return [(FAMILIES.index(m.replace('soft', '').rstrip('~@')), KIND[family(m)]) for m in methods]


def model_job(shared=True):
    """WIMJob on the geometry of e2_n8_L3 with the weights of the golden's model case (tools/gen_wim_golden.py::det_wim_state)."""
    from jvae_compat.wim import WIMJob
    kw = get_case('e2_n8_L3')['net']
    job = WIMJob(**kw)
    load_det_state(job, seed=0)
    with torch.no_grad():
        for k in ('mean', '_var_parameter'):
            t = getattr(job.encoder.prior, k)
            t.copy_(det_tensor('encoder.prior.' + k, t.shape, 0))
    job.set_alternate_prior(**dict(WIM_CASES['w2_n8']['alternate_prior'], num_priors=1, dim=kw['latent_dim']))
    job.to(DEV)
    job.eval()
    job.WIM_SHARED_PASS = shared
    return job, kw


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('C,N', SCORE_CASES)
def test_wim_scores_match_the_reference_rows(C, N):
    from jvae_hip import ops
    name = f'scores_C{C}_N{N}'
    t = device_inputs(load_case(name)['inputs'])
    M, width, col = 40, N + 11, 3
    rows = [2 * i + 1 for i in range(len(METHODS))][::-1]                            # odd rows, descending
    sentinel = torch.arange(M * width, dtype=torch.float32, device=DEV).view(M, width) * -1.5 - 7.
    buf = sentinel.clone()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.wim_scores(sources_of(t), t['y_est_already'], specs_of(METHODS), out=buf, rows=rows, col=col, status=status)
    assert out is buf and int(status) == 0
    check_rows(name, {m: buf[r, col:col + N].cpu().numpy() for m, r in zip(METHODS, rows)})
    untouched = torch.ones_like(buf, dtype=torch.bool)
    untouched[rows, col:col + N] = False
    assert torch.equal(buf[untouched], sentinel[untouched])
    fresh = ops.wim_scores(sources_of(t), t['y_est_already'], specs_of(METHODS), status=status)
    assert fresh.shape == (len(METHODS), N)
    for i, (m, r) in enumerate(zip(METHODS, rows)):                                  # a second launch: the same bits
        assert fresh[i].cpu().numpy().tobytes() == buf[r, col:col + N].cpu().numpy().tobytes(), m
    ops.wim_check_status(status)


def test_subsets_of_rows_and_sources():
    """One source, rows without an alternate loss, LSE_AT alone (no labels read): each as in the full launch."""
    from jvae_hip import ops
    t = device_inputs(load_case('scores_C10_N257')['inputs'])
    full = ops.wim_scores(sources_of(t), t['y_est_already'], specs_of(METHODS))
    one = ops.wim_scores([(t['zdist'], -.5, None)], t['y_est_already'], [(0, 'SOFT_Y'), (0, 'Y')])
    assert torch.equal(one[0], full[METHODS.index('softzdist~')]) and torch.equal(one[1], full[METHODS.index('zdist~')])
    lse = ops.wim_scores([(t['total'], -1., t['total@'])], t['y_est_already'], [(0, 'LSE_AT')])
    assert torch.equal(lse[0], full[METHODS.index('elbo@')])
    with pytest.raises(ops.L.JvaeHipError):
        ops.wim_scores([(t['zdist'], -.5, None)], t['y_est_already'], [(0, 'Y_AT')])
    with pytest.raises(ops.L.JvaeHipError):
        ops.wim_scores(sources_of(t), t['y_est_already'], specs_of(METHODS[:2]), out=full, rows=[1, 1])
    with pytest.raises(ops.L.JvaeHipError):
        ops.wim_scores(sources_of(t), t['y_est_already'].int(), specs_of(METHODS[:2]))


def test_more_than_128_classes_is_unsupported_and_falls_back():
    from jvae_compat.wim import WIMJob
    from jvae_hip import ops
    rng = np.random.default_rng(3)
    C, N = ops.MISCLASS_MAX_CLASSES + 1, 70
    t = {k: rng.normal(20., 3., (C, N)).astype(np.float32) for k in ('kl', 'zdist', 'iws', 'total')}
    t.update({k + '@': rng.normal(20., 3., N).astype(np.float32) for k in ('kl', 'zdist', 'iws', 'total')})
    t['y_est_already'] = rng.integers(0, C, N)
    d = device_inputs(t)
    with pytest.raises(ops.L.JvaeHipError, match='unsupported'):
        ops.wim_scores(sources_of(d), d['y_est_already'], specs_of(METHODS))
    job = WIMJob(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))
    got = job.batch_dist_measures(None, d, METHODS)
    exact = fp64_rows(t)
    for m in METHODS:
        row = got[m].cpu().numpy()
        assert row.dtype == np.float32 and np.abs(row - exact[m]).max() <= 1e-5 * max(1., np.abs(exact[m]).max()), m
    assert torch.equal(got['kl~'], -d['kl'].gather(0, d['y_est_already'][None])[0])


def test_label_outside_the_classes_gives_nan_and_raises():
    from jvae_hip import ops
    c = load_case('scores_C10_N257')
    t = device_inputs(c['inputs'])
    y = t['y_est_already'].clone()
    bad = [0, 64, 200, 256]
    y[bad[0]], y[bad[1]], y[bad[2]], y[bad[3]] = 10, -1, 1 << 40, -(1 << 33)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.wim_scores(sources_of(t), y, specs_of(METHODS), status=status).cpu()
    good = torch.ones(257, dtype=torch.bool)
    good[bad] = False
    for m, row in zip(METHODS, out):
        ref = torch.from_numpy(c['rows'][m])
        if family(m) == '@':                                     # no label in it
            assert not row.isnan().any()
        else:
            assert row[bad].isnan().all() and not row[good].isnan().any(), m
        if family(m) in ('~', '~@'):
            assert torch.equal(row[good], ref[good]), m
    assert int(status) == 1
    with pytest.raises(ops.L.JvaeHipError, match='label'):
        ops.wim_check_status(status)
    assert int(status) == 0                                      # read and cleared
    ops.wim_check_status(status)


# ---------------------------------------------------------------------------------------------- 2. the model
@pytest.fixture(scope='module')
def model_run():
    """One both-prior evaluation of the golden's model, shared pass: (job, x, y_est, eps, output)."""
    g = load_case('model_e2_n8_L3')
    job, kw = model_job()
    x, _, eps = det_inputs(8, kw['input_shape'], kw['num_labels'], int(g['raw']['L']), kw['latent_dim'])
    x, eps = x.to(DEV), eps.to(DEV)
    y_est = torch.from_numpy(g['inputs']['y_est_already']).to(DEV)
    with torch.no_grad(), job.evaluate_on_both_priors():
        out = job.evaluate((x, y_est), epsilon=eps)
    return job, x, y_est, eps, out


def test_both_prior_evaluation_matches_the_reference(model_run):
    job, x, y_est, eps, out = model_run
    g = load_case('model_e2_n8_L3')['raw']
    losses = out[2]
    assert job.latent_sampling == int(g['L']) and job.is_original_prior and job.num_labels == 10
    assert losses['y_est_already'] is y_est
    for f in g.files:
        if f.startswith('orig.') or f.startswith('alt.'):
            k = f.split('.', 1)[1] + ('@' if f.startswith('alt.') else '')
            assert tuple(losses[k].shape) == g[f].shape, k
            assert rel(losses[k], g[f]) < RTOL, (k, rel(losses[k], g[f]))
    assert {k for k in losses if k.endswith('@')} == {f[4:] + '@' for f in g.files if f.startswith('alt.')} | {'y_est_already@'}
    assert 'dzdist@' not in losses and losses['kl@'].shape == (8,) and losses['kl'].shape == (10, 8)


def test_model_rows(model_run):
    """The kernel through batch_dist_measures: on the golden's own losses to the bars of the score cases; on this model's losses
    against the reference's rows within the 1e-4 of the two losses a row is made of."""
    job, x, y_est, eps, out = model_run
    c = load_case('model_e2_n8_L3')
    t = device_inputs(c['inputs'])
    before = set(t)
    got = job.batch_dist_measures(None, t, METHODS)
    assert set(t) == before
    check_rows('model_e2_n8_L3', {m: v.cpu().numpy() for m, v in got.items()})
    mine = job.batch_dist_measures(out[1], out[2], METHODS)
    for m in METHODS:
        if family(m) == 'soft~':
            continue                                   # a softmax of losses near 3000: 1e-4 of them moves it by O(1)
        k = m.replace('soft', '').rstrip('~@')
        key = 'total' if k == 'elbo' else k
        scale = abs(FACTORS[k]) * max(np.abs(c['inputs'][key]).max(), np.abs(c['inputs'][key + '@']).max())
        err = np.abs(mine[m].cpu().numpy().astype(np.float64) - c['rows'][m]).max()
        assert err <= 2 * RTOL * scale, (m, err, scale)
    assert job._wim_status is not None and int(job._wim_status) == 0


def test_shared_pass_and_two_passes_give_the_same_bits(model_run):
    job, x, y_est, eps, shared = model_run
    two, _ = model_job(shared=False)
    with torch.no_grad(), two.evaluate_on_both_priors():
        other = two.evaluate((x, y_est), epsilon=eps, z_output=True)
    assert set(other[2]) == set(shared[2])
    for k, v in shared[2].items():
        assert torch.equal(v, other[2][k]), k
    assert torch.equal(shared[0], other[0]) and torch.equal(shared[1], other[1])
    assert as_dict(shared[3]) == as_dict(other[3]) and len(other) == 7
    with torch.no_grad(), job.no_estimated_labels():             # outside the context: the base class's evaluate
        plain = job.evaluate(x, epsilon=eps)
    assert not any(k.endswith('@') for k in plain[2]) and 'y_est_already' not in plain[2]
    for k, v in plain[2].items():
        assert torch.equal(v, shared[2][k]), k


def test_base_model_evaluation_is_unchanged_by_the_split(golden_dir):
    """evaluate(x) of the base class on e2_n8_L3: the values the evaluation golden pins, and the same bits from two calls."""
    import os
    from cvae import ClassificationVariationalNetwork as Net
    g = np.load(os.path.join(golden_dir, 'e2_n8_L3.npz'))
    case = get_case('e2_n8_L3')
    kw = case['net']
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(DEV)
    net.eval()
    x, _, eps = det_inputs(case['N'], kw['input_shape'], kw['num_labels'], int(g['L']), kw['latent_dim'])
    a = net.evaluate(x.to(DEV), epsilon=eps.to(DEV))
    b = net.evaluate(x.to(DEV), epsilon=eps.to(DEV))
    keys = [f[5:] for f in g.files if f.startswith('loss.')]
    assert list(a[2]) == ['kl', 'zdist', 'var_kl', 'dzdist', 'wmse', 'cross_x', 'total', 'iws'] and set(keys) == set(a[2])
    for k in keys:
        assert tuple(a[2][k].shape) == g['loss.' + k].shape and rel(a[2][k], g['loss.' + k]) < RTOL, k
        assert torch.equal(a[2][k], b[2][k]), k
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and as_dict(a[3]) == as_dict(b[3])
    for k in [f[8:] for f in g.files if f.startswith('measure.')]:
        ref = float(g['measure.' + k])
        assert abs(a[3][k] - ref) <= 2e-4 * max(1.0, abs(ref)), k


def test_finetune_batch_is_the_hand_driven_step():
    """finetune_batch against the sequence tests/test_2_model_gpu.py drives by hand (two evaluations, the prior swapped by
    assignment), on a twin model whose BatchNorm layers are put in eval mode as WIMJob.train() keeps them."""
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.wim import WIMJob
    from module.priors import build_prior
    case = get_case('w2_n8')
    kw, N, K = case['net'], case['N'], case['net']['latent_dim']
    job = WIMJob(**kw, alternate_prior=dict(case['alternate_prior'], num_priors=1, dim=K))
    twin = Net(**kw)
    for net in (job, twin):
        load_det_state(net, seed=0)
        net.to(DEV)
    with torch.no_grad():
        for k in ('mean', '_var_parameter'):
            getattr(job.encoder.prior, k).copy_(getattr(twin.encoder.prior, k))
            getattr(job._alternate_prior, k).copy_(build_prior(dim=K, num_priors=1, **case['alternate_prior']).to(DEV).state_dict()[k])
    x_in, y_in, _ = det_inputs(N, kw['input_shape'], kw['num_labels'], 1, K, seed=1234)
    x_mix, _, _ = det_inputs(N, kw['input_shape'], kw['num_labels'], 1, K, seed=777)
    x_in, y_in, x_mix = x_in.to(DEV), y_in.to(DEV), x_mix.to(DEV)
    job.optimizer.zero_grad()
    torch.manual_seed(11)
    L, in_loss, mix_loss = job.finetune_batch(0, 0, x_in, y_in, x_mix, alpha=case['alpha'])
    assert job.is_alternate_prior and job._evaluate_on_both_priors and job.training
    twin.train()
    for m in twin.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    torch.manual_seed(11)
    _, _, a, _ = twin.evaluate(x_in, y_in, batch=0, with_beta=True)
    original = twin.encoder.prior
    twin.encoder.prior, twin.num_labels = job._alternate_prior, 1
    _, _, b, _ = twin.evaluate(x_mix, torch.zeros(N, dtype=torch.int64, device=DEV), batch=0, with_beta=True)
    twin.encoder.prior, twin.num_labels = original, kw['num_labels']
    want = a['total'].mean() + case['alpha'] * b['total'].mean()
    assert set(in_loss) == set(a) and set(mix_loss) == set(b) and 'dzdist' not in mix_loss
    for k in a:
        assert torch.equal(in_loss[k], a[k]), k
    for k in b:
        assert torch.equal(mix_loss[k], b[k]), k
    assert torch.equal(L, want)
    L.backward()
    assert job.encoder.dense_mean.weight.grad is not None and job._original_prior.mean.grad is None


# ---------------------------------------------------------------------------------------------- 3. ood_detection_rates
class _Images(torch.utils.data.Dataset):
    def __init__(self, n, seed, name, shift=0.):
        g = torch.Generator().manual_seed(seed)
        self.x = (torch.rand((n, 3, 32, 32), generator=g) * (1 - shift) + shift * torch.rand((n, 3, 1, 1), generator=g)).contiguous()
        self.y = torch.randint(0, 10, (n,), generator=g)
        self.name = name

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


def test_ood_detection_rates_over_estimated_label_items():
    from jvae_compat.wim import EstimatedLabelsDataset
    from jvae_hip import ops
    job, kw = model_job()
    g = torch.Generator().manual_seed(9)
    sets = [EstimatedLabelsDataset(_Images(96, 1, 'in'), torch.randint(0, 10, (96,), generator=g)),
            EstimatedLabelsDataset(_Images(64, 2, 'out', shift=.6), torch.randint(0, 10, (64,), generator=g))]
    torch.manual_seed(5)
    res = job.ood_detection_rates(oodsets=[sets[1]], testset=sets[0], batch_size=32)
    assert set(res) == {'out'} and list(res['out']) == job.ood_methods and len(job.ood_methods) == 8
    for m, r in res['out'].items():
        assert r['n'] == 64 and 0. <= r['auc'] <= 1. and len(r['fpr']) == len(job.OOD_KEPT_TPR), m
    assert job.is_original_prior and not job._evaluate_on_both_priors
    torch.manual_seed(5)                                         # the same epsilon draws, batch by batch
    rows = []
    with torch.no_grad():
        for s in sets:
            got = []
            for (x, y_est), _ in torch.utils.data.DataLoader(s, batch_size=32):
                with job.evaluate_on_both_priors():
                    _, logits, losses, _ = job.evaluate((x.to(DEV), y_est.to(DEV)))
                got.append(job.batch_dist_measures(logits, losses, ['zdist~@', 'elbo@'])['zdist~@'])
            rows.append(torch.cat(got))
    r = ops.roc_curve(rows[0], rows[1], job.OOD_KEPT_TPR)
    assert float(r['auc']) == res['out']['zdist~@']['auc']
    assert [float(f) for f in r['fpr']] == res['out']['zdist~@']['fpr']
    with job.no_estimated_labels():                              # plain (x, y) items: the base class's pass and names
        plain = job.ood_detection_rates(oodsets=[sets[1].dataset], testset=sets[0].dataset, batch_size=32, update_self_ood=False)
    assert list(plain['out']) == ['zdist', 'elbo']
