"""Semi-supervised training on the device: csrc/semisup.hip through ops.class_marginal_kl against the fp64 restatement and the derived
bounds of tests/semi_cases.py (every output of every case and label pattern, |error| <= 2^-24 B), then the model: SEMI_SUPERVISED
with and without unlabelled rows, class_marginal(), train_model over HiddenLabels.

Common to every kernel call: each fp32 result the op allocates lies inside a NaN-filled buffer with a guard band of 64 floats on
either side (test_38's `Guarded`, restated), the guards must be intact and every element written; each call runs twice and must
give the same bits; the measured error over the bound is printed before it is held.

Model level, gradients: the gradients of the prior means and of the encoder's two head weights under the HIP op are compared with a
second backward in which the op is replaced by the same objective as a torch expression (semi_cases.classes / marginal on the
device) in fp32 and in fp64.  Per parameter, e = max|torch32 - torch64| is the error of the torch fp32 expression, and the HIP op is
allowed 4 e, for its distance to either.  The ratios are printed; DESIGN.md section 7x records them."""
import contextlib
import math

import numpy as np
import pytest
import torch

import semi_cases as sc
from jvae_hip import lib, ops
from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
F64 = torch.float64
_cache = {}


def ref64(c, pattern):
    if (c.name, pattern) not in _cache:
        d = sc.make(c, pattern)
        r = sc.ref(c, d)
        _cache[c.name, pattern] = (d, r, sc.bounds(c, d, r))
    return _cache[c.name, pattern]


class Guarded:
    """Stands in for the `torch` of jvae_hip.ops: fp32 results are carved out of NaN-filled buffers with guard bands."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, k):
        return getattr(torch, k)

    def _alloc(self, shape, dtype, device):
        shape = tuple(int(s) for s in shape)
        if dtype not in (None, torch.float32):
            return torch.empty(shape, dtype=dtype, device=device)
        n = math.prod(shape)
        buf = torch.full((n + 2 * GUARD,), math.nan, device=device)
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def empty(self, *size, device=None, dtype=None):
        return self._alloc(size[0] if len(size) == 1 and not isinstance(size[0], int) else size, dtype, device)

    def empty_like(self, t):
        return self._alloc(t.shape, t.dtype, t.device)

    def check(self):
        for buf, n in self.bufs:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'a guard band was written'
            assert not bool(torch.isnan(buf[GUARD:GUARD + n]).any()), 'a result element was not written'
        return len(self.bufs)


@contextlib.contextmanager
def guarded(least):
    g = Guarded()
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = torch
    assert g.check() >= least


def bits(t):
    return t.contiguous().view(torch.int32)


def twice(f):
    a, b = f(), f()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f'two runs differ in {k}'
    return a


def run_case(c, d, class_grads=True):
    """Forward and backward of one case through ops.class_marginal_kl -> every output."""
    t = {k: (v.to(DEV) if v is not None else None) for k, v in d.items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in ('mu', 'lv', 'kl_in')}
    means = t['means'].clone().requires_grad_(class_grads)
    T = t['T'].clone().requires_grad_(class_grads and c.var == 'diag')
    with guarded(7 + (class_grads + (class_grads and c.var == 'diag') if c.N else 0)):    # kl, zdist, var_kl, r, g_kl_in, g_mu, g_lv
        kl, zd, vkl, r = ops.class_marginal_kl(leaves['mu'], leaves['lv'], t['y'], means, T, leaves['kl_in'], t['zd_in'], t['vkl_in'],
                                               log_pi=t['log_pi'], w=c.w, var_dim=c.var)
        assert kl.requires_grad and not zd.requires_grad and not vkl.requires_grad and not r.requires_grad
        torch.autograd.backward(kl, grad_tensors=t['g'])
    out = dict(kl=kl.detach(), zdist=zd, var_kl=vkl, r=r, g_mu=leaves['mu'].grad, g_lv=leaves['lv'].grad, g_kl_in=leaves['kl_in'].grad)
    if class_grads:
        out['g_means'] = means.grad
        if c.var == 'diag':
            out['g_T'] = T.grad
    else:
        assert means.grad is None and T.grad is None
    return out


def hold(name, got, r, B, keys=None):
    ex = {k: sc.excess(got[k], r[k], B[k]) for k in (keys or B)}
    print(name, 'measured / bound:', {k: round(v, 4) for k, v in ex.items()})
    assert all(v <= 1 for v in ex.values()), (name, ex)
    return ex


def check_rows(c, d, got):
    """What holds bit for bit: a labelled row is its input, its r row is one-hot, g goes straight back to its incoming kl."""
    y = d['y']
    lab = (y >= 0).to(DEV)
    for out, src in (('kl', 'kl_in'), ('zdist', 'zd_in'), ('var_kl', 'vkl_in')):
        assert torch.equal(bits(got[out][lab]), bits(d[src].to(DEV)[lab])), out
    onehot = (y.view(-1, 1) == torch.arange(c.C).view(1, -1)).float().to(DEV)
    assert torch.equal(got['r'][lab], onehot[lab])
    assert torch.equal(bits(got['g_kl_in'][lab]), bits(d['g'].to(DEV)[lab])) and not bool(got['g_kl_in'][~lab].any())
    assert not bool(got['g_mu'][lab].any()) and not bool(got['g_lv'][lab].any())
    rows = got['r'][~lab].double().sum(1)
    assert rows.numel() == 0 or float((rows - 1).abs().max()) <= 8 * sc.U


# ============================================================================================ kernels against the restatement
@pytest.mark.parametrize('pattern', sc.PATTERNS)
@pytest.mark.parametrize('c', sc.SHAPE_CASES, ids=sc.ids)
def test_kernels_against_the_restatement(c, pattern):
    d, r, B = ref64(c, pattern)
    got = twice(lambda: run_case(c, d))
    assert set(got) == set(B)
    check_rows(c, d, got)
    hold(c.name + '/' + pattern, got, r, B)
    bare = twice(lambda: run_case(c, d, class_grads=False))                       # the class gradients only when asked for
    for k in bare:
        assert torch.equal(bits(bare[k]), bits(got[k])), k


@pytest.mark.parametrize('pattern', sc.PATTERNS)
@pytest.mark.parametrize('c', sc.STRESS_CASES, ids=sc.ids)
def test_stress_rows(c, pattern):
    d, r, B = ref64(c, pattern)
    got = twice(lambda: run_case(c, d))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    check_rows(c, d, got)
    hold(c.name + '/' + pattern, got, r, B)
    unl = (d['y'] < 0).to(DEV)
    if c.stress == 'spread':                                                      # exactly one-hot
        ru = got['r'][unl]
        assert bool(((ru == 0) | (ru == 1)).all()) and torch.equal(ru.sum(1), torch.ones_like(ru[:, 0]))
    if c.stress == 'empty':
        assert not bool(got['r'][:, 2].any()) and not bool(got['g_means'][2].any()) and not bool(got['g_T'][2].any())
    if c.stress == 'equal' and bool(unl.any()):
        assert float((got['r'][unl] - 1 / c.C).abs().max()) <= sc.U / c.C


def test_empty_batch():
    c = sc._c('empty', 0, 3, 5, var='diag')
    got = run_case(c, sc.make(c))
    assert got['kl'].shape == (0,) and got['r'].shape == (0, 3) and got['g_mu'].shape == (0, 5)
    assert not bool(got['g_means'].any()) and not bool(got['g_T'].any())


def test_a_label_past_the_last_class_is_never_an_index():
    """Such a row is a labelled row: it passes through with its bits as in the plain step, belongs to no class, and the rows
    around it are what they are without it."""
    c = sc.SHAPE_CASES[1]
    d, r, B = ref64(c, 'half')
    d = dict(d, y=d['y'].clone())
    lab = (d['y'] >= 0).nonzero().flatten()
    d['y'][lab[:3]] = torch.tensor([c.C, c.C + 5, 1 << 40])
    got = twice(lambda: run_case(c, d))
    r2 = sc.ref(c, d)
    assert not bool(got['r'][lab[:3].to(DEV)].any())
    for out, src in (('kl', 'kl_in'), ('zdist', 'zd_in'), ('var_kl', 'vkl_in')):
        assert torch.equal(bits(got[out][lab[:3].to(DEV)]), bits(d[src][lab[:3]].to(DEV)))
    hold('label >= C', got, r2, sc.bounds(c, d, r2))


# ============================================================================================ the model
N_MODEL = 16


def build(name, semi=None, seed=0, **kw):
    from cvae import ClassificationVariationalNetwork as Net
    case = get_case(name)
    cfg = dict(case['net'], **kw)
    net = Net(**cfg)
    load_det_state(net, seed=seed)
    net.to(DEV)
    net.train()
    if semi is not None:
        net.SEMI_SUPERVISED = semi
    x, y, eps = det_inputs(N_MODEL, cfg['input_shape'], cfg['num_labels'], cfg['latent_sampling'], cfg['latent_dim'], seed=42)
    return net, x.to(DEV), y.to(DEV), eps.to(DEV)


def half_hidden(y):
    y = y.clone()
    y[::2] = -1
    return y


def grads_of(net, total):
    for p in net.parameters():
        p.grad = None
    total.mean().backward()
    lib.join_side_stream()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def params_of(net):
    return {k: p.detach().clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize('name', ['c2_n8', 'c3_n8_diag'])
def test_switch_on_without_unlabelled_rows_is_the_plain_step_bit_for_bit(name):
    runs = {}
    for semi in (False, True):
        net, x, y, eps = build(name, semi=semi)
        losses = net.evaluate(x, y, with_beta=True, epsilon=eps)[2]
        rows = {k: v.detach().clone() for k, v in losses.items()}
        grads = grads_of(net, losses['total'])
        net2, x, y, eps = build(name, semi=semi)
        net2.train_step(x, y, epsilon=eps)
        torch.cuda.synchronize()
        runs[semi] = (rows, grads, params_of(net2))
    for part_off, part_on in zip(runs[False], runs[True]):
        assert set(part_off) == set(part_on)
        for k in part_off:
            assert torch.equal(part_off[k], part_on[k]), k
    assert any(not torch.equal(runs[True][2][k], p.detach()) for k, p in build(name)[0].named_parameters())      # the step moved them


@contextlib.contextmanager
def op_replaced_by_torch(dt):
    """ops.class_marginal_kl as a torch expression in `dt` (the model looks the op up in the module at every call)."""
    real = ops.class_marginal_kl

    def expression(mu, log_var, y, means, T, kl, zdist, var_kl, log_pi=None, w=1., var_dim='scalar'):
        c = sc._c('model', mu.shape[0], means.shape[0], mu.shape[1], var=var_dim, w=w)
        d = dict(mu=mu, lv=log_var, means=means, T=T, log_pi=log_pi)
        cl = sc.classes(c, d, dt, leaves=dict(mu=mu.to(dt), lv=log_var.to(dt), means=means.to(dt), T=T.to(dt)))
        U_, r, _ = sc.marginal(cl)
        unl = y < 0
        return (torch.where(unl, U_.to(torch.float32), kl), torch.where(unl, (r * cl['dist']).sum(1).float().detach(), zdist),
                torch.where(unl, (r * cl['v']).sum(1).float().detach(), var_kl), r.float().detach())
    ops.class_marginal_kl = expression
    try:
        yield
    finally:
        ops.class_marginal_kl = real


def restate(net, y, mu, log_var, w=1.):
    pr = net.encoder.prior
    N, K = mu.shape
    c = sc._c('model', N, pr.mean.shape[0], K, var=pr.var_dim, w=w, pi=net.UNLABELLED_CLASS_WEIGHTS is not None)
    log_pi = net._semi_log_pi(pr.mean.shape[0], 'cpu')
    zero = torch.zeros(N)
    d = dict(mu=mu.detach().cpu(), lv=log_var.detach().cpu(), y=y.cpu(), means=pr.mean.detach().cpu(), T=pr._var_parameter.detach().cpu(),
             log_pi=log_pi, g=torch.ones(N), kl_in=zero, zd_in=zero, vkl_in=zero)
    r = sc.ref(c, d)
    return c, d, r, sc.bounds(c, d, r)


@pytest.mark.parametrize('name,w,weights', [('c2_n8', 1., None), ('c3_n8_diag', 0.5, 'ramp')], ids=['c2', 'c3_diag_w05_pi'])
def test_half_the_labels_hidden(name, w, weights):
    plain, x, y, eps = build(name, semi=True)
    base = plain.evaluate(x, y, with_beta=True, epsilon=eps, kl_var_weighting=w)[2]
    base = {k: v.detach().clone() for k, v in base.items()}
    net, x, y, eps = build(name, semi=True)
    C = net.encoder.prior.mean.shape[0]
    if weights:
        net.UNLABELLED_CLASS_WEIGHTS = [1. + k % 7 for k in range(C)]
    yh = half_hidden(y)
    unl = yh < 0
    _, _, losses, measures, mu, log_var, _ = net.evaluate(x, yh, with_beta=True, epsilon=eps, kl_var_weighting=w, z_output=True)
    # (b) the reconstruction rows of every sample and the KL rows of the labelled ones are those of the fully labelled batch
    for k in ('wmse', 'cross_x'):
        assert torch.equal(losses[k], base[k]), k
    for k in ('kl', 'zdist', 'var_kl'):
        assert torch.equal(losses[k][~unl], base[k][~unl]), k
    c, d, r, B = restate(net, yh, mu, log_var, w)
    got = {k: losses[k2].detach() for k, k2 in (('kl', 'kl'), ('zdist', 'zdist'), ('var_kl', 'var_kl'))}
    sel = unl.cpu()
    ex = {k: sc.excess(got[k][unl], r[k][sel], B[k][sel]) for k in got}
    print(name, 'unlabelled rows, measured / bound:', {k: round(v, 4) for k, v in ex.items()})
    assert all(v <= 1 for v in ex.values()), ex
    assert torch.equal(losses['total'][unl], (losses['cross_x'] + net.beta * losses['kl'])[unl]) or net.y_is_decoded
    assert all(np.isfinite(float(v)) for v in measures.copy().values())
    # (c) the gradients of the dictionary and of the encoder's heads against the same objective written in torch
    keys = ['encoder.prior.mean', 'encoder.dense_mean.weight', 'encoder.dense_log_var.weight']
    if net.encoder.prior.var_dim == 'diag':
        keys.append('encoder.prior._var_parameter')
    g_hip = grads_of(net, losses['total'])
    assert set(keys) <= set(g_hip)
    g = {}
    for dt in (torch.float32, F64):
        with op_replaced_by_torch(dt):
            total = net.evaluate(x, yh, with_beta=True, epsilon=eps, kl_var_weighting=w)[2]['total']
            g[dt] = grads_of(net, total)
    worst = 0.
    for k in keys:
        e_hip = float((g_hip[k] - g[torch.float32][k]).abs().max())
        e_h64 = float((g_hip[k].double() - g[F64][k].double()).abs().max())
        e_t32 = float((g[torch.float32][k].double() - g[F64][k].double()).abs().max())
        ratio = max(e_hip, e_h64) / e_t32 if e_t32 else (0. if max(e_hip, e_h64) == 0 else math.inf)
        worst = max(worst, ratio)
        print('%-34s |hip - torch32| %.3e  |hip - torch64| %.3e  |torch32 - torch64| %.3e  ratio %.3f' % (k, e_hip, e_h64, e_t32, ratio))
    print(name, 'largest ratio %.3f (allowed 4)' % worst)
    assert worst <= 4, (name, worst)


def test_cross_y_is_zero_with_zero_gradient_on_unlabelled_rows():
    net, x, y, eps = build('c2_n8_gamma', semi=True)
    base = net.evaluate(x, y, with_beta=True, epsilon=eps, gamma_weighting=0.5)[2]['cross_y'].detach().clone()
    yh = half_hidden(y)
    unl = yh < 0
    losses = net.evaluate(x, yh, with_beta=True, epsilon=eps, gamma_weighting=0.5)[2]
    ce = losses['cross_y']
    assert not bool(ce[..., unl].any()) and torch.equal(ce[..., ~unl], base[..., ~unl]) and bool((base[..., unl] > 0).all())
    assert any('classifier' in k and bool(v.any()) for k, v in grads_of(net, losses['total']).items())
    none = torch.full_like(y, -1)
    losses = net.evaluate(x, none, with_beta=True, epsilon=eps, gamma_weighting=0.5)[2]
    assert not bool(losses['cross_y'].any())
    g = grads_of(net, losses['total'])
    assert all(not bool(v.any()) for k, v in g.items() if 'classifier' in k)       # no label anywhere: the classifier learns nothing


@pytest.mark.parametrize('name,weights', [('c2_n8', None), ('c3_n8_diag', 'ramp')], ids=['c2', 'c3_diag_pi'])
def test_class_marginal(name, weights):
    net, x, y, eps = build(name)
    C = net.encoder.prior.mean.shape[0]
    if weights:
        net.UNLABELLED_CLASS_WEIGHTS = [1. + k % 7 for k in range(C)]
    U_, r = net.class_marginal(x)
    assert net.training and U_.shape == (N_MODEL,) and r.shape == (N_MODEL, C) and not U_.requires_grad
    net.eval()
    mu, log_var = net.latent_posterior(x)
    none = torch.full((N_MODEL,), -1, dtype=torch.int64)
    c, d, ref, B = restate(net, none, mu, log_var)
    ex = {'U': sc.excess(U_, ref['kl'], B['kl']), 'r': sc.excess(r, ref['r'], B['r'])}
    print(name, 'class_marginal, measured / bound:', ex)
    assert all(v <= 1 for v in ex.values()), ex
    assert torch.equal(r.argmax(1).cpu(), ref['parts']['Q'].argmin(1))
    assert float((r.double().sum(1) - 1).abs().max()) <= 8 * sc.U
    # the same op with every label -1 in a training-mode batch gives these rows when the posterior is the same: the op itself
    zero = torch.zeros(N_MODEL, device=DEV)
    pr = net.encoder.prior
    kl, _, _, r2 = ops.class_marginal_kl(mu.contiguous(), log_var.contiguous(), none.to(DEV), pr.mean.detach(), pr._var_parameter.detach(),
                                         zero, zero, zero, log_pi=net._semi_log_pi(C, DEV), w=1., var_dim=pr.var_dim)
    assert torch.equal(kl, U_) and torch.equal(r2, r)


def synth(n, name, seed, shape, C=10):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset(torch.rand(n, *shape, generator=g), torch.arange(n) % C)
    d.name = name
    return d


def test_one_epoch_of_train_model_over_hidden_labels(tmp_path):
    from jvae_compat.semi import HiddenLabels
    net = build('c2_n8', semi=True)[0]
    data = synth(64, 'synthetic', 5, tuple(net.input_shape))
    hidden = HiddenLabels(data, keep_per_class=2, seed=1)
    hidden.name = 'synthetic'
    assert int((~hidden.hidden).sum()) == 20
    seen = []
    step = net.train_step

    def spy(x, y, *a, **kw):
        seen.append(y.clone())
        return step(x, y, *a, **kw)
    net.train_step = spy
    hist = net.train_model(hidden, epochs=1, batch_size=16, save_dir=str(tmp_path), validation=0, device=DEV)
    assert hist['epochs'] == 1 and len(seen) == 4 and int(sum((s < 0).sum() for s in seen)) == 44
    assert all(np.isfinite(v) for v in hist[0]['train_loss'].values()) and all(np.isfinite(v) for v in hist[0]['train_measures'].values())
    assert net.training_parameters['semi_supervised'] is True
    from cvae import ClassificationVariationalNetwork as Net
    assert Net.load(str(tmp_path), load_state=False).training_parameters['semi_supervised'] is True
    # the same call with the switch off over the labelled set: the job directory a default run always wrote
    off = build('c2_n8')[0]
    hist = off.train_model(data, epochs=1, batch_size=16, save_dir=str(tmp_path / 'off'), validation=0, device=DEV)
    assert hist['epochs'] == 1 and 'semi_supervised' not in off.training_parameters


def test_train_model_with_validation_and_train_accuracy_over_hidden_labels(tmp_path):
    """The default train_model() cuts a validation set out of the set it is given, and train_accuracy scores the rest: both hold
    hidden labels, which must be neither an index nor an error.  accuracy() of a set with hidden labels is the accuracy of its
    labelled samples."""
    from jvae_compat.semi import HiddenLabels
    net = build('c2_n8', semi=True)[0]
    data = synth(64, 'synthetic', 5, tuple(net.input_shape))
    hidden = HiddenLabels(data, keep_per_class=2, seed=1)
    hidden.name = 'synthetic'
    hist = net.train_model(hidden, epochs=1, batch_size=16, test_batch_size=16, save_dir=str(tmp_path), validation=24, train_accuracy=True,
                           device=DEV)
    assert hist['epochs'] == 1
    for e in (0, 1):
        assert all(0. <= v <= 1. for v in hist[e]['validation_accuracy'].values()), hist[e]['validation_accuracy']
        assert all(np.isfinite(v) for v in hist[e]['validation_loss'].values()), hist[e]['validation_loss']
    assert all(0. <= v <= 1. for v in hist[0]['train_accuracy'].values())
    assert all(np.isfinite(v) for v in hist[0]['train_loss'].values())
    # accuracy() itself: the hidden rows are not scored
    kept = torch.utils.data.Subset(data, (~hidden.hidden).nonzero().flatten().tolist())
    kept.name = 'kept'
    with torch.no_grad():
        acc_h = net.accuracy(hidden, batch_size=64, update_self_testing=False)
        loss_h = dict(net.test_losses)
        acc_k = net.accuracy(kept, batch_size=64, update_self_testing=False)
        loss_k = dict(net.test_losses)
    # 'closest' and the analytic kl / zdist rows do not depend on the noise the two passes draw ('iws' and the totals do)
    assert set(acc_h) == set(acc_k) and acc_h['closest'] == acc_k['closest'] and set(loss_h) == set(loss_k)
    assert loss_h['kl'] == pytest.approx(loss_k['kl'], rel=1e-5) and loss_h['zdist'] == pytest.approx(loss_k['zdist'], rel=1e-5)
    net.SEMI_SUPERVISED = False                              # a labelled set: the switch does not enter its scores
    with torch.no_grad():
        acc_off = net.accuracy(kept, batch_size=64, update_self_testing=False)
        loss_off = dict(net.test_losses)
    assert acc_off['closest'] == acc_k['closest'] and loss_off['kl'] == pytest.approx(loss_k['kl'], rel=1e-6)


@pytest.mark.parametrize('row', sc.refusal_table(), ids=lambda r: r[0])
def test_every_refusal_raises_by_name(row):
    name, kwargs, tweak, ev_kw, word = row
    m = sc.refusal_model(kwargs, tweak, device=DEV)
    x = torch.rand(4, *m.input_shape, device=DEV)
    y = torch.tensor([0, -1, 1, -1], device=DEV)
    ev_kw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in ev_kw.items()}
    with pytest.raises(NotImplementedError, match='SEMI_SUPERVISED: .*' + word):
        m.train_step(x, y, **ev_kw)
