"""The MMD objective on the device: csrc/mmd.hip through ops.mmd_objective against the fp64 restatement and the derived bounds of
tests/mmd_cases.py (every output of every case, |error| <= 2^-24 B), then the model: TRAIN_OBJECTIVE = 'mmd', prior_mmd(), the
default objective untouched, train_model's bookkeeping and every refusal by name.

Common to every kernel call: each fp32 result the op allocates lies inside a NaN-filled buffer with a guard band of 64 floats on
either side (test_38's `Guarded`, restated), the guards must be intact and every element written; each call runs twice and must
give the same bits; the measured error over the bound is printed before it is held.

The out-of-range label: that sample's outputs are NaN, and the OTHER samples' bits are those of the same batch with that row
MASKED - given a class of its own (one more class), so that it is in nobody's set and adds to no class the others see.

Model level: the parameter gradients of one evaluate() + backward under 'mmd' are compared with the same objective written as a
torch expression of that evaluation's own z (total of the ELBO evaluation with its KL rescaled, plus mmd_weight times the rows in
torch; autograd then runs back through the same HIP ops).  Per parameter, e = max|torch32 - torch64| is the error of the torch fp32
expression against its fp64 form, and the HIP tail is allowed 4 e, for its distance to either.  The ratios are printed; DESIGN.md
section 7y records them.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

import mmd_cases as mc
from jvae_hip import lib, ops
from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
F64 = torch.float64
_cache = {}


def ref64(c):
    if c.name not in _cache:
        d = mc.make(c)
        r = mc.ref(c, d)
        _cache[c.name] = (d, r, mc.bounds(c, d, r))
    return _cache[c.name]


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

    def check(self, written=True):
        for buf, n in self.bufs:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'a guard band was written'
            if written:
                assert not bool(torch.isnan(buf[GUARD:GUARD + n]).any()), 'a result element was not written'
        return len(self.bufs)


@contextlib.contextmanager
def guarded(written=True):
    g = Guarded()
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = torch
    assert g.check(written) >= 4                   # m, g_z, g_means, g_T


def same_bits(a, b):
    return torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num()))


def twice(f):
    a, b = f(), f()
    assert set(a) == set(b)
    for k in a:
        assert same_bits(a[k], b[k]), f'two runs differ in {k}'
    return a


def run_case(c, d, written=True, g=None):
    """Forward and backward of one case through ops.mmd_objective -> every output."""
    t = {k: v.to(DEV) for k, v in d.items()}
    z, means, T = (t[k].clone().requires_grad_(True) for k in ('z', 'means', 'T'))
    with guarded(written):
        m = ops.mmd_objective(z, t['eps_p'], t['y'], means, T, kernel=mc.kernel_of(c), joint=c.joint, var_dim=c.var)
        torch.autograd.backward(m, grad_tensors=t['g'] if g is None else g)
    return dict(m=m.detach(), g_z=z.grad, g_means=means.grad, g_T=T.grad)


def hold(c, got, r, B, keys=None):
    ex = {k: mc.excess(got[k], r[k], B[k]) for k in (keys or B)}
    print(c.name, 'measured / bound:', {k: round(v, 4) for k, v in ex.items()})
    assert all(v <= 1 for v in ex.values()), (c.name, ex)
    return ex


# ============================================================================================ kernels against the restatement
@pytest.mark.parametrize('c', mc.SHAPE_CASES, ids=mc.ids)
def test_kernels_against_the_restatement(c):
    d, r, B = ref64(c)
    got = twice(lambda: run_case(c, d))
    assert set(got) == set(B)
    assert bool((got['g_z'][0] == 0).all())                                       # the mean latent takes no part
    assert got['g_T'].shape == d['T'].shape and got['g_means'].shape == d['means'].shape
    hold(c, got, r, B)
    if c.classes == 'own':                                                        # all within sums are 0: m_i = -2/N mean_l k(z_i, p_i)
        assert bool((got['m'] < 0).all())


@pytest.mark.parametrize('c', mc.STRESS_CASES, ids=mc.ids)
def test_stress_rows(c):
    d, r, B = ref64(c)
    got = twice(lambda: run_case(c, d))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    hold(c, got, r, B)


@pytest.mark.parametrize('c', [mc.SHAPE_CASES[3], mc.SHAPE_CASES[2], mc.STRESS_CASES[1]], ids=mc.ids)
def test_zero_incoming_gradient_gives_zero_gradients(c):
    d, _, _ = ref64(c)
    got = run_case(c, d, g=torch.zeros(c.N, device=DEV))
    for k in ('g_z', 'g_means', 'g_T'):
        assert bool((got[k] == 0).all()), k


def test_coincident_points_count_every_scale_and_add_nothing():
    """Two rows, one class, one draw, z_0 = z_1 and p_0 = p_1 = z: every squared distance is 0, so every kernel value is the
    number of scales S and every difference a_k - b_k is exactly 0: m = S + S - 2 S = 0 and all gradients are exactly 0."""
    K = 5
    row = torch.randn(K, device=DEV)
    z = row.expand(2, 2, K).contiguous()
    means = row.view(1, K).clone()
    for kernel, S in ((('imq', None), 7), (('rbf', (3., 9.)), 2)):
        zz, mm = z.clone().requires_grad_(True), means.clone().requires_grad_(True)
        T = torch.ones(1, device=DEV, requires_grad=True)
        m = ops.mmd_objective(zz, torch.zeros(1, 2, K, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), mm, T, kernel=kernel)
        assert torch.equal(m, torch.zeros(2, device=DEV)), (kernel, S)
        m.sum().backward()
        assert bool((zz.grad == 0).all()) and bool((mm.grad == 0).all()) and bool((T.grad == 0).all())


def test_empty_batch():
    c = mc._c('empty', 5, 3, 0, C=2, var='diag')
    got = run_case(c, mc.make(c), written=True)
    assert got['m'].shape == (0,) and got['g_z'].shape == (4, 0, 5)
    for k in ('g_means', 'g_T'):                                                  # empty sums: zeros, written
        assert bool((got[k] == 0).all()), k


def test_bad_label_is_never_an_index():
    c = mc.SHAPE_CASES[3]                                                         # K 65, L 3, N 64, C 3, diag
    d, _, _ = ref64(c)
    bad = torch.zeros(c.N, dtype=torch.bool)
    bad[[3, 40, 63]] = True
    y = d['y'].clone()
    y[3], y[40], y[63] = c.C, -1, 2 ** 40
    db = dict(d, y=y)
    got = twice(lambda: run_case(c, db, written=False))
    good = ~bad
    assert bool(torch.isnan(got['m'][bad]).all()) and bool(torch.isfinite(got['m'][good]).all())
    assert bool(torch.isnan(got['g_z'][1:, bad]).all()) and bool((got['g_z'][0] == 0).all())
    assert bool(torch.isfinite(got['g_z'][1:, good]).all())
    assert bool(torch.isfinite(got['g_means']).all()) and bool(torch.isfinite(got['g_T']).all())
    # every output against the restatement, which gives the bad samples NaN, no set and no class
    rb = mc.ref(c, db)
    hold(c, got, rb, mc.bounds(c, db, rb))
    # the other samples' bits: the same batch with each bad row MASKED - a class of its own
    cm = c._replace(C=c.C + 3)
    ym = d['y'].clone()
    ym[3], ym[40], ym[63] = c.C, c.C + 1, c.C + 2
    extra = torch.ones(3, c.K)
    dm = dict(d, y=ym, means=torch.cat([d['means'], 0 * extra]), T=torch.cat([d['T'], extra]))
    masked = run_case(cm, dm)
    assert torch.equal(got['m'][good], masked['m'][good])
    assert torch.equal(got['g_z'][:, good], masked['g_z'][:, good])
    assert torch.equal(got['g_means'], masked['g_means'][:c.C]) and torch.equal(got['g_T'], masked['g_T'][:c.C])


def test_operands_are_refused_as_the_neighbouring_ops_refuse_them():
    c = mc.SHAPE_CASES[3]
    d = {k: v.to(DEV) for k, v in mc.make(c).items()}

    def call(**kw):
        a = dict(d, **kw)
        return ops.mmd_objective(a['z'], a['eps_p'], a['y'], a['means'], a['T'], kernel=mc.kernel_of(c), joint=c.joint,
                                 var_dim=kw.get('var_dim', c.var))
    assert call().shape == (c.N,)
    with pytest.raises(lib.JvaeHipError, match='contiguous'):
        call(eps_p=d['eps_p'].transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(lib.JvaeHipError, match='resident on the GPU'):
        call(means=d['means'].cpu())
    with pytest.raises(lib.JvaeHipError, match='torch.float32'):
        call(z=d['z'].double())
    with pytest.raises(lib.JvaeHipError, match='unsupported configuration'):      # var_dim='full': refused by the library
        call(var_dim='full', T=torch.eye(c.K, device=DEV).repeat(c.C, 1, 1))


def test_the_limits_are_refused_without_a_launch():
    h = lib.load()
    p = torch.zeros(64, device=DEV)
    before = p.clone()
    P_ = lib.ptr
    import ctypes
    sc = (ctypes.c_float * 1)(1.)
    for L, N, K in ((1, 8193, 4), (1, 4, 1025), (65536, 4, 4)):
        assert h.jvae_mmd_fwd_workspace_bytes(L, N, K) == 0 and h.jvae_mmd_bwd_workspace_bytes(L, N, K) == 0
        rc = h.jvae_mmd_objective_fwd_f32(P_(p), P_(p), P_(p), P_(p), P_(p), 0, 0, sc, 1, 1, L, N, K, 1, P_(p), P_(p), 1 << 40,
                                          lib.stream_ptr())
        assert rc == -2, (L, N, K)
    torch.cuda.synchronize()
    assert torch.equal(p, before)


# ============================================================================================ the model
MODELS = {'c1_n16_mlp': {}, 'c2_n8': {}, 'c3_n8_diag': {},
          'c1_n16_mlp_vae': dict(type='vae', prior=dict(distribution='gaussian', init_mean=0., var_dim='scalar'))}
L_TRAIN = 3


def build(name, L=None, objective=None, seed=0):
    from cvae import ClassificationVariationalNetwork as Net
    case = get_case(name.replace('_vae', ''))
    L = case['net']['latent_sampling'] if L is None else L
    kw = dict(case['net'], latent_sampling=L, test_latent_sampling=L, **MODELS.get(name, {}))
    net = Net(**kw)
    load_det_state(net, seed=seed)
    net.to(DEV)
    net.train()
    if objective is not None:
        net.TRAIN_OBJECTIVE = objective
    x, y, eps = det_inputs(case['N'], kw['input_shape'], kw['num_labels'], L, kw['latent_dim'], seed=42)
    eps_p = torch.randn(L, case['N'], kw['latent_dim'], generator=torch.Generator().manual_seed(7))
    return net, x.to(DEV), y.to(DEV), eps.to(DEV), eps_p.to(DEV)


@contextlib.contextmanager
def captured_mmd_objective():
    """The operands the model hands to ops.mmd_objective, call by call (the model looks the op up in the module at every call)."""
    calls, real = [], ops.mmd_objective

    def spy(z, eps_p, y, means, T, kernel=('imq', None), joint=True, var_dim='scalar'):
        calls.append(dict(z=z, eps_p=eps_p, y=y, means=means, T=T, kernel=kernel, joint=joint, var_dim=var_dim))
        return real(z, eps_p, y, means, T, kernel=kernel, joint=joint, var_dim=var_dim)
    ops.mmd_objective = spy
    try:
        yield calls
    finally:
        ops.mmd_objective = real


def restate_call(call):
    L, N, K = call['eps_p'].shape
    kind, scales = call['kernel']
    c = mc._c('model', K, L, N, C=call['means'].shape[0], var=call['var_dim'], kind=kind, scales=scales, joint=call['joint'])
    d = {k: call[k].detach().cpu() for k in ('z', 'eps_p', 'y', 'means', 'T')}
    d['g'] = torch.ones(N)
    d['p'] = mc.prior_draws32(d['y'], d['means'], d['T'], d['eps_p'], c.C)
    r = mc.ref(c, d)
    return c, d, r, mc.bounds(c, d, r)


def torch_total(net, x, y, eps, eps_p, dt):
    """One ELBO-mode evaluate() of `net` for its differentiable z, then total = its total + beta (kl_weight - 1) kl + mmd_weight m
    with m written in torch (mmd_cases.rows on the device, the prior draws formed from the prior's own parameters), in `dt`."""
    _, _, losses, _, mu, log_var, z = net.evaluate(x, y, with_beta=True, epsilon=eps, z_output=True)
    pr = net.encoder.prior
    N = x.shape[0]
    lab, means, T = pr._kernel_operands(y if pr.conditional else None, N, x.device)
    kind, scales = net.MMD_KERNEL
    c = mc._c('model', net.latent_dim, eps_p.shape[0], N, C=means.shape[0], var=pr.var_dim, kind=kind, scales=scales,
              joint=net.MMD_JOINT)
    p = mc.prior_draws32(lab, means.to(dt), T.to(dt), eps_p.to(dt), c.C)
    m = mc.rows(c, dict(y=lab), leaves=dict(z=z.to(dt), p=p))
    kl_weight, mmd_weight = net.MMD_WEIGHTS
    return losses['total'].to(dt) + net.beta * (kl_weight - 1.) * losses['kl'].to(dt) + mmd_weight * m


def grads_of(net, total):
    for p in net.parameters():
        p.grad = None
    total.mean().backward()
    lib.join_side_stream()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('L', [1, L_TRAIN], ids=lambda v: 'L%d' % v)
@pytest.mark.parametrize('name', list(MODELS))
def test_model_losses_and_gradients(name, L):
    net, x, y, eps, eps_p = build(name, L=L, objective='mmd')
    if L != 1:
        net.MMD_WEIGHTS, net.MMD_KERNEL, net.MMD_JOINT = (0.25, 50.), ('rbf', (4., 16., 64.)), False
    with captured_mmd_objective() as calls:
        losses = net.evaluate(x, y, with_beta=True, epsilon=eps, prior_epsilon=eps_p)[2]
    assert {'mmd', 'kl', 'zdist', 'var_kl', 'wmse', 'cross_x', 'total'} <= set(losses)
    assert not ({'iwae', 'mi'} & set(losses)) and losses['mmd'].shape == (x.shape[0],)
    # the rows the model reports: the restatement on the very operands the op was handed, which must be the evaluation's own
    assert len(calls) == 1 and calls[0]['eps_p'].data_ptr() == eps_p.data_ptr() and net._last_prior_epsilon is eps_p
    assert torch.equal(net._last_epsilon, eps[1:])
    assert calls[0]['z'].shape == (L + 1, x.shape[0], net.latent_dim) and calls[0]['kernel'] == net.MMD_KERNEL
    assert calls[0]['var_dim'] == net.encoder.prior.var_dim and calls[0]['joint'] == net.MMD_JOINT
    c, d, r, B = restate_call(calls[0])
    hold(c, {'m': losses['mmd']}, r, B, keys=['m'])
    g_hip = grads_of(net, losses['total'])
    assert any('encoder.dense_log_var' in k for k in g_hip) and any('imager' in k for k in g_hip)
    net.TRAIN_OBJECTIVE = 'elbo'
    g32 = grads_of(net, torch_total(net, x, y, eps, eps_p, torch.float32))
    g64 = grads_of(net, torch_total(net, x, y, eps, eps_p, F64))
    assert set(g_hip) == set(g32) == set(g64)
    worst = 0.
    for k in sorted(g_hip):
        e_hip = float((g_hip[k] - g32[k]).abs().max())
        e_h64 = float((g_hip[k].double() - g64[k].double()).abs().max())
        e_t32 = float((g32[k].double() - g64[k].double()).abs().max())
        ratio = max(e_hip, e_h64) / e_t32 if e_t32 else (0. if max(e_hip, e_h64) == 0 else math.inf)
        worst = max(worst, ratio)
        print('%-34s |hip - torch32| %.3e  |hip - torch64| %.3e  |torch32 - torch64| %.3e  ratio %.3f' % (k, e_hip, e_h64, e_t32, ratio))
    print(name, 'L', L, 'largest ratio %.3f (allowed 4)' % worst)
    assert worst <= 4, (name, L, worst)


def test_the_prior_noise_is_drawn_after_the_encoders_and_kept():
    net, x, y, eps, _ = build('c1_n16_mlp', L=L_TRAIN, objective='mmd')
    torch.manual_seed(11)
    want = torch.randn(L_TRAIN, x.shape[0], net.latent_dim, device=DEV)
    torch.manual_seed(11)
    losses = net.evaluate(x, y, with_beta=True, epsilon=eps)[2]                   # the encoder's noise is given: one draw is left
    assert torch.equal(net._last_prior_epsilon, want) and bool(torch.isfinite(losses['mmd']).all())
    with pytest.raises(ValueError, match='prior_epsilon'):
        net.evaluate(x, y, epsilon=eps, prior_epsilon=want[:1])


def params_of(net):
    return {k: p.detach().clone() for k, p in net.named_parameters()}


def three_steps(objective):
    net, x, y, eps, eps_p = build('c1_n16_mlp', L=L_TRAIN, objective=objective)
    before = params_of(net)
    seen = []
    for i in range(3):
        losses, _ = net.train_step(x, y, batch=i, epsilon=eps, **({'prior_epsilon': eps_p} if objective == 'mmd' else {}))
        seen.append(set(losses))
    torch.cuda.synchronize()
    return net, before, params_of(net), seen


def test_three_mmd_steps_move_every_parameter_and_repeat_bit_for_bit():
    net, before, after, seen = three_steps('mmd')
    assert all('mmd' in s for s in seen)
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    assert trainable
    for k in trainable:
        assert bool(torch.isfinite(after[k]).all()), k
        assert not torch.equal(after[k], before[k]), k + ' did not move'
    _, before2, after2, _ = three_steps('mmd')
    for k in after:
        assert torch.equal(before[k], before2[k]) and torch.equal(after[k], after2[k]), k


def test_default_objective_is_the_parents_step_bit_for_bit():
    """A model that never touches the attributes against one that sets the default by hand: the same parameters, bit for bit, no
    new key in its losses, no new training parameter, no second noise tensor drawn (the device's random stream is where the
    steps left it without the switch); switched to 'mmd', the second model then takes another road.  Both models run the same
    branch of THIS build: that the default path computes what the parent computed is held by the tests that were there before."""
    state = torch.cuda.get_rng_state(0)
    _, _, plain, seen = three_steps(None)
    after_plain = torch.cuda.get_rng_state(0)
    torch.cuda.set_rng_state(state, 0)
    net, _, explicit, seen2 = three_steps('elbo')
    assert torch.equal(torch.cuda.get_rng_state(0), after_plain)
    assert all('mmd' not in s for s in seen + seen2) and seen == seen2
    for k in plain:
        assert torch.equal(plain[k], explicit[k]), k
    assert not ({'objective', 'mmd_weights', 'mmd_kernel'} & set(net.training_parameters))
    assert not hasattr(net, '_last_prior_epsilon')
    net.TRAIN_OBJECTIVE = 'mmd'
    x, y, eps = build('c1_n16_mlp', L=L_TRAIN)[1:4]
    losses, _ = net.train_step(x, y, epsilon=eps)
    assert 'mmd' in losses and net._last_prior_epsilon.shape == eps[1:].shape


def synth(n, name, seed, shape=(1, 28, 28)):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset(torch.rand(n, *shape, generator=g), torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


@pytest.mark.parametrize('name', ['c1_n16_mlp', 'c1_n16_mlp_vae'])
def test_train_model_keeps_the_books(name, tmp_path):
    net = build(name, L=2, objective='mmd')[0]
    net.MMD_WEIGHTS = (0., 100.)                                                  # WAE-MMD: no KL in the loss
    data = synth(32, 'synthetic', 5, shape=tuple(net.input_shape))
    hist = net.train_model(data, epochs=2, batch_size=16, save_dir=str(tmp_path), validation=0, device=DEV)
    assert hist['epochs'] == 2
    for e in range(2):
        assert 'mmd' in hist[e]['train_loss'] and all(np.isfinite(v) for v in hist[e]['train_loss'].values())
    tp = net.training_parameters
    assert tp['objective'] == 'mmd' and tp['mmd_weights'] == [0., 100.]
    assert tp['mmd_kernel'] == {'kind': 'imq', 'scales': [2. * net.latent_dim * s for s in mc.WAE_SCALES], 'joint': True}


@pytest.mark.parametrize('name', ['c1_n16_mlp', 'c1_n16_mlp_vae'])
def test_prior_mmd_against_the_restatement(name):
    net = build(name)[0]
    conditional = net.encoder.prior.conditional
    M, K = 70, net.latent_dim
    gen = torch.Generator().manual_seed(3)
    codes = torch.randn(M, K, generator=gen).to(DEV)
    e = torch.randn(M, K, generator=gen).to(DEV)
    y = torch.randint(0, net.num_labels, (M,), generator=gen).to(DEV) if conditional else None
    net.eval()
    with captured_mmd_objective() as calls:
        value, rows = net.prior_mmd(codes, y, epsilon=e)
    assert not net.training and rows.shape == (M,) and value.shape == () and not rows.requires_grad
    assert torch.equal(value, rows.mean())
    c, d, r, B = restate_call(calls[0])
    assert torch.equal(d['z'][1], codes.cpu()) and c.L == 1
    hold(c, {'m': rows}, r, B, keys=['m'])
    a, b = net.prior_mmd(codes, y)[0], net.prior_mmd(codes, y)[0]                # its own noise: another estimate each time
    assert bool(torch.isfinite(a)) and not torch.equal(a, b)
    with pytest.raises(ValueError, match='labels' if conditional else 'must be None'):
        net.prior_mmd(codes, None if conditional else torch.zeros(M, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match='codes must be'):
        net.prior_mmd(codes[:, :-1], y)


# ============================================================================================ refusals
@pytest.mark.parametrize('row', mc.refusal_table(), ids=lambda r: r[0])
def test_every_refusal_raises_by_name(row):
    name, kwargs, tweak, ev_kw, word = row
    m = mc.refusal_model(kwargs, tweak, device=DEV)
    x = torch.rand(4, *m.input_shape, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'mmd'.*" + word):
        m.train_step(x, y, **ev_kw)
    if name == 'train_captured':
        for who in (m.graph_train_step, m.capture_train_step):
            with pytest.raises(NotImplementedError, match='TRAIN_OBJECTIVE.*' + who.__name__):
                who(x, y)


def test_malformed_settings_and_a_free_kl_warmup():
    net, x, y, eps, eps_p = build('c1_n16_mlp', L=2, objective='mmd')
    losses = net.evaluate(x, y, kl_var_weighting=0.5, epsilon=eps, prior_epsilon=eps_p)[2]       # allowed: the KL keeps its own path
    assert bool(torch.isfinite(losses['total']).all())
    for attr, value in (('MMD_WEIGHTS', (1.,)), ('MMD_WEIGHTS', (1., float('inf'))), ('MMD_KERNEL', ('laplace', None)),
                        ('MMD_KERNEL', ('imq', (1., -2.))), ('MMD_KERNEL', ('rbf', tuple(range(1, 10)))), ('MMD_KERNEL', 'imq')):
        net = build('c1_n16_mlp', L=2, objective='mmd')[0]
        setattr(net, attr, value)
        with pytest.raises(ValueError, match=attr):
            net.evaluate(x, y, epsilon=eps)
