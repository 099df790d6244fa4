"""The importance-weighted bound on the device: csrc/iwae.hip through ops.iw_bound against the fp64 restatement and the derived
bounds of tests/iwae_cases.py (every output of every case, |error| <= 2^-24 B), then the model: TRAIN_OBJECTIVE = 'iwae', the
default objective untouched, net.iw_bound over slabs of draws, and every refusal by name.

Common to every kernel call: each fp32 result the op allocates lies inside a NaN-filled buffer with a guard band of 64 floats
on either side (the idea of test_35's `Guarded`, restated here), the guards must be intact and every element written; each
call runs twice and must give the same bits; the measured error over the bound is printed before it is held.

Model level: the parameter gradients of one evaluate() + backward under 'iwae' are compared with the same bound written as a
torch fp32 expression of that evaluation's own x_reco, z, log_var (autograd then runs back through the same HIP ops).  Per
parameter, e = max|torch32 - torch64| is the error of that torch fp32 expression against the same expression with its tail in
fp64, and the HIP tail is allowed 4 e (the 4 covers the different summation orders over L and over a class's samples) - held both
for its distance to the torch fp32 expression and for its distance to the fp64 tail.  Each model runs with the draw of its case
(L = 1: every weight is 1, the torch tail forms the rows itself) AND with three draws.  With three draws the torch tails start
from the fp32 rows wmse_s that ops.recon_wmse returned - the rows the HIP tail is handed: a weight hangs on those rows times
D / (2 sigma^2), and with the rows shared the ratio measures the tail.  The same three-draw comparison with the torch tails forming
their own rows (fp32 mean against fp64 mean) is printed beside it, not held: there the figure is the ratio of two roundings of
the rows.  In every run losses['iwae'] and losses['ess'] are held to the restatement on the operands ops.iw_bound was handed.
Measured on an MI355X, largest ratio max(|hip - torch32|, |hip - torch64|) / e over the parameters:

                     L = 1, own rows    L = 3, shared rows (held)    L = 3, own rows (printed)
    c1_n16_mlp           1.333                 1.000                       10.750
    c2_n8                1.000                 1.000                        1.333
    c3_n8_diag           1.000                 1.000                        1.333
    c1_n16_mlp_vae       1.333                 1.333                        2.000        (allowed where held: 4)

c1_n16_mlp at three draws is the one model with samples whose draws share the weight (mean ess 1.004): 10.75 with the torch tails
forming their own rows, 1.000 with the rows shared - the rows are the cause, the tail is not.  losses['iwae'] / losses['ess']
against the restatement on the op's own operands: at most 0.43 / 0.006 of the derived bound over the eight runs.
"""
import contextlib
import math

import pytest
import torch

import iwae_cases as ic
from jvae_hip import lib, ops
from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
P_ = lib.ptr
_cache = {}


def ref64(c):
    if c.name not in _cache:
        d = ic.make(c)
        r = ic.ref(c, d)
        _cache[c.name] = (d, r, ic.bounds(c, d, r))
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
    assert g.check(written) >= 3


def twice(f):
    a, b = f(), f()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]) or (torch.equal(torch.isnan(a[k]), torch.isnan(b[k]))
                                           and torch.equal(a[k].nan_to_num(), b[k].nan_to_num())), f'two runs differ in {k}'
    return a


def run_case(c, d, written=True):
    """Forward and backward of one case through ops.iw_bound -> every output, wt included (the tensor kept for backward)."""
    t = {k: v.to(DEV) for k, v in d.items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in ('wmse_s', 'z', 'lv', 'means', 'sigma')}
    T = t['T'].clone().requires_grad_(c.var == 'diag')
    with guarded(written):
        bound, ess = ops.iw_bound(leaves['wmse_s'], leaves['z'], leaves['lv'], t['eps'], t['y'], leaves['means'], T,
                                  leaves['sigma'], c.sig, c.D, beta=c.beta, var_dim=c.var)
        assert not ess.requires_grad
        wt = bound.grad_fn.saved_tensors[0].clone()
        torch.autograd.backward(bound, grad_tensors=t['g'])
    out = dict(bound=bound.detach(), wt=wt, ess=ess, **{'g_' + k: v.grad for k, v in leaves.items()})
    if c.var == 'diag':
        out['g_T'] = T.grad
    return out


def hold(c, got, r, B, keys=None):
    ex = {k: ic.excess(got[k], r[k], B[k]) for k in (keys or B)}
    print(c.name, 'measured / bound:', {k: round(v, 3) for k, v in ex.items()})
    assert all(v <= 1 for v in ex.values()), (c.name, ex)


# ============================================================================================ kernels against the restatement
@pytest.mark.parametrize('c', ic.SHAPE_CASES, ids=ic.ids)
def test_kernels_against_the_restatement(c):
    d, r, B = ref64(c)
    got = twice(lambda: run_case(c, d))
    assert set(got) == set(B)
    assert bool((got['g_z'][0] == 0).all())                                       # the mean latent takes no part
    hold(c, got, r, B)


@pytest.mark.parametrize('c', ic.STRESS_CASES, ids=ic.ids)
def test_stress_rows(c):
    d, r, B = ref64(c)
    got = twice(lambda: run_case(c, d))
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    wt, ess = got['wt'], got['ess']
    if c.stress == 'lead':                                                        # exactly one-hot, ess exactly 1
        assert bool((wt.max(0).values == 1).all()) and bool((wt.sum(0) == 1).all()) and bool((ess == 1).all())
        assert torch.equal(wt.argmax(0).cpu(), r['wt'].argmax(0))
    if c.stress == 'equal':                                                       # every e is exp(0): S = Q = L exactly
        assert bool((ess == c.L).all()) and bool((wt == wt[0]).all())
    if c.stress == 'deep':
        assert bool((got['bound'] < -9e4).all())
    if c.stress == 'huge':
        assert float(wt[1, 0]) == 0 and bool((wt[:, 1] > 0).all())
    hold(c, got, r, B)


def raw_backward(c, t, wt, g):
    """jvae_iw_bound_bwd_f32 itself (ops never hands it a missing upstream gradient) -> its outputs, NaN-filled beforehand."""
    h = lib.load()
    L, N, K, C = c.L, c.N, c.K, c.C
    nan = lambda *s: torch.full(s, math.nan, device=DEV)                          # noqa: E731
    o = dict(g_wmse_s=nan(L, N), g_z=nan(L + 1, N, K), g_lv=nan(N, K), g_means=nan(C, K), g_sigma=nan(*t['sigma'].shape))
    if c.var == 'diag':
        o['g_T'] = nan(C, K)
    ws = torch.empty(h.jvae_iw_bound_bwd_workspace_bytes(N, K), dtype=torch.uint8, device=DEV)
    rc = h.jvae_iw_bound_bwd_f32(P_(g), P_(wt), P_(t['z']), P_(t['y']), P_(t['means']), P_(t['T']), P_(t['sigma']), c.sig, 0,
                                 ops.VAR_KIND[c.var], c.beta, L, N, K, C, c.D, P_(o['g_wmse_s']), P_(o['g_z']), P_(o['g_lv']),
                                 P_(o['g_means']), P_(o.get('g_T')), P_(o['g_sigma']), P_(ws), ws.numel(), lib.stream_ptr())
    assert rc == 0
    return o


def test_missing_upstream_gradient_gives_the_bits_of_an_explicit_zero():
    c = ic.SHAPE_CASES[1]                                                         # diag, log sigma, an empty class
    d, r, B = ref64(c)
    t = {k: v.to(DEV) for k, v in d.items()}
    wt = run_case(c, d)['wt']
    none, zero = raw_backward(c, t, wt, None), raw_backward(c, t, wt, torch.zeros(c.N, device=DEV))
    for k in zero:
        assert not bool(torch.isnan(zero[k]).any()), k
        assert torch.equal(none[k].view(torch.int32), zero[k].view(torch.int32)), k
        assert bool((zero[k] == 0).all()), k


def test_empty_batch():
    c = ic.Case('empty', 5, 3, 0, 2, 'rand', 'diag', ic.SIG_VALUE, 1., 7, None)
    d = ic.make(c)
    got = run_case(c, d)
    assert got['bound'].shape == (0,) and got['ess'].shape == (0,) and got['wt'].shape == (3, 0)
    assert got['g_z'].shape == (4, 0, 5) and got['g_wmse_s'].shape == (3, 0)
    for k in ('g_means', 'g_T', 'g_sigma'):                                       # empty sums: zeros, written
        assert bool((got[k] == 0).all()), k


def test_bad_label_is_never_an_index():
    c = ic.SHAPE_CASES[5]                                                         # K 200, L 5, N 257, diag, coded sigma
    d, _, _ = ref64(c)
    d = dict(d)
    y = d['y'].clone()
    bad = torch.zeros(c.N, dtype=torch.bool)
    bad[[3, 100, 256]] = True
    y[3], y[100], y[256] = c.C, -1, 2 ** 40
    got = twice(lambda: run_case(c, dict(d, y=y), written=False))
    good = ~bad
    for k in ('bound', 'ess'):
        assert bool(torch.isnan(got[k][bad]).all()) and bool(torch.isfinite(got[k][good]).all()), k
    for k in ('wt', 'g_wmse_s'):
        assert bool(torch.isnan(got[k][:, bad]).all()) and bool(torch.isfinite(got[k][:, good]).all()), k
    assert bool(torch.isnan(got['g_z'][1:, bad]).all()) and bool((got['g_z'][0] == 0).all())
    assert bool(torch.isnan(got['g_lv'][bad]).all()) and bool(torch.isnan(got['g_sigma'][bad]).all())
    # the good samples and the class sums are those of the batch without the bad samples' gradient
    d2 = dict(d, g=d['g'] * good)
    r2 = ic.ref(c, d2)
    B2 = ic.bounds(c, d2, r2)
    sub = dict(bound=got['bound'][good], ess=got['ess'][good], wt=got['wt'][:, good], g_means=got['g_means'], g_T=got['g_T'])
    r2s = dict(r2, bound=r2['bound'][good], ess=r2['ess'][good], wt=r2['wt'][:, good])
    B2s = dict(B2, bound=B2['bound'][good], ess=B2['ess'][good], wt=B2['wt'][:, good])
    assert bool(torch.isfinite(got['g_means']).all()) and bool(torch.isfinite(got['g_T']).all())
    hold(c, sub, r2s, B2s, keys=list(sub))


def test_operands_are_refused_as_the_neighbouring_ops_refuse_them():
    c = ic.SHAPE_CASES[2]
    d = {k: v.to(DEV) for k, v in ic.make(c).items()}

    def call(**kw):
        a = dict(d, **kw)
        return ops.iw_bound(a['wmse_s'], a['z'], a['lv'], a['eps'], a['y'], a['means'], a['T'], a['sigma'], kw.get('sig', c.sig),
                            c.D, beta=c.beta, var_dim=kw.get('var_dim', c.var))
    assert call()[0].shape == (c.N,)
    with pytest.raises(lib.JvaeHipError, match='contiguous'):
        call(eps=d['eps'].transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(lib.JvaeHipError, match='resident on the GPU'):
        call(lv=d['lv'].cpu())
    with pytest.raises(lib.JvaeHipError, match='torch.float32'):
        call(z=d['z'].double())
    with pytest.raises(lib.JvaeHipError, match='unsupported configuration'):      # var_dim='full': refused by the library
        call(var_dim='full', T=torch.eye(c.K, device=DEV).repeat(c.C, 1, 1))
    with pytest.raises(lib.JvaeHipError, match='unsupported configuration'):      # the rmse sigma kind
        call(sig=ic.SIG_RMSE)
    with pytest.raises(lib.JvaeHipError, match='no gradient'):
        ops.iw_bound(d['wmse_s'].clone().requires_grad_(True), d['z'], d['lv'], d['eps'], d['y'], d['means'], d['T'], d['sigma'],
                     c.sig, c.D, state=torch.zeros(4, c.N, device=DEV, dtype=torch.float64))


def test_state_merges_slabs_of_draws():
    """The same draws in one call and in slabs of 2 merged through `state`: the same log w bits on both sides, so the two
    results differ by the roundings of the two folds alone.  Derived: the one-call fold is good to (102 + n_S) u in S (iwae_cases),
    a slab's likewise, each merge adds the rounded exponent difference (<= 100 u for a side that matters), expf (2 u), a product
    and a sum; the logarithms and the two sums of max + log S - log L add 2 (|log S| + log L) + 2 (|max| + |log S| + log L) each."""
    c = ic.SHAPE_CASES[2]._replace(name='slabs', L=7, sig=ic.SIG_LOG)
    d = ic.make(c)
    t = {k: v.to(DEV) for k, v in d.items()}
    args = lambda sl: (t['wmse_s'][sl].contiguous(), torch.cat([t['z'][:1], t['z'][1:][sl]]), t['lv'], t['eps'][sl].contiguous(),     # noqa: E731
                       t['y'], t['means'], t['T'], t['sigma'], c.sig, c.D)
    with torch.no_grad():
        b1, e1 = ops.iw_bound(*args(slice(0, 7)), beta=c.beta, var_dim=c.var)
        state = torch.zeros(4, c.N, device=DEV, dtype=torch.float64)
        for l0 in range(0, 7, 2):
            b2, e2 = ops.iw_bound(*args(slice(l0, l0 + 2)), beta=c.beta, var_dim=c.var, state=state)
    assert torch.equal(state[3], torch.full((c.N,), 7., device=DEV, dtype=torch.float64))
    r = ic.ref(c, d)
    M = r['log_w'].max(0).values.abs()
    logS = (r['bound'] + math.log(7) - r['log_w'].max(0).values).abs()
    ends = 2 * (logS + math.log(7)) + 2 * (M + logS + math.log(7)) + 1
    n7, n2, merges = ic.n_S(7), ic.n_S(2), 4
    B = (102 + n7) + (102 + n2 + merges * 104) + 2 * ends
    # ess = S^2 / Q: S twice, Q once (its addends are squares: 2 x 102 + 1 each, the merge scales by a squared factor), a product
    # and a division, on either side
    B_ess = r['ess'] * ((2 * (102 + n7) + (205 + n7) + 2) + (2 * (102 + n2 + merges * 104) + (205 + n2 + merges * 208) + 2))
    ex, ex_ess = ic.excess(b1, b2.cpu().double(), B), ic.excess(e1, e2.cpu().double(), B_ess)
    print('slabs: measured / bound', round(ex, 3), round(ex_ess, 3))
    assert ex <= 1 and ex_ess <= 1
    # and the merged result against the restatement: the one-call bound plus what the merges add
    hold(c, dict(bound=b2), r, {'bound': ic.bounds(c, d, r)['bound'] + merges * 104 + ends}, keys=['bound'])


# ============================================================================================ the model
MODELS = {'c1_n16_mlp': {}, 'c2_n8': {}, 'c3_n8_diag': {},
          'c1_n16_mlp_vae': dict(type='vae', prior=dict(distribution='gaussian', init_mean=0., var_dim='scalar'))}
L_TRAIN = 3           # the steps below train with three draws, so that the weights are at work


def build(name, L=None, objective=None, seed=0):
    """L None: the draws of the case itself (one, in all four)."""
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
    return net, x.to(DEV), y.to(DEV), eps.to(DEV)


@contextlib.contextmanager
def captured_iw_bound():
    """The operands the model hands to ops.iw_bound, call by call (the model looks the op up in the module at every call)."""
    calls, real = [], ops.iw_bound

    def spy(wmse_s, z, lv, eps, y, means, T, sigma, sigma_is_log, D, beta=1., var_dim='scalar', state=None):
        calls.append(dict(wmse_s=wmse_s, z=z, lv=lv, eps=eps, y=y, means=means, T=T, sigma=sigma, sigma_kind=int(sigma_is_log), D=int(D),
                          beta=float(beta), var_dim=var_dim))
        return real(wmse_s, z, lv, eps, y, means, T, sigma, sigma_is_log, D, beta=beta, var_dim=var_dim, state=state)
    ops.iw_bound = spy
    try:
        yield calls
    finally:
        ops.iw_bound = real


def restate_calls(calls):
    """The restatement on the operands of one or more calls (slabs of draws of one batch put back together)."""
    first = calls[0]
    N, K = first['lv'].shape
    L = sum(r['eps'].shape[0] for r in calls)
    c = ic.Case('model', K, L, N, first['means'].shape[0], 'rand', first['var_dim'], first['sigma_kind'], first['beta'], first['D'], None)
    d = dict(wmse_s=torch.cat([r['wmse_s'] for r in calls]), z=torch.cat([first['z'][:1]] + [r['z'][1:] for r in calls]),
             lv=first['lv'], eps=torch.cat([r['eps'] for r in calls]), y=first['y'], means=first['means'], T=first['T'],
             sigma=first['sigma'].reshape(-1), g=torch.ones(N))
    d = {k: v.detach().cpu() for k, v in d.items()}
    r = ic.ref(c, d)
    return c, d, r, ic.bounds(c, d, r)


def torch_total(net, x, y, eps, dt, rows='own'):
    """One ELBO-mode evaluate() of `net` for its differentiable x_reco, z, log_var (and cross_y), then total = -bound (+ cw
    cross_y) with the bound written in torch, its tail in `dt`.  rows 'own': the tail forms the reconstruction rows itself, in
    `dt`; 'shared': it starts from the fp32 rows of ops.recon_wmse, as the HIP tail does."""
    x_reco, _, losses, _, mu, log_var, z = net.evaluate(x, y, with_beta=True, epsilon=eps, z_output=True)
    pr = net.encoder.prior
    N, L = x.shape[0], eps.shape[0] - 1
    D = x[0].numel()
    sg = net.sigma.to(dt)
    ls = sg if net.sigma.is_log else sg.log()
    if rows == 'shared':
        wmse_s = ops.recon_wmse(x_reco, x, net.sigma, ops.SIGMA_LOG if net.sigma.is_log else ops.SIGMA_VALUE).to(dt)
    else:
        wmse_s = (x_reco[1:].to(dt) - x.to(dt)).pow(2).flatten(2).mean(-1) * (-2 * ls).exp()         # (L, N)
    a = -0.5 * D * (wmse_s + 2 * ls + ic.LOG2PI)
    lab, means, T = pr._kernel_operands(y if pr.conditional else None, N, x.device)
    m, t = means.to(dt)[lab], T.to(dt)[lab]
    if pr.var_dim == 'scalar':
        t = t.unsqueeze(-1)
    dist = (t * (z[1:].to(dt) - m)).pow(2).sum(-1)
    slog = t.abs().log().sum(-1) if pr.var_dim == 'diag' else net.latent_dim * t.squeeze(-1).abs().log()
    q = (eps[1:].to(dt).pow(2) + log_var.to(dt)).sum(-1)
    lw = a + net.beta * (0.5 * (q - dist) + slog)
    top = lw.detach().max(0).values
    bound = top + (lw - top).exp().sum(0).log() - math.log(L)
    total = -bound
    if net.y_is_decoded and net.gamma:
        total = total + net.gamma * losses['cross_y'].to(dt)
    return total, bound


def grads_of(net, total):
    for p in net.parameters():
        p.grad = None
    total.mean().backward()
    lib.join_side_stream()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def gradient_ratios(net, x, y, eps, g_hip, rows):
    """-> (largest ratio, lines): per parameter max(|hip - torch32|, |hip - torch64|) / |torch32 - torch64|."""
    g32 = grads_of(net, torch_total(net, x, y, eps, torch.float32, rows)[0])
    t64, b64 = torch_total(net, x, y, eps, torch.float64, rows)
    g64 = grads_of(net, t64)
    assert set(g_hip) == set(g32) == set(g64)
    worst, lines = 0., []
    for k in sorted(g_hip):
        e_hip = float((g_hip[k] - g32[k]).abs().max())                            # the HIP tail against the torch fp32 expression
        e_h64 = float((g_hip[k].double() - g64[k].double()).abs().max())          # ... and against its fp64 tail
        e_t32 = float((g32[k].double() - g64[k].double()).abs().max())            # the torch fp32 expression's own error
        ratio = max(e_hip, e_h64) / e_t32 if e_t32 else (0. if max(e_hip, e_h64) == 0 else math.inf)
        worst = max(worst, ratio)
        lines.append('%-34s |hip - torch32| %.3e  |hip - torch64| %.3e  |torch32 - torch64| %.3e  ratio %.3f' % (
            k, e_hip, e_h64, e_t32, ratio))
    return worst, lines, b64.detach()


@pytest.mark.parametrize('L', [1, L_TRAIN], ids=lambda v: 'L%d' % v)
@pytest.mark.parametrize('name', list(MODELS))
def test_model_gradients_against_the_torch_expression(name, L):
    net, x, y, eps = build(name, L=L, objective='iwae')
    assert net.latent_sampling == L and (L > 1 or get_case(name.replace('_vae', ''))['net']['latent_sampling'] == 1)
    with captured_iw_bound() as calls:
        losses = net.evaluate(x, y, with_beta=True, epsilon=eps)[2]
    assert {'iwae', 'ess', 'kl', 'zdist', 'var_kl', 'wmse', 'cross_x', 'total'} <= set(losses)
    # the bound and the effective sample size the model reports: the restatement on the very operands the op was handed,
    # which must be the evaluation's own (the noise that made z, the labels, the prior's tensors)
    assert len(calls) == 1 and calls[0]['eps'].data_ptr() == net._last_epsilon.data_ptr()
    assert torch.equal(calls[0]['eps'], eps[1:]) and calls[0]['z'].shape == (L + 1, x.shape[0], net.latent_dim)
    assert calls[0]['beta'] == net.beta and calls[0]['var_dim'] == net.encoder.prior.var_dim
    c, d, r, B = restate_calls(calls)
    hold(c, dict(bound=losses['iwae'], ess=losses['ess']), r, B, keys=['bound', 'ess'])
    g_hip = grads_of(net, losses['total'])
    assert any('encoder.dense_log_var' in k for k in g_hip) and any('imager' in k for k in g_hip)
    bound_hip = losses['iwae'].detach().double()
    net.TRAIN_OBJECTIVE = 'elbo'
    held = 'own' if L == 1 else 'shared'
    worst, lines, b64 = gradient_ratios(net, x, y, eps, g_hip, held)
    print('\n'.join(lines))
    print(name, 'L', L, 'rows', held, 'bound |hip - torch64| %.3e' % float((bound_hip - b64).abs().max()),
          'mean ess %.3f' % float(losses['ess'].mean()), 'largest ratio %.3f (allowed 4)' % worst)
    if L > 1:         # measured, not held: the torch tails form their own rows - the ratio of two roundings of the rows
        own, _, _ = gradient_ratios(net, x, y, eps, g_hip, 'own')
        print(name, 'L', L, 'rows own: largest ratio %.3f (shared rows: %.3f)' % (own, worst))
    assert worst <= 4, (name, L, worst)


def params_of(net):
    return {k: p.detach().clone() for k, p in net.named_parameters()}


def three_steps(objective):
    net, x, y, eps = build('c1_n16_mlp', L=L_TRAIN, objective=objective)
    before = params_of(net)
    seen = []
    for i in range(3):
        losses, _ = net.train_step(x, y, batch=i, epsilon=eps)
        seen.append(set(losses))
    torch.cuda.synchronize()
    return net, before, params_of(net), seen


def test_three_iwae_steps_move_every_parameter_and_repeat_bit_for_bit():
    net, before, after, seen = three_steps('iwae')
    assert all({'iwae', 'ess'} <= s for s in seen)
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    assert trainable
    for k in trainable:
        assert bool(torch.isfinite(after[k]).all()), k
        assert not torch.equal(after[k], before[k]), k + ' did not move'
    _, before2, after2, _ = three_steps('iwae')
    for k in after:
        assert torch.equal(before[k], before2[k]) and torch.equal(after[k], after2[k]), k


def test_default_objective_is_the_parents_step_bit_for_bit():
    """A model that never touches TRAIN_OBJECTIVE against one that sets the default by hand: the same parameters, bit for bit,
    and no new key in its losses; switched to 'iwae', the second model then takes another road."""
    _, _, plain, seen = three_steps(None)
    net, _, explicit, seen2 = three_steps('elbo')
    assert all('iwae' not in s and 'ess' not in s for s in seen + seen2) and seen == seen2
    for k in plain:
        assert torch.equal(plain[k], explicit[k]), k
    assert 'objective' not in net.training_parameters
    net.TRAIN_OBJECTIVE = 'iwae'
    x, y, eps = build('c1_n16_mlp', L=L_TRAIN)[1:]
    losses, _ = net.train_step(x, y, epsilon=eps)
    assert 'iwae' in losses and 'ess' in losses


# ============================================================================================ net.iw_bound
def eval_net(name='c1_n16_mlp'):
    net, x, y, _ = build(name, L=1)
    net.eval()
    return net, x, (y if net.encoder.prior.conditional else None)


def test_net_iw_bound_in_one_slab_and_in_slabs_of_two(monkeypatch):
    net, x, y = eval_net()
    N, K, L = x.shape[0], net.latent_dim, 7
    eps = det_inputs(N, net.input_shape, 10, L, K, seed=7)[2].to(DEV)
    with captured_iw_bound() as rec1:
        b1, e1 = net.iw_bound(x, y, samples=L, epsilon=eps)
    monkeypatch.setenv('JVAE_EVAL_SLAB_ROWS', str(3 * N))                         # three decoder rows per image: two draws
    with captured_iw_bound() as rec2:
        b2, e2 = net.iw_bound(x, y, samples=L, epsilon=eps)
    monkeypatch.delenv('JVAE_EVAL_SLAB_ROWS')
    assert len(rec1) == 1 and [r['eps'].shape[0] for r in rec2] == [2, 2, 2, 1]
    assert not net.training and b1.shape == (N,) and e1.shape == (N,)
    c, d, r, B = restate_calls(rec1)
    assert c.L == L and c.beta == 1.
    hold(c, dict(bound=b1, ess=e1), r, B, keys=['bound', 'ess'])                  # equals the restatement on its own tensors
    # one slab against slabs of two: the merge's derived bound (test_state_merges_slabs_of_draws) plus, the logsumexp moving by
    # no more than its inputs do, the largest difference between the two runs' log w (zero when the decoder gives a row the same
    # bits in a batch of 8 N rows and of 3 N)
    c2, d2, r2, _ = restate_calls(rec2)
    moved = float((r['log_w'] - r2['log_w']).abs().max())
    M = r['log_w'].max(0).values.abs()
    logS = (r['bound'] + math.log(L) - r['log_w'].max(0).values).abs()
    ends = 2 * (logS + math.log(L)) + 2 * (M + logS + math.log(L)) + 1
    Bm = (102 + ic.n_S(L)) + (102 + ic.n_S(2) + 4 * 104) + 2 * ends
    err = (b1.double() - b2.double()).abs().cpu()
    print('one slab / slabs of two: log w moved by %.3e; measured / bound %.3f' % (moved, float((err / (ic.U * Bm + moved)).max())))
    assert bool((err <= ic.U * Bm + moved).all())


def test_net_iw_bound_tightens_with_the_draws_and_serves_a_single_prior():
    net, x, y = eval_net()
    torch.manual_seed(11)
    b1 = net.iw_bound(x, y, samples=1)[0].mean()
    b64, e64 = net.iw_bound(x, y, samples=64)
    print('mean bound over 16 images: L = 1 %.4f   L = 64 %.4f   mean ess at 64 %.2f' % (float(b1), float(b64.mean()), float(e64.mean())))
    assert float(b64.mean()) >= float(b1) and bool((e64 >= 1).all()) and bool((e64 <= 64 * (1 + 1e-5)).all())
    with pytest.raises(ValueError, match='labels y'):
        net.iw_bound(x)
    vae, xv, yv = eval_net('c1_n16_mlp_vae')
    assert yv is None
    bv, ev = vae.iw_bound(xv, samples=5)
    assert bv.shape == (16,) and bool(torch.isfinite(bv).all()) and bool((ev >= 1).all())
    with pytest.raises(ValueError, match='must be None'):
        vae.iw_bound(xv, torch.zeros(16, dtype=torch.int64, device=DEV))


def test_coded_sigma_model_trains_and_scores():
    """The coded sigma kind through the model: log sigma_n comes out of the encoder, so its gradient (-D g_n, per sample) must
    reach the sigma head; net.iw_bound reads the same head without storing into the parameter."""
    net, x, y, eps = build('c2_n8_coded', L=L_TRAIN, objective='iwae')
    before = net.sigma.detach().clone()
    losses = net.evaluate(x, y, with_beta=True, epsilon=eps)[2]
    assert bool(torch.isfinite(losses['iwae']).all()) and bool((losses['ess'] >= 1).all())
    grads = grads_of(net, losses['total'])
    head = [k for k in grads if k.startswith('encoder.sigma.')]
    assert head and all(bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0 for k in head)
    after_train = net.sigma.detach().clone()
    b, e = net.iw_bound(x, y, samples=5)
    assert net.training and torch.equal(net.sigma.detach(), after_train) and before.shape == after_train.shape
    assert b.shape == (8,) and bool(torch.isfinite(b).all()) and bool((e >= 1).all()) and bool((e <= 5 * (1 + 1e-5)).all())


# ============================================================================================ refusals
@pytest.mark.parametrize('row', ic.refusal_table(), ids=lambda r: r[0])
def test_every_refusal_raises_by_name(row):
    name, kwargs, tweak, ev_kw, word = row
    m = ic.refusal_model(kwargs, tweak, device=DEV)
    x = torch.rand(4, *m.input_shape, device=DEV)
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'iwae'.*" + word):
        m.train_step(x, y, **ev_kw)
    if name == 'train_captured':
        for who in (m.graph_train_step, m.capture_train_step):
            with pytest.raises(NotImplementedError, match='TRAIN_OBJECTIVE.*' + who.__name__):
                who(x, y)
    if name in ('tilted', 'full_variance', 'rmse_sigma', 'bf16', 'jvae'):        # net.iw_bound refuses the same about the model
        with pytest.raises(NotImplementedError, match='iw_bound'):
            m.iw_bound(x, y)
