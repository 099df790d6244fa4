"""The likelihood regret (cvae.likelihood_regret) restated twice, without the code under test (no GPU):

`refine_step_restatement`  one launch of csrc/latent.hip::latent_refine_kernel - gradient, Adam step, forward of the next
                           iteration - in torch fp64 with the derivatives WRITTEN OUT from the formulas of the priors; held here
                           to torch.autograd + torch.optim.Adam on leaf (mu, lv_raw) tensors.  It is the checker of the kernel
                           tests of tests/test_27_regret_gpu.py.
`regret_restatement`       the whole loop in plain torch on the functional model of oracle/jvae_oracle.py (run_stack,
                           recon_terms, prior_kl) with torch.optim.Adam; tools/gen_regret_golden.py runs it in fp64 and fp32 and
                           writes tests/golden/regret/*.npz, which this file re-derives.

oracle/jvae_oracle.py::make_spec restates type 'cvae' only; the eval-mode forward of the three types is written out here as
tests/test_odin_restatement.py does for vib (the key / shape list of the state comes from the drop-in on the CPU)."""
import contextlib
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import jvae_oracle as O
from oracle.cases import get_case
from test_odin_restatement import det_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden', 'regret')
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
PRIORS = [('gaussian', 'scalar'), ('gaussian', 'diag'), ('gaussian', 'full'), ('tilted', 'scalar'), ('uniform', 'scalar')]


def uniform_alpha(tau):
    return math.log(2 * tau) - math.log(2 * (0.5 * (1 + math.erf(tau / math.sqrt(2)))) - 1)


# ------------------------------------------------------------------------------------------- one refinement step
def _prior_terms(mu, lv, y, means, T, prior, var_dim, tau):
    """-> (kl (N,), zdist (N,), dkl/dmu (N, K), dkl/dlv (N, K)) of KL(N(mu, exp lv) || p(z | y)), both weights 1, from the
    formulas of module/priors.py; T is the WHITENING factor (precision = T^T T)."""
    K = mu.shape[1]
    d = mu - means[y]
    if prior == 'uniform':
        c, alpha = math.log(2 * math.pi), uniform_alpha(tau)
        span = 2 * math.sqrt(3) * torch.exp(0.5 * lv)
        lo, hi = (d - 0.5 * span) / tau, (d + 0.5 * span) / tau
        a, b = tau * lo.clamp(-1, 1), tau * hi.clamp(-1, 1)
        da, db = ((lo > -1) & (lo < 1)).to(mu.dtype), ((hi > -1) & (hi < 1)).to(mu.dtype)
        coef = alpha - 0.5 * c
        elogq = -0.5 * lv - 0.5 * math.log(12)
        nel = (c + d * d + span * span / 12) / 2 + coef * (b - a) / span - (b ** 3 - a ** 3) / span / 6
        first, vk = elogq.sum(1) + nel.sum(1), elogq.sum(1) + K * alpha
        took_first = (first >= vk).to(mu.dtype)[:, None]
        dnel_da = -coef / span + a * a / (2 * span)
        dnel_db = coef / span - b * b / (2 * span)
        dnel_dspan = span / 12 - coef * (b - a) / span ** 2 + (b ** 3 - a ** 3) / (6 * span ** 2) - 0.5 * dnel_da * da + 0.5 * dnel_db * db
        g_mu = took_first * (d + dnel_da * da + dnel_db * db)
        g_lv = took_first * dnel_dspan * 0.5 * span - 0.5
        return torch.maximum(first, vk), (d * d).sum(1), g_mu, g_lv
    if var_dim == 'scalar':
        t = T[y][:, None]
        wd, Td, pd, logdet_p = d * t, t * t * d, (t * t).expand_as(d), -2 * K * torch.log(T[y])
    elif var_dim == 'diag':
        t = T[y]
        wd, Td, pd, logdet_p = d * t, t * t * d, t * t, -2 * torch.log(t.abs()).sum(1)
    else:
        Tc = T[y].tril()
        wd = torch.einsum('nkj,nj->nk', Tc, d)
        Td = torch.einsum('nik,ni->nk', Tc, wd)
        pd = (Tc * Tc).sum(1)
        logdet_p = -2 * torch.log(torch.diagonal(Tc, dim1=1, dim2=2).abs()).sum(1)
    dist = (wd * wd).sum(1)
    if prior == 'tilted':
        r = dist.sqrt()
        return 0.5 * (r - tau) ** 2, dist, (1 - tau / r)[:, None] * Td, torch.zeros_like(lv)
    var_kl = (torch.exp(lv) * pd).sum(1) - lv.sum(1) + logdet_p - K
    return 0.5 * (dist + var_kl), dist, Td, 0.5 * (torch.exp(lv) * pd - 1)


def refine_step_restatement(mu, raw, eps_cur, eps_next, y, means, T, dz, state, step, lr, prior='gaussian', var_dim='scalar',
                            tau=0., sampled=True, forced_lv=None):
    """One refinement launch in fp64.  mu, raw (N, K) (raw None with forced_lv); eps_* (L+1, N, K); dz (L+1, N, K) the decoder's
    part of the gradient; state = (m_mu, v_mu, m_lv, v_lv).  dz None: the forward alone.  -> dict(mu, raw, lv, z, kl, zdist,
    g_mu, g_lv, state): the moved posterior, the forward at it with eps_next, and the gradients the step used."""
    s = float(bool(sampled))
    clip = (lambda r: torch.full_like(mu, forced_lv)) if forced_lv is not None else (lambda r: r.clamp(-20, 20))
    out = {}
    if dz is not None:
        lv = clip(raw)
        _, _, g_mu, g_lv = _prior_terms(mu, lv, y, means, T, prior, var_dim, tau)
        g_mu = g_mu + dz.sum(0)
        g_lv = g_lv + (dz * 0.5 * torch.exp(0.5 * lv) * eps_cur * s).sum(0)
        if forced_lv is not None:
            g_lv = torch.zeros_like(g_lv)
        else:
            g_lv = g_lv * ((raw >= -20) & (raw <= 20)).to(mu.dtype)

        def adam(p, g, m, v):
            m = B1 * m + (1 - B1) * g
            v = B2 * v + (1 - B2) * g * g
            return p - lr / (1 - B1 ** step) * m / (v.sqrt() / math.sqrt(1 - B2 ** step) + ADAM_EPS), m, v
        mu, m_mu, v_mu = adam(mu, g_mu, state[0], state[1])
        m_lv, v_lv = state[2], state[3]
        if forced_lv is None:
            raw, m_lv, v_lv = adam(raw, g_lv, m_lv, v_lv)
        out.update(g_mu=g_mu, g_lv=g_lv, state=(m_mu, v_mu, m_lv, v_lv))
    lv = clip(raw)
    out.update(mu=mu, raw=raw, lv=lv)
    if eps_next is not None:
        kl, zdist = _prior_terms(mu, lv, y, means, T, prior, var_dim, tau)[:2]
        out.update(z=mu + torch.exp(0.5 * lv) * eps_next * s, kl=kl, zdist=zdist)
    return out


def decoder_gradient(L, N, K, g):
    """A stand-in for d(sum cross_x)/dz (L+1, N, K), row 0 zero: random signs, magnitudes in [0.5, 1.5) / (L + 1).  Bounded
    away from zero on purpose: with L = 1 and a prior whose KL has no log-variance gradient (tilted) that gradient is the
    PRODUCT dz * sd * eps / 2, and the product of two normal draws falls below 1e-3 of the largest in 5 % of the elements."""
    u = torch.rand(L + 1, N, K, generator=g, dtype=torch.float64)
    dz = (0.5 + u) * torch.where(torch.rand(L + 1, N, K, generator=g, dtype=torch.float64) < 0.5, -1., 1.) / (L + 1)
    dz[0] = 0
    return dz


def step_case(prior, var_dim, N, K, L, seed, forced=False, warm=True, C=5):
    """Random fp64 inputs of one refinement step; a log-variance exactly at the lower clip (its gradient passes; at the upper
    one it would be e^20 and the only figure a max-norm sees), one beyond it on either side (the upper one in the LAST sample,
    whose z and kl it dominates)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    mu, raw = rnd(N, K), 0.3 * rnd(N, K)      # variances within a factor of a few: the gradients of a case stay near-normal
    raw[0, 0] = -20.
    if K > 1:
        raw[0, 1] = -30.
    if N > 1:
        raw[N - 1, 0] = 25.
    eps_cur, eps_next, dz = rnd(L + 1, N, K), rnd(L + 1, N, K), decoder_gradient(L, N, K, g)
    eps_cur[0], eps_next[0] = 0, 0
    y = torch.randint(0, C, (N,), generator=g)
    means = 0.5 * rnd(C, K)
    T = {'scalar': lambda: 1 + 0.2 * (2 * torch.rand(C, generator=g, dtype=torch.float64) - 1),
         'diag': lambda: 1 + 0.2 * (2 * torch.rand(C, K, generator=g, dtype=torch.float64) - 1),
         'full': lambda: torch.eye(K, dtype=torch.float64) + 0.05 * rnd(C, K, K)}[var_dim]()
    if warm:
        state = (0.3 * rnd(N, K), 0.5 + torch.rand(N, K, generator=g, dtype=torch.float64),
                 0.3 * rnd(N, K), 0.5 + torch.rand(N, K, generator=g, dtype=torch.float64))
    else:
        state = tuple(torch.zeros(N, K, dtype=torch.float64) for _ in range(4))
    tau = {'tilted': 5., 'uniform': 1.5}.get(prior, 0.)
    if prior == 'uniform':
        # An element of variance e^-20 whose interval lies INSIDE the support has, in the shared fp32 body (training included),
        # a mean gradient d + (a^2 - b^2) / (2 span) that cancels to 2^-24 tau^2 / span ~ 6e-4: no fp32 bar of the latent
        # kernel applies to it.  The two clipped elements sit outside the support instead (a = b = +-tau: nothing cancels).
        mu[0, 0] = means[y[0], 0] + 2 * tau
        if K > 1:
            mu[0, 1] = means[y[0], 1] - 2 * tau
    return dict(mu=mu, raw=None if forced else raw, eps_cur=eps_cur, eps_next=eps_next, y=y, means=means, T=T, dz=dz, state=state,
                prior=prior, var_dim=var_dim, tau=tau, forced_lv=math.log(0.3) if forced else None)


def autograd_adam_step(c, step, lr):
    """The same step by torch.autograd (KL from the oracle's prior_kl, the decoder's part as <dz, z>) and torch.optim.Adam."""
    forced = c['forced_lv'] is not None
    mu = c['mu'].clone().requires_grad_(True)
    raw = (torch.zeros_like(mu) if forced else c['raw'].clone()).requires_grad_(True)
    opt = torch.optim.Adam([mu, raw], lr=lr, betas=(B1, B2), eps=ADAM_EPS)
    for p, (m, v) in ((mu, c['state'][:2]), (raw, c['state'][2:])):
        opt.state[p] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
    lv = torch.full_like(mu, c['forced_lv']) if forced else raw.clamp(-20, 20)
    z = mu + torch.exp(0.5 * lv) * c['eps_cur']
    sp = dict(K=mu.shape[1], prior=dict(distribution=c['prior'], tau=c['tau'], var_dim=c['var_dim']))
    kd = O.prior_kl(sp, {'encoder.prior.mean': c['means'], 'encoder.prior._var_parameter': c['T']}, mu, lv, c['y'], 1.0)
    ((c['dz'] * z).sum() + kd['kl'].sum()).backward()
    if forced:
        raw.grad = None                       # only mu moves
    g_mu, g_lv = mu.grad.clone(), None if forced else raw.grad.clone()
    opt.step()
    return mu.detach(), None if forced else raw.detach(), g_mu, g_lv, kd


def _rel(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@pytest.mark.parametrize('forced', [False, True])
@pytest.mark.parametrize('warm', [True, False])
@pytest.mark.parametrize('prior,var_dim', PRIORS)
def test_refine_step_restatement(prior, var_dim, warm, forced):
    """The written-out derivatives and the Adam arithmetic against torch's own, to 1e-10 relative: every prior kind, forced
    variance, log-variances at and beyond the clip; warm state at step 10 and zero state at step 1."""
    for N, K, L in ((5, 7, 2), (3, 1, 1), (6, 33, 3)):
        c = step_case(prior, var_dim, N, K, L, seed=N * 100 + K + L, forced=forced, warm=warm)
        step, lr = (10 if warm else 1), 0.05
        got = refine_step_restatement(step=step, lr=lr, **c)
        mu, raw, g_mu, g_lv, kd = autograd_adam_step(c, step, lr)
        assert _rel(got['g_mu'], g_mu) < 1e-10 and _rel(got['mu'], mu) < 1e-10
        if not forced:
            assert _rel(got['g_lv'], g_lv) < 1e-10 and _rel(got['raw'], raw) < 1e-10
            assert float(got['g_lv'][0, 0]) != 0. or prior == 'tilted'             # AT the clip the gradient passes
            if K > 1:
                assert float(got['g_lv'][0, 1]) == 0.                              # beyond it: none
        else:
            assert got['raw'] is None and torch.equal(got['lv'], torch.full_like(mu, c['forced_lv']))
        # the forward of the next iteration, at the moved posterior, against the oracle's prior_kl
        sp = dict(K=K, prior=dict(distribution=prior, tau=c['tau'], var_dim=var_dim))
        kd = O.prior_kl(sp, {'encoder.prior.mean': c['means'], 'encoder.prior._var_parameter': c['T']}, got['mu'], got['lv'],
                        c['y'], 1.0)
        assert _rel(got['kl'], kd['kl']) < 1e-10 and _rel(got['zdist'], kd['distance']) < 1e-10
        assert _rel(got['z'], got['mu'] + torch.exp(0.5 * got['lv']) * c['eps_next']) < 1e-15
        only = refine_step_restatement(**dict(c, dz=None), step=0, lr=0.)          # the first draw of a loop: nothing moves
        assert torch.equal(only['mu'], c['mu']) and 'state' not in only


# ------------------------------------------------------------------------------------------- the whole loop
def regret_cases():
    """name -> (model kwargs, N).  L = 2 evaluation draws; the conv geometry of the a2_n8_vae / e2_n8 goldens."""
    conv = dict(get_case('e2_n8_L3')['net'], test_latent_sampling=2)
    vae = dict(get_case('ea2_n8_vae_L3')['net'], test_latent_sampling=2)
    diag = dict(conv, prior=dict(distribution='gaussian', init_mean=0., learned_means=True, var_dim='diag', freeze_means=0))
    mlp = dict(conv, input_shape=(1, 28, 28), features=None, upsampler=None, encoder=[64], decoder=[48], batch_norm=False,
               latent_dim=16, sigma={'value': 0.5})
    return {'ra2_n6_vae': (vae, 6), 're2_n6_cvae': (conv, 6), 're2_n6_cvae_leaky': (dict(conv, activation='leaky'), 6),
            'rm2_n6_cvae_mlp': (mlp, 6), 're2_n6_cvae_diag': (diag, 6)}


STEPS, LR = 3, 0.05


def regret_state(kw, dtype):
    """The deterministic state of the model (oracle/det_init.py); sigma keeps its constructor value, as load_det_state leaves it."""
    P = det_state(kw, dtype)
    sg = kw['sigma']
    P['sigma'] = torch.full((1,), math.log(sg['value']) if sg.get('learned') else float(sg['value']), dtype=dtype)
    return P


@contextlib.contextmanager
def watch_activations(seen):
    """Record the input of every hidden activation the oracle's stacks apply (their `_act`) while the block runs."""
    real = O._act

    def spy(x, name):
        if name in ('relu', 'leaky') and seen is not None:
            seen.append(x.detach())
        return real(x, name)
    O._act = spy
    try:
        yield
    finally:
        O._act = real


def _encode(kw, P, x):
    act, h = kw.get('activation', 'relu'), x
    if kw.get('features'):
        layers = O.parse_stack(kw['features'], kw['input_shape'], False)
        h = O.run_stack(P, 'features', layers, kw['batch_norm'] in ('encoder', 'both'), x, None, training=False, hidden_act=act)
    h = h.flatten(1)
    for i in range(len(kw['encoder'])):
        h = O._act(F.linear(h, P[f'encoder.dense_projs.{2 * i}.weight'], P[f'encoder.dense_projs.{2 * i}.bias']), act)
    return (F.linear(h, P['encoder.dense_mean.weight'], P['encoder.dense_mean.bias']),
            F.linear(h, P['encoder.dense_log_var.weight'], P['encoder.dense_log_var.bias']))


def _decode(kw, P, z):
    """z (L+1, N, K) -> x_reco (L+1, N, *input_shape), eval mode."""
    act, h = kw.get('activation', 'relu'), z
    for i in range(len(kw['decoder'])):
        h = O._act(F.linear(h, P[f'decoder.{2 * i}.weight'], P[f'decoder.{2 * i}.bias']), act)
    if kw.get('upsampler'):
        hw = O.find_imager_hw(kw['upsampler'], kw['input_shape'][1:])
        shape = (h.shape[-1] // (hw[0] * hw[1]), *hw)
        layers = O.parse_stack(kw['upsampler'], shape, True)
        xr = O.run_stack(P, 'imager', layers, bool(kw.get('features')) and kw['batch_norm'] == 'both', h.reshape(-1, *shape),
                         kw['output_activation'], training=False, hidden_act=act)
    else:
        xr = O._act(F.linear(h, P['imager.0.weight'], P['imager.0.bias']), kw['output_activation'])
    return xr.reshape(*z.shape[:2], *kw['input_shape'])


def regret_restatement(kw, P, x, y, eps, steps, lr, seen=None):
    """-> (regret (N,), [(mu_t, lv_t, J_t) for t = 0 .. steps]).  eps (steps + 1, L, N, K); y (N,) classes (ignored by a single
    prior).  J = mean_l(-log p(x | z_l)) + KL(q || p(z | y)) = cross_x + kl of the oracle's evaluate(with_beta=False).
    `seen`: a list that receives, per iteration, the list of the decoder's hidden pre-activations of the gradient pass."""
    N, K = x.shape[0], kw['latent_dim']
    L, D = eps.shape[1], int(np.prod(kw['input_shape']))
    sp = dict(K=K, prior=dict(kw['prior']), sigma=dict(kw['sigma']), input_shape=tuple(kw['input_shape']))
    mean, vp = P['encoder.prior.mean'].reshape(-1, K), P['encoder.prior._var_parameter']
    Pk = {'encoder.prior.mean': mean, 'encoder.prior._var_parameter': vp.reshape(1) if vp.ndim == 0 else vp, 'sigma': P['sigma']}
    y = y if mean.shape[0] > 1 else torch.zeros_like(y)
    with torch.no_grad():
        mu0, raw0 = _encode(kw, P, x)

    def J(mu, raw, e, watch=None):
        lv = raw.clip(-20, 20)
        z = torch.cat((mu[None], mu[None] + torch.exp(0.5 * lv)[None] * e), 0)
        with watch_activations(watch):
            x_reco = _decode(kw, P, z)
        _, wmse, _, log_sigma, _ = O.recon_terms(sp, Pk, None, x, x_reco, L, N, False)
        cross_x = D * (2 * log_sigma + wmse + math.log(2 * math.pi)) / 2
        return cross_x + O.prior_kl(sp, Pk, mu, lv, y, 1.0)['kl']
    mu, raw = mu0.clone().requires_grad_(True), raw0.clone().requires_grad_(True)
    opt = torch.optim.Adam([mu, raw], lr=lr, betas=(B1, B2), eps=ADAM_EPS)
    traj = []
    for t in range(steps):
        opt.zero_grad()
        watch = [] if seen is not None else None
        Jt = J(mu, raw, eps[t], watch)
        traj.append((mu.detach().clone(), raw.detach().clip(-20, 20), Jt.detach().clone()))
        if seen is not None:
            seen.append(watch)
        Jt.sum().backward()
        opt.step()
    with torch.no_grad():
        J_end = J(mu, raw, eps[steps])
        traj.append((mu.detach().clone(), raw.detach().clip(-20, 20), J_end))
        return J(mu0, raw0, eps[steps]) - J_end, traj


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def left_out(gd):
    """Samples with a decoder ReLU unit closer to zero, in the fp64 run of any iteration, than the fp32 forward error there: their
    gradient is the other side's in fp32 and the trajectories part.  The goldens' seeds keep them to at most 1 of the N."""
    out = (gd['preact_min64'] < gd['preact_err32']).any(0)
    assert out.sum() <= 1
    return out


@pytest.mark.parametrize('name', sorted(regret_cases()))
def test_regret_restatement_reproduces_the_golden(name):
    """fp64: trajectory and regret at fp64 rounding; fp32: inside the golden's own fp32-vs-fp64 distance (a few of it: another
    thread count sums in another order).  The regret is positive on average: three Adam steps improve the sample's own ELBO."""
    kw, N = regret_cases()[name]
    gd = load_golden(name)
    x, y, eps = torch.from_numpy(gd['x']), torch.from_numpy(gd['y']), torch.from_numpy(gd['eps'])
    assert int(gd['steps']) == STEPS and float(gd['lr']) == LR and x.shape[0] == N
    reg, traj = regret_restatement(kw, regret_state(kw, torch.float64), x.double(), y, eps.double(), STEPS, LR)
    keep = ~left_out(gd)
    assert _rel(reg, torch.from_numpy(gd['regret64'])) < 1e-9
    for t, (mu, lv, J) in enumerate(traj):
        assert _rel(mu, torch.from_numpy(gd['mu64'][t])) < 1e-9 and _rel(lv, torch.from_numpy(gd['lv64'][t])) < 1e-9
        assert _rel(J, torch.from_numpy(gd['J64'][t])) < 1e-9
    reg32, traj32 = regret_restatement(kw, regret_state(kw, torch.float32), x, y, eps, STEPS, LR)
    for key, got in (('mu', torch.stack([t[0] for t in traj32])), ('lv', torch.stack([t[1] for t in traj32])),
                     ('J', torch.stack([t[2] for t in traj32])), ('regret', reg32)):
        ref = torch.from_numpy(gd[key + '64'])
        d = _rel(got.double()[keep], ref[keep]) if key == 'regret' else _rel(got.double()[:, keep], ref[:, keep])
        print(name, key, 'fp32 distance', d, 'golden', float(gd['d_ref_' + key]))
        assert d <= 4 * float(gd['d_ref_' + key]) + 1e-7
    assert float(gd['regret64'].mean()) > 0


def test_abi_of_the_refinement_entry():
    """include/jvae_hip.h, the ctypes table of jvae_hip/lib.py and the built library agree on jvae_latent_refine_f32."""
    import ctypes
    from jvae_hip import lib
    name = 'jvae_latent_refine_f32'
    with open(os.path.join(REPO, 'include', 'jvae_hip.h')) as f:
        decl = re.search(r'^int ' + name + r'\(([^;]*)\);', f.read(), re.M | re.S)
    assert decl, name + ' is not declared in include/jvae_hip.h'
    params = [p.strip() for p in decl.group(1).split(',')]
    table = next(v for v in vars(lib).values() if isinstance(v, dict) and 'jvae_latent_fwd_f32' in v)
    assert name in table, name + ' is not bound in jvae_hip/lib.py'
    restype, argtypes = table[name]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 32
    kinds = {'int': ctypes.c_int, 'float': ctypes.c_float, 'long': ctypes.c_long}
    for p, a in zip(params, argtypes):
        want = ctypes.c_void_p if '*' in p else kinds[p.split()[0]]
        assert a is want, (p, a)
    so = os.path.join(os.path.dirname(lib.__file__), 'libjvae_hip.so')
    if os.path.exists(so):                    # built: the symbol is exported, and refuses a call without pointers by its code
        with open(so, 'rb') as f:
            assert name.encode() in f.read()


def test_names_and_the_switch():
    """`regret-<steps>-<lr:.4f>` names; off: refused by name, 'all' untouched; on: 'all' and 'regret*' expand on cvae / vae / xvae."""
    from cvae import ClassificationVariationalNetwork as Net
    from module import score_rows
    assert Net.OOD_REGRET_METHODS is False and all(len(p) == 2 for p in Net.REGRET_PARAMS)
    kw = regret_cases()['rm2_n6_cvae_mlp'][0]
    net = Net(**kw)
    net.REGRET_PARAMS = [(3, 0.05), (10, 0.001)]
    names = ['regret-3-0.0500', 'regret-10-0.0010']
    assert net._regret_names() == names
    before = net._ood_methods('all')
    assert not any(m.startswith('regret') for m in before)
    for m in ('regret*', names[0]):
        with pytest.raises(NotImplementedError, match='regret'):
            net._ood_methods(m)
    with pytest.raises(NotImplementedError, match=names[0]):
        score_rows.parse(names[0], score_rows.traits_of(net))
    net.OOD_REGRET_METHODS = True
    assert net._ood_methods('all') == before + names and net._ood_methods('regret*') == names
    assert net._ood_methods(['elbo', names[1]]) == ['elbo', names[1]]
    with pytest.raises(ValueError):
        net._ood_methods('regret-4-0.0500')
    row = score_rows.parse(names[0], score_rows.traits_of(net))
    assert row.source == names[0] and row.kind is None and row.roc_mode is False
    vib = Net(**dict(get_case('eb2_n8_vib_L2')['net']))
    vib.OOD_REGRET_METHODS = True
    assert not any(m.startswith('regret') for m in vib._ood_methods('all'))
    with pytest.raises(NotImplementedError, match='regret'):
        vib._ood_methods('regret*')
