"""tests/tail_cases.py held to account on the CPU: its fp64 references agree (in fp32, at the tolerances of test_0_ops_gpu.py) with
oracle.jvae_oracle and with torch's own ops; the fp32 restatement of EVERY case lies inside its bound - the condition that keeps
tests/test_35_loss_tail_sweep_gpu.py honest; every planted mistake leaves the bound on at least one case - the condition that
makes it worth running; and the branch conditions the references rely on hold with a margin, so that no case needs an
exclusion."""
import math

import pytest
import torch
import torch.nn.functional as F

import tail_cases as tc
from oracle import jvae_oracle as O

F32, F64 = torch.float32, torch.float64
_cache = {}


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def ref64(fam, c):
    key = (fam.name, c.name)
    if key not in _cache:
        d = fam.make(c)
        r = fam.ref(c, d, F64)
        _cache[key] = (d, r, fam.bound(c, d, r))
    return _cache[key]


def worst(got, r, b):
    return max(tc.excess(got[k], r[k], b[k]) for k in r if k[0] != '_')


# ---------------------------------------------------------------------------------------------- every case inside its bound
@pytest.mark.parametrize('fam', tc.FAMILIES, ids=lambda f: f.name)
def test_fp32_restatement_lies_inside_every_bound(fam):
    for c in fam.cases:
        d, r, b = ref64(fam, c)
        assert set(b) | {'_aux'} >= set(r), (c, set(r) - set(b))
        r32 = fam.ref(c, d, F32)
        for k in (k for k in r if k[0] != '_'):
            assert r32[k].dtype == F32 and torch.isfinite(r[k]).all(), (c, k)
            e = tc.excess(r32[k], r[k], b[k])
            assert e <= 1, (c, k, e)


@pytest.mark.parametrize('fam,plant', [(f, p) for f in tc.FAMILIES for p in f.plants], ids=lambda v: getattr(v, 'name', v))
def test_every_planted_mistake_leaves_the_bound(fam, plant):
    hit = 0.
    for c in fam.cases:
        d, r, b = ref64(fam, c)
        hit = max(hit, worst(fam.ref(c, d, F64, plant), r, b))
        if hit > 1:
            return
    assert hit > 1, (fam.name, plant, hit)


def test_intrinsic_allowance_is_the_measured_one():
    """EXP_ULPS / LOG_ULPS are 4 times what torch's CPU fp32 exp / log lose against fp64 over this module's own arguments."""
    tc.EXP_ARGS.clear()
    tc.LOG_ARGS.clear()
    for fam in tc.FAMILIES:
        for c in fam.cases:
            fam.ref(c, fam.make(c), F64)
    e, l = tc.measure_intrinsics()
    print(f'measured: exp {e:.3f} ulp, log {l:.3f} ulp')
    assert e <= tc.EXP_MEASURED <= e + 0.01 and l <= tc.LOG_MEASURED <= l + 0.01, (e, l)
    assert tc.EXP_ULPS == 4 * tc.EXP_MEASURED and tc.LOG_ULPS == 4 * tc.LOG_MEASURED


# ---------------------------------------------------------------------------------------------- optimiser (stateful families)
def _opt_run(c, dt, plant=None, local=True):
    """STEPS steps; local: every step starts from the fp32 state of the fp64 reference of the step before (rounded)."""
    d = tc.opt_make(c)
    st = tc.opt_state0(c, d)
    out = []
    for i, g in enumerate(d['grads']):
        sq = g.double().square().sum().float().reshape(1) if c.max_norm > 0 else None
        r = tc.opt_step_ref(c, st, g, sq, i, F64)
        got = tc.opt_step_ref(c, st, g, sq, i, dt, plant)
        out.append((r, got, tc.opt_step_bound(c, st, g, sq, i, r)))
        st = {k: v.float() for k, v in r.items()}
    return out


@pytest.mark.parametrize('c', tc.OPT_CASES, ids=tc.ids)
def test_optimiser_fp32_restatement_inside_bound(c):
    for i, (r, got, b) in enumerate(_opt_run(c, F32)):
        for k in r:
            e = tc.excess(got[k], r[k], b[k])
            assert e <= 1, (c, i, k, e)


@pytest.mark.parametrize('plant', tc.OPT_PLANTS)
def test_optimiser_plants(plant):
    hit = 0.
    for c in tc.OPT_CASES:
        if c.n == 0 or c.n > 2000:
            continue
        for r, got, b in _opt_run(c, F64, plant):
            hit = max(hit, worst(got, r, b))
    assert hit > 1, (plant, hit)


@pytest.mark.parametrize('c', [c for c in tc.OPT_CASES if c.n == 1023 and c.step0 == 1], ids=tc.ids)
def test_optimiser_reference_is_torchs(c):
    """Free-running fp32 restatement against torch.optim.Adam / SGD behind clip_grad_norm_ (test_0_ops_gpu.py: rel < 1e-6)."""
    d = tc.opt_make(c)
    pr = torch.nn.Parameter(d['p'].clone())
    if c.kind == 'adam':
        opt = torch.optim.Adam([pr], lr=tc.LR, betas=(tc.B1, tc.B2), eps=tc.AEPS, weight_decay=c.wd)
    else:
        opt = torch.optim.SGD([pr], lr=tc.LR, momentum=c.mu, nesterov=c.nesterov, weight_decay=c.wd)
    st = tc.opt_state0(c, d)
    for i, g in enumerate(d['grads']):
        pr.grad = g.clone()
        sq = None
        if c.max_norm > 0:
            tn = torch.nn.utils.clip_grad_norm_([pr], c.max_norm)
            sq = g.square().sum().reshape(1)
            assert abs(float(sq.sqrt()) - float(tn)) < 1e-4 * float(tn)
        opt.step()
        st = tc.opt_step_ref(c, st, g, sq, i, F32)
        assert rel(st['p'], pr) < 1e-6, (c, i)


def test_clip_scale_reference_and_plant():
    for c in tc.CLIP_CASES:
        d = tc.clip_make(c)
        sq = d['g'].double().square().sum().float().reshape(1)
        r = tc.clip_ref(c, d, sq, F64)
        b = tc.clip_bound(c, d, r)
        assert tc.excess(tc.clip_ref(c, d, sq, F32)['g'], r['g'], b['g']) <= 1
        if not c.clips:
            assert torch.equal(r['g'].float(), d['g'])
        elif 0 < c.n <= 1023:
            assert tc.excess(tc.clip_ref(c, d, sq, F64, 'no_clip')['g'], r['g'], b['g']) > 1
            pr = torch.nn.Parameter(d['g'].clone())
            pr.grad = d['g'].clone()
            torch.nn.utils.clip_grad_norm_([pr], d['max_norm'])
            assert rel(tc.clip_ref(c, d, sq, F32)['g'], pr.grad) < 1e-6


# ---------------------------------------------------------------------------------------------- the references are right
@pytest.mark.parametrize('c', [c for c in tc.RECON_CASES if not c.snapshot], ids=tc.ids)
def test_recon_reference_is_the_oracles(c):
    d = tc.recon_make(c)
    r = tc.recon_ref(c, d, F32)
    xr = d['xr'].clone().requires_grad_(True)
    if c.rows:
        ref = F.mse_loss(xr, d['x'].expand_as(xr), reduction='none').mean(-1)
    elif c.mode == tc.SIG_CODED:
        sig = d['sigma'].exp().view(-1, 1)
        ref = ((xr[1:] / sig - d['x'] / sig) ** 2).mean(-1)
    else:
        sg = dict(is_rmse=True) if c.mode == tc.SIG_RMSE else dict(learned=c.mode == tc.SIG_LOG)
        ref = O.recon_terms(dict(sigma=sg), dict(sigma=d['sigma'].clone()), None, d['x'], xr, c.L, c.N, False)[0]
        if c.mode == tc.SIG_RMSE:
            ref = ref * ref.new_tensor(1.) * ((xr[1:] - d['x']) ** 2).mean(-1).mean(0)     # the kernel leaves the division to elbo
    assert rel(r['wmse'], ref) < 1e-5
    (ref * d['gw']).sum().backward()
    assert rel(r['gxr'], xr.grad) < 1e-5 and float(r['gxr'][0].abs().max() if not c.rows else 0.) == 0.


@pytest.mark.parametrize('c', [c for c in tc.ELBO_CASES if c.mode != tc.SIG_CODED], ids=tc.ids)
def test_elbo_reference_is_the_oracles(c):
    """wmse, mse and log sigma of oracle.recon_terms for the value, log and rmse kinds (the coded
    kind needs the encoder head inside recon_terms: tail_cases restates it), from an x_reco that has the case's wmse_s."""
    d = tc.elbo_make(c)
    r = tc.elbo_ref(c, d, F32)
    s = d['sigma']
    sig = {0: s, 1: s.exp(), 3: torch.ones(1)}[c.mode]
    xr = torch.zeros(c.L + 1, c.N, 1)
    xr[1:, :, 0] = d['wmse_s'].sqrt() * sig            # D = 1: (x_reco - 0)^2 / sigma^2 = wmse_s
    sg = dict(is_rmse=True) if c.mode == 3 else dict(learned=c.mode == 1)
    _, wmse, mse, log_sigma, _ = O.recon_terms(dict(sigma=sg), dict(sigma=s.clone()), None, torch.zeros(c.N, 1), xr, c.L, c.N, False)
    assert rel(r['wmse'], wmse) < 1e-5 and rel(r['mse'], mse) < 1e-5
    cx = 0.5 * c.D * (2 * log_sigma + wmse + math.log(2 * math.pi))
    assert rel(r['cross_x'], cx) < 1e-5
    tot = cx + (tc.CW * d['ce'] if c.ce else 0.) + tc.BETA * d['kl']
    assert rel(r['total'], tot) < 1e-5


def test_coded_sigma_mse_keeps_its_mean_mean_form():
    """cvae.py:668 (sic): with a coded sigma the reported mse is mean(wmse) * mean(sigma^2); the kernel hands out the per-sample
    factors wmse and wmse * sigma_n^2 / wmse = sigma_n^2, from which that product is formed: the reference keeps both."""
    c = next(c for c in tc.ELBO_CASES if c.mode == tc.SIG_CODED and c.N > 1)
    d = tc.elbo_make(c)
    r = tc.elbo_ref(c, d, F64)
    sig2 = (2 * d['sigma'].double()).exp()
    assert rel(r['mse'] / r['wmse'], sig2) < 1e-12
    assert abs(float(r['wmse'].mean() * sig2.mean()) - float((r['mse'] / r['wmse']).mean() * r['wmse'].mean())) < 1e-12


@pytest.mark.parametrize('c', tc.XENT_CASES, ids=tc.ids)
def test_xent_reference_is_torchs(c):
    d = tc.xent_make(c)
    r = tc.xent_ref(c, d, F32)
    a = d['logits'].clone().requires_grad_(True)
    ref = F.cross_entropy(a.reshape(-1, c.C), d['y'].repeat(c.L), reduction='none').reshape(c.L, c.N)
    (ref * d['gw']).sum().backward()
    assert float((r['ce'] - ref).abs().max()) <= 1e-5 * max(float(ref.abs().max()), 1.)
    assert float((r['glogits'] - a.grad).abs().max()) <= 1e-5 * max(float(a.grad.abs().max()), 1e-30) + 1e-30
    # each backward row sums to zero within the sum of its elements' bounds
    _, r64, b = ref64(tc.XENT, c)
    assert bool((r64['glogits'].sum(-1).abs() <= b['glogits'].sum(-1)).all())


@pytest.mark.parametrize('c', tc.ACT_CASES, ids=tc.ids)
def test_act_reference_is_torchs(c):
    d = tc.act_make(c)
    r = tc.act_ref(c, d, F32)
    x = d['x'].clone().requires_grad_(True)
    y = [lambda t: t * 1, torch.relu, torch.sigmoid, F.leaky_relu][c.kind](x)
    y.backward(d['g'])
    assert float((r['y'] - y).abs().max()) <= 1e-6 * float(y.abs().max()) + 1e-37
    assert float((r['dx'] - x.grad).abs().max()) <= 1e-6 * float(x.grad.abs().max())


@pytest.mark.parametrize('c', tc.LATENT_CASES, ids=tc.ids)
def test_latent_reference_is_the_oracles(c):
    """lat_graph against oracle.jvae_oracle.prior_kl, unchanged, on fp64 tensors: values and all four gradients."""
    prior, var = tc.KINDS[c.kind]
    d = tc.latent_make(c)
    r = tc.latent_ref(c, d, F64)
    mu, lr, means, T = (tc.leaf(d[k], F64) for k in ('mu', 'lv_raw', 'means', 'T'))
    sp = dict(K=c.K, prior=dict(distribution=prior, tau=tc.TAU[prior], var_dim=var))
    lvc = torch.full_like(mu, tc.f32(c.forced)) if c.forced is not None else torch.clip(lr, -20, 20)
    z = mu + torch.exp(0.5 * lvc) * d['eps'].double() * float(c.sampled)
    kd = O.prior_kl(sp, {'encoder.prior.mean': means, 'encoder.prior._var_parameter': T}, mu, lvc, d['y'], c.w)
    obj = (z * d['gz']).sum() + (kd['kl'] * d['gk']).sum() + (kd['distance'] * d['gd']).sum() + (kd['var_kl'] * d['gv']).sum()
    obj.backward()
    tol = 1e-6          # the oracle takes alpha as a double, the kernels as the fp32 the C ABI hands over
    assert rel(r['z'], z) < tol and rel(r['kl'], kd['kl']) < tol and rel(r['zdist'], kd['distance']) < tol
    assert float((r['var_kl'] - kd['var_kl']).abs().max()) <= tol * max(float(kd['var_kl'].abs().max()), 1.)
    assert rel(r['gmu'], mu.grad) < tol and rel(r['gmeans'], means.grad) < tol
    if c.forced is None:
        assert rel(r['glv'], lr.grad) < tol
    else:
        assert float(r['glv'].abs().max()) == 0.
    if var != 'scalar':
        assert rel(r['gT'], T.grad) < tol
    dm = d['means'].double().mean(0)
    dz = (d['mu'].double() - dm).pow(2).sum(1) + (d['means'].double().pow(2).sum(1).mean(0) - dm.pow(2).sum())
    assert rel(r['dzdist'], dz) < 1e-12


@pytest.mark.parametrize('c', tc.LATENT_CASES, ids=tc.ids)
def test_latent_branch_conditions_hold_with_a_margin(c):
    """No case needs an exclusion: the clip's edge elements sit on +-20 or far outside; under the uniform prior every sample's
    gap first - vk and every element's distance to a hardtanh kink exceed the fp32 bounds of those quantities.

    first - vk = sum_k (nel_k - alpha) >= 0 for every input (nel_k - alpha is a KL term), with equality when all K intervals lie
    inside [-tau, tau]: the max() of the forward can not select its second operand by a margin, so the cases keep every sample on
    the first with one, and the second branch of the backward is reachable through rounding alone."""
    d, r, b = ref64(tc.LATENT, c)
    lr = d['lv_raw'].double().abs()
    assert bool(((lr <= 19.) | (lr == 20.) | (lr >= 29.)).all())
    if c.kind == 'ti':
        assert float(r['zdist'].min()) > 1.
    if c.kind != 'un':
        return
    k = tc.latent_counts(c, d)['kl']
    A = tc.latent_ref(c, d, F64, mag=True, branch=r['_aux']['branch'])['_aux']
    gap = (r['_aux']['first'] - r['_aux']['vk']).abs()
    assert bool((gap > k * tc.U * (A['first'] + A['vk'])).all()), (gap, k * tc.U * (A['first'] + A['vk']))
    assert bool(r['_aux']['branch'].all())
    tau = tc.TAU['uniform']
    dd = (d['mu'].double() - d['means'].double()[d['y']]).abs()
    e = k * tc.U * (dd + 0.5 * r['_aux']['span']) / tau
    for v in (r['_aux']['lo'], r['_aux']['hi']):
        assert bool((torch.minimum((v - 1).abs(), (v + 1).abs()) > e).all())


@pytest.mark.parametrize('c', [c for c in tc.MEAS_CASES if c.CK], ids=tc.ids)
def test_measures_dictionary_slots_are_torchs(c):
    """ld-norm, the capacity bound and d-mind (layers.py:323-348) from torch.cdist / logsumexp; the special rows do what they say."""
    d, r, _ = ref64(tc.MEASURES, c)
    m = d['means'].double()
    C = m.shape[0]
    cd = torch.cdist(m, m, compute_mode='donot_use_mm_for_euclid_dist')
    o = r['out'][0]
    assert abs(float(o[6]) - float(m.pow(2).mean())) < 1e-12 * max(float(o[6]), 1.)
    assert abs(float(o[7]) - float(math.log(C) - torch.logsumexp(-cd.pow(2) / 4, 1).mean())) < 1e-9
    cap = 2 * float(m.norm(dim=1).max())
    dmin = float((cd + cap * torch.eye(C, dtype=F64)).min())
    assert abs(float(o[8]) - dmin) <= 1e-12 * max(dmin, 1.)
    off = float((cd + torch.diag(torch.full((C,), math.inf, dtype=F64))).min()) if C > 1 else math.inf
    if c.special == 'twin':
        assert float(o[8]) == 0.
    if c.special == 'cap':
        assert C == 1 and cap < off and float(o[8]) == cap
    assert cap >= off * (1 - 1e-12) or C == 1          # the triangle inequality: a pair is never farther apart than the cap
    assert torch.equal(r['out'][0, 6:9], r['out'][2, 6:9])
