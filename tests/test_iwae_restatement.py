"""The fp64 restatement of the importance-weighted bound (tests/iwae_cases.py) checked on its own, without a device: its
hand-written gradients against torch.autograd on its own forward, the identities of the bound, and the derived error bound
against an independent fp32 evaluation of the same formulas."""
import math

import pytest
import torch

import iwae_cases as ic


@pytest.fixture(scope='module')
def refs():
    out = {}
    for c in ic.CASES:
        d = ic.make(c)
        out[c.name] = (d, ic.ref(c, d))
    return out


@pytest.mark.parametrize('c', ic.CASES, ids=ic.ids)
def test_hand_written_gradients_equal_autograd(c, refs):
    d, r = refs[c.name]
    auto = ic.autograd_ref(c, d)
    for k, want in auto.items():
        got = r[k]
        assert got.shape == want.shape, k
        scale = float(want.abs().max()) or 1.
        err = float((got - want).abs().max()) / scale
        assert err < 1e-10, (c.name, k, err)


@pytest.mark.parametrize('c', ic.CASES, ids=ic.ids)
def test_identities(c, refs):
    d, r = refs[c.name]
    lw, bound, wt, ess = r['log_w'], r['bound'], r['wt'], r['ess']
    assert float((wt.sum(0) - 1).abs().max()) < 1e-12
    assert bool((ess >= 1 - 1e-12).all()) and bool((ess <= c.L + 1e-9).all())
    top = lw.max(0).values
    slack = 1e-12 * top.abs().clamp(min=1.)
    assert bool((bound <= top + slack).all()) and bool((bound >= top - math.log(c.L) - slack).all())
    if c.L == 1:
        assert torch.equal(bound, lw[0]) and torch.equal(wt, torch.ones_like(wt))


def test_stress_rows_are_what_they_claim(refs):
    by = {c.stress: (c, *refs[c.name]) for c in ic.STRESS_CASES}
    c, d, r = by['lead']
    lw = r['log_w']
    second = lw.sort(0).values[-2]
    assert bool((lw.max(0).values - second > 1e4).all())
    assert bool((r['wt'].max(0).values == 1).all()) and bool((r['ess'] == 1).all())      # exactly one-hot in fp64 as well
    c, d, r = by['equal']
    assert bool((r['log_w'] == r['log_w'][0]).all()) and float((r['ess'] - c.L).abs().max()) < 1e-9
    c, d, r = by['deep']
    assert bool((r['log_w'] < -9e4).all()) and bool((r['log_w'] > -1.1e5).all())
    c, d, r = by['huge']
    assert float(d['wmse_s'].max()) > 9e29 and r['wt'][1, 0] == 0
    assert all(bool(torch.isfinite(v).all()) for v in r.values())


def test_case_table_covers_what_the_kernels_branch_on():
    cs = ic.SHAPE_CASES
    assert {c.K for c in cs} >= {1, 3, 63, 64, 65, 200}
    assert {c.L for c in cs} >= {1, 2, 5, 64, 65, 257}
    assert {c.N for c in cs} >= {1, 3, 257}
    assert {c.C for c in cs} >= {1, 3} and {c.classes for c in cs} == {'rand', 'empty1', 'one'}
    assert {c.var for c in cs} == {'scalar', 'diag'} and {c.sig for c in cs} == {ic.SIG_VALUE, ic.SIG_LOG, ic.SIG_CODED}
    assert {c.beta for c in cs} == {1., 0.25} and {c.D for c in cs} == {1, 3072}
    assert {c.stress for c in ic.STRESS_CASES} == {'lead', 'equal', 'deep', 'huge'}
    for c in cs:
        if c.classes == 'empty1':
            y = ic.make(c)['y']
            assert c.C == 3 and not bool((y == 1).any())


def mixed(c, d):
    """The restatement at the kernel's precisions, by torch: log w in fp64, parked as fp32(log w - max), fold and weights in fp32,
    the gradients' chains in fp64 from THOSE weights, every result rounded to fp32."""
    lw = ic.log_w(c, d)
    top = lw.max(0).values
    e = (lw - top).float().exp()
    S, Q = e.sum(0), (e * e).sum(0)
    wt = e / S
    out = dict(bound=(top + S.double().log() - math.log(c.L)).float(), wt=wt, ess=S * S / Q)
    r = ic.ref(c, d)
    g, y = d['g'].double(), d['y']
    t = (d['T'][y] if c.var == 'diag' else d['T'][y].unsqueeze(-1).expand(c.N, c.K)).double()
    dz = d['z'][1:].double() - d['means'][y].double()
    w = wt.double().unsqueeze(-1)
    onehot = torch.nn.functional.one_hot(y, c.C).double()
    out['g_wmse_s'] = (-g * wt.double() * (0.5 * c.D)).float()
    gz = torch.zeros_like(d['z'], dtype=torch.float64)
    gz[1:] = -(g * c.beta).view(1, -1, 1) * w * (t * t * dz)
    out['g_z'] = gz.float()
    out['g_means'] = (onehot.T @ ((g * c.beta).view(-1, 1) * (w * (t * t * dz)).sum(0))).float()
    if c.var == 'diag':
        out['g_T'] = (onehot.T @ ((g * c.beta).view(-1, 1) * (w * (1 / t - t * dz * dz)).sum(0))).float()
    out['g_lv'], out['g_sigma'] = r['g_lv'].float(), r['g_sigma'].float()
    return out


@pytest.mark.parametrize('c', ic.CASES, ids=ic.ids)
def test_bound_is_positive_finite_and_holds_an_evaluation_at_the_kernels_precisions(c, refs):
    """B is a derivation for the kernel's arithmetic: log w in fp64, the parked differences and their fold in fp32.  The same
    formulas evaluated by torch at those precisions (its sums are no deeper than the kernel's) must sit under it - a check of
    the derivation that needs no device."""
    d, r = refs[c.name]
    B = ic.bounds(c, d, r)
    assert set(B) == set(r) - {'log_w'}
    for k, b in B.items():
        assert b.shape == r[k].shape or b.numel() == 1, k
        assert bool(torch.isfinite(b).all()) and bool((b >= 0).all()), k
    got = mixed(c, d)
    ex = {k: ic.excess(got[k], r[k], B[k]) for k in B}
    print(c.name, {k: round(v, 3) for k, v in ex.items()})
    assert all(v <= 1 for v in ex.values()), (c.name, ex)
