"""The fp64 restatement of the class-marginal KL (tests/semi_cases.py) checked on its own, on the CPU: its hand-written gradients
against autograd, the sandwich min_c KL_c <= U <= min_c (KL_c - log pi_c), U against a quadrature of the true KL at K = 1, and the
HiddenLabels wrapper (jvae_compat/semi.py).  DESIGN.md section 7x."""
import math

import pytest
import torch

import semi_cases as sc

F64 = torch.float64
ALL = [(c, p) for c in sc.SHAPE_CASES + sc.STRESS_CASES for p in sc.PATTERNS]
pair_id = lambda v: v.name if hasattr(v, 'name') else v      # noqa: E731


@pytest.mark.parametrize('c,pattern', ALL, ids=pair_id)
def test_hand_gradients_are_autograd_s(c, pattern):
    d = sc.make(c, pattern)
    r, ag = sc.ref(c, d), sc.autograd_ref(c, d)
    for name, want in ag.items():
        got = r[name]
        scale = max(float(want.abs().max()), 1e-300)
        assert float((got - want).abs().max()) <= 1e-12 * scale + 1e-13, (name, float((got - want).abs().max()), scale)


@pytest.mark.parametrize('c,pattern', ALL, ids=pair_id)
def test_the_sandwich_and_the_rows(c, pattern):
    d = sc.make(c, pattern)
    r = sc.ref(c, d)
    p = r['parts']
    U_, KL, Q = p['U'], p['KL'], p['Q']
    slack = 1e-12 * (1 + U_.abs())
    assert bool((KL.min(1).values <= U_ + slack).all()) and bool((U_ <= Q.min(1).values + slack).all())
    assert bool(torch.isfinite(U_).all()) and bool(torch.isfinite(p['r_all']).all())
    assert float((p['r_all'].sum(1) - 1).abs().max()) <= 1e-14
    lab = d['y'] >= 0
    assert torch.equal(r['kl'][lab], d['kl_in'].to(F64)[lab]) and torch.equal(r['g_kl_in'][lab], d['g'].to(F64)[lab])
    assert not bool(r['g_mu'][lab].any()) and not bool(r['g_lv'][lab].any()) and not bool(r['g_kl_in'][~lab].any())
    B = sc.bounds(c, d, r)
    for name, b in B.items():
        assert bool(torch.isfinite(b).all()) and bool((b >= 0).all()), name
        assert b.shape == r[name].shape, name


def test_stress_cases_say_what_they_are_for():
    spread, equal, tinypi, empty = sc.STRESS_CASES
    p = sc.ref(spread, sc.make(spread, 'all_unlabelled'))['parts']
    KL = p['KL'].sort(1).values
    assert float((KL[:, 1] - KL[:, 0]).min()) > 1e4
    assert bool(((p['r_all'] == 0) | (p['r_all'] == 1)).all()) and torch.equal(p['U'], p['Q'].min(1).values)
    p = sc.ref(equal, sc.make(equal, 'all_unlabelled'))['parts']
    assert float((p['r_all'] - 1 / equal.C).abs().max()) <= 1e-15 and float((p['U'] - p['KL'][:, 0]).abs().max()) <= 1e-12
    d = sc.make(tinypi, 'all_unlabelled')
    assert float(d['log_pi'].min()) < -60
    r = sc.ref(tinypi, d)
    assert all(bool(torch.isfinite(r[k]).all()) for k in ('kl', 'zdist', 'var_kl', 'r', 'g_mu', 'g_lv', 'g_means'))
    r = sc.ref(empty, sc.make(empty, 'half'))
    assert not bool(r['r'][:, 2].any()) and not bool(r['g_means'][2].any()) and not bool(r['g_T'][2].any())


def test_U_bounds_the_true_kl_at_K1():
    """KL(q || sum_c pi_c p_c) by quadrature on a fine grid, one coordinate: true KL <= U <= min_c (KL_c - log pi_c)."""
    c = sc._c('quad', 6, 3, 1, pi=True)
    d = sc.make(c, 'all_unlabelled')
    p = sc.ref(c, d)['parts']
    mu, lv = d['mu'].to(F64)[:, 0], d['lv'].to(F64)[:, 0]
    m, t = d['means'].to(F64)[:, 0], d['T'].to(F64)
    sd = (0.5 * lv).exp()
    z = mu.view(-1, 1) + sd.view(-1, 1) * torch.linspace(-12, 12, 200001, dtype=F64).view(1, -1)          # (N, G)
    log_q = -0.5 * ((z - mu.view(-1, 1)) / sd.view(-1, 1)) ** 2 - 0.5 * lv.view(-1, 1) - 0.5 * math.log(2 * math.pi)
    log_pc = (-0.5 * (t.view(1, -1, 1) * (z.unsqueeze(1) - m.view(1, -1, 1))) ** 2 + t.abs().log().view(1, -1, 1)
              - 0.5 * math.log(2 * math.pi))
    log_p = torch.logsumexp(log_pc + d['log_pi'].view(1, -1, 1), 1)
    true_kl = torch.trapezoid(log_q.exp() * (log_q - log_p), z, dim=1)
    assert bool((true_kl <= p['U'] + 1e-9).all()) and bool((true_kl > 0).all())
    assert bool((p['U'] <= p['Q'].min(1).values + 1e-12).all())
    assert float((p['U'] - true_kl).max()) > 1e-3             # a bound, not the KL itself: the test could tell them apart


def test_hidden_labels():
    from jvae_compat.semi import HiddenLabels
    gen = torch.Generator().manual_seed(5)
    y = torch.randint(0, 4, (200,), generator=gen)
    y[:3] = 5                                                # a rare class keeps a label too
    ds = torch.utils.data.TensorDataset(torch.rand(200, 2, generator=gen), y)
    a, b = HiddenLabels(ds, keep_per_class=2, seed=3), HiddenLabels(ds, keep_per_class=2, seed=3)
    assert torch.equal(a.hidden, b.hidden) and torch.equal(a.targets, b.targets) and len(a) == 200
    assert not torch.equal(a.hidden, HiddenLabels(ds, keep_per_class=2, seed=4).hidden)
    kept = a.targets[~a.hidden]
    assert torch.equal(kept, y[~a.hidden]) and bool((a.targets[a.hidden] == -1).all())
    assert torch.equal(torch.bincount(kept, minlength=6), torch.tensor([2, 2, 2, 2, 0, 2]))
    x0, y0 = a[int(a.hidden.nonzero()[0])]
    assert y0 == -1 and torch.equal(x0, ds[int(a.hidden.nonzero()[0])][0])
    i = int((~a.hidden).nonzero()[0])
    assert a[i][1] == int(y[i])
    f = HiddenLabels(ds, keep_fraction=0.25, seed=0)
    counts = torch.bincount(y, minlength=6)
    want = torch.tensor([max(int(round(0.25 * int(n))), 1) if n else 0 for n in counts])
    assert torch.equal(torch.bincount(f.targets[~f.hidden], minlength=6), want)
    assert int(f.hidden.sum()) == 200 - int(want.sum())
    z = HiddenLabels(ds, keep_fraction=0., seed=0)            # every class keeps at least one label
    assert torch.equal(torch.bincount(z.targets[~z.hidden], minlength=6), (counts > 0).long())
    ds.targets = y.tolist()                                  # read from .targets where the dataset carries them
    assert torch.equal(HiddenLabels(ds, keep_per_class=2, seed=3).hidden, a.hidden)
    for kw in ({}, dict(keep_per_class=1, keep_fraction=0.5), dict(keep_per_class=0), dict(keep_fraction=1.5)):
        with pytest.raises(ValueError, match='HiddenLabels'):
            HiddenLabels(ds, **kw)
    # the batches a DataLoader collates from it: int64 labels with -1 in them
    xb, yb = next(iter(torch.utils.data.DataLoader(a, batch_size=50)))
    assert yb.dtype == torch.int64 and int((yb == -1).sum()) == int(a.hidden[:50].sum())
