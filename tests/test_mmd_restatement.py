"""The yardstick of the MMD objective measures something (no GPU): the fp64 restatement of tests/mmd_cases.py against an
independent form (Gram matrices from torch.cdist, masked and normalised), its hand-written gradients against autograd of its own
forward, and three WRONG references - N instead of N - 1 in the within sums, the diagonal pair included, the label factor
dropped - each of which must leave the derived bound on at least one element in every case where it changes the value at all."""
import math

import pytest
import torch

import mmd_cases as mc

F64 = torch.float64
_cache = {}


def ref64(c):
    if c.name not in _cache:
        d = mc.make(c)
        r = mc.ref(c, d)
        _cache[c.name] = (d, r, mc.bounds(c, d, r))
    return _cache[c.name]


def gram_form(c, d):
    """m (N,) from three Gram matrices per draw: squared Euclidean distances of torch.cdist, the kernel written out per scale,
    a mask from the labels and the three normalisations - no code shared with mmd_cases.rows but the scales."""
    N, L = c.N, c.L
    y = d['y']
    z, p = d['z'].to(F64)[1:], d['p'].to(F64)
    same = torch.ones(N, N, dtype=F64)
    if c.joint:
        for i in range(N):
            for j in range(N):
                same[i, j] = 1. if int(y[i]) == int(y[j]) else 0.
    eye = torch.eye(N, dtype=F64)
    total = torch.zeros(N, dtype=F64)
    for l in range(L):
        def gram(a, b):
            d2 = torch.cdist(a, b, p=2., compute_mode='donot_use_mm_for_euclid_dist') ** 2
            out = torch.zeros_like(d2)
            for s in mc.scales_of(c):
                out = out + (s / (s + d2) if c.kind == 'imq' else (-d2 / (2 * s)).exp())
            return out * same
        zz, pp, zp = gram(z[l], z[l]), gram(p[l], p[l]), gram(z[l], p[l])
        within = ((zz + pp) * (1 - eye)).sum(1) / (N - 1) if N > 1 else torch.zeros(N, dtype=F64)
        total += within - 2 * zp.sum(1) / N
    return total / L


@pytest.mark.parametrize('c', mc.CASES, ids=mc.ids)
def test_restatement_against_the_gram_form(c):
    d, r, _ = ref64(c)
    want = gram_form(c, d)
    # cdist takes a square root and squares it again: a few fp64 roundings of the squared distance, seen through the kernel
    scale = float(want.abs().max()) + 2. * len(mc.scales_of(c))
    assert float((r['m'] - want).abs().max()) <= 1e-12 * scale, c.name
    assert math.isclose(float(r['m'].mean()), float(want.mean()), rel_tol=0., abs_tol=1e-12 * scale)


@pytest.mark.parametrize('c', mc.CASES, ids=mc.ids)
def test_hand_gradients_against_autograd_of_the_same_forward(c):
    d, r, _ = ref64(c)
    a = mc.autograd_ref(c, d)
    for k in ('g_z', 'g_means', 'g_T'):
        assert r[k].shape == a[k].shape, k
        scale = float(a[k].abs().max())
        assert float((r[k] - a[k]).abs().max()) <= 1e-12 * scale + 1e-300, (c.name, k)
    assert bool((r['g_z'][0] == 0).all())                                          # the mean latent takes no part


def test_definitions_at_the_edges():
    # N = 1: the within sums are 0 by definition, m = -2 k(z, p)
    c = mc.SHAPE_CASES[0]
    d, r, _ = ref64(c)
    assert c.N == 1
    d2 = ((d['z'].to(F64)[1, 0] - d['p'].to(F64)[0, 0]) ** 2).sum()
    assert math.isclose(float(r['m'][0]), -2. * float(mc.kernel_value(c, d2)), rel_tol=1e-14)
    # every sample its own class: only the pair (z_i, p_i) is left
    c = next(k for k in mc.SHAPE_CASES if k.classes == 'own')
    d, r, _ = ref64(c)
    d2 = ((d['z'].to(F64)[1:] - d['p'].to(F64)) ** 2).sum(-1)                      # (L, N)
    assert torch.allclose(r['m'], (-2. / c.N) * mc.kernel_value(c, d2).mean(0), rtol=1e-14, atol=0.)
    # coincident points: k = the number of scales, and the pair adds exactly nothing to either gradient
    c = next(k for k in mc.STRESS_CASES if k.stress == 'coincident')
    assert float(mc.kernel_value(c, torch.zeros((), dtype=F64))) == len(mc.scales_of(c))
    # the default scales: 2 K s for WAE's seven s
    assert mc.scales_of(mc.SHAPE_CASES[2]) == tuple(2. * 64 * s for s in (.1, .2, .5, 1., 2., 5., 10.))
    # the far rows: every rbf term between two rows is 0 in fp64 as well
    c = next(k for k in mc.STRESS_CASES if k.stress == 'far')
    d, r, B = ref64(c)
    assert all(bool(torch.isfinite(v).all()) for v in r.values()) and all(bool(torch.isfinite(v).all()) for v in B.values())


def test_a_label_out_of_range_is_in_nobodys_set():
    c = mc.SHAPE_CASES[3]
    d, r, _ = ref64(c)
    y = d['y'].clone()
    y[5] = c.C
    db = dict(d, y=y)
    rb = mc.ref(c, db)
    assert math.isnan(float(rb['m'][5])) and bool(torch.isnan(rb['g_z'][1:, 5]).all()) and bool((rb['g_z'][0] == 0).all())
    # the others: the batch with that row given a class of its own (joint: it meets nobody)
    cm = c._replace(C=c.C + 1)
    dm = dict(d, y=y, means=torch.cat([d['means'], torch.zeros(1, c.K)]), T=torch.cat([d['T'], torch.ones(1, c.K)]))
    rm = mc.ref(cm, dm)
    keep = torch.arange(c.N) != 5
    assert torch.equal(rb['m'][keep], rm['m'][keep]) and torch.equal(rb['g_z'][:, keep], rm['g_z'][:, keep])
    assert torch.equal(rb['g_means'], rm['g_means'][:c.C]) and torch.equal(rb['g_T'], rm['g_T'][:c.C])


WRONG = {
    'N_for_N_minus_1': lambda c: dict(within=c.N),
    'diagonal_included': lambda c: dict(diagonal=True),
    'label_factor_dropped': lambda c: dict(labels=False),
}


@pytest.mark.parametrize('wrong', list(WRONG))
@pytest.mark.parametrize('c', mc.CASES, ids=mc.ids)
def test_a_wrong_reference_leaves_the_bound(c, wrong):
    d, r, B = ref64(c)
    bad = mc.rows(c, d, **WRONG[wrong](c))
    changed = not torch.equal(bad.nan_to_num(), r['m'].nan_to_num())
    if wrong == 'N_for_N_minus_1':
        # it changes the value wherever a within sum is not empty
        mask, _ = mc.sets(c, d)
        assert changed == bool((mask.sum(1) > 1).any()), c.name
    if wrong == 'diagonal_included':
        assert changed == (c.N > 1), c.name                     # N = 1: the divisor is 0 by definition, nothing to include
    if wrong == 'label_factor_dropped':
        mask, ok = mc.sets(c, d)
        assert changed == (c.joint and not bool(mask.all())), c.name
    if not changed:
        return
    ex = mc.excess(bad, r['m'], B['m'])
    print(c.name, wrong, 'error / bound: %.3g' % ex)
    assert ex > 1, (c.name, wrong, ex)


def test_excess_is_a_measure():
    want = torch.tensor([1., math.nan, 0.], dtype=F64)
    B = torch.tensor([2., 1., 0.], dtype=F64)
    assert mc.excess(want.clone(), want, B) == 0.
    assert mc.excess(torch.tensor([1. + 3. * mc.U, math.nan, 0.], dtype=F64), want, B) == pytest.approx(1.5)
    assert mc.excess(torch.tensor([1., 0., 0.], dtype=F64), want, B) == math.inf          # NaN must meet NaN
    assert mc.excess(torch.tensor([math.inf, math.nan, 0.], dtype=F64), want, B) == math.inf


def test_refusal_table_names_what_this_objective_adds_and_drops():
    names = [row[0] for row in mc.refusal_table()]
    assert 'kl_var_weighting' not in names and 'semi_supervised' in names and 'world' in names and 'train_captured' in names
