"""The fp64 restatement of the beta-TCVAE split (tests/tc_cases.py) checked on its own, without a device: its hand-written
gradients against torch.autograd on its own forward, the identities and closed forms of the three terms, and the derived error
bound against an evaluation of the same formulas by torch at the kernel's precisions.  These tests check the REFERENCE the GPU
tests hold the kernels to, not the kernels: csrc/tcvae.hip, ops.tc_objective and the model are tested by tests/test_tc_host.py
and tests/test_38_tc_gpu.py.  What ties this file to the code is the first test: the piece sizes the bound counts with and the
limits of the cases are read from jvae_hip.ops and the library and must agree with tc_cases.

Closed forms (derived here, asserted below; z is formed in fp64 from mu, lv and eps so that z - mu_i = sigma_i eps exactly enough):
  * every case: mi + tc + dwkl = A - Bp, the Monte-Carlo KL of the draws;
  * equal weights alpha = beta_tc = gamma: reg = alpha (A - Bp), g_mu = 0, g_lv = -alpha g / 2, g_z = alpha g / L t^2 (z - m): nothing of
    the mixture is left;
  * singleton sets (|S_i| = 1: N = 1, or every sample its own class): sum_k l_iik = A, so J = A - c_i and P = A - K c_i:
    mi = c_i = log n_i,  tc = (K - 1) c_i,  dwkl = A - K c_i - Bp;
  * identical posteriors in a set of B rows: every l_ijk = l_iik, each logsumexp adds log B:  J = A - log n_i,  P = A - K log n_i:
    mi = log n_i,  tc = (K - 1) log n_i,  dwkl = A - K log n_i - Bp   (n_i = B without a data-set size: the section 7u figures)."""
import math

import pytest
import torch

import tc_cases as tcc
from jvae_hip.ops import TC_MAX_K, TC_MAX_N, TC_MAX_Q, aggpost_partition, tc_joint_partition
from test_aggpost_restatement import P as MARGINAL_PART

F64 = torch.float64


def test_the_bound_counts_with_the_kernels_own_constants():
    """The one tie of this file to the code under test (host only: the library's queries launch nothing).  The bound counts one
    merge step per piece of the joint sum, tc_cases.JOINT_PART rows each, and per piece of the marginal sum, aggpost's partition:
    both must be what the kernels cut the batch into.  The limits of ops.tc_objective must be the library's, and every case must
    lie within them."""
    from jvae_hip import lib
    h = lib.load()
    assert tcc.JOINT_PART == tc_joint_partition() == h.jvae_tc_joint_partition()
    assert MARGINAL_PART == aggpost_partition()
    assert MARGINAL_PART % tcc.JOINT_PART == 0
    assert (TC_MAX_K, TC_MAX_N, TC_MAX_Q) == (1024, 8192, 1 << 26)
    assert h.jvae_tc_keep_bytes(1, TC_MAX_N, TC_MAX_K) > 0
    assert h.jvae_tc_keep_bytes(1, TC_MAX_N + 1, 1) == 0 and h.jvae_tc_keep_bytes(1, 1, TC_MAX_K + 1) == 0
    L = TC_MAX_Q // (256 * 256)
    assert h.jvae_tc_keep_bytes(L, 256, 1) > 0 and h.jvae_tc_keep_bytes(L + 1, 256, 1) == 0
    for c in tcc.CASES:
        assert c.K <= TC_MAX_K and c.N <= TC_MAX_N and c.L * c.N * c.N <= TC_MAX_Q, c.name


@pytest.fixture(scope='module')
def refs():
    out = {}
    for c in tcc.CASES:
        d = tcc.make(c)
        out[c.name] = (d, tcc.ref(c, d))
    return out


@pytest.mark.parametrize('c', tcc.CASES, ids=tcc.ids)
def test_hand_written_gradients_equal_autograd(c, refs):
    d, r = refs[c.name]
    auto = tcc.autograd_ref(c, d)
    assert set(auto) == {k for k in r if k.startswith('g_')}
    for k, want in auto.items():
        got = r[k]
        assert got.shape == want.shape, k
        scale = float(want.abs().max()) or 1.
        err = float((got - want).abs().max()) / scale
        assert err < 1e-10, (c.name, k, err)
    assert bool((r['g_z'][0] == 0).all())


@pytest.mark.parametrize('c', tcc.CASES, ids=tcc.ids)
def test_the_three_terms_add_up_to_the_sampled_kl(c, refs):
    d, r = refs[c.name]
    p = r['per_draw']
    kl = (p['A'] - p['Bp']).mean(0)
    tot = r['mi'] + r['tc'] + r['dwkl']
    assert float((tot - kl).abs().max()) <= 1e-12 * float(kl.abs().max() + p['P'].abs().max() + 1)
    a, b, g = c.weights
    assert torch.allclose(r['reg'], a * r['mi'] + b * r['tc'] + g * r['dwkl'], rtol=1e-13, atol=0)


@pytest.mark.parametrize('c', [c for c in tcc.CASES if len(set(c.weights)) == 1], ids=tcc.ids)
def test_equal_weights_leave_nothing_of_the_mixture(c, refs):
    d, r = refs[c.name]
    a = c.weights[0]
    p = r['per_draw']
    assert float((r['reg'] - a * (p['A'] - p['Bp']).mean(0)).abs().max()) <= 1e-12 * float(p['P'].abs().max() + 1)
    assert bool((r['g_mu'] == 0).all())
    g = d['g'].double()
    assert torch.equal(r['g_lv'], (-0.5 * a * g).view(-1, 1).expand(c.N, c.K))
    m, t = tcc._prior(c, {k: (v if k == 'y' else v.double()) for k, v in d.items() if v is not None})
    want = (a * g / c.L).view(1, -1, 1) * t * t * (d['z'][1:].double() - m)
    assert torch.equal(r['g_z'][1:], want)


def exact_z(d):
    """The operands in fp64 with z formed there: z - mu_i is sigma_i eps to the last bits of fp64."""
    v = {k: (x if k == 'y' or x is None else x.double()) for k, x in d.items()}
    v['z'] = torch.cat([v['mu'].unsqueeze(0), v['mu'] + (0.5 * v['lv']).exp() * v['eps']])
    return v


@pytest.mark.parametrize('name,logn', [('K1_L1_N1_C1', False), ('K3_L1_N5_own', False), ('K3_L1_N5_own', True)])
def test_singleton_sets(name, logn):
    c = next(c for c in tcc.CASES if c.name == name)._replace(logn=logn)
    d = exact_z(tcc.make(c))
    r = tcc.ref(c, d)
    p = r['per_draw']
    ci = tcc.sets(c, d)[2]
    want_c = d['log_n'][d['y']] if logn else torch.zeros(c.N, dtype=F64)
    assert torch.allclose(ci, want_c, rtol=0, atol=1e-15)
    tol = 1e-12 * float(p['A'].abs().max() + 1)
    assert float((r['mi'] - ci).abs().max()) <= tol
    assert float((r['tc'] - (c.K - 1) * ci).abs().max()) <= tol
    assert float((r['dwkl'] - (p['A'] - c.K * ci - p['Bp']).mean(0)).abs().max()) <= tol


@pytest.mark.parametrize('logn', [False, True])
def test_identical_posteriors_in_a_set(logn):
    c = tcc._c('identical', 5, 3, 12, C=3, classes='rand', var='diag', logn=logn)
    d = tcc.make(c)
    first = {int(k): int((d['y'] == k).nonzero()[0]) for k in d['y'].unique()}
    rows = torch.tensor([first[int(k)] for k in d['y']])
    d['mu'], d['lv'] = d['mu'][rows].clone(), d['lv'][rows].clone()
    d = exact_z(d)
    r = tcc.ref(c, d)
    p = r['per_draw']
    mask, ok, ci = tcc.sets(c, d)
    B = mask.sum(1).double()
    log_ni = d['log_n'][d['y']] if logn else B.log()
    tol = 1e-12 * float(p['A'].abs().max() + 1)
    assert float((r['mi'] - log_ni).abs().max()) <= tol
    assert float((r['tc'] - (c.K - 1) * log_ni).abs().max()) <= tol
    assert float((r['dwkl'] - (p['A'] - c.K * log_ni - p['Bp']).mean(0)).abs().max()) <= tol


def test_the_data_set_size_moves_the_terms_by_constants_and_no_gradient():
    c = next(c for c in tcc.CASES if c.name == 'K65_L3_N64_C3_diag_w523')
    d = tcc.make(c)
    r0 = tcc.ref(c, d)
    d1 = dict(d, log_n=torch.tensor([50000., 6000., 700.], dtype=F64).log())
    r1 = tcc.ref(c, d1)
    shift = tcc.sets(c, d1)[2] - tcc.sets(c, d)[2]
    assert float((r1['mi'] - r0['mi'] - shift).abs().max()) < 1e-9
    assert float((r1['tc'] - r0['tc'] - (c.K - 1) * shift).abs().max()) < 1e-9
    assert float((r1['dwkl'] - r0['dwkl'] + c.K * shift).abs().max()) < 1e-9
    for k in r0:
        if k.startswith('g_'):
            assert torch.equal(r0[k], r1[k]), k


def test_the_stress_rows_are_what_they_claim(refs):
    c = tcc.STRESS_CASES[0]
    d, r = refs[c.name]
    sigma = (0.5 * d['lv']).exp().max()
    gaps = (d['mu'].unsqueeze(1) - d['mu'].unsqueeze(0)).abs().min(-1).values + torch.eye(c.N) * 1e9
    assert float(gaps.min() / sigma) > 9e3
    assert all(bool(torch.isfinite(v).all()) for k, v in r.items() if k != 'per_draw')
    # the own row is all that is left of every sum: the singleton closed form (with z formed in fp64: at 6 x 10^5 the fp32 z
    # carries an eps rounded to 1 / 16)
    ci = tcc.sets(c, d)[2]
    assert float((tcc.ref(c, exact_z(d))['mi'] - ci).abs().max()) < 1e-9


def test_case_table_covers_what_the_kernels_branch_on():
    cs = tcc.SHAPE_CASES
    assert {c.K for c in cs} >= {1, 3, 64, 65, 200} and {c.N for c in cs} >= {1, 2, 63, 64, 65, 257} and {c.L for c in cs} == {1, 3}
    assert {c.C for c in cs} >= {1, 3} and {c.var for c in cs} == {'scalar', 'diag'}
    assert {c.weights for c in cs} == {(1., 6., 1.), (1., 1., 1.), (0.5, 2., 3.)}
    assert {c.spread for c in cs} == {'wide', 'near'} and {c.logn for c in cs} == {False, True}
    for c in cs:
        d = tcc.make(c)
        if c.classes == 'es':
            assert c.C == 3 and not bool((d['y'] == 1).any()) and int((d['y'] == 2).sum()) == 1
        if c.spread == 'wide':
            assert float(d['lv'].min()) >= math.log(1e-4) - 1e-6 and float(d['lv'].max()) <= 0
            assert d['lv'].numel() < 100 or float(d['lv'].min()) < math.log(1e-3)


@pytest.mark.parametrize('c', tcc.CASES, ids=tcc.ids)
def test_bound_is_positive_finite_and_holds_an_evaluation_at_the_kernels_precisions(c, refs):
    """B is a derivation for the kernel's arithmetic: the exponents, the two logsumexp and the weights in fp32, A, Bp, the ends and
    every gradient sum in fp64.  The same formulas evaluated by torch at those precisions must sit under it - a check of the
    derivation that needs no device."""
    d, r = refs[c.name]
    B = tcc.bounds(c, d, r)
    assert set(B) == set(r) - {'per_draw'}
    for k, b in B.items():
        assert b.shape == r[k].shape, k
        assert bool(torch.isfinite(b).all()) and bool((b >= 0).all()), k
    got = tcc.ref(c, d, torch.float32)
    ex = {k: tcc.excess(got[k].float(), r[k], B[k]) for k in B}
    print(c.name, {k: round(v, 3) for k, v in ex.items()})
    assert all(v <= 1 for v in ex.values()), (c.name, ex)
