"""Model ensembles on the device: the three kernels of csrc/aggregate.hip (ops.class_posterior, ops.latent_mutual_info,
ops.aggregate_scores) and module.aggregation, against the fp64 restatement and the inputs of
tests/test_aggregation_restatement.py and what the REFERENCE's module/aggregation.py returned
(tools/gen_aggregation_golden.py -> tests/golden/aggregation).

Bars.  Exact where the arithmetic is: VOTE rows (count / E), JOINT's aggregated row (f sum_e x_e in ascending e: the fp32 torch
expression x_0 + x_1 + ... written out - torch's own stacked sum takes another order from E = 5 on, recorded in the golden),
slots of a NaN temperature (the aggregated row itself), the predicted classes of every golden record (the generator keeps the
top-two gap of every column above 1e-3 of its magnitude).  Everything that goes through exp / log or a re-ordered sum (logp, P, Im,
MEAN, MEAN_SOFT, the soft-max slots): of each tensor the largest error against the fp64 restatement is at most 4 x the largest error the
reference's fp32 CPU result shows against fp64 on the same inputs (stored in the golden; without a golden the fp32 torch
expression is computed on the CPU here), both relative to the largest magnitude of the tensor, asserted for every case on its
own; the reference's error counts as at least one fp32 ulp of that magnitude (2^-23: on a tensor of one or two elements its
error is a draw from [0, 1 ulp] - at K = 5, C = 2, R = 1, T = 5 it came out at 0.16 ulp with the kernel at 0.9 ulp - and no fp32
result can be asked to sit closer to fp64 than its own rounding); a non-finite error fails.  4 x is the margin
tests/test_14_wim_gpu.py and tests/test_16_sample_gpu.py give their soft-max and triangular-solve rows: a differently ordered
fp32 sum is as good as torch's.  Model level: Im within 4 x `im_sens` of the
golden (the change of Im under a 1e-4 relative perturbation of z, the bar of the evaluation goldens), y_ equal wherever the
top-two gap of the mean log-density exceeds 2 * 1e-4 * max |logp|.

Measured on the MI355X (error against fp64 relative to the largest magnitude of the tensor: kernel, and in brackets the fp32
reference on the same inputs; the case of each test with the largest kernel error):
    class posteriors            logp                     P (from z, T = 1, 5, 100)
      K = 1                     5.48e-08 (1.09e-07)      5.84e-08 (9.50e-08)
      K = 5                     5.11e-08 (1.86e-07)      5.45e-08 (1.58e-07)
      K = 64                    4.99e-08 (7.28e-08)      5.11e-08 (2.95e-07)
      K = 200                   5.33e-08 (1.73e-07)      5.31e-08 (5.71e-07)
      K = 300 / 1000 (diag)     4.52e-08 (1.08e-07) / 3.09e-08 (1.07e-07)
      K = 127 / 128 / 256, C = 128   5.58e-08 (1.77e-07) / 5.24e-08 (1.36e-07) / 5.03e-08 (1.42e-07); P 3.3e-08 (1.7e-06 .. 4.3e-06)
      golden z, C = 100         5.12e-08 (1.59e-07)      3.42e-08 (3.51e-06)
    Im, (L0, L1) = (1, 1)       1.67e-07 (5.67e-08)      (3, 5)   8.60e-08 (1.04e-07)      (16, 3)  8.83e-08 (1.32e-07)
        (128, 128)              8.69e-08 (9.03e-08)      (7, 18)  9.19e-08 (2.56e-08)
      golden pairs              8.91e-08 (1.16e-07), 7.21e-08 (8.40e-08), 1.07e-07 (8.81e-08)
    scores (all modes, slots)   C = 2  3.98e-06 (3.98e-06)   C = 10  3.02e-06 (3.07e-06)   C = 100  3.34e-06 (3.51e-06)
The class posteriors are taken in fp64 and rounded once: their error is the rounding of the output.  With an fp32 walk and a
compensated sum the K = 200, C = 10, R = 7, T = 1 case sat at 6.0e-06 against the reference's 1.4e-06 (4.2 x: the rounding of a
log-density near 300 carried through exp), which is why they are not.
"""
import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state
from test_aggregation_restatement import (AGG_TEMPS, CP_C, CP_K, CP_R, MI_C, MI_L, MI_N, MI_TEMPS, PAIR_EPS_SEEDS, PAIR_N, PAIR_SEEDS,
                                          PAIRS, SCORE_CASES, SCORE_MODES, agg64, argmax_lowest, im64, load_golden, logp64,
                                          mi_inputs, posterior_inputs, prior_of, score_inputs, score_name, softmax64, torch_im,
                                          torch_logp)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGIN = 4.


def same_bits(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def err(a, exact):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    with np.errstate(invalid='ignore'):
        d = np.abs(a - exact)
    d[(a == exact)] = 0.                   # equal infinities
    return float(d.max()) if not np.isnan(d).any() else float('nan')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


ULP = 2. ** -23                        # one unit in the last place of an fp32 value, relative to the binade's lower end


class Worst:
    """Per case: the error of the kernel, relative to the largest magnitude of the tensor, is finite and at most
    MARGIN x max(the fp32 reference's error on the same inputs, ULP).  The worst case is printed by report() (the figures of the
    docstring)."""

    def __init__(self, what):
        self.what, self.kernel, self.ref = what, -1., 0.

    def check(self, got, ref32, exact, where):
        top = float(np.abs(exact[np.isfinite(exact)]).max()) if np.isfinite(exact).any() else 0.
        scale = top if top > 0. else 1.
        e = err(got, exact) / scale
        r = (float(ref32) if np.isscalar(ref32) else err(ref32, exact)) / scale
        assert np.isfinite(e) and np.isfinite(r), (self.what, where, e, r)
        if e > self.kernel:
            self.kernel, self.ref = e, r
        assert e <= MARGIN * max(r, ULP), (self.what, where, e, r)

    def report(self):
        print(f'{self.what}: kernel {self.kernel:.2e} (reference {self.ref:.2e})')

    settle = report


# --------------------------------------------------------------------------------------------- 1. class posteriors
@pytest.mark.parametrize('K', CP_K)
def test_class_posterior_against_the_fp64_restatement(K):
    from jvae_hip import ops
    temps = [1, 5, 100]
    w_logp, w_post = Worst(f'logp K={K}'), Worst(f'P K={K}')
    for C in CP_C:
        for R in CP_R:
            p = posterior_inputs(K, C, R)
            d = {k: dev(v) for k, v in p.items()}
            for var_dim in ('scalar', 'diag') + (('full',) if K in (5, 64) else ()):
                ld = 'log_det_' + var_dim
                logp, P = ops.class_posterior(d['z'], d['means'], d[var_dim], d[ld], var_dim=var_dim, temps=temps)
                again = ops.class_posterior(d['z'], d['means'], d[var_dim], d[ld], var_dim=var_dim, temps=temps)
                assert same_bits(logp, again[0]) and same_bits(P, again[1])
                assert tuple(logp.shape) == (C, R) and tuple(P.shape) == (3, C, R)
                exact = logp64(p['z'], p['means'], p[var_dim], p[ld], var_dim)
                ref_logp, ref_P = torch_logp(p, var_dim, temps)
                w_logp.check(logp, ref_logp, exact, (C, R, var_dim))
                exact_P = softmax64(exact, temps)                  # the whole chain from z, for the kernel and for torch
                for j in range(3):
                    w_post.check(P[j], ref_P[j], exact_P[j], (C, R, var_dim, temps[j]))
                one, P1 = ops.class_posterior(d['z'], d['means'], d[var_dim], d[ld], var_dim=var_dim, temps=[1], logp=False)
                assert one is None and same_bits(P1[0], P[0])
    w_logp.report()
    w_post.report()


def test_class_posterior_on_the_golden_draws_of_the_100_class_pair():
    from jvae_hip import ops
    g, gl = load_golden('e3L32_e3L32'), load_golden('e3L32_e3L32_logp')
    w = Worst('logp golden C=100')
    wp = Worst('P golden C=100')
    for i, name in enumerate(PAIRS['e3L32_e3L32']):
        means, T, log_det = prior_of(name, PAIR_SEEDS[i])
        z = g[f'z{i}']
        L, N, K = z.shape
        logp, P = ops.class_posterior(dev(z), dev(means), dev(T), dev(log_det), temps=MI_TEMPS)
        assert tuple(logp.shape) == (100, L, N) and tuple(P.shape) == (2, 100, L, N)
        exact = logp64(z.reshape(L * N, K), means, T, log_det, 'scalar').reshape(100, L, N)
        w.check(logp, float(g[f'logp{i}_err']), exact, i)
        # the whole chain from z for both: the reference's P is the fp32 soft-max of its stored fp32 logp, as the generator took it
        exact_P = softmax64(exact, MI_TEMPS)
        ref = torch.from_numpy(gl[f'logp{i}'])
        for j, t in enumerate(MI_TEMPS):
            wp.check(P[j], (ref / t).softmax(0).numpy(), exact_P[j], (i, t))
        assert same_bits(P, ops.class_posterior(dev(z.reshape(L * N, K)), dev(means), dev(T), dev(log_det), temps=MI_TEMPS,
                                                logp=False)[1].view(2, 100, L, N))
    w.report()
    wp.report()


def test_class_posterior_nan_temperature_and_wide_K():
    """A temperature of NAN_TEMPS passes logp through; K = 1000 takes the 8-row tile (K > 512), K = 300 the 16-row one."""
    from jvae_hip import ops
    for K in (300, 1000):
        p = posterior_inputs(K, 3, 21)
        d = {k: dev(v) for k, v in p.items()}
        logp, P = ops.class_posterior(d['z'], d['means'], d['diag'], d['log_det_diag'], var_dim='diag', temps=[None, 1, -1, 0])
        assert same_bits(P[0], logp) and same_bits(P[2], logp) and same_bits(P[3], logp)
        ref_logp, _ = torch_logp(p, 'diag', [1])
        w = Worst(f'logp K={K}')
        w.check(logp, ref_logp, logp64(p['z'], p['means'], p['diag'], p['log_det_diag'], 'diag'), K)
        w.report()
        assert abs(float(P[1].sum(0).min()) - 1.) < 1e-5


@pytest.mark.parametrize('K', [127, 128, 256])
def test_class_posterior_at_the_largest_tile(K):
    """C = 128: K = 127 is the largest tile of 32 rows (exactly 48 KiB of LDS), K = 128 the first that halves it to 16."""
    from jvae_hip import ops
    p = posterior_inputs(K, 128, 65)
    d = {k: dev(v) for k, v in p.items()}
    w, wp = Worst(f'logp K={K} C=128'), Worst(f'P K={K} C=128')
    for var_dim in ('scalar', 'diag'):
        ld = 'log_det_' + var_dim
        logp, P = ops.class_posterior(d['z'], d['means'], d[var_dim], d[ld], var_dim=var_dim, temps=[1, 5])
        exact = logp64(p['z'], p['means'], p[var_dim], p[ld], var_dim)
        ref_logp, ref_P = torch_logp(p, var_dim, [1, 5])
        w.check(logp, ref_logp, exact, var_dim)
        exact_P = softmax64(exact, [1, 5])
        for j in range(2):
            wp.check(P[j], ref_P[j], exact_P[j], (var_dim, j))
    w.report()
    wp.report()


# ------------------------------------------------------------------------------------- 2. latent mutual information
def chunked(fn, P0, P1, step=8):
    """fn on slices of the sample axis (the pairwise mean is per sample): bounds the (C, L1, L0, n) temporaries of the yardsticks."""
    return np.concatenate([fn(np.ascontiguousarray(P0[..., n:n + step]), np.ascontiguousarray(P1[..., n:n + step]))
                           for n in range(0, P0.shape[-1], step)], axis=-1)


@pytest.mark.parametrize('L0,L1', MI_L)
def test_latent_mi_against_the_fp64_restatement(L0, L1):
    """(7, 18) straddles the 4 x 4 register tile on both sides and the round-robin of the four waves over the tiles of P1."""
    from jvae_hip import ops
    w = Worst(f'Im L=({L0}, {L1})')
    for C in MI_C:
        for N in MI_N:
            nT = 1 if L0 * L1 > 1000 else 2
            P0, P1 = mi_inputs(C, L0, L1, N, nT)
            Im = ops.latent_mutual_info(dev(P0), dev(P1))
            assert tuple(Im.shape) == (nT, N) and same_bits(Im, ops.latent_mutual_info(dev(P0), dev(P1)))
            exact = chunked(im64, P0, P1)
            assert np.isfinite(exact).all()
            w.check(Im, chunked(torch_im, P0, P1), exact, N)
    w.report()


def test_latent_mi_minus_infinity_stays_in_its_sample():
    from jvae_hip import ops
    P0, P1 = mi_inputs(10, 5, 6, 7, 2)
    before = ops.latent_mutual_info(dev(P0), dev(P1))
    P0[:, :, :, 3], P1[:, :, :, 3] = 0., 0.
    P0[:, 0, :, 3], P1[:, 1, :, 3] = 1., 1.                       # sample 3: every draw one-hot, the two models on different classes
    Im = ops.latent_mutual_info(dev(P0), dev(P1))
    exact = im64(P0, P1)
    assert np.array_equal(np.isneginf(exact), np.isneginf(Im.cpu().numpy())) and np.isneginf(exact[:, 3]).all()
    Worst('Im beside a -inf sample').check(Im, torch_im(P0, P1), exact, 'disjoint one-hot')
    keep = torch.arange(7, device=DEV) != 3
    assert bool(torch.isinf(Im[:, 3]).all()) and bool((Im[:, 3] < 0).all())
    assert bool(torch.isfinite(Im[:, keep]).all()) and same_bits(Im[:, keep], before[:, keep])
    P1[:, 1, 2, 3], P1[:, 0, 2, 3] = 0., 1.                        # ONE pair-row with a class in common is not enough
    assert bool(torch.isinf(ops.latent_mutual_info(dev(P0), dev(P1))[:, 3]).all())


@pytest.mark.parametrize('pair', list(PAIRS))
def test_latent_mi_on_the_golden_posteriors(pair):
    from jvae_hip import ops
    g, gl = load_golden(pair), load_golden(pair + '_logp')
    P = [torch.stack([(torch.from_numpy(gl[f'logp{i}']) / t).softmax(0) for t in MI_TEMPS]) for i in range(2)]
    Im = ops.latent_mutual_info(P[0].to(DEV), P[1].to(DEV))
    exact = im64(softmax64(gl['logp0'], MI_TEMPS), softmax64(gl['logp1'], MI_TEMPS))
    w = Worst(f'Im golden {pair}')
    for j, t in enumerate(MI_TEMPS):
        w.check(Im[j], float(g[f'Im_{t}_err']), exact[j], t)
    w.report()


# --------------------------------------------------------------------------------------------- 3. score aggregation
@pytest.mark.parametrize('C', [2, 10, 100])
def test_aggregate_scores_on_the_golden_records(C):
    """Every record of C classes (N = 1, 7, 65, 300, E by SCORE_CASES): the exact checks per record, one bar per (mode, slot)."""
    w = Worst(f'scores C={C}')
    for case in SCORE_CASES:
        if case[1] == C:
            one_score_record(case, w)
    w.settle()


def one_score_record(case, w):
    from jvae_hip import ops
    E, C, N = case
    g, name = load_golden('scores'), score_name(*case)
    s = score_inputs(E, C, N)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for key, mode, f in SCORE_MODES:
        src = [dev(v) for v in s[key]]
        soft = mode == 'mean_soft'
        post, a, top, arg = ops.aggregate_scores(src, mode, factors=f, temps=AGG_TEMPS, a=not soft, amax=True, argmax=True, slot=0,
                                                 status=status)
        again = ops.aggregate_scores(src, mode, factors=f, temps=AGG_TEMPS, a=not soft, amax=True, argmax=True, slot=0, status=status)
        assert all(x is None and y is None or same_bits(x, y) for x, y in zip((post, a, top, arg), again))
        assert np.array_equal(arg.cpu().numpy(), g[f'{name}.{mode}.y']), mode
        assert same_bits(top, post[0].max(0)[0])
        exact, exact_a = agg64(s[key], mode, f, AGG_TEMPS)
        for j in range(len(AGG_TEMPS)):
            w.check(post[j], float(g[f'{name}.{mode}.err'][j]), exact[j], name)
        if not soft:
            assert same_bits(post[0], a)                           # a NaN temperature: the aggregated row itself
            # without the buffers the kernel keeps x in (post, a): the same values, recomputed
            _, _, top1, arg1 = ops.aggregate_scores(src, mode, factors=f, temps=AGG_TEMPS, post=False, amax=True, argmax=True, slot=1)
            assert same_bits(top1, post[1].max(0)[0]) and same_bits(arg1, arg)
        if mode == 'joint':
            total = torch.from_numpy(s[key][0])
            for more in s[key][1:]:
                total = total + torch.from_numpy(more)
            assert same_bits(a, -total / 2)
        if mode == 'mean':
            _, _, lpxy, _ = ops.aggregate_scores(src, 'mean', post=False, amax=True)
            assert same_bits(lpxy, a.max(0)[0])
            w.check(lpxy, float(g[f'{name}.log_p_x_y_err']), exact_a.max(0), name)
    votes = [dev(v) for v in s['y']]
    post, a, top, arg = ops.aggregate_scores(votes, 'vote', temps=AGG_TEMPS, a=True, amax=True, argmax=True, slot=0, num_classes=C,
                                             status=status)
    count = sum(torch.nn.functional.one_hot(torch.from_numpy(v), C).T for v in s['y'])
    assert same_bits(a, count / E) and all(same_bits(post[j], a) for j in range(len(AGG_TEMPS)))
    assert np.array_equal(a.cpu().numpy()[:, :g[f'{name}.vote.post'].shape[1]], g[f'{name}.vote.post'])
    assert np.array_equal(arg.cpu().numpy(), g[f'{name}.vote.y']) and same_bits(top, a.max(0)[0])
    assert int(status) == 0


def test_a_vote_outside_the_classes_is_flagged_and_never_indexed():
    from jvae_hip import ops
    s = score_inputs(3, 10, 65)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    good = ops.aggregate_scores([dev(v) for v in s['y']], 'vote', post=False, a=True, num_classes=10, status=status)[1]
    for bad in (10, -1, 1 << 40):
        votes = [dev(v) for v in s['y']]
        votes[1][17] = bad
        status.zero_()
        post, a, top, arg = ops.aggregate_scores(votes, 'vote', temps=[None], a=True, amax=True, argmax=True, slot=0, num_classes=10,
                                                 status=status)
        keep = torch.arange(65, device=DEV) != 17
        assert int(status) & 1 and bool(torch.isnan(a[:, 17]).all()) and bool(torch.isnan(post[0, :, 17]).all())
        assert bool(torch.isnan(top[17])) and same_bits(a[:, keep], good[:, keep])
        with pytest.raises(ops.L.JvaeHipError):
            ops.wim_check_status(status)
        assert int(status) == 0


def test_amax_keeps_a_nan_and_ties_take_the_lowest_class():
    from jvae_hip import ops
    x = torch.tensor([[1., 2., 0.], [1., float('nan'), 3.], [0., 5., 3.]], device=DEV)
    _, a, top, arg = ops.aggregate_scores([x], 'joint', factors=1., post=False, a=True, amax=True, argmax=True)
    assert same_bits(a, x) and arg.tolist() == [0, 1, 1] and bool(torch.isnan(top[1])) and top[0] == 1. and top[2] == 3.


# --------------------------------------------------------------------------------------------- 4. the public module
def test_module_functions_return_the_reference_dictionaries():
    from module import aggregation as A
    E, C, N = 5, 10, 65
    g, name = load_golden('scores'), score_name(E, C, N)
    s = {k: [dev(v) for v in vs] for k, vs in score_inputs(E, C, N).items()}
    keep = g[f'{name}.mean.post'].shape[2]
    # the arithmetic is held to the golden's own error at the op level (test_aggregate_scores_on_the_golden_records); here the
    # dictionaries, their keys and shapes are what is checked, the values only to 1e-5 of the slot's magnitude
    for fn, key, mode in ((A.mean_posterior, 'iws', 'mean'), (A.joint_posterior, 'zdist', 'joint')):
        out = fn(*s[key], temps=AGG_TEMPS)
        assert list(out) == AGG_TEMPS
        for j, t in enumerate(AGG_TEMPS):
            ref = g[f'{name}.{mode}.post'][j]
            assert tuple(out[t].shape) == (C, N) and np.abs(out[t].cpu().numpy()[:, :keep] - ref).max() <= 1e-5 * np.abs(ref).max()
    out = A.mean_of_posteriors(*s['kl'], temps=AGG_TEMPS, factor=-1)
    ref = g[f'{name}.mean_soft.post']
    assert all(np.abs(out[t].cpu().numpy()[:, :keep] - ref[j]).max() <= 1e-5 * np.abs(ref[j]).max() for j, t in enumerate(AGG_TEMPS))
    lme = A.log_mean_exp(*s['iws'])
    assert same_bits(lme, A.mean_posterior(*s['iws'], temps=[-1])[-1])
    assert tuple(A.log_mean_exp(*[v[:1] for v in s['iws']]).shape) == (N,)         # the reference's squeeze(0)
    post = A.posterior(s['iws'][0])
    assert list(post) == A.TEMPS and same_bits(post[None], s['iws'][0])
    assert same_bits(post[5], A.posterior(s['iws'][0], axis=1, temps=[5])[5])       # axis 0 whatever `axis` says
    cube = s['iws'][0].view(C, 5, 13)
    assert same_bits(A.posterior(cube, temps=[1])[1], post[1].view(C, 5, 13))
    vp = A.voting_posterior(*s['y'], temps=AGG_TEMPS)
    width = int(max(int(v.max()) for v in s['y'])) + 1
    assert list(vp) == AGG_TEMPS and all(vp[t] is vp[-1] for t in AGG_TEMPS) and tuple(vp[-1].shape) == (width, N)
    assert np.array_equal(vp[-1].cpu().numpy()[:, :keep], g[f'{name}.vote.post'][:width])
    assert tuple(A.voting_posterior(*s['y'], num_classes=12)[None].shape) == (12, N)
    for agg, mode in (('mean', 'mean'), ('joint', 'joint'), ('mean~', 'mean_soft')):
        e = A.ensemble(s, agg, temps=AGG_TEMPS)
        assert np.array_equal(e['y'].cpu().numpy(), g[f'{name}.{mode}.y']) and list(e['p_y_x']) == AGG_TEMPS
        assert same_bits(e['max_p_y_x'], e['p_y_x'][-1].max(0)[0]) and ('log_p_x_y' in e) == (agg == 'mean')
    assert same_bits(A.ensemble(s, 'mean')['log_p_x_y'], lme.max(0)[0])
    e = A.ensemble({'y': s['y'], 'num_classes': C}, 'vote', temps=AGG_TEMPS)
    assert np.array_equal(e['y'].cpu().numpy(), g[f'{name}.vote.y'])


def test_module_functions_raise_on_a_vote_outside_the_classes():
    from jvae_hip import JvaeHipError, ops
    from module import aggregation as A
    y = [torch.tensor([0, 2, 1], device=DEV), torch.tensor([1, 2, 2], device=DEV)]
    shared = ops.wim_status(torch.device(DEV))
    shared.zero_()
    for bad in (lambda: A.voting_posterior(*y, num_classes=2), lambda: A.voting_posterior(y[0], -y[1]),
                lambda: A.ensemble({'y': y, 'num_classes': 2}, 'vote')):
        with pytest.raises(JvaeHipError, match='label'):
            bad()
    assert int(shared) == 0                                        # the shared per-device word is left alone
    assert tuple(A.voting_posterior(*y)[None].shape) == (3, 3)


# --------------------------------------------------------------------------------------------- 5. memory
def test_the_kernel_chain_never_holds_an_expanded_z():
    """C = 10, L = 16, N = 64, K = 64, two temperatures: what latent_mutual_info runs after the models' forward passes."""
    from jvae_hip import ops
    from module import aggregation as A
    C, Ls, N, K, temps = 10, 16, 64, 64, [1, 5]
    p = posterior_inputs(K, C, 2 * Ls * N)
    d = {k: dev(v) for k, v in p.items()}
    z = d['z'].view(2, Ls, N, K)

    class Prior:
        distribution, conditional, var_dim = 'gaussian', True, 'scalar'
        mean, _var_parameter = d['means'], d['scalar']

        def log_det_per_class(self):
            return d['log_det_scalar']

    def chain():
        logp, P0 = A.class_posteriors(Prior(), z[0], temps)
        _, P1 = A.class_posteriors(Prior(), z[1], temps, logp=False)
        _, _, _, y_ = ops.aggregate_scores([logp.mean(1)], 'joint', factors=1., post=False, argmax=True)
        return ops.latent_mutual_info(P0, P1), y_
    chain()                                                        # the per-device status word and the library are in place
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    Im, y_ = chain()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    outputs = Im.numel() * 4 + y_.numel() * 8
    budget = outputs + 2 * (len(temps) + 1) * C * Ls * N * 4
    print(f'peak rise {rise} bytes, budget {budget}, one expanded z {C * Ls * N * K * 4}')
    assert rise < budget < C * Ls * N * K * 4


# --------------------------------------------------------------------------------------------- 6. models
def drop_in(name, seed):
    from cvae import ClassificationVariationalNetwork as Net
    torch.manual_seed(0)
    net = Net(**get_case(name)['net'])
    load_det_state(net, seed=seed)
    return net.to(DEV).eval()


@pytest.mark.parametrize('pair', list(PAIRS))
def test_latent_mutual_info_of_two_models(pair):
    from jvae_hip import ops
    from module import aggregation as A
    g, gl = load_golden(pair), load_golden(pair + '_logp')
    nets = [drop_in(n, s) for n, s in zip(PAIRS[pair], PAIR_SEEDS)]
    kw = get_case(PAIRS[pair][0])['net']
    x, y, _ = det_inputs(PAIR_N, kw['input_shape'], kw['num_labels'], 1, kw['latent_dim'], seed=PAIR_EPS_SEEDS[0])
    x, y = x.to(DEV), y.to(DEV)
    eps = tuple(dev(g[f'eps{i}']) for i in range(2))
    Im, y_ = A.latent_mutual_info(nets[0], nets[1], x, y, temps=MI_TEMPS, epsilon=eps)
    assert list(Im) == MI_TEMPS and all(tuple(v.shape) == (PAIR_N,) and not v.names[0] for v in Im.values())
    # the op chain on the models' own draws, bit for bit
    P, logp0 = [], None
    with torch.no_grad():
        for i, net in enumerate(nets):
            z = net.forward(x, epsilon=eps[i])[-1][1:]
            assert np.abs(z.cpu().numpy() - g[f'z{i}']).max() <= 1e-4 * np.abs(g[f'z{i}']).max()
            pr = net.encoder.prior
            logp, Pi = ops.class_posterior(z, pr.mean.detach(), pr._var_parameter.detach(), pr.log_det_per_class().detach(),
                                           var_dim=pr.var_dim, temps=MI_TEMPS)
            P.append(Pi)
            logp0 = logp if i == 0 else logp0
    chain = ops.latent_mutual_info(P[0], P[1])
    assert all(same_bits(Im[t], chain[j]) for j, t in enumerate(MI_TEMPS))
    assert same_bits(y_, ops.aggregate_scores([logp0.mean(1)], 'joint', factors=1., post=False, argmax=True)[3])
    for t in MI_TEMPS:
        d, sens = float(np.abs(Im[t].cpu().numpy() - g[f'Im_{t}']).max()), float(g[f'im_sens_{t}'])
        print(f'{pair} T={t}: |Im - golden| {d:.2e}, im_sens {sens:.2e}')
        assert d <= MARGIN * sens
    top = float(np.abs(gl['logp0']).max())
    assert np.abs(logp0.cpu().numpy() - gl['logp0']).max() <= 1e-4 * top
    if pair != 'e3L32_e3L32':
        sure = g['y_gap'] > 2 * 1e-4 * top
        assert sure.all() and np.array_equal(y_.cpu().numpy(), g['y_'])
    else:                                                          # 100 classes: gaps down to 0.008 - the model's own logp decides
        mean = logp0.double().cpu().numpy().mean(1)
        s = np.sort(mean, axis=0)
        sure = s[-1] - s[-2] > 2 * 1e-4 * float(np.abs(mean).max())
        assert sure.any() and np.array_equal(y_.cpu().numpy()[sure], argmax_lowest(mean)[sure])
        both = sure & (g['y_gap'] > 2 * 1e-4 * top)
        assert np.array_equal(y_.cpu().numpy()[both], g['y_'][both])


def test_other_priors_are_refused_by_name():
    from module import aggregation as A
    kw = get_case('c2_n8_tilted')['net']
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**kw).to(DEV).eval()
    x = det_inputs(4, kw['input_shape'], 10, 1, kw['latent_dim'])[0].to(DEV)
    with pytest.raises(NotImplementedError, match='tilted'):
        A.latent_mutual_info(net, net, x, None)
