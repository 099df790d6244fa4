"""WIMJob.finetune() on the device: the two-prior latent kernel (ops.latent_mixed), the running tally of the printed losses
(ops.group_tally), the one-pass fine-tuning step (finetune_step) against the two-pass finetune_batch(), and the loop.

Bars.  The mixed latent kernel runs, per sample, the body of the single-prior kernel: torch.equal on every output and
gradient.  The tally accumulates in fp64: exact counts, sums within 1e-12 relative of an fp64 host sum, the same bits run to
run.  The fused step's per-sample losses and L were asked to be within RTOL = 1e-4 of the two-pass step's; they came out
bit-identical at 8 + 8 and at 5 + 3 images (no BatchNorm statistics, and the forward kernels give a sample the same bits in a
batch of 16 as in one of 8), so torch.equal is asserted.  Its gradients are the same per-sample terms summed in another
order: per parameter tensor, the distance from the two-pass step may be at most 4 x the two-pass step's OWN order noise - the
largest distance between the two-pass step and the two-pass step on the same samples in a permuted order, over three
permutations - both measured as |a - b|_2 / max(|b|_2, 1e-3 |g|_2), the floor of
test_wim_finetune_step_matches_reference_golden.  The loop's group means: 1e-6 relative of the reference's running-mean rule
restated in fp64 (the rule's own fp32 .mean() over at most 16 values).

Measured on the MI355X (distance of the gradient per parameter tensor, fused step | order noise of the two-pass step):
    sizes   largest over the tensors      largest ratio (tensor)                    tensors at distance 0 (fused | noise)
    8 + 8   1.249e-07 | 8.855e-08        1.41  (features.12.weight)                11 | 1   (sigma: 0 | 0)
    5 + 3   1.006e-07 | 7.285e-08        2.46  (imager.12.bias: 6.37e-08 | 2.59e-08)  1 | 0
Every tensor of both sizes is in the table of DESIGN.md section 7d.  Tally: relative error 0 at N = 1, 7, 300.  Loop: the
shown group means differ from the rule by at most 2.5e-08 relative."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RTOL = 1e-4


def rel(a, b, floor=1e-30):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


# ---------------------------------------------------------------------------------------------- 1. the two-prior latent kernel
SPLITS = [(8, 4), (8, 5), (9, 0), (9, 9), (1, 0), (1, 1)]
C_A = 10


def prior_a(var_dim, K, g):
    means = torch.randn(C_A, K, generator=g)
    if var_dim == 'scalar':
        T = torch.rand(C_A, generator=g) + 0.5
    elif var_dim == 'diag':
        T = torch.rand(C_A, K, generator=g) + 0.5
    else:
        T = (0.1 * torch.randn(C_A, K, K, generator=g)).tril(-1) + torch.diag_embed(torch.rand(C_A, K, generator=g) + 0.5)
    return dict(means=means.to(DEV), T=T.contiguous().to(DEV), prior='gaussian', var_dim=var_dim, tau=0., alpha=0.)


def prior_b(kind, K, g):
    means = (torch.randn(1, K, generator=g) * 0.3 + 1.5).to(DEV)
    if kind == 'gaussian':
        return dict(means=means, T=torch.full((1,), 0.8, device=DEV), prior='gaussian', var_dim='scalar', tau=0., alpha=0.)
    if kind == 'tilted':
        return dict(means=means, T=torch.ones(1, device=DEV), prior='tilted', var_dim='scalar', tau=5., alpha=0.)
    tau = 3.
    alpha = math.log(2 * tau) - math.log(2 * (0.5 * (1 + math.erf(tau / math.sqrt(2)))) - 1)
    return dict(means=means, T=torch.ones(1, device=DEV), prior='uniform', var_dim='scalar', tau=tau, alpha=alpha)


def describe(p):
    from jvae_hip import ops
    return ops.latent_prior(p['means'], p['T'], prior=p['prior'], var_dim=p['var_dim'], tau=p['tau'], alpha=p['alpha'])


def latent_inputs(N, K, L, split, g):
    mu = torch.randn(N, K, generator=g)
    raw = torch.randn(N, K, generator=g) * 3
    raw.view(-1)[::7] = 25.                                   # both sides of the +-20 clip
    raw.view(-1)[3::11] = -25.
    eps = torch.randn(L + 1, N, K, generator=g)
    eps[0] = 0
    y = torch.cat((torch.randint(0, C_A, (split,), generator=g), torch.zeros(N - split, dtype=torch.int64)))
    up = dict(lv=torch.randn(N, K, generator=g), z=torch.randn(L + 1, N, K, generator=g), kl=torch.randn(N, generator=g),
              zd=torch.randn(N, generator=g), vkl=torch.randn(N, generator=g))
    return mu.to(DEV), raw.to(DEV), eps.to(DEV), y.to(DEV), {k: v.to(DEV) for k, v in up.items()}


def backward_of(outs, up, rows=slice(None)):
    lv, z, kl, zd, vkl, _ = outs
    torch.autograd.backward([lv, z, kl, zd, vkl], [up['lv'][rows], up['z'][:, rows].contiguous(), up['kl'][rows], up['zd'][rows],
                                                   up['vkl'][rows]])


def run_mixed(mu, raw, eps, y, A, B, split, up):
    from jvae_hip import ops
    mu, raw = mu.clone().requires_grad_(), raw.clone().requires_grad_()
    outs = ops.latent_mixed(mu, raw, eps, y, describe(A), describe(B), split)
    backward_of(outs, up)
    return [o.detach() for o in outs] + [mu.grad, raw.grad]


def run_single(mu, raw, eps, y, p, rows, up):
    from jvae_hip import ops
    mu, raw = mu[rows].clone().requires_grad_(), raw[rows].clone().requires_grad_()
    outs = ops.latent(mu, raw, eps[:, rows].contiguous(), y[rows].contiguous(), p['means'], p['T'], prior=p['prior'],
                      var_dim=p['var_dim'], tau=p['tau'], alpha=p['alpha'])
    backward_of(outs, up, rows)
    return [o.detach() for o in outs] + [mu.grad, raw.grad]


NAMES = ['lv', 'z', 'kl', 'zdist', 'var_kl', 'dzdist', 'gmu', 'glv_raw']


@pytest.mark.parametrize('var_a', ['scalar', 'diag', 'full'])
@pytest.mark.parametrize('N,split', SPLITS)
def test_latent_mixed_is_the_single_prior_kernel_per_sample(N, split, var_a):
    g = torch.Generator().manual_seed(1000 * N + 10 * split + len(var_a))
    for K in (3, 64, 100):
        for L in (1, 3):
            A = prior_a(var_a, K, g)
            mu, raw, eps, y, up = latent_inputs(N, K, L, split, g)
            for kind_b in ('gaussian', 'tilted', 'uniform'):
                B = prior_b(kind_b, K, g)
                what = (K, L, kind_b)
                mixed = run_mixed(mu, raw, eps, y, A, B, split, up)
                again = run_mixed(mu, raw, eps, y, A, B, split, up)
                for name, a, b in zip(NAMES, mixed, again):                  # two launches: the same bits
                    assert torch.equal(a, b), (what, name)
                parts = [(slice(0, split), A), (slice(split, N), B)]
                for rows, p in parts:
                    if rows.stop == rows.start:
                        continue
                    single = run_single(mu, raw, eps, y, p, rows, up)
                    for name, m, s in zip(NAMES, mixed, single):
                        m = m[:, rows] if name == 'z' else m[rows]
                        if name == 'dzdist' and p is B:                       # the dictionary belongs to the A part
                            assert torch.equal(m, torch.zeros_like(m)), what
                            continue
                        assert not s.isnan().any(), (what, name)
                        assert torch.equal(m, s), (what, name, float((m - s).abs().max()))


@pytest.mark.parametrize('N,split', SPLITS)
def test_latent_mixed_writes_its_outputs_only(N, split):
    """The C entry points on buffers of the caller: a sentinel in front of, behind and (backward) around every output stays."""
    from jvae_hip import lib as L, ops
    K, Ls, PAD, SENT = 100, 1, 37, -777.25
    g = torch.Generator().manual_seed(5 + N + split)
    A, B = prior_a('diag', K, g), prior_b('tilted', K, g)
    mu, raw, eps, y, up = latent_inputs(N, K, Ls, split, g)
    want = run_mixed(mu, raw, eps, y, A, B, split, up)
    ins = [t.clone() for t in (mu, raw, eps, y, A['means'], A['T'], B['means'], B['T'])]
    dict_ = torch.empty(K + 1, device=DEV)
    lib = L.load()
    L.check(lib.jvae_dict_stats_f32(L.ptr(A['means']), L.ptr(dict_), C_A, K, L.stream_ptr()), 'dict_stats')
    sizes = dict(lv=N * K, z=(Ls + 1) * N * K, kl=N, zdist=N, var_kl=N, dzdist=N, gmu=N * K, glv_raw=N * K)
    bufs = {k: torch.full((n + 2 * PAD,), SENT, device=DEV) for k, n in sizes.items()}

    def at(k):
        return bufs[k].data_ptr() + 4 * PAD
    kinds = (C_A, 0, 1, 0., 0., 1, 1, 0, 5., 0.)
    rc = lib.jvae_latent_mixed_fwd_f32(L.ptr(mu), L.ptr(raw), L.ptr(eps), L.ptr(y), L.ptr(A['means']), L.ptr(A['T']), L.ptr(dict_),
                                       L.ptr(B['means']), L.ptr(B['T']), at('lv'), at('z'), at('kl'), at('zdist'), at('var_kl'),
                                       at('dzdist'), N, K, Ls, split, *kinds, 1., 1, 0, 0., L.stream_ptr())
    L.check(rc, 'fwd')
    lv = bufs['lv'][PAD:PAD + N * K].view(N, K).clone()
    rc = lib.jvae_latent_mixed_bwd_f32(L.ptr(mu), L.ptr(raw), L.ptr(lv), L.ptr(eps), L.ptr(y), L.ptr(A['means']), L.ptr(A['T']),
                                       L.ptr(B['means']), L.ptr(B['T']), L.ptr(up['z']), L.ptr(up['kl']), L.ptr(up['zd']),
                                       L.ptr(up['vkl']), None, L.ptr(up['lv']), at('gmu'), at('glv_raw'), None, None,
                                       N, K, Ls, split, *kinds, 1., 1, 0, None, 0, L.stream_ptr())
    L.check(rc, 'bwd')
    for (k, n), ref in zip(sizes.items(), want):
        b = bufs[k]
        assert torch.equal(b[PAD:PAD + n], ref.reshape(-1)), k
        assert bool((b[:PAD] == SENT).all()) and bool((b[PAD + n:] == SENT).all()), k
    for t, was in zip((mu, raw, eps, y, A['means'], A['T'], B['means'], B['T']), ins):
        assert torch.equal(t, was)
    # prior gradients are refused by the entry point itself, and so is a split outside [0, N]
    gm = torch.zeros_like(A['means'])
    args = (L.ptr(mu), L.ptr(raw), L.ptr(lv), L.ptr(eps), L.ptr(y), L.ptr(A['means']), L.ptr(A['T']), L.ptr(B['means']),
            L.ptr(B['T']), L.ptr(up['z']), L.ptr(up['kl']), L.ptr(up['zd']), L.ptr(up['vkl']), None, L.ptr(up['lv']), at('gmu'),
            at('glv_raw'))
    assert lib.jvae_latent_mixed_bwd_f32(*args, L.ptr(gm), None, N, K, Ls, split, *kinds, 1., 1, 0, None, 0, L.stream_ptr()) == -1
    assert lib.jvae_latent_mixed_bwd_f32(*args, None, None, N, K, Ls, N + 1, *kinds, 1., 1, 0, None, 0, L.stream_ptr()) == -1
    assert not bool(gm.any())


def test_latent_mixed_refuses_prior_gradients_and_bad_host_labels():
    from jvae_hip import ops
    N, K, split = 8, 64, 5
    g = torch.Generator().manual_seed(3)
    A, B = prior_a('scalar', K, g), prior_b('gaussian', K, g)
    mu, raw, eps, y, up = latent_inputs(N, K, 1, split, g)
    A['means'].requires_grad_()
    outs = ops.latent_mixed(mu.clone().requires_grad_(), raw, eps, y, describe(A), describe(B), split)
    with pytest.raises(ops.L.JvaeHipError):
        outs[2].sum().backward()
    A['means'].requires_grad_(False)
    host = y.cpu()
    ok = ops.latent_mixed(mu, raw, eps, host, describe(A), describe(B), split)          # labels on the host: checked, then used
    assert torch.equal(ok[2], ops.latent_mixed(mu, raw, eps, y, describe(A), describe(B), split)[2])
    for n, bad in ((0, C_A), (split - 1, -1), (split, 1), (N - 1, 3)):                   # [0, 10) before the split, [0, 1) from it on
        wrong = host.clone()
        wrong[n] = bad
        with pytest.raises(ops.L.JvaeHipError):
            ops.latent_mixed(mu, raw, eps, wrong, describe(A), describe(B), split)
    with pytest.raises(ops.L.JvaeHipError):
        ops.latent_mixed(mu, raw, eps, y, describe(A), describe(B), N + 1)


def test_a_device_label_outside_its_prior_is_never_an_index():
    """Labels that exist on the device only: the sample's outputs and gradients are NaN, every other sample is untouched."""
    N, K, split = 9, 64, 5
    g = torch.Generator().manual_seed(4)
    A, B = prior_a('full', K, g), prior_b('uniform', K, g)
    mu, raw, eps, y, up = latent_inputs(N, K, 1, split, g)
    good = run_mixed(mu, raw, eps, y, A, B, split, up)
    wrong = y.clone()
    bad = [1, 4, 5, 8]
    wrong[1], wrong[4], wrong[5], wrong[8] = C_A, -(1 << 40), 1, 1 << 33
    got = run_mixed(mu, raw, eps, wrong, A, B, split, up)
    keep = torch.ones(N, dtype=torch.bool, device=DEV)
    keep[bad] = False
    for name, a, b in zip(NAMES, got, good):
        a, b = (a.transpose(0, 1), b.transpose(0, 1)) if name == 'z' else (a, b)
        assert torch.equal(a[keep], b[keep]), name
        if name == 'dzdist':
            assert a[[1, 4]].isnan().all() and bool((a[[5, 8]] == 0).all())
        else:
            assert a[~keep].isnan().all(), name


# ---------------------------------------------------------------------------------------------- 2. the tally kernel
@pytest.mark.parametrize('N', [1, 7, 300])
def test_group_tally(N):
    from jvae_hip import ops
    R, G = 2, 3
    g = torch.Generator().manual_seed(N)

    def accumulate():
        sums = torch.zeros((R, G), dtype=torch.float64, device=DEV)
        counts = torch.zeros(G, dtype=torch.int64, device=DEV)
        for _ in batches:
            ops.group_tally(_[0], _[1], sums, counts)
        return sums.cpu(), counts.cpu()

    batches = []
    for b in range(3):
        values = (torch.randn(R, N, generator=g) * 10 ** b).to(DEV)
        group = torch.randint(-2, G, (N,), generator=g).to(torch.int32).to(DEV)          # -2, -1: skipped
        batches.append((values, group))
    sums, counts = accumulate()
    want_s, want_c = np.zeros((R, G)), np.zeros(G, dtype=np.int64)
    for values, group in batches:
        v, grp = values.cpu().numpy().astype(np.float64), group.cpu().numpy()
        for j in range(G):
            want_c[j] += int((grp == j).sum())
            want_s[:, j] += np.array([math.fsum(v[r, grp == j]) for r in range(R)])
    assert counts.tolist() == want_c.tolist()
    got = sums.numpy()
    err = np.abs(got - want_s) / np.maximum(np.abs(want_s), 1e-300)
    print(f'group_tally N={N}: largest relative error of a sum {err.max():.3e}')
    assert (np.abs(got - want_s) <= 1e-12 * np.abs(want_s)).all(), (got, want_s)
    again = accumulate()
    assert torch.equal(again[0], sums) and torch.equal(again[1], counts)
    with pytest.raises(ops.L.JvaeHipError):
        ops.group_tally(batches[0][0], batches[0][1].long(), torch.zeros((R, G), dtype=torch.float64, device=DEV),
                        torch.zeros(G, dtype=torch.int64, device=DEV))
    with pytest.raises(ops.L.JvaeHipError):
        ops.group_tally(batches[0][0], batches[0][1], torch.zeros((R, G), dtype=torch.float32, device=DEV),
                        torch.zeros(G, dtype=torch.int64, device=DEV))


# ---------------------------------------------------------------------------------------------- 3. the fused step
def wim_job(fused=True, **over):
    """WIMJob on the geometry and the weights of case w2_n8 (as tests/test_14_wim_gpu.py builds it)."""
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.wim import WIMJob
    from module.priors import build_prior
    case = get_case('w2_n8')
    kw, K = dict(case['net'], **over), case['net']['latent_dim']
    job = WIMJob(**kw, alternate_prior=dict(case['alternate_prior'], num_priors=1, dim=K))
    twin = Net(**kw)
    for net in (job, twin):
        load_det_state(net, seed=0)
        net.to(DEV)
    with torch.no_grad():
        for k in ('mean', '_var_parameter'):
            getattr(job.encoder.prior, k).copy_(getattr(twin.encoder.prior, k))
            getattr(job._alternate_prior, k).copy_(build_prior(dim=K, num_priors=1, **case['alternate_prior']).to(DEV).state_dict()[k])
    job.WIM_FUSED_STEP = fused
    return job, case


def step_inputs(case, n_in, n_mix):
    kw, K = case['net'], case['net']['latent_dim']
    x_in, y_in, _ = det_inputs(n_in, kw['input_shape'], kw['num_labels'], 1, K, seed=1234)
    x_mix, _, _ = det_inputs(n_mix, kw['input_shape'], kw['num_labels'], 1, K, seed=777)
    return x_in.to(DEV), y_in.to(DEV), x_mix.to(DEV)


def grads_of(job):
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in job.named_parameters() if p.grad is not None}


def state_of(job):
    return dict(alternate=job.is_alternate_prior, both=job._evaluate_on_both_priors, training=job.training,
                prior=job.encoder.prior is job._alternate_prior, num_labels=job.num_labels, estimated=job._with_estimated_labels,
                methods=list(job.ood_methods), mixed=job.encoder.mixed_prior,
                bn=[m.training for m in job.modules() if isinstance(m, torch.nn.BatchNorm2d)])


def distances(a, b):
    """Per parameter tensor: |a - b|_2 / max(|b|_2, 1e-3 x the global norm of b)."""
    tot = math.sqrt(sum(float(v.double().pow(2).sum()) for v in b.values()))
    return {k: float((a[k].double() - b[k].double()).norm()) / max(float(b[k].double().norm()), 1e-3 * tot) for k in b}


@pytest.mark.parametrize('n_in,n_mix', [(8, 8), (5, 3)])
def test_fused_step_against_the_two_pass_step(n_in, n_mix):
    job, case = wim_job(fused=True)
    two, _ = wim_job(fused=False)
    x_in, y_in, x_mix = step_inputs(case, n_in, n_mix)
    alpha = case['alpha']
    out = {}
    for name, net in (('fused', job), ('two', two)):
        net.optimizer.zero_grad()
        torch.manual_seed(11)
        out[name] = net.finetune_step(0, 0, x_in, y_in, x_mix, alpha=alpha)
        out[name][0].backward()
    assert job.last_finetune_route == 'fused' and two.last_finetune_route == 'two_pass'
    assert state_of(job) == state_of(two)
    assert job.is_alternate_prior and job._evaluate_on_both_priors and job.training and job.encoder.mixed_prior is None
    assert job._original_prior.mean.grad is None and job._alternate_prior.mean.grad is None
    (L, in_loss, mix_loss), (L2, in2, mix2) = out['fused'], out['two']
    assert set(in_loss) == set(in2) and set(mix_loss) == set(mix2) and 'dzdist' not in mix_loss and 'dzdist' in in_loss
    worst, same = 0., True
    for mine, ref in ((in_loss, in2), (mix_loss, mix2)):
        for k in ref:
            assert mine[k].shape == ref[k].shape, k
            worst = max(worst, rel(mine[k], ref[k]))
            same = same and torch.equal(mine[k], ref[k])
    print(f'fused step {n_in}+{n_mix}: per-sample losses max rel {worst:.3e}, bit-identical {same}; '
          f'L rel {abs(float(L.detach()) - float(L2.detach())) / abs(float(L2.detach())):.3e}')
    for mine, ref in ((in_loss, in2), (mix_loss, mix2)):
        for k in ref:
            assert rel(mine[k], ref[k]) < RTOL and torch.equal(mine[k], ref[k]), (k, rel(mine[k], ref[k]))
    assert torch.equal(L.detach(), L2.detach())

    # the two-pass step's own order noise: the same samples, permuted inside each half, the same noise per sample
    g_fused, g_two = grads_of(job), grads_of(two)
    assert set(g_fused) == set(g_two)
    L1 = two.encoder.sampling_size
    gen = torch.Generator().manual_seed(2)
    eps = torch.randn(L1 + 1, n_in + n_mix, two.latent_dim, generator=gen).to(DEV)
    eps[0] = 0

    def two_pass_grads(p_in, p_mix):
        two.optimizer.zero_grad()
        e = torch.cat((eps[:, :n_in][:, p_in], eps[:, n_in:][:, p_mix]), 1)
        two.finetune_step(0, 0, x_in[p_in], y_in[p_in], x_mix[p_mix], alpha=alpha, epsilon=e)[0].backward()
        return grads_of(two)

    ident = (torch.arange(n_in, device=DEV), torch.arange(n_mix, device=DEV))
    base = two_pass_grads(*ident)
    noise = {k: 0. for k in base}
    perms = [(ident[0].flip(0), ident[1].flip(0)), (ident[0].roll(3), ident[1].roll(1)),
             (torch.randperm(n_in, generator=gen).to(DEV), torch.randperm(n_mix, generator=gen).to(DEV))]
    for p in perms:
        for k, d in distances(two_pass_grads(*p), base).items():
            noise[k] = max(noise[k], d)
    job.optimizer.zero_grad()
    job.finetune_step(0, 0, x_in, y_in, x_mix, alpha=alpha, epsilon=eps)[0].backward()
    assert job.last_finetune_route == 'fused'
    dist = distances(grads_of(job), base)
    print(f'fused step {n_in}+{n_mix}: gradient distance per tensor, fused | order noise of the two-pass step')
    for k in base:
        print(f'    {k:40s} {dist[k]:.3e} | {noise[k]:.3e}')
    print(f'    largest: {max(dist.values()):.3e} | {max(noise.values()):.3e}')
    for k in base:
        assert dist[k] <= 4 * noise[k], (k, dist[k], noise[k])
    # ... and with the noise drawn from the seed (the comparison of the first part): the same bar
    for k, d in distances(g_fused, g_two).items():
        assert d <= 4 * noise[k], (k, d, noise[k])


def test_switch_off_or_a_classifier_term_takes_the_two_pass_form():
    for fused, over in ((False, {}), (True, dict(gamma=2.0, classifier=[20]))):
        a, case = wim_job(fused=fused, **over)
        b, _ = wim_job(fused=fused, **over)
        x_in, y_in, x_mix = step_inputs(case, 8, 8)
        torch.manual_seed(7)
        got = a.finetune_step(0, 0, x_in, y_in, x_mix, alpha=case['alpha'])
        torch.manual_seed(7)
        want = b.finetune_batch(0, 0, x_in, y_in, x_mix, alpha=case['alpha'])
        assert a.last_finetune_route == 'two_pass' and b.last_finetune_route is None
        assert torch.equal(got[0], want[0]) and state_of(a) == state_of(b)
        for mine, ref in zip(got[1:], want[1:]):
            assert set(mine) == set(ref)
            for k in ref:
                assert torch.equal(mine[k], ref[k]), k


# ---------------------------------------------------------------------------------------------- 4. the loop
class _Images(torch.utils.data.Dataset):
    def __init__(self, n, seed, name):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.rand((n, 3, 32, 32), generator=g)
        self.y = torch.randint(0, 10, (n,), generator=g)
        self.name = name

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


class _Sink:
    def __init__(self):
        self.calls = []

    def results(self, i, per_epoch, epoch, epochs, **kw):
        self.calls.append(dict(kw, i=i, per_epoch=per_epoch, epoch=epoch, epochs=epochs))


def loop_sets():
    return _Images(24, 1, 'train'), _Images(8, 2, 'cifar'), {'svhn': _Images(8, 3, 'other')}


def test_finetune_loop_is_the_hand_written_loop(tmp_path):
    from jvae_compat.ft_datasets import MovingSet
    from jvae_compat.wim import WIMJob
    job, case = wim_job(fused=False)
    twin, _ = wim_job(fused=False)
    trainset, ind, oods = loop_sets()
    trained = job.trained
    torch.manual_seed(21)
    res = job.finetune(trainset, ind, oods, batch_size=8, epochs=2, test_batch_size=8, alpha=case['alpha'])
    assert job.last_finetune_route == 'two_pass'

    torch.manual_seed(21)
    train_loader = torch.utils.data.DataLoader(trainset, batch_size=8, shuffle=True, num_workers=0)
    moving_loader = torch.utils.data.DataLoader(MovingSet(ind, oods), drop_last=True, batch_size=8, shuffle=True, num_workers=0)
    for epoch in range(2):
        twin.eval()
        train_iter, moving_iter = iter(train_loader), iter(moving_loader)
        for batch in range(2):
            x_u, _ = next(moving_iter)
            x_a, y_a = next(train_iter)
            twin.optimizer.zero_grad()
            L, _, _ = twin.finetune_batch(epoch, batch, x_a.to(DEV), y_a.to(DEV), x_u.to(DEV), alpha=case['alpha'])
            L.backward()
            twin.optimizer.step()
            twin.optimizer.clip(twin.parameters())
    torch.cuda.synchronize()
    twin.original_prior = True                 # finetune_batch() leaves the alternate prior in place, finetune() the original
    mine, theirs = job.state_dict(), twin.state_dict()
    assert set(mine) == set(theirs)
    for k in mine:
        assert torch.equal(mine[k], theirs[k]), k
    fresh, _ = wim_job(fused=False)
    assert not torch.equal(fresh.state_dict()['features.0.weight'], mine['features.0.weight'])        # the run did train

    assert job.trained == trained
    fp = job.ft_params
    assert fp['sets'] == ['svhn'] and fp['train_size'] == 32 and fp['moving_size'] == 16 and fp['mix'] == 0.5
    assert fp['padding'] == 0 and fp['padding_sets'] == [] and fp['mix_padding'] == 0 and fp['alpha'] == case['alpha']
    assert set(res) == {'svhn'} and list(res['svhn']) == job.ood_methods
    assert {'zdist~', 'zdist@', 'zdist~@', 'elbo~', 'elbo@', 'elbo~@'} <= set(res['svhn'])
    assert set(job.ood_results) == {job.trained} and set(job.ood_results[job.trained]) == {'cifar', 'svhn'}
    for m, r in job.ood_results[job.trained]['svhn'].items():
        assert r['n'] == 8 and 0. <= r['auc'] <= 1., m
    assert job.is_original_prior and not job._evaluate_on_both_priors and not job.training

    d = job.save(str(tmp_path / 'job'))
    with open(os.path.join(d, 'wim.json')) as f:
        on_disk = json.load(f)
    assert set(WIMJob.FT_RUN_KEYS) >= {'sets', 'train_size', 'moving_size', 'mix', 'padding', 'padding_sets', 'mix_padding', 'alpha'}
    assert on_disk['sets'] == ['svhn'] and on_disk['train_size'] == 32 and on_disk['mix'] == 0.5
    back = WIMJob.load(d)
    assert back.ft_params == on_disk and back._alternate_prior is not None
    assert back._alternate_prior.distribution == 'gaussian' and not back._alternate_prior.conditional


def test_finetune_loop_fused_reports_the_running_means():
    job, case = wim_job(fused=True)
    trainset, ind, oods = loop_sets()
    sink, seen = _Sink(), []

    def on_batch(epoch, batch, in_loss, mix_loss, tags):
        seen.append((epoch, batch, in_loss['zdist'].detach().clone(), mix_loss['zdist'].detach().clone(), tags.clone()))

    torch.manual_seed(22)
    job.finetune(trainset, ind, oods, batch_size=8, epochs=2, test_batch_size=8, alpha=case['alpha'], outputs=sink,
                 on_batch=on_batch)
    assert job.last_finetune_route == 'fused' and len(seen) == 4
    lines = [c for c in sink.calls if c.get('preambule') == 'finetune']
    assert [(c['epoch'], c['i'], c['per_epoch'], c['epochs']) for c in lines] == [(1, 0, 2, 2), (1, 1, 2, 2), (2, 0, 2, 2), (2, 1, 2, 2)]
    assert all(c['batch_size'] == 16 and set(c['losses']) == {'ind_zdist', 'ood_zdist', 'in_zdist'} for c in lines)
    for epoch in range(2):
        # ft/job.py:401-417 in fp64: the batch's masked fp32 .mean() per group, folded into the mean weighted by the counts
        mean, n = {}, {'ind': 0, 'ood': 0, 'in': 0}
        for e, b, zin, zmix, tags in seen:
            if e != epoch:
                continue
            ind_mask = (tags == 0).to(zmix.device)
            batch_of = {'ind': zmix[ind_mask], 'ood': zmix[~ind_mask], 'in': zin}
            for grp, v in batch_of.items():
                if len(v):
                    r = float(v.mean())
                    mean[grp] = r if not n[grp] else (mean[grp] * n[grp] + r * len(v)) / (n[grp] + len(v))
                    n[grp] += len(v)
        shown = [c for c in lines if c['epoch'] == epoch + 1][-1]['losses']
        assert n['ind'] + n['ood'] == 16 and n['in'] == 16
        for grp in mean:
            got, want = shown[f'{grp}_zdist'], mean[grp]
            print(f'epoch {epoch + 1} {grp}_zdist: shown {got!r}, running-mean rule {want!r}')
            assert abs(got - want) <= 1e-6 * abs(want), (epoch, grp, got, want)


def test_finetune_refuses_named_sets():
    job, case = wim_job()
    trainset, ind, oods = loop_sets()
    with pytest.raises(NotImplementedError):
        job.finetune('cifar10', ind, oods, batch_size=8, epochs=1)
    with pytest.raises(NotImplementedError):
        job.finetune(trainset, 'cifar10', oods, batch_size=8, epochs=1)
    with pytest.raises(NotImplementedError):
        job.finetune(trainset, ind, {'svhn': 'svhn'}, batch_size=8, epochs=1)
    with pytest.raises(NotImplementedError):
        job.finetune(trainset, ind, ['svhn'], batch_size=8, epochs=1)
