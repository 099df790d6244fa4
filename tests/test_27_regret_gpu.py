"""Likelihood-regret OOD scores on the MI355X (cvae.likelihood_regret, ops.latent_refine, csrc/latent.hip::latent_refine_kernel,
DESIGN.md section 7o) against the restatements of tests/test_regret_restatement.py and the goldens of tests/golden/regret
(tools/gen_regret_golden.py).

Bars.  Kernel alone, warm state: those of tests/test_0_ops_gpu.py::test_latent_against_oracle - log-variance 1e-6, z 1e-5, kl and
zdist 2e-5 of the largest reference value; the moved mean is held like z and the moved raw log-variance like the clipped one
(the update is lr x a smooth function of a gradient the latent kernel has to 5e-5: far inside either).  Zero state, steps 1-3
chained: the first update is lr * g / (|g| + eps), a sign, so elements with 0 < |g64| < 1e-3 max|g64| of the case are left out
(at most 2 % of a case's elements; gated elements, whose gradient is exactly 0, stay in and must not move) and the rest is held
absolutely to lr x 5e-5, the relative gradient bar of test_latent_against_oracle.
The loop against the goldens: d <= max(3 d_ref, floor), d_ref the golden's own fp32-vs-fp64 distance - the rule of
tests/test_2_model_gpu.py and tests/test_6_odin_gpu.py.  Floor for J and the regret: 1e-4 of the largest reference value, the RTOL
of the label-free goldens.  Floor for mu and the log-variance: 2e-5 of the largest reference value, the max-norm bar of one
convolution's data gradient (tests/test_0_ops_gpu.py::test_conv_all_directions) that test_6_odin_gpu.py takes as the floor of an
input gradient through the same stacks: an Adam update is lr (0.05) times a ratio of such gradients of magnitude <= 1.
Samples left out follow the golden's rule (a decoder ReLU unit nearer to zero than the fp32 forward error), at most 1 of the 6.
Every distance is printed before its assertion."""
import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_regret_restatement import (LR, PRIORS, STEPS, decoder_gradient, left_out, load_golden, refine_step_restatement, regret_cases, step_case,
                                     uniform_alpha)
from test_roc_restatement import auc_bound, roc_restatement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEPT = [pc / 100 for pc in range(90, 100)]
SHAPES = [(1, 67, 1), (32, 5, 3), (65, 1, 1), (100, 5, 3), (65, 67, 1)]          # (K, N, L): K in {1, 32, 65, 100}, N in {1, 5, 67}
# every prior kind at every shape; the forced variance at two of them
KERNEL_CASES = [(p, v, K, N, L, False) for p, v in PRIORS for K, N, L in SHAPES] + \
               [(p, v, K, N, L, True) for p, v in PRIORS for K, N, L in ((32, 67, 3), (65, 1, 1))]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def f32(c):
    """The case with every floating tensor rounded to fp32 (what the kernel gets), still as fp64 for the restatement."""
    r = lambda t: t.float().double() if torch.is_tensor(t) and t.is_floating_point() else t
    return {k: tuple(r(t) for t in v) if isinstance(v, tuple) else r(v) for k, v in c.items()}


def dev_step(c, mu, raw, lv, state, step, lr, eps_cur, dz, eps_next):
    from jvae_hip import ops
    d = lambda t: None if t is None else t.float().to(DEV).contiguous()
    return ops.latent_refine(mu, raw, lv, c['y'].to(DEV), d(c['means']), d(c['T']), eps_cur=d(eps_cur), dz=d(dz), state=state,
                             step=step, lr=lr, eps_next=d(eps_next), prior=c['prior'], var_dim=c['var_dim'], tau=c['tau'],
                             alpha=uniform_alpha(c['tau']) if c['prior'] == 'uniform' else 0., forced_lv=c['forced_lv'])


def dev_start(c):
    """mu, raw, lv on the device after the forward-only launch (the first draw of a loop), checked on the way."""
    mu = c['mu'].float().to(DEV)
    raw = None if c['raw'] is None else c['raw'].float().to(DEV)
    lv = torch.full_like(mu, float('nan'))
    z, kl, zd, _ = dev_step(c, mu, raw, lv, None, 0, 0., None, None, c['eps_cur'])
    ref = refine_step_restatement(c['mu'], c['raw'], None, c['eps_cur'], c['y'], c['means'], c['T'], None, None, 0, 0.,
                                  c['prior'], c['var_dim'], c['tau'], True, c['forced_lv'])
    assert torch.equal(mu.cpu(), c['mu'].float()) and (raw is None or torch.equal(raw.cpu(), c['raw'].float()))
    assert rel(lv, ref['lv']) < 1e-6 and rel(z, ref['z']) < 1e-5 and rel(kl, ref['kl']) < 2e-5 and rel(zd, ref['zdist']) < 2e-5
    return mu, raw, lv


@pytest.mark.parametrize('prior,var_dim,K,N,L,forced', KERNEL_CASES)
def test_refine_kernel_warm_state(prior, var_dim, K, N, L, forced):
    c = f32(step_case(prior, var_dim, N, K, L, seed=K * 1000 + N * 10 + L, forced=forced, warm=True))
    mu, raw, lv = dev_start(c)
    state = tuple(None if (forced and i > 1) else t.float().to(DEV) for i, t in enumerate(c['state']))
    z, kl, zd, _ = dev_step(c, mu, raw, lv, state, 10, 0.05, c['eps_cur'], c['dz'], c['eps_next'])
    ref = refine_step_restatement(step=10, lr=0.05, **c)
    fig = dict(mu=rel(mu, ref['mu']), lv=rel(lv, ref['lv']), z=rel(z, ref['z']), kl=rel(kl, ref['kl']), zdist=rel(zd, ref['zdist']),
               m=rel(state[0], ref['state'][0]), v=rel(state[1], ref['state'][1]))
    if not forced:
        fig['raw'] = rel(raw, ref['raw'])
    print((prior, var_dim, K, N, L, forced), fig)
    assert fig['mu'] < 1e-5 and fig['lv'] < 1e-6 and fig['z'] < 1e-5 and fig['kl'] < 2e-5 and fig['zdist'] < 2e-5
    assert fig['m'] < 5e-5 and fig['v'] < 5e-5 and fig.get('raw', 0.) < 1e-6
    if N > 1:                                        # without the last sample, whose e^20 variance is all a max-norm over z and kl sees
        rest = dict(z=rel(z[:, :-1], ref['z'][:, :-1]), kl=rel(kl[:-1], ref['kl'][:-1]), zdist=rel(zd[:-1], ref['zdist'][:-1]))
        print('  without the last sample', rest)
        assert rest['z'] < 1e-5 and rest['kl'] < 2e-5 and rest['zdist'] < 2e-5
    if not forced:                                   # beyond the clip before and after the step
        assert K == 1 or float(lv[0, 1]) == -20.
        assert N == 1 or float(lv[N - 1, 0]) == 20.
    # the update alone (no forward) moves the posterior to the same bits and leaves lv alone
    mu2, raw2, lv2 = dev_start(c)
    state2 = tuple(None if (forced and i > 1) else t.float().to(DEV) for i, t in enumerate(c['state']))
    before = lv2.clone()
    assert dev_step(c, mu2, raw2, lv2, state2, 10, 0.05, c['eps_cur'], c['dz'], None) is None
    assert torch.equal(mu2, mu) and (forced or torch.equal(raw2, raw)) and torch.equal(lv2, before)
    assert all(a is None or torch.equal(a, b) for a, b in zip(state2, state))


@pytest.mark.parametrize('prior,var_dim,K,N,L,forced', KERNEL_CASES)
def test_refine_kernel_zero_state_chained(prior, var_dim, K, N, L, forced):
    lr = 0.1
    c = f32(step_case(prior, var_dim, N, K, L, seed=K * 1000 + N * 10 + L + 13, forced=forced, warm=False))      # + 13: the
    # first offset from 7 on at which the fp64 reference leaves out at most 2 % of every case (a property of the inputs alone)
    g = torch.Generator().manual_seed(K + N + L)
    noise = [c['eps_cur']] + [torch.randn(L + 1, N, K, generator=g).double() for _ in range(3)]
    grads = [c['dz']] + [decoder_gradient(L, N, K, g).float().double() for _ in range(2)]
    for t in noise:
        t[0] = 0
    mu, raw, lv = dev_start(c)
    state = tuple(None if (forced and i > 1) else t.float().to(DEV) for i, t in enumerate(c['state']))
    ref = dict(mu=c['mu'], raw=c['raw'], state=c['state'])
    out_mu, out_lv = torch.zeros(N, K, dtype=torch.bool), torch.zeros(N, K, dtype=torch.bool)
    for s in range(3):
        z, kl, zd, _ = dev_step(c, mu, raw, lv, state, s + 1, lr, noise[s], grads[s], noise[s + 1])
        ref = refine_step_restatement(ref['mu'], ref['raw'], noise[s], noise[s + 1], c['y'], c['means'], c['T'], grads[s],
                                      ref['state'], s + 1, lr, prior, var_dim, c['tau'], True, c['forced_lv'])
        for gr, out in ((ref['g_mu'], out_mu), (ref['g_lv'], out_lv)):
            out |= (gr.abs() > 0) & (gr.abs() < 1e-3 * gr.abs().max())
        n_out = int(out_mu.sum()) + (0 if forced else int(out_lv.sum()))
        share = n_out / (N * K * (1 if forced else 2))
        d_mu = float((mu.double().cpu() - ref['mu'])[~out_mu].abs().max())
        d_lv = 0. if forced else float((raw.double().cpu() - ref['raw'])[~out_lv].abs().max())
        print((prior, var_dim, K, N, L, forced), 'step', s + 1, 'left out', n_out, 'share', share, 'mu', d_mu, 'raw', d_lv,
              'bar', lr * 5e-5)
        assert share <= 0.02
        assert d_mu <= lr * 5e-5 and d_lv <= lr * 5e-5
    if not forced:                                   # gated elements never moved: exactly the input's bits
        assert K == 1 or float(raw[0, 1]) == -30.
        assert N == 1 or float(raw[N - 1, 0]) == 25.


def test_refine_argument_checks():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    c = f32(step_case('gaussian', 'scalar', 4, 8, 1, seed=3))
    mu, raw, lv = dev_start(c)
    y, means, T = c['y'].to(DEV), c['means'].float().to(DEV), c['T'].float().to(DEV)
    eps = c['eps_cur'].float().to(DEV)
    with pytest.raises(JvaeHipError):
        ops.latent_refine(mu, raw, lv, y, means, T)                                   # neither an update nor a forward
    with pytest.raises(JvaeHipError):
        ops.latent_refine(mu.t().contiguous().t(), raw, lv, y, means, T, eps_next=eps)    # not contiguous: no copy can stand in
    with pytest.raises(JvaeHipError):
        ops.latent_refine(mu, raw, lv, y, means, T, eps_cur=eps, dz=eps, state=ops.latent_refine_state(mu), step=0, lr=.1)
    with pytest.raises(JvaeHipError):
        ops.latent_refine(mu, raw, lv, torch.full((4,), 5), means, T, eps_next=eps)   # a host label outside [0, C)
    bad = y.clone()
    bad[2] = 5                                                                        # on the device: never an index, NaN
    z, kl, _, _ = ops.latent_refine(mu, raw, lv, bad, means, T, eps_next=eps)
    assert bool(kl[2].isnan()) and bool(z[:, 2].isnan().all()) and not bool(kl[[0, 1, 3]].isnan().any())


# ------------------------------------------------------------------------------------------- the loop
def build(name):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(regret_cases()[name][0]))
    load_det_state(net, seed=0)
    net.to(DEV)
    net.eval()
    return net


_RUNS = {}


def golden_run(name):
    """One product run per case, shared by the tests that read it (never modified)."""
    if name not in _RUNS:
        gd = load_golden(name)
        net = build(name)
        x, y, eps = (torch.from_numpy(gd[k]).to(DEV) for k in ('x', 'y', 'eps'))
        traj = []
        out = net.likelihood_regret(x, y, steps=STEPS, lr=LR, epsilon=eps, trajectory=traj)
        _RUNS[name] = (net, gd, x, y, eps, out, traj)
    return _RUNS[name]


def check_against_golden(name, gd, regret, traj, tag=''):
    keep = torch.from_numpy(~left_out(gd))
    got = dict(mu=torch.stack([t[0] for t in traj]), lv=torch.stack([t[1] for t in traj]), J=torch.stack([t[2] for t in traj]))
    floors = dict(mu=2e-5, lv=2e-5, J=1e-4, regret=1e-4)
    for key in ('mu', 'lv', 'J'):
        d = rel(got[key][:, keep], torch.from_numpy(gd[key + '64'])[:, keep])
        bar = max(3 * float(gd['d_ref_' + key]), floors[key])
        print(name, tag, key, 'distance', d, 'reference', float(gd['d_ref_' + key]), 'bar', bar)
        assert d <= bar
    d = rel(regret[keep], torch.from_numpy(gd['regret64'])[keep])
    bar = max(3 * float(gd['d_ref_regret']), floors['regret'])
    print(name, tag, 'regret distance', d, 'reference', float(gd['d_ref_regret']), 'bar', bar, 'left out', int((~keep).sum()))
    assert d <= bar


@pytest.mark.parametrize('name', sorted(regret_cases()))
def test_loop_against_the_golden(name):
    net, gd, x, y, eps, (regret, mu, lv), traj = golden_run(name)
    assert len(traj) == STEPS + 1 and torch.equal(traj[-1][0], mu) and torch.equal(traj[-1][1], lv)
    check_against_golden(name, gd, regret, traj)


@pytest.mark.parametrize('name', ['ra2_n6_vae', 're2_n6_cvae'])
def test_zero_steps_and_repeatability(name):
    net, gd, x, y, eps, out, _ = golden_run(name)
    regret, mu, lv = net.likelihood_regret(x, y, steps=0, epsilon=eps[:1])
    pm, plv = net.latent_posterior(x)
    assert torch.equal(regret, torch.zeros_like(regret)) and torch.equal(mu, pm) and torch.equal(lv, plv)
    again = net.likelihood_regret(x, y, steps=STEPS, lr=LR, epsilon=eps)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    torch.manual_seed(5)
    drawn = net.likelihood_regret(x, y, steps=2, lr=LR)                # noise drawn on the device: finite, positive on average
    assert bool(drawn[0].isfinite().all()) and float(drawn[0].mean()) > 0


def test_nothing_leaks():
    net, gd, x, y, eps, out, _ = golden_run('re2_n6_cvae')
    net.train()
    params = list(net.named_parameters())
    for i, (_, p) in enumerate(params):
        p.grad = None if i % 3 == 0 else torch.full_like(p, float(i))
    flags = [p.requires_grad for _, p in params]
    buffers = {k: v.clone() for k, v in net.named_buffers()}
    try:
        got = net.likelihood_regret(x, y, steps=STEPS, lr=LR, epsilon=eps)
        assert net.training and net.latent_sampling == net._latent_samplings['train']
    finally:
        net.eval()
    assert all(torch.equal(a, b) for a, b in zip(out, got))             # evaluation mode inside, whatever the flag was
    assert [p.requires_grad for _, p in params] == flags
    for i, (k, p) in enumerate(params):
        assert (p.grad is None) if i % 3 == 0 else torch.equal(p.grad, torch.full_like(p, float(i))), k
        p.grad = None
    for k, v in net.named_buffers():
        assert torch.equal(v, buffers[k]), k
    assert any(k.endswith('running_var') for k in buffers) and any(k.endswith('num_batches_tracked') for k in buffers)


def test_supplied_and_predicted_class_agree():
    net, gd, x, y, eps, _, _ = golden_run('re2_n6_cvae')
    first = torch.cat((torch.zeros_like(eps[0, :1]), eps[0]), 0)
    with torch.no_grad():
        _, logits, losses, _ = net.evaluate(x, epsilon=first)
    pred = net.predict_after_evaluate(logits, losses)
    a = net.likelihood_regret(x, None, steps=STEPS, lr=LR, epsilon=eps)
    b = net.likelihood_regret(x, pred, steps=STEPS, lr=LR, epsilon=eps)
    c = net.likelihood_regret(x, None, steps=STEPS, lr=LR, epsilon=eps, evaluated=(logits, losses))
    assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a, b, c))


@pytest.mark.parametrize('name', ['re2_n6_cvae', 'rm2_n6_cvae_mlp'])
def test_slabs(name, monkeypatch):
    net, gd, x, y, eps, one, _ = golden_run(name)
    monkeypatch.setenv('JVAE_EVAL_SLAB_ROWS', '4')                      # (L + 1) = 3 rows per sample: one sample per slab
    assert net._eval_slab_rows() == 4
    traj = []
    regret, mu, lv = net.likelihood_regret(x, y, steps=STEPS, lr=LR, epsilon=eps, trajectory=traj)
    print(name, 'slabs against one slab: regret', rel(regret, one[0]), 'mu', rel(mu, one[1]), 'lv', rel(lv, one[2]))
    check_against_golden(name, gd, regret, traj, 'slabs')


def synth(n, name, seed, shift=0.):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset((torch.rand(n, 1, 28, 28, generator=g) + shift).clamp(0, 1), torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


def test_rates(monkeypatch):
    net = build('rm2_n6_cvae_mlp')
    net.REGRET_PARAMS = [(2, 0.05), (1, 0.1)]
    names = ['regret-2-0.0500', 'regret-1-0.1000']
    sets = [synth(40, 'ind', 1), synth(40, 'ood', 2, .3)]
    for m in ('regret*', names[0]):                                     # off: refused by name
        with pytest.raises(NotImplementedError, match='regret'):
            net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=16, method=m)
    assert not any(m.startswith('regret') for m in net._ood_methods('all'))
    net.OOD_REGRET_METHODS = True
    assert net._ood_methods('all')[-2:] == names
    recorders = {}
    torch.manual_seed(11)
    first = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=16, method=['elbo', 'regret*'],
                                    recorders=recorders, update_self_ood=False)
    assert list(first['ood']) == ['elbo'] + names
    for m in names:
        ins, outs = (recorders[s][m].float().cpu().numpy() for s in ('ind', 'ood'))
        assert ins.shape == outs.shape == (40,) and np.isfinite(ins).all() and np.isfinite(outs).all()
        r = first['ood'][m]
        auc, fpr, tpr, low, up = roc_restatement(ins, outs, KEPT)
        print(m, 'auc', r['auc'], 'restated', auc, 'mean regret in / out', -ins.mean(), -outs.mean())
        assert r['n'] == 40 and r['fpr'] == fpr.tolist() and abs(r['auc'] - auc) <= auc_bound(40)
        assert [t[0] for t in r['thresholds']] == low.tolist()
    assert 'regret-2-0.0500' not in net.test_losses                    # test_losses: the loss components only
    calls = []
    real_eval, real_regret = net.evaluate, net.likelihood_regret
    monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append('e') or real_eval(*a, **k))
    monkeypatch.setattr(net, 'likelihood_regret', lambda *a, **k: calls.append('r') or real_regret(*a, **k))
    again = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=16, method=['elbo', 'regret*'],
                                    recorders=recorders, update_self_ood=False)
    assert not calls and again == first                                 # a full recorder is read back: no refinement runs
    one = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=16, method=names[1], update_self_ood=False)
    # one evaluate per batch serves both the rows and the class: 3 batches per set, every pair of REGRET_PARAMS per batch
    assert list(one['ood']) == [names[1]] and calls.count('r') == 12 and calls.count('e') == 6
    scores = net.regret_scores(sets[0].tensors[0][:5].to(DEV))
    assert list(scores) == names and all(v.shape == (5,) for v in scores.values())


def test_refusals():
    from cvae import ClassificationVariationalNetwork as Net
    x = torch.rand(4, 3, 32, 32, device=DEV)
    for case, what in (('eb2_n8_vib_L2', 'vib'), ('j2_n8_jvae', 'jvae'), ('eg2_n4_categorical_L2', 'categorical')):
        net = Net(**dict(get_case(case)['net'])).to(DEV)
        with pytest.raises(NotImplementedError, match=what):
            net.likelihood_regret(x)
    net = Net(**dict(get_case('e2_n8_rmse_L2')['net'])).to(DEV)
    with pytest.raises(NotImplementedError, match='is_rmse'):
        net.likelihood_regret(x)
    net = Net(**dict(get_case('e2_n8_L3')['net'])).to(DEV)
    with pytest.raises(ValueError):
        net.likelihood_regret(x, epsilon=torch.zeros(2, 3, 4, 64, device=DEV), steps=3)
    net.set_compute_dtype('bf16')
    with pytest.raises(NotImplementedError, match='fp32'):
        net.likelihood_regret(x)
