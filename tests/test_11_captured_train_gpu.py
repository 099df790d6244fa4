"""GPU: train_model() with TRAIN_CAPTURED - every full-size batch of the train phase is a replay of one captured HIP graph.

The network is config 2 (conv32 / deconv32, BatchNorm on both sides) at batch size 32 on 5 x 32 + 7 = 167 device-resident
samples: five full batches and a ragged one per epoch, two epochs, KL warm-up over [0, 2] (weight 1/3, then 2/3: the
device-scalar weight takes two values), a read-back every 2 batches.  What the captured loop did is compared with the same
batches - recorded by the loop's test hook - replayed through the eager train_step() on a twin: bit for bit (the step is
deterministic and a capture reorders no arithmetic, so there is no tolerance).
"""
import math

import pytest
import torch

from oracle.cases import full_config
from oracle.det_init import load_det_state

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
N, FULL, RAGGED = 32, 5, 7
EPOCHS, WARMUP, REPORT = 2, [0, 2], 2
PER_EPOCH = FULL + 1


def _dataset(seed=0):
    g = torch.Generator().manual_seed(seed)
    n = FULL * N + RAGGED
    return torch.utils.data.TensorDataset(torch.rand(n, 3, 32, 32, generator=g).to(DEV),
                                          torch.randint(0, 10, (n,), generator=g).to(DEV))


def _net(kw, seed=0):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**kw)
    load_det_state(net, seed=seed)
    return net.to(DEV)


def _train(net, data, **kw):
    args = dict(epochs=EPOCHS, batch_size=N, warmup=WARMUP, report_every=REPORT, validation=0, device=DEV)
    args.update(kw)
    return net.train_model(data, **args)


def _recorder(log):
    def hook(epoch, i, x, y, eps, losses):
        log.append((epoch, i, x.clone(), y.clone(), eps.clone()))
    return hook


def _captured_run_and_eager_twin(kw):
    """A: two epochs through train_model() with the switch on.  B: the recorded batches through train_step().
    -> (A, B, per-epoch fp64 loss means of B, B's last Measures per epoch)"""
    a, b = _net(kw), _net(kw)
    b.load_state_dict(a.state_dict())
    a.TRAIN_CAPTURED = True
    log = []
    a._train_batch_hook = _recorder(log)
    _train(a, _dataset())
    assert len(log) == EPOCHS * PER_EPOCH
    loss_means, last_measures = [], []
    for epoch in range(EPOCHS):
        b.encoder.prior.thaw_means(epoch)
        b.train()
        w = max(0., min(1., (epoch + 1 - WARMUP[0]) / (WARMUP[1] + 1)))       # cvae.py:1787-1788
        sums, measures = {}, None
        for e, i, x, y, eps in log[epoch * PER_EPOCH:(epoch + 1) * PER_EPOCH]:
            assert e == epoch
            full_eps = torch.cat([torch.zeros_like(eps[:1]), eps])
            losses, measures = b.train_step(x, y, batch=i, current_measures=measures, kl_var_weighting=w,
                                            gamma_weighting=1., epsilon=full_eps)
            for k, v in losses.items():
                sums[k] = sums.get(k, 0.) + float(v.detach().double().mean())
            del losses
        b.eval()
        loss_means.append({k: v / PER_EPOCH for k, v in sums.items()})
        last_measures.append(dict(measures))
    return a, b, loss_means, last_measures


def _assert_same_training_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:                                  # parameters, BatchNorm running statistics and batch counts
        assert torch.equal(sa[k], sb[k]), k
    assert len(a.optimizer._groups) == len(b.optimizer._groups)
    for ga, gb in zip(a.optimizer._groups, b.optimizer._groups):
        assert ga.step == gb.step
        assert torch.equal(ga.p, gb.p)
        assert torch.equal(ga.m, gb.m), 'first Adam moment'
        assert torch.equal(ga.v, gb.v), 'second Adam moment'


@pytest.fixture(scope='module')
def pair():
    return _captured_run_and_eager_twin(full_config(2, N)['net'])


def test_captured_epochs_equal_the_same_steps_of_train_step_bit_for_bit(pair):
    a, b, _, _ = pair
    assert a._captures_built == 1               # one capture served both epochs: the KL weight is a device word
    _assert_same_training_state(a, b)


def test_history_of_the_captured_run(pair):
    a, _, loss_means, last_measures = pair
    hist = a.train_history
    assert hist['epochs'] == EPOCHS and set(hist) == {'epochs', 0, 1, 2}
    for epoch in range(EPOCHS):
        assert set(hist[epoch]) == {'train_loss', 'train_measures', 'lr'}
        got, want = hist[epoch]['train_loss'], loss_means[epoch]
        assert set(got) == set(want)
        for k in want:
            # every row is non-negative with at most (L+1) N = 64 entries: an fp32 mean in any order is within 64 x 6e-8
            print(epoch, k, got[k], want[k])
            assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (epoch, k, got[k], want[k])
        gm, wm = hist[epoch]['train_measures'], last_measures[epoch]
        assert set(gm) == set(wm)
        for k in wm:                             # running means continued across the replays
            print(epoch, k, gm[k], wm[k])
            assert abs(gm[k] - wm[k]) <= 1e-6 * abs(wm[k]), (epoch, k, gm[k], wm[k])
    assert set(a.training_parameters['sigma']) == set(a.sigma.params)


def test_capture_takes_no_extra_optimizer_step(pair):
    a, b, _, _ = pair
    steps = EPOCHS * PER_EPOCH
    assert steps == 12
    assert a.optimizer._groups[0].step == steps and b.optimizer._groups[0].step == steps
    assert float(a.optimizer._groups[0].hyper[3]) == steps          # the device-side count the replays advanced


def test_switch_off_never_builds_a_graph():
    net = _net(full_config(2, N)['net'])
    assert net.TRAIN_CAPTURED is False
    seen = []
    net._train_batch_hook = lambda epoch, i, x, y, eps, losses: seen.append((epoch, i, tuple(eps.shape), sorted(losses)))
    hist = _train(net, _dataset(), epochs=1)
    assert net._captures_built == 0 and getattr(net, '_captured_step', None) is None
    assert not getattr(net.optimizer, '_device_hyper', False)
    assert [s[:2] for s in seen] == [(0, i) for i in range(PER_EPOCH)]
    assert seen[0][2] == (1, N, 64) and seen[-1][2] == (1, RAGGED, 64) and 'total' in seen[0][3]
    assert all(math.isfinite(v) for v in hist[0]['train_loss'].values())


@pytest.mark.parametrize('captured', [True, False])
def test_nan_exit(captured, capsys):
    """A parameter poisoned at batch 1 ends the run as the eager loop ends it (print + sys.exit(1)); with the switch on
    no later than the next read-back."""
    net = _net(full_config(2, N)['net'])
    net.TRAIN_CAPTURED = captured
    seen = []

    def hook(epoch, i, x, y, eps, losses):
        seen.append((epoch, i))
        if (epoch, i) == (0, 1):
            net.encoder.dense_mean.weight.data[0, 0] = float('inf')
    net._train_batch_hook = hook
    with pytest.raises(SystemExit) as err:
        _train(net, _dataset())
    assert err.value.code == 1
    assert 'GRAD NAN' in capsys.readouterr().out
    assert seen[-1][0] == 0 and 1 < seen[-1][1] <= 1 + REPORT, seen
    if captured:
        assert net._captures_built == 1 and seen[-1] == (0, 2)       # batch 2 is a replay; its read-back ends the run


def test_thawed_prior_means_force_one_new_capture():
    kw = dict(full_config(2, N)['net'])
    kw['prior'] = dict(kw['prior'], freeze_means=1, init_mean=0.5)
    m0 = _net(kw).encoder.prior.mean.detach().clone()
    a, b, _, _ = _captured_run_and_eager_twin(kw)
    assert a._captures_built == 2               # epoch 1: mean.requires_grad came on, the key changed
    assert a.encoder.prior.mean.requires_grad
    assert not torch.equal(a.encoder.prior.mean.detach(), m0)       # the means moved from then on
    assert len(a.optimizer._groups) == 2 and a.optimizer._groups[1].step == PER_EPOCH
    _assert_same_training_state(a, b)


# ---------------------------------------------------------------------------------------------- the new kernels alone
def test_loss_sums_kernel():
    from jvae_hip import ops
    g = torch.Generator().manual_seed(3)
    shapes = [(1,), (7,), (32,), (3, 32), (513,)]
    rows = [(torch.rand(s, generator=g) * 10 ** (i - 1)).to(DEV) for i, s in enumerate(shapes)]
    want = torch.stack([r.double().mean() for r in rows]).cpu()
    acc = torch.zeros(len(rows), device=DEV)
    ops.loss_sums(rows, acc)
    once = acc.clone()
    assert ((once.cpu().double() - want).abs() <= 1e-6 * want.abs()).all(), (once, want)
    ops.loss_sums(rows, acc)
    assert ((acc.cpu().double() - 2 * want).abs() <= 1e-6 * 2 * want.abs()).all(), (acc, want)
    again = torch.zeros(len(rows), device=DEV)
    ops.loss_sums(rows, again)
    assert torch.equal(again, once)
    ops.loss_sums(rows, again)
    assert torch.equal(again, acc)
    with pytest.raises(Exception):
        ops.loss_sums([rows[0]] * 17, torch.zeros(17, device=DEV))


def _latent_once(w, prior, var_dim, seed=5):
    from jvae_hip import ops
    g = torch.Generator().manual_seed(seed)
    n, K, L, C = 37, 64, 2, 10
    mu = torch.randn(n, K, generator=g).to(DEV).requires_grad_()
    lv = (torch.randn(n, K, generator=g) * 0.5).to(DEV).requires_grad_()
    eps = torch.randn(L + 1, n, K, generator=g)
    eps[0] = 0
    y = torch.randint(0, C, (n,), generator=g).to(DEV)
    means = torch.randn(C, K, generator=g).to(DEV).requires_grad_()
    T = (torch.rand((C, K) if var_dim == 'diag' else (C,), generator=g) + 0.5).to(DEV).requires_grad_(var_dim == 'diag')
    tau = 3. if prior == 'uniform' else 0.
    alpha = 0.
    if prior == 'uniform':
        alpha = math.log(2 * tau) - math.log(2 * 0.5 * (1 + math.erf(tau / math.sqrt(2))) - 1)
    out = ops.latent(mu, lv, eps.to(DEV), y, means, T, prior=prior, var_dim=var_dim, tau=tau, alpha=alpha, w=w)
    gz = torch.randn(L + 1, n, K, generator=g).to(DEV)
    gk = torch.randn(n, generator=g).to(DEV)
    leaves = [mu, lv, means] + ([T] if T.requires_grad else [])
    grads = torch.autograd.grad([out[1], out[2], out[4]], leaves, [gz, gk, gk.flip(0)])
    return [o.detach() for o in out] + list(grads)


@pytest.mark.parametrize('w', [0., 1 / 3, 1.])
@pytest.mark.parametrize('prior,var_dim', [('gaussian', 'scalar'), ('gaussian', 'diag'), ('uniform', 'scalar')])
def test_latent_device_scalar_weight_is_bit_identical(w, prior, var_dim):
    host = _latent_once(w, prior, var_dim)
    dev = _latent_once(torch.tensor([w], dtype=torch.float32, device=DEV), prior, var_dim)
    assert len(host) == len(dev)
    for i, (h, d) in enumerate(zip(host, dev)):
        assert torch.equal(h, d), i
    if prior == 'gaussian' and w != 1.:          # the weight is really read: another value, another kl
        other = _latent_once(torch.ones(1, device=DEV), prior, var_dim)
        assert not torch.equal(other[2], dev[2])


def _elbo_once(cw, seed=7):
    from jvae_hip import ops
    g = torch.Generator().manual_seed(seed)
    n, L, D = 37, 2, 3072
    wmse_s = torch.rand(L, n, generator=g).to(DEV).requires_grad_()
    kl = (torch.rand(n, generator=g) * 30).to(DEV).requires_grad_()
    ce = (torch.rand(n, generator=g) * 3).to(DEV).requires_grad_()
    sigma = torch.tensor([0.7], device=DEV)
    out = ops.elbo(wmse_s, kl, ce, sigma, ops.SIGMA_VALUE, D, 1.5, cw)
    gt = torch.randn(n, generator=g).to(DEV)
    grads = torch.autograd.grad(out[2], [wmse_s, kl, ce], gt)
    return [o.detach() for o in out] + list(grads)


@pytest.mark.parametrize('w', [0., 1 / 3, 1.])
def test_elbo_device_scalar_weight_is_bit_identical(w):
    host = _elbo_once(w)
    dev = _elbo_once(torch.tensor([w], dtype=torch.float32, device=DEV))
    for i, (h, d) in enumerate(zip(host, dev)):
        assert torch.equal(h, d), i
    if w != 1.:
        assert not torch.equal(_elbo_once(torch.ones(1, device=DEV))[2], dev[2])
