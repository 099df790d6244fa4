"""ODIN out-of-distribution scores of vib models on the MI355X (cvae.odin_scores, csrc/odin.hip, the eval-mode BatchNorm backward
and the few-channel input gradient) against the reference's goldens of tests/golden/odin (tools/gen_odin_golden.py) and, where a
case has no golden, against the plain-torch restatement of tests/test_odin_restatement.py, which reproduces every golden.

Bars.  Scores: 1e-4 of the largest reference value - RTOL of the label-free evaluation goldens (tests/test_2_model_gpu.py).
Input gradient: max-norm distance to the reference's fp64 gradient relative to max|g64|, held to max(3 x the reference's own
fp32-vs-fp64 distance stored in the golden, 2e-5): the factor 3 is the one the training-step gradients are held to against
`grad64.*` (test_2_model_gpu.py: d <= max(3 d_ref, floor)); the floor is the max-norm bar of ONE convolution's data gradient
(tests/test_0_ops_gpu.py::test_conv_all_directions, 2e-5), which a chain of four such layers on the split-bf16 matrix-core
kernels cannot be asked to beat.  Measured reference distances: 4.7e-7 .. 5.0e-7 (eb2_n8_vib_L2), 6.6e-7 .. 6.8e-7 (leaky),
1.9e-7 .. 2.0e-7 (MLP); the product's figures are printed before each assertion."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.det_init import load_det_state
from test_odin_restatement import det_state, load_golden, odin_cases, odin_restatement
from test_roc_restatement import auc_bound, roc_restatement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RTOL = 1e-4
CASES = sorted(odin_cases())
KEPT = [pc / 100 for pc in range(90, 100)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def build(name, temps=None, sizes=None):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(odin_cases()[name]))
    load_det_state(net, seed=0)
    net.to(DEV)
    net.eval()
    if temps is not None:
        net.ODIN_TEMPS, net.ODIN_EPS = list(temps), list(sizes)
    return net


def golden_net(name):
    gd = load_golden(name)
    net = build(name, gd['temps'].tolist(), gd['sizes'].tolist())
    return net, gd, torch.from_numpy(gd['x']).to(DEV), torch.from_numpy(gd['eps_noise']).to(DEV)


def left_out(gd):
    """Samples whose fp64 forward has a ReLU unit closer to zero than the fp32 forward error: at most 1 of the 8."""
    out = gd['preact_min64'] < gd['preact_err32']
    assert out.sum() <= 1
    return out


@pytest.mark.parametrize('name', CASES)
def test_input_gradient_against_the_fp64_reference(name):
    net, gd, x, noise = golden_net(name)
    accs = []
    net.odin_scores(x, epsilon=noise, acc_out=accs)
    keep = ~left_out(gd)
    for t, acc in enumerate(accs):
        g64 = gd['acc64'][t][keep]
        err = float(np.abs(acc.double().cpu().numpy()[keep] - g64).max() / np.abs(g64).max())
        bar = max(3 * float(gd['grad_err'][t]), 2e-5)
        print(name, 'T', gd['temps'][t], 'gradient error', err, 'reference', float(gd['grad_err'][t]), 'bar', bar)
        assert err <= bar


@pytest.mark.parametrize('N,C,P,act', [(3, 32, 1024, 1), (5, 7, 81, 2), (8, 64, 256, 0), (1, 3, 64, 1)])
def test_eval_batchnorm_backward(N, C, P, act):
    """jvae_bn_eval_bwd_f32 through both BatchNorm ops against fp64 torch; bar: test_batchnorm_train's for the input gradient."""
    from jvae_hip import ops
    g = torch.Generator().manual_seed(N * 100 + C)
    H = int(P ** .5)
    x, gy = torch.randn(N, C, H, P // H, generator=g), torch.randn(N, C, H, P // H, generator=g)
    gamma, beta = 1 + .3 * torch.randn(C, generator=g), .3 * torch.randn(C, generator=g)
    rm, rv = .3 * torch.randn(C, generator=g), 1 + .5 * torch.rand(C, generator=g)
    xr = x.double().requires_grad_(True)
    yr = F.batch_norm(xr, rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, 1e-5)
    yr = {0: lambda t: t, 1: torch.relu, 2: F.leaky_relu}[act](yr)
    yr.backward(gy.double())
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    xd = x.to(DEV).requires_grad_(True)
    gd_, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    yd = ops.batchnorm_act(xd, gd_, bd, rm.to(DEV), rv.to(DEV), nbt, False, act, C=C)
    assert rel(yd, yr) < 1e-5
    gx, = torch.autograd.grad(yd, xd, gy.to(DEV))
    print('eval BatchNorm backward', (N, C, P, act), rel(gx, xr.grad))
    assert rel(gx, xr.grad) < 1e-4
    xa, aff = ops.batchnorm_defer(xd, gd_, bd, rm.to(DEV), rv.to(DEV), nbt, False, act, C=C)      # the deferred form: same backward
    gx2, = torch.autograd.grad(xa, xd, gy.to(DEV))
    assert torch.equal(gx2, gx) and int(nbt) == 0


@pytest.mark.parametrize('N,cin,H', [(3, 3, 32), (7, 1, 32), (5, 3, 64), (2, 4, 32), (3, 3, 16)])
def test_few_channel_input_gradient(N, cin, H):
    """The data gradient of a Conv2d(cin <= 4 -> 32, 5x5, padding 2) - the vector-ALU route at 32 / 64 wide, the older routes at
    16 - against fp64 torch at the bar of test_conv_all_directions."""
    from jvae_hip import ops
    g = torch.Generator().manual_seed(N * 10 + cin + H)
    x = torch.randn(N, cin, H, H, generator=g)
    w = torch.randn(32, cin, 5, 5, generator=g) / (cin * 25) ** .5
    gy = torch.randn(N, 32, H, H, generator=g)
    xr = x.double().requires_grad_(True)
    F.conv2d(xr, w.double(), None, padding=2).backward(gy.double())
    spec = ops.ConvSpec(cin, 32, 5, 1, 2)
    gx = ops.conv_dgrad_raw(gy.to(DEV), w.to(DEV), spec, tuple(x.shape))
    print('few-channel dgrad', (N, cin, H), rel(gx, xr.grad))
    assert rel(gx, xr.grad) < 2e-5
    xd = x.to(DEV).requires_grad_(True)
    gx2, = torch.autograd.grad(ops.conv2d(xd, w.to(DEV), None, spec), xd, gy.to(DEV))
    assert torch.equal(gx2, gx)


def test_head_and_perturb_kernels():
    from jvae_hip import ops
    g = torch.Generator().manual_seed(3)
    for Fw, L, N, C in ((3, 2, 8, 10), (1, 16, 100, 100), (5, 1, 7, 3), (2, 3, 33, 17)):
        lg = torch.randn(Fw, L + 1, N, C, generator=g) * 3
        lg[0, 1:, 0, :] = 0.5                                       # a full tie: the first index wins
        temps = torch.tensor([1., 10., 1000., 2., 5.][:Fw])
        lr = lg.double().requires_grad_(True)
        p = (lr[:, 1:].mean(1) / temps.double()[:, None, None]).softmax(-1)
        sr = p.max(-1)[0]
        sr.sum().backward()
        s, d = ops.odin_head(lg.to(DEV), temps.to(DEV), want_grad=True)
        assert rel(s, sr) < 1e-5 and rel(d, lr.grad) < 1e-5 and float(d[:, 0].abs().max()) == 0
        assert float(d[0, 1, 0, 0]) > 0 and float(d[0, 1, 0, 1:].max()) < 0
        s2 = ops.odin_head(lg.transpose(0, 1).contiguous().to(DEV), temps.to(DEV), forwards_first=False)
        assert torch.equal(s2, s)
    for shape in ((8, 3, 32, 32), (5, 1, 3, 3)):
        x, acc0, gr = (torch.randn(shape, generator=g) for _ in range(3))
        acc0[0, 0, 0] = 0
        gr[0, 0, 0] = 0
        eps = torch.tensor([0., 0.0014, 0.004])
        acc = acc0.clone().to(DEV)
        out = ops.odin_perturb(acc, gr.to(DEV), x.to(DEV), eps.to(DEV))
        ref = torch.cat([x + e * (acc0 + gr).sign() for e in eps])
        assert torch.equal(acc.cpu(), acc0 + gr) and torch.equal(out.cpu(), ref)
        out2 = ops.odin_perturb(acc, None, x.to(DEV), eps.to(DEV))
        assert torch.equal(out2, out) and torch.equal(acc.cpu(), acc0 + gr)


def batched_scores(net, gd, x, noise, signs):
    """The perturbed half of odin_scores with given signs: perturb kernel (acc = sign, g = 0), batched forward, head."""
    from jvae_hip import ops
    T, E, N = len(net.ODIN_TEMPS), len(net.ODIN_EPS), x.shape[0]
    L, K, C = net.latent_sampling, net.latent_dim, net.num_labels
    e_dev = torch.tensor(net.ODIN_EPS, dtype=torch.float32, device=DEV)
    rows = []
    with torch.no_grad():
        for t in range(T):
            acc = signs[t].float().contiguous()
            xp = ops.odin_perturb(acc, torch.zeros_like(acc), x, e_dev)
            slab = net._odin_slab_rows()
            fp = torch.cat([net._features_of(xp[r:r + slab]).reshape(min(slab, E * N - r), -1) for r in range(0, E * N, slab)])
            lg = net._odin_logits(fp, noise[t, 1:].transpose(0, 1).reshape(L + 1, E * N, K))
            temps = torch.full((E,), float(net.ODIN_TEMPS[t]), device=DEV)
            rows.append(ops.odin_head(lg.view(L + 1, E, N, C), temps, forwards_first=False))
    return torch.stack(rows)


@pytest.mark.parametrize('name', CASES)
def test_scores_given_the_reference_signs(name, monkeypatch):
    monkeypatch.setenv('JVAE_EVAL_SLAB_ROWS', '7')
    net, gd, x, noise = golden_net(name)
    sc = batched_scores(net, gd, x, noise, torch.from_numpy(gd['sign']).to(DEV))
    print(name, 'scores given the signs', rel(sc, torch.from_numpy(gd['scores32'])))
    assert rel(sc, torch.from_numpy(gd['scores32'])) < RTOL


@pytest.mark.parametrize('name', CASES)
def test_odin_scores_end_to_end(name):
    net, gd, x, noise = golden_net(name)
    accs = []
    scores = net.odin_scores(x, epsilon=noise, acc_out=accs)
    assert list(scores) == gd['names'].tolist()
    a64 = gd['acc64']
    T = a64.shape[0]
    mine = np.stack([np.sign(a.cpu().numpy()) for a in accs])
    flipped = mine != gd['sign']
    for t in range(T):
        tau = float(gd['grad_err'][t])
        assert np.all(np.abs(a64[t])[flipped[t]] <= tau * np.abs(a64[t]).max()), (name, t)
    share = float(flipped.mean())
    print(name, 'flipped sign elements', int(flipped.sum()), 'share', share)
    assert share <= 0.005
    g64 = np.diff(np.concatenate([np.zeros_like(a64[:1]), a64]), axis=0)              # the gradient of each temperature's score
    l1 = float(np.abs(g64).reshape(T, a64.shape[1], -1).sum(-1).max())
    ref = torch.from_numpy(gd['scores32']).reshape(-1, x.shape[0])
    got = torch.stack([scores[k] for k in gd['names'].tolist()]).cpu()
    bar = RTOL * float(ref.abs().max()) + 2 * max(net.ODIN_EPS) * share * l1
    err = float((got.double() - ref.double()).abs().max())
    print(name, 'score error', err, 'bar', bar)
    assert err <= bar


def test_structure(monkeypatch):
    name = 'eb2_n8_vib_L2'
    net, gd, x, noise = golden_net(name)
    T, E, N = len(net.ODIN_TEMPS), len(net.ODIN_EPS), x.shape[0]
    entered = []
    real = type(net.features).forward
    monkeypatch.setattr(type(net.features), 'forward', lambda self, t: entered.append(t.shape[0]) or real(self, t))
    before = [p.requires_grad for p in net.parameters()]
    results = {}
    for slab in (5, 4096):
        monkeypatch.setenv('JVAE_EVAL_SLAB_ROWS', str(slab))
        del entered[:]
        results[slab] = net.odin_scores(x, epsilon=noise)
        print('slab', slab, 'features entered', len(entered), 'times:', entered)
        assert len(entered) <= T * -(-E * N // slab) + T and max(entered) <= max(slab, N)
    for k in results[5]:
        assert torch.equal(results[5][k], results[4096][k]), k
    again = net.odin_scores(x, epsilon=noise)
    assert all(torch.equal(again[k], results[4096][k]) for k in again)
    assert all(p.grad is None for p in net.parameters()) and [p.requires_grad for p in net.parameters()] == before
    drawn = net.odin_scores(x)                                       # without injection: its own draws, same keys
    assert list(drawn) == list(again) and all(v.shape == (N,) and v.is_cuda for v in drawn.values())
    count = {'n': 0}
    for attr in ('cpu', 'item', 'tolist', 'numpy'):
        real_m = getattr(torch.Tensor, attr)

        def counted(self, *a, _real=real_m, **k):
            count['n'] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, attr, counted)
    net.odin_scores(x, epsilon=noise)
    assert count['n'] == 0


def test_full_grid_against_the_restatement():
    """10 x 21 grid, N = 100, the MLP case (no golden): the scores given the restatement's own fp64 signs."""
    name = 'mb2_n8_vib_L2_mlp'
    kw = odin_cases()[name]
    net = build(name)
    assert len(net.ODIN_TEMPS) == 10 and len(net.ODIN_EPS) == 21
    g = torch.Generator().manual_seed(9)
    N, L, K = 100, kw['test_latent_sampling'], kw['latent_dim']
    x = torch.rand((N, *kw['input_shape']), generator=g)
    noise = torch.randn((10, 22, L + 1, N, K), generator=g)
    noise[:, :, 0] = 0
    acc64, sc64 = odin_restatement(kw, det_state(kw, torch.float64), x.double(), noise.double(), net.ODIN_TEMPS, net.ODIN_EPS)
    sc = batched_scores(net, None, x.to(DEV), noise.to(DEV), acc64.sign().to(DEV))
    print('full grid, scores given the signs', rel(sc, sc64))
    assert rel(sc, sc64) < RTOL
    accs = []
    scores = net.odin_scores(x.to(DEV), epsilon=noise.to(DEV), acc_out=accs)
    assert len(scores) == 210
    for t in (0, 9):
        err = rel(accs[t], acc64[t])
        print('full grid gradient error, temperature', t, err)
        assert err <= 2e-5


def synth(n, name, seed, shift=0.):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset((torch.rand(n, 3, 32, 32, generator=g) + shift).clamp(0, 1),
                                       torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


def test_public_interface(tmp_path, monkeypatch):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.recorders import LossRecorder
    from oracle.cases import get_case
    net = build('eb2_n8_vib_L2', [1, 10], [0, 0.0014])
    assert len(Net.methods_params['odin']) == 210
    methods = net._ood_methods('all')
    odin = ['odin-1-0.0000', 'odin-1-0.0014', 'odin-10-0.0000', 'odin-10-0.0014']
    assert methods == ['baseline', 'logits'] + odin and net._ood_methods('odin*') == odin
    sets = [synth(150, 'ind', 1), synth(90, 'ood', 2, .3)]
    torch.manual_seed(31)
    res = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64)
    assert list(res['ood']) == methods

    torch.manual_seed(31)
    by_hand = []
    for d in sets:
        rows, measures = {m: [] for m in methods}, None
        with torch.no_grad():
            for i, (xb, _) in enumerate(torch.utils.data.DataLoader(d, batch_size=64, num_workers=0, shuffle=False)):
                xb = net._device_batch(xb.to(DEV))
                _, logits, losses, measures = net.evaluate(xb, batch=i, current_measures=measures)
                sc = net.batch_dist_measures(logits, dict(losses, **net.odin_scores(xb)), methods)
                for m in methods:
                    rows[m].append(sc[m].float().cpu().numpy())
        by_hand.append({m: np.concatenate(rows[m]) for m in methods})
    for m in methods:
        r = res['ood'][m]
        auc, fpr, tpr, low, up = roc_restatement(by_hand[0][m], by_hand[1][m], KEPT)
        print(m, 'auc', r['auc'], 'restated', auc)
        assert r['n'] == 90 and r['fpr'] == fpr.tolist() and abs(r['auc'] - auc) <= auc_bound(150)
        assert [t[0] for t in r['thresholds']] == low.tolist()

    recorders = {}
    first = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64, recorders=recorders,
                                    sample_dirs=[str(tmp_path)], update_self_ood=False)
    for d in sets:
        rec = LossRecorder.load(os.path.join(tmp_path, f'record-{d.name}.pth'), device=DEV)
        assert rec.recorded_samples == len(d) and set(odin) <= set(rec.keys())
    calls = []
    real_eval, real_odin = net.evaluate, net.odin_scores
    monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append(1) or real_eval(*a, **k))
    monkeypatch.setattr(net, 'odin_scores', lambda *a, **k: calls.append(1) or real_odin(*a, **k))
    again = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64, recorders=recorders, update_self_ood=False)
    assert not calls and again == first
    one = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64, method='odin-10-0.0014', update_self_ood=False)
    assert list(one['ood']) == ['odin-10-0.0014'] and calls
    with pytest.raises(ValueError):
        net._ood_methods('odin-3-0.0014')

    cvae_net = Net(**dict(get_case('e2_n8_L3')['net'])).to(DEV)
    with pytest.raises(NotImplementedError):
        cvae_net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], method='odin-10-0.0014')
    net.set_compute_dtype('bf16')
    with pytest.raises(NotImplementedError):
        net.odin_scores(torch.rand(4, 3, 32, 32, device=DEV))
