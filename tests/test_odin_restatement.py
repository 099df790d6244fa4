"""The ODIN loop of the reference (cvae.py:1645-1663) restated in plain torch, with torch.autograd.grad with respect to x only.

It reproduces every golden of tests/golden/odin (generated from the reference by tools/gen_odin_golden.py) - scores and
accumulated gradients at fp64 rounding when run in fp64, signs identical - and is therefore the checker of the GPU tests
(tests/test_6_odin_gpu.py) for cases without a golden: the full 10 x 21 grid, N = 100.  The role tests/test_roc_restatement.py
plays for the ROC.

oracle/jvae_oracle.py::make_spec restates type 'cvae' only, so the vib forward is written out here: the conv stack through the
oracle's run_stack(..., training=False), then the dense heads, the draws and the classifier as torch expressions on the
deterministic state of oracle/det_init.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import jvae_oracle as O
from oracle.cases import get_case
from oracle.det_init import det_tensor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'odin')
FULL_TEMPS = [m * 10 ** i for i in (0, 1, 2) for m in (1, 2, 5)] + [1000]
FULL_EPS = [k / 20 * 0.004 for k in range(21)]


def odin_cases():
    """The model kwargs of the goldens (as tools/gen_odin_golden.py builds them)."""
    base = dict(get_case('eb2_n8_vib_L2')['net'])
    mlp = dict(base, input_shape=(1, 28, 28), features=None, encoder=[64], batch_norm=False, latent_dim=16)
    return {'eb2_n8_vib_L2': base, 'eb2_n8_vib_L2_leaky': dict(base, activation='leaky'), 'mb2_n8_vib_L2_mlp': mlp}


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def det_state(kw, dtype):
    """The deterministic state of the model `kw`, keyed as its state_dict (key / shape list from the drop-in on the CPU)."""
    from cvae import ClassificationVariationalNetwork as Net
    return {k: det_tensor(k, v.shape).to(dtype) if v.dtype.is_floating_point else v.clone()
            for k, v in Net(**kw).state_dict().items()}


def vib_logits(kw, P, x, eps):
    """forward(x)[1] of an eval-mode vib model: x (N, ...), eps (L+1, N, K) with eps[0] = 0 -> logits (L+1, N, C)."""
    act = kw.get('activation', 'relu')
    h = x
    if kw.get('features'):
        layers = O.parse_stack(kw['features'], kw['input_shape'], False)
        h = O.run_stack(P, 'features', layers, kw['batch_norm'] in ('encoder', 'both'), x, None, training=False, hidden_act=act)
    h = h.flatten(1)
    for i in range(len(kw['encoder'])):
        h = O._act(F.linear(h, P[f'encoder.dense_projs.{2 * i}.weight'], P[f'encoder.dense_projs.{2 * i}.bias']), act)
    mu = F.linear(h, P['encoder.dense_mean.weight'], P['encoder.dense_mean.bias'])
    log_var = F.linear(h, P['encoder.dense_log_var.weight'], P['encoder.dense_log_var.bias']).clip(-20, 20)
    z = mu + torch.exp(0.5 * log_var) * eps                                   # layers.py:243 (is_sampled: beta > 0)
    n = len(kw['classifier'])
    for i in range(n):
        z = O._act(F.linear(z, P[f'classifier.{2 * i}.weight'], P[f'classifier.{2 * i}.bias']), act)
    return F.linear(z, P[f'classifier.{2 * n}.weight'], P[f'classifier.{2 * n}.bias'])


def odin_restatement(kw, P, x, noise, temps, sizes, signs=None):
    """-> (accumulated gradients (T, N, ...), scores (T, E, N)).  noise (T, 1+E, L+1, N, K): slot [t, 0] the gradient pass of
    temperature t, [t, 1+e] perturbed forward e.  signs (T, N, ...): use these instead of sign(acc) (the scores given a sign)."""
    def score(xx, eps, T):
        return (vib_logits(kw, P, xx, eps)[1:].mean(0) / T).softmax(-1).max(-1)[0]
    acc = torch.zeros_like(x)
    accs, scores = [], []
    for t, T in enumerate(temps):
        xg = x.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad(score(xg, noise[t, 0], T).sum(), xg)
        acc = acc + g                                                        # x.grad is never zeroed: cvae.py:1655-1656
        accs.append(acc)
        dx = acc.sign() if signs is None else signs[t].to(x.dtype)
        with torch.no_grad():
            scores.append(torch.stack([score(x + eps * dx, noise[t, 1 + e], T) for e, eps in enumerate(sizes)]))
    return torch.stack(accs), torch.stack(scores)


@pytest.mark.parametrize('name', sorted(odin_cases()))
def test_restatement_reproduces_the_golden(name):
    """fp64: gradients and scores at fp64 rounding (1e-12 relative to the largest: sums of < 1e4 terms of mixed sign), signs of
    the fp32 run identical; fp32: inside the reference's own fp32-vs-fp64 error (a few of it: another summation order)."""
    kw, gd = odin_cases()[name], load_golden(name)
    temps, sizes = gd['temps'].tolist(), gd['sizes'].tolist()
    x, noise = torch.from_numpy(gd['x']), torch.from_numpy(gd['eps_noise'])
    acc, sc = odin_restatement(kw, det_state(kw, torch.float64), x.double(), noise.double(), temps, sizes)
    for t in range(len(temps)):
        err = float((acc[t] - torch.from_numpy(gd['acc64'][t])).abs().max() / np.abs(gd['acc64'][t]).max())
        print(name, 'T', temps[t], 'fp64 gradient error', err)
        assert err <= 1e-12
    err = float((sc - torch.from_numpy(gd['scores64'])).abs().max())
    print(name, 'fp64 score error', err)
    assert err <= 1e-12
    acc32, sc32 = odin_restatement(kw, det_state(kw, torch.float32), x, noise, temps, sizes)
    assert np.array_equal(acc32.sign().numpy().astype(np.int8), gd['sign'])
    for t in range(len(temps)):
        err = float((acc32[t].double() - torch.from_numpy(gd['acc64'][t])).abs().max() / np.abs(gd['acc64'][t]).max())
        print(name, 'T', temps[t], 'fp32 gradient error', err, 'reference', gd['grad_err'][t])
        assert err <= 4 * gd['grad_err'][t]
    assert float((sc32 - torch.from_numpy(gd['scores32'])).abs().max()) <= 1e-5


@pytest.mark.parametrize('name', sorted(odin_cases()))
def test_the_committed_seed_keeps_the_reference_inside_the_caps(name):
    """What tests/test_6_odin_gpu.py allows the product, the reference's own fp32 run needs none of: no sample is left out
    (no ReLU unit of the fp64 forward closer to zero than the fp32 forward error) and its signs differ from the fp64 run's
    in at most 0.5 % of the elements - all of them where |acc64| <= tau * max|acc64|, tau the measured gradient error."""
    gd = load_golden(name)
    assert int((gd['preact_min64'] < gd['preact_err32']).sum()) == 0
    flips = np.sign(gd['acc32']) != np.sign(gd['acc64'])
    assert flips.mean() <= 0.005 and abs(flips.mean() - gd['flips32']) < 1e-12
    for t in range(flips.shape[0]):
        tau = gd['grad_err'][t]
        assert np.all(np.abs(gd['acc64'][t])[flips[t]] <= tau * np.abs(gd['acc64'][t]).max())


def test_full_grid_names_and_first_order_effect():
    """The 10 x 21 grid on the MLP case (no golden): 210 names as the reference formats them, eps = 0 scores independent of
    the sign, and the score moves with eps to first order as the gradient says (the sign is the steepest-ascent direction:
    the score of the temperature's own gradient cannot fall for a small eps when the noise is shared)."""
    kw = odin_cases()['mb2_n8_vib_L2_mlp']
    names = ['odin-{:.0f}-{:.4f}'.format(T, e) for T in FULL_TEMPS for e in FULL_EPS]
    assert len(names) == len(set(names)) == 210 and names[0] == 'odin-1-0.0000' and names[-1] == 'odin-1000-0.0040'
    from cvae import ClassificationVariationalNetwork as Net
    assert Net.methods_params['odin'] == names and Net(**kw)._odin_names() == names
    g = torch.Generator().manual_seed(5)
    N, L, K = 100, kw['test_latent_sampling'], kw['latent_dim']
    x = torch.rand((N, *kw['input_shape']), generator=g, dtype=torch.float64)
    one = torch.randn((L + 1, N, K), generator=g, dtype=torch.float64)
    one[0] = 0
    noise = one.expand(len(FULL_TEMPS), 1 + len(FULL_EPS), L + 1, N, K)          # shared noise: the effect of eps alone
    acc, sc = odin_restatement(kw, det_state(kw, torch.float64), x, noise, FULL_TEMPS, FULL_EPS)
    assert sc.shape == (10, 21, N) and acc.shape == (10, N, *kw['input_shape'])
    # first temperature: acc is its own gradient, so d(score)/d(eps) = |g|_1 >= 0 at eps = 0
    l1 = acc[0].abs().flatten(1).sum(1)
    slope = (sc[0, 1] - sc[0, 0]) / FULL_EPS[1]
    assert torch.all(slope >= 0) and float(((slope - l1).abs() / l1).median()) < 0.2
