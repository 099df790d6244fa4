"""Chained models on the device: the two kernels of csrc/cascad.hip (ops.cascade_mse, ops.iterate_prior) and module.cascad,
against the fp64 restatement and the inputs of tests/test_cascad_restatement.py and what the REFERENCE's module/cascad.py
returned (tools/gen_cascad_golden.py -> tests/golden/cascad).

Bars.  Kernels: the rule of tests/test_17_aggregation_gpu.py (its `Worst`): of each tensor the largest error against the fp64
restatement is at most 4 x the largest error the fp32 torch expressions of the reference show on the same inputs, both relative
to the largest magnitude of the tensor; torch's error counts as at least one fp32 ulp; a non-finite error fails.  Exact where
the arithmetic is: two calls, and a view and its 16-byte aligned copy, give the same bits; a sample beside an all-zero stage is
bit-identical to the run without it.  Models: every stacked loss, `mse`, `Im-1`, `Im-5` and `y_` of both golden chains within
1e-4 of the golden tensor's largest magnitude (the project's parity bar; on the reference a 1e-4 relative perturbation of the
input moves each of them by less than 2e-6 of that magnitude, so the compounding through the stages has room); `Im-T` bit
for bit the chain ops.class_posterior -> ops.latent_mutual_info on the cascade's own z, `mse` bit for bit ops.cascade_mse on
its own x_.

Measured on the MI355X (error against fp64 relative to the largest magnitude: kernel, and in brackets fp32 torch on the same
inputs):
    cascade_mse   (1, 1, 1, 1) 8.14e-09 (8.14e-09)    (2, 3, 7, 75) 4.53e-08 (8.17e-08)     (3, 3, 8, 3072) 4.25e-08 (7.57e-08)
                  (8, 2, 5, 257) 2.84e-08 (9.69e-08)  (3, 16, 65, 192) 4.21e-08 (1.44e-07)  (2, 1, 300, 12) 3.81e-08 (1.29e-07)
                  views (2, 3, 7, 75) 4.53e-08 (8.17e-08), (3, 2, 5, 257) 3.85e-08 (7.75e-08)
                  peak rise at (3, 16, 65, 3072): 39 936 bytes (one stage: 12 779 520)
    iterate_prior (1, 1, 1) 0 (0)   (2, 2, 7) 3.24e-08 (4.46e-08)   (3, 10, 65) 4.19e-08 (1.82e-07)
                  (8, 128, 300) 7.31e-08 (3.53e-07)   (5, 100, 1) 3.10e-08 (5.07e-08)   golden 4.19e-08 (1.82e-07)
Not measured yet: the differences of the two chains to their goldens (test_cascade_of_models_against_the_reference prints
them per tensor; the model-level tests have not run on an MI355X).
"""
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import det_inputs, load_det_state
from test_17_aggregation_gpu import DEV, Worst, dev, same_bits
from test_cascad_restatement import (CHAIN_N, CHAIN_TEMPS, CHAIN_X_SEED, CHAINS, ITER_SHAPES, MSE_SHAPES, iter64, iter_inputs,
                                     load_golden, mse64, mse_inputs, pairs, torch_iter, torch_mse)

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------- 1. stage-pair MSE
@pytest.mark.parametrize('shape', MSE_SHAPES, ids=str)
def test_cascade_mse_against_the_fp64_restatement(shape):
    from jvae_hip import ops
    M, L, N, D = shape
    x, stages = mse_inputs(*shape)
    dx, ds = dev(x), [dev(s) for s in stages]
    mse = ops.cascade_mse(dx, ds)
    assert tuple(mse.shape) == (M * (M + 1) // 2, N) and mse.dtype == torch.float32
    assert same_bits(mse, ops.cascade_mse(dx, ds))
    w = Worst(f'cascade_mse {shape}')
    w.check(mse, torch_mse(x, stages), mse64(x, stages), shape)
    w.report()
    # image-shaped arguments are the same call
    if D == 3072:
        assert same_bits(mse, ops.cascade_mse(dx.view(N, 3, 32, 32), [s.view(L, N, 3, 32, 32) for s in ds]))


@pytest.mark.parametrize('shape', [(2, 3, 7, 75), (3, 2, 5, 257)], ids=str)
def test_cascade_mse_takes_the_views_of_odd_sized_reconstructions(shape):
    """Stages that are the [1:] views of (L + 1, N, D) tensors with N D odd: the base pointer is 4-byte aligned only."""
    from jvae_hip import ops
    M, L, N, D = shape
    assert N * D % 2 == 1
    x, stages = mse_inputs(*shape)
    full = [torch.cat([torch.full((1, N, D), float('nan')), torch.from_numpy(s)]).to(DEV) for s in stages]
    views = [f[1:] for f in full]
    assert all(v.data_ptr() % 16 and v.data_ptr() == f.data_ptr() + 4 * N * D for v, f in zip(views, full))
    before = [f.clone() for f in full]
    mse = ops.cascade_mse(dev(x), views)
    assert all(same_bits(f, b) for f, b in zip(full, before))
    w = Worst(f'cascade_mse views {shape}')
    w.check(mse, torch_mse(x, stages), mse64(x, stages), shape)
    w.report()
    assert same_bits(mse, ops.cascade_mse(dev(x), [dev(s) for s in stages]))


def test_cascade_mse_gives_the_same_bits_on_both_load_paths():
    """D % 4 == 0 with every base aligned takes the 16-byte loads; the same data one float further on takes the 4-byte loads."""
    from jvae_hip import ops
    M, L, N, D = 3, 5, 6, 260
    x, stages = mse_inputs(M, L, N, D)
    aligned = ops.cascade_mse(dev(x), [dev(s) for s in stages])
    shifted = []
    for s in stages:
        flat = torch.empty(s.size + 1, device=DEV)
        flat[1:].copy_(torch.from_numpy(s).reshape(-1))
        shifted.append(flat[1:].view(L, N, D))
    assert all(s.data_ptr() % 16 == 4 and s.is_contiguous() for s in shifted)
    assert same_bits(aligned, ops.cascade_mse(dev(x), shifted))
    Worst('cascade_mse shifted').check(aligned, torch_mse(x, stages), mse64(x, stages), (M, L, N, D))


def test_cascade_mse_adds_less_memory_than_one_stage():
    from jvae_hip import ops
    M, L, N, D = 3, 16, 65, 3072
    x = torch.rand(N, D, device=DEV)
    stages = [torch.rand(L, N, D, device=DEV) for _ in range(M)]
    ops.cascade_mse(x, stages)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    mse = ops.cascade_mse(x, stages)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f'peak rise {rise} bytes, one stage {L * N * D * 4}, mse {mse.numel() * 4}')
    assert rise < L * N * D * 4


# --------------------------------------------------------------------------------------------- 2. sequential update
@pytest.mark.parametrize('shape', ITER_SHAPES, ids=str)
def test_iterate_prior_against_the_fp64_restatement(shape):
    from jvae_hip import ops
    p = iter_inputs(*shape)
    post = ops.iterate_prior(dev(p))
    assert tuple(post.shape) == shape and same_bits(post, ops.iterate_prior(dev(p)))
    w = Worst(f'iterate_prior {shape}')
    w.check(post, torch_iter(p), iter64(p), shape)
    w.report()


def test_iterate_prior_a_zero_stage_is_nan_from_there_on_in_its_sample_only():
    from jvae_hip import ops
    from module.cascad import iterate_with_prior
    M, C, N = 4, 10, 65
    p = iter_inputs(M, C, N)
    clean = ops.iterate_prior(dev(p))
    p[2, :, 17] = 0.
    post = iterate_with_prior(dev(p))
    keep = torch.arange(N, device=DEV) != 17
    assert bool(torch.isfinite(post[:2, :, 17]).all()) and same_bits(post[:2], clean[:2])
    assert bool(torch.isnan(post[2:, :, 17]).all())
    assert same_bits(post[:, :, keep], clean[:, :, keep])
    exact = iter64(p)
    assert np.array_equal(np.isnan(exact), torch.isnan(post).cpu().numpy())


def test_iterate_prior_on_the_golden():
    from jvae_hip import ops
    from test_cascad_restatement import ITER_GOLDEN
    g = load_golden('iterate')
    p = iter_inputs(*ITER_GOLDEN)
    w = Worst('iterate_prior golden')
    w.check(ops.iterate_prior(dev(p)), float(g['err']), iter64(p), ITER_GOLDEN)
    w.report()


# --------------------------------------------------------------------------------------------- 3. refusals of the wrappers
def test_wrappers_refuse_before_any_launch():
    from jvae_hip import JvaeHipError, ops
    x = torch.rand(4, 6, device=DEV)
    s = torch.rand(2, 4, 6, device=DEV)
    for bad in (lambda: ops.cascade_mse(x, [s] * 9), lambda: ops.cascade_mse(x, []),
                lambda: ops.cascade_mse(x, [s, torch.rand(3, 4, 6, device=DEV)]), lambda: ops.cascade_mse(x, [s, s[:, :, :5]]),
                lambda: ops.cascade_mse(x[:, :5], [s]), lambda: ops.cascade_mse(x, [s.transpose(0, 1)]),
                lambda: ops.cascade_mse(x.cpu(), [s]), lambda: ops.cascade_mse(x, [s, s.cpu()]),
                lambda: ops.cascade_mse(x.double(), [s.double()]),
                lambda: ops.iterate_prior(torch.rand(9, 3, 4, device=DEV)), lambda: ops.iterate_prior(torch.rand(2, 129, 4, device=DEV)),
                lambda: ops.iterate_prior(torch.rand(3, 4, device=DEV)), lambda: ops.iterate_prior(torch.rand(2, 3, 4))):
        with pytest.raises(JvaeHipError):
            bad()
    assert tuple(ops.cascade_mse(x[:0], [s[:, :0]]).shape) == (1, 0)


# --------------------------------------------------------------------------------------------- 4. models
def drop_in(name, seed, device=DEV):
    from cvae import ClassificationVariationalNetwork as Net
    torch.manual_seed(0)
    net = Net(**get_case(name)['net'])
    load_det_state(net, seed=seed)
    return net.to(device).eval()


@pytest.mark.parametrize('chain', list(CHAINS))
def test_cascade_of_models_against_the_reference(chain):
    from jvae_hip import ops
    from module.cascad import CascadModels
    g = load_golden(chain)
    name, seeds = CHAINS[chain]
    kw = get_case(name)['net']
    M, N, C = len(seeds), CHAIN_N, kw['num_labels']
    nets = [drop_in(name, s) for s in seeds]
    L = nets[0].latent_sampling
    seen = []
    for net in nets:                                               # what every stage was given and what it returned
        def spy(x, *a, _real=net.evaluate, **k):
            out = _real(x, *a, **k)
            seen.append((x, out))
            return out
        net.evaluate = spy
    model = CascadModels(*nets)
    model.eval()
    assert all(not n.training for n in nets) and len(list(model.parameters())) == sum(len(list(n.parameters())) for n in nets)
    x = det_inputs(N, kw['input_shape'], C, 1, kw['latent_dim'], seed=CHAIN_X_SEED)[0].to(DEV)
    eps = [dev(g[f'eps{i}']) for i in range(M)]
    with torch.no_grad():
        x_, y_, losses, measures = model.evaluate(x, z_output=True, temps=CHAIN_TEMPS, epsilon=eps)
    assert tuple(x_.shape) == (M, L + 1, N) + tuple(kw['input_shape']) and tuple(y_.shape) == (M, N, C)
    # stage k + 1 read x_reco[1] of stage k where it lies
    assert len(seen) == M and seen[0][0] is x
    for k in range(M - 1):
        assert seen[k + 1][0].data_ptr() == seen[k][1][0][1].data_ptr() and same_bits(seen[k + 1][0], x_[k][1])
    stage_in = torch.stack([s[0] for s in seen]).reshape(M, N, -1)
    worst = 0.
    compared = {'stage_in': stage_in, 'y_': y_, 'mse': losses['mse']}
    compared.update({f'Im-{T}': losses[f'Im-{T}'] for T in CHAIN_TEMPS})
    compared.update({'loss.' + k: v for k, v in losses.items() if 'loss.' + k in g})
    assert sorted(k for k in g if k.startswith('loss.')) == sorted(k for k in compared if k.startswith('loss.'))
    assert sorted(losses) == sorted([k[5:] for k in g if k.startswith('loss.')] + ['mse'] + [f'Im-{T}' for T in CHAIN_TEMPS])
    for k, v in compared.items():
        ref = g[k]
        assert tuple(v.shape) == ref.shape, k
        d = float(np.abs(v.double().cpu().numpy() - ref).max()) / float(np.abs(ref).max())
        worst = max(worst, d)
        print(f'{chain} {k}: {d:.2e} of the largest magnitude')
        assert d <= 1e-4, (k, d)
    print(f'{chain}: the largest difference to the golden {worst:.2e}')
    assert sorted(measures) == sorted(k[8:] for k in g if k.startswith('measure.'))
    for k, v in measures.items():                                  # running means of one batch: the parity bar again
        ref = g['measure.' + k]
        assert tuple(v.shape) == (M,) and ref.shape == (M,), k
        d = float(np.abs(v.double().numpy() - ref).max()) / float(np.abs(ref).max())
        print(f'{chain} measure.{k}: {d:.2e} of the largest magnitude')
        assert d <= 1e-4, (k, d)
    # mse: the one-pass kernel on the cascade's own reconstructions, and in the reference's row order
    assert same_bits(losses['mse'], ops.cascade_mse(x, [x_[k][1:] for k in range(M)]))
    for p, (i, j) in enumerate(pairs(M)):
        a, b = x_[i - 1][1:], (x_[j - 1][1:] if j else x.unsqueeze(0))
        row = (a - b).pow(2).mean((0, 2, 3, 4))
        assert float((losses['mse'][p] - row).abs().max()) <= 1e-5 * float(row.max()), (i, j)
    # Im-T: the op chain on the cascade's own draws
    P = []
    for (_, out), net in zip(seen, nets):
        z = out[-1][1:]
        assert tuple(z.shape) == (L, N, kw['latent_dim'])
        pr = net.encoder.prior
        P.append(ops.class_posterior(z, pr.mean.detach(), pr._var_parameter.detach(), pr.log_det_per_class().detach(),
                                     var_dim=pr.var_dim, temps=CHAIN_TEMPS, logp=False)[1])
    rows = [ops.latent_mutual_info(P[i], P[j]) for i in range(M) for j in range(i)]
    for t, T in enumerate(CHAIN_TEMPS):
        assert same_bits(losses[f'Im-{T}'], torch.stack([r[t] for r in rows]))
    # predictions
    logits = y_.permute(0, 2, 1)
    top, arg = model.predict_after_evaluate(logits, losses, method='iter')
    want = logits[-1].max(0)
    assert same_bits(top, want[0]) and same_bits(arg, want[1])
    assert same_bits(model.predict_after_evaluate(logits, losses, method='iws'), losses['iws'][-1].argmax(0))
    # without z_output: no Im rows, the same mse
    with torch.no_grad():
        _, _, plain, _ = model.evaluate(x, epsilon=eps)
    assert not [k for k in plain if k.startswith('Im-')] and same_bits(plain['mse'], losses['mse'])


def test_cascade_refusals_by_name():
    from cvae import ClassificationVariationalNetwork as Net
    from module.cascad import CascadModels
    base = Net(**get_case('e2_n8_L3')['net'])
    with pytest.raises(ValueError, match='latent_sampling'):
        CascadModels(base, Net(**get_case('e2_n16_L16')['net']))
    other = dict(get_case('e2_n8_L3')['net'], input_shape=(1, 32, 32))
    with pytest.raises(ValueError, match='input_shape'):
        CascadModels(base, Net(**other))
    with pytest.raises(NotImplementedError, match='coded labels'):
        CascadModels(Net(**get_case('j2_n8_jvae')['net']))
    with pytest.raises(NotImplementedError, match='categorical'):
        CascadModels(Net(**get_case('eg2_n4_categorical_L2')['net']))
    with pytest.raises(ValueError, match='decoder'):
        CascadModels(Net(**get_case('eb2_n8_vib_L2')['net']))
    with pytest.raises(ValueError, match='models'):
        CascadModels()
    kw = get_case('c2_n8_tilted')['net']
    tilted = CascadModels(Net(**kw).to(DEV).eval(), Net(**kw).to(DEV).eval())
    x = det_inputs(4, kw['input_shape'], 10, 1, kw['latent_dim'])[0].to(DEV)
    with pytest.raises(NotImplementedError, match='tilted'):
        tilted.evaluate(x, z_output=True)
    with pytest.raises(NotImplementedError, match='without labels'):
        tilted.evaluate(x, torch.zeros(4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match='temperatures'):
        tilted.evaluate(x, z_output=True, temps=[None, 1])
    with torch.no_grad():
        x_, y_, losses, _ = tilted.evaluate(x)                     # without z_output any prior runs
    assert tuple(losses['mse'].shape) == (3, 4) and tuple(x_.shape)[:3] == (2, tilted.latent_sampling + 1, 4)


# --------------------------------------------------------------------------------------------- 5. record_sets
def test_record_sets_writes_the_recorder_and_the_samples(tmp_path):
    from jvae_compat.recorders import LossRecorder
    from module.cascad import CascadModels, record_sets
    name = 'e2_n8_L3'
    kw = get_case(name)['net']
    nets = [drop_in(name, s) for s in (0, 1)]
    for i, net in enumerate(nets):
        net.training_parameters['set'] = 'letters'
        net.job_number = 40 + i
    model = CascadModels(*nets)
    n, M, L, C = 10, 2, nets[0].latent_sampling, kw['num_labels']
    x, y, _ = det_inputs(n, kw['input_shape'], C, 1, kw['latent_dim'], seed=7)
    sets = {'letters': torch.utils.data.TensorDataset(x, y), 'digits': torch.utils.data.TensorDataset(x.flip(0), y.flip(0))}
    where = record_sets(model, sets, batch_size=4, temps=[1, 5], job_dir=str(tmp_path / 'cascad-jobs'))
    assert where == model.saved_dir == os.path.join(str(tmp_path / 'cascad-jobs'), 'letters', '40-41')
    assert sorted(os.listdir(where)) == sorted(['params.json', 'test.json', 'ood.json'] + [f'{k}-{s}.pth' for k in ('record', 'sample')
                                                                                          for s in sets])
    for s in sets:
        rec = LossRecorder.load(os.path.join(where, f'record-{s}.pth'))
        assert rec.recorded_samples == n and len(rec) == 3 and rec.batch_size == 4 and rec.last_batch_size == 2
        want = {'kl': (M, C, n), 'zdist': (M, C, n), 'var_kl': (M, C, n), 'total': (M, C, n), 'iws': (M, C, n), 'dzdist': (M, n),
                'wmse': (M, n), 'cross_x': (M, n), 'mse': (3, n), 'Im-1': (1, n), 'Im-5': (1, n), 'y_true': (n,), 'logits': (M, C, n)}
        assert {k: tuple(rec[k].shape) for k in rec.keys()} == want
        labels = y if s == 'letters' else y.flip(0)
        assert torch.equal(rec['y_true'].cpu(), labels)
        samples = torch.load(os.path.join(where, f'sample-{s}.pth'))
        assert sorted(samples) == ['x', 'x_', 'y']
        assert tuple(samples['x'].shape) == (6,) + tuple(kw['input_shape']) and tuple(samples['y'].shape) == (6,)
        assert tuple(samples['x_'].shape) == (M, 2, 6) + tuple(kw['input_shape'])
        images = x if s == 'letters' else x.flip(0)
        keep = [0, 1, 4, 5, 8, 9]
        assert torch.equal(samples['x'], images[keep]) and torch.equal(samples['y'], labels[keep])
        assert bool(torch.isfinite(samples['x_']).all())
