"""The OOD phase of train_model (TRAIN_OOD_PHASE), batch_dist_measures(out=...) and the class-axis score rows of csrc/misclass.hip
(kinds 5 .. 13 of ops.misclass_scores).

Kernel rows: the checker is the reference's own expression (test_ood_rows_restatement.reference_row, cvae.py:985-1068) evaluated by
torch on the CPU in float64 on the same fp32 inputs.  Inputs: C in {1, 2, 3, 10, 128} x N in {1, 63, 64, 70, 193} x a class spread
of 1, 30 and 3000 (at 3000, the all-class ELBO of an image, every exp but the largest underflows); from N = 3 on, one column with a
NaN and one with C equal values.  The bar, per kind and spread (the inputs of one scale): the largest distance from the fp64 value
of the SAME expression evaluated by torch in fp32 on the GPU, times two, plus one fp32 ulp of the result; a NaN must sit where the
fp64 value has one.  `mag`, `neg` and `id` are bit-equal to torch.  `nstd` and `IYx` cancel when the classes are nearly equal; they
are measured on the same inputs as the others: the smallest spread here is 1, for which the fp32 torch expression stays finite, and
the column of exactly equal values gives exactly 0 on every side.

Largest distance from fp64 over all inputs of a spread, kernel / torch fp32, measured on the MI355X:
    kind    spread 1                  spread 30                 spread 3000
    lse-    5.434e-07 / 5.015e-07     3.816e-06 / 3.816e-06     4.678e-04 / 4.678e-04
    lse+    1.154e-06 / 1.120e-06     1.294e-05 / 1.287e-05     9.355e-04 / 9.355e-04
    mean    3.990e-07 / 3.421e-07     3.709e-06 / 3.709e-06     2.264e-04 / 2.264e-04
    std     1.632e-07 / 2.055e-07     5.738e-06 / 5.789e-06     4.255e-04 / 5.992e-04
    nstd    4.861e-06 / 3.384e-06     1.926e-04 / 1.889e-04     6.026e-05 / 5.418e-05
    IYx     5.022e-07 / 5.022e-07     8.417e-07 / 7.735e-07     1.733e-07 / 3.675e-07
    mag     bit-equal (2.384e-07, 7.629e-06, 4.883e-04 from fp64 on both sides); neg, id: bit-equal, 0
(at the larger spreads the distance is half an ulp of a result of that size: both sides are as close as fp32 gets).
"""
import json
import logging
import math
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_ood_rows_restatement import (CLASSES, EXACT_KINDS, FLAT_KINDS, NEW_KINDS, SAMPLES, SPREADS, make_source, reference_row,
                                       ulp32)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def same_bits(a, b):
    """Bit-equal, a NaN standing for any NaN (its sign and payload are not part of a score)."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and \
        a.nan_to_num(nan=0.).numpy().tobytes() == b.nan_to_num(nan=0.).numpy().tobytes()


# ---------------------------------------------------------------------------------------------- 1. the new kinds against fp64
def kernel_rows(v_dev, specs):
    from jvae_hip import ops
    return ops.misclass_scores(v_dev, specs)


def measure_kind(kind, C, spread, run_kernel=kernel_rows, device=DEV):
    """-> per N: (kernel fp32 row, torch fp32 row, fp64 row) for the inputs of one (kind, C, spread)."""
    const = math.log(C) if kind == 'lse+' else 0.
    const32 = float(np.float32(const))
    out = []
    for N in SAMPLES:
        v = make_source(1 if kind in FLAT_KINDS else C, N, spread, seed=1000 * C + N)
        exact = reference_row(kind, v.double(), const32)
        v_dev = v.to(device)
        got = run_kernel(v_dev, [(kind, const32)])[0].cpu().double()
        by_torch = reference_row(kind, v_dev, const).cpu().double()
        out.append((N, got, by_torch, exact))
    return out


def distance(row, exact):
    """Largest |row - exact| over the columns where the fp64 value is a number; the NaN columns must agree."""
    nan = exact.isnan()
    assert torch.equal(row.isnan(), nan), (row, exact)
    return float((row - exact)[~nan].abs().max()) if (~nan).any() else 0.


@pytest.mark.parametrize('kind', NEW_KINDS + FLAT_KINDS)
def test_new_kinds_against_fp64(kind):
    for spread in SPREADS:
        runs = [r for C in ((1,) if kind in FLAT_KINDS else CLASSES) for r in
                [(C,) + t for t in measure_kind(kind, C, spread)]]
        torch_dist = max(distance(t, e) for _, _, _, t, e in runs)
        kernel_dist = max(distance(g, e) for _, _, g, _, e in runs)
        print(f'{kind:5} spread {spread:6g}: kernel {kernel_dist:.3e}  torch fp32 {torch_dist:.3e}')
        for C, N, got, by_torch, exact in runs:
            if kind in EXACT_KINDS:
                assert same_bits(got.float(), by_torch.float()), (kind, C, N, spread)
                continue
            ok = ~exact.isnan()
            over = (got - exact).abs()[ok] - (2 * torch_dist + ulp32(exact[ok]))
            assert not len(over) or float(over.max()) <= 0, (kind, C, N, spread, float(over.max()), kernel_dist, torch_dist)
    if kind == 'std':                                      # torch.std of one class is 0 / 0
        assert bool(measure_kind('std', 1, 1.)[0][1].isnan().all())


# ---------------------------------------------------------------------------------------------- 2. kinds 0 .. 4 are unchanged
def test_old_kinds_are_unchanged_in_a_mixed_launch():
    from jvae_hip import ops
    old = [('soft-', 1.), ('soft-', 5.), ('soft+', 1.), ('soft+', 20.), ('max-', 1.), ('max+', 1.), ('hyz', 1.)]
    for C, N in ((10, 193), (128, 70), (3, 1), (1, 64)):
        v = make_source(C, N, 1., seed=C + N).to(DEV)
        alone = ops.misclass_scores(v, old)
        mixed = [(k, 0.) for k in NEW_KINDS] + old[:3] + [('lse+', 2.)] + old[3:] + [(k, 0.) for k in NEW_KINDS[::-1]]
        got = ops.misclass_scores(v, mixed)
        at = [i for i, s in enumerate(mixed) if s in old and ops.MISCLASS_KINDS[s[0]] < 5]
        assert len(at) == len(old) and same_bits(got[at], alone), (C, N)
        # ... and through out= / rows= / col= into a wider buffer, whose other cells stay as they were
        buf = torch.full((len(mixed) + 2, N + 5), -7., device=DEV)
        rows = list(range(1, len(mixed) + 1))
        ops.misclass_scores(v, mixed, out=buf, rows=rows, col=3)
        assert same_bits(buf[1:-1, 3:3 + N], got)
        buf[1:-1, 3:3 + N] = -7.
        assert bool((buf == -7.).all())
    from jvae_hip.lib import JvaeHipError
    v = torch.zeros(4, 8, device=DEV)
    for bad in (dict(specs=[('neg', 0.)]), dict(specs=[('lse-', float('inf'))]), dict(specs=[('soft-', 0.)]),
                dict(specs=[('std', 0.)], out=torch.zeros(2, 10, device=DEV), rows=[0], col=3)):
        with pytest.raises(JvaeHipError):
            ops.misclass_scores(v, **bad)


# ---------------------------------------------------------------------------------------------- 3. batch_dist_measures
def synth(n, name, seed, shift=0.):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset((torch.rand(n, 3, 32, 32, generator=g) + shift).clamp(0, 1),
                                       torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


def build_net(case):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case(case)['net']))
    load_det_state(net, seed=0)
    net.to(DEV)
    return net


SIX = ['sum', 'mean', 'std', 'nstd', 'mag', 'IYx']
# bit-identical between batch_dist_measures(out=...) and the plain call: pure max / negation rows, and the median row
BIT_IDENTICAL = ['max', 'elbo', 'elbo-2s', 'zdist', 'kl', 'mse', 'wmse', 'mag']
ROW_KIND = {'sum': 'lse-', 'iws': 'lse+', 'mean': 'mean', 'std': 'std', 'nstd': 'nstd', 'IYx': 'IYx'}


def test_batch_dist_measures_of_a_label_free_evaluation(monkeypatch):
    from jvae_hip import ops
    net = build_net('e2_n8_L3')
    net.eval()
    x = synth(70, 'ind', 1)[:][0].to(DEV)
    torch.manual_seed(5)
    with torch.no_grad():
        _, logits, losses, _ = net.evaluate(x)
        plain = net.batch_dist_measures(logits, losses, SIX)          # NotImplementedError before the six names were built
        for m in SIX:
            assert plain[m].shape == (70,) and bool(torch.isfinite(plain[m]).all()), m
            want = reference_row(ROW_KIND.get(m, m), losses['total'].cpu().double())
            print(m, 'plain (torch fp32) vs fp64', float((plain[m].cpu().double() - want).abs().max()))
        methods = SIX + [m for m in BIT_IDENTICAL if m not in SIX] + ['iws', 'iws-2s', 'soft', 'softkl-10', 'softzdist-5', 'softiws', 'softiws-2']
        plain = net.batch_dist_measures(logits, losses, methods)
        launches = []
        real = ops.misclass_scores
        monkeypatch.setattr(ops, 'misclass_scores', lambda src, specs, **k: launches.append(len(specs)) or real(src, specs, **k))
        buf = torch.full((len(methods) + 1, 100), -7., device=DEV)
        rows = list(range(len(methods), 0, -1))
        into = net.batch_dist_measures(logits, losses, methods, out=buf, rows=rows, col=20)
    assert list(into) == methods and sum(launches) == len(methods)
    assert len(launches) == 6                                      # total, zdist, kl, cross_x, wmse, iws: one launch each
    assert bool((buf[0] == -7.).all() and (buf[:, :20] == -7.).all() and (buf[:, 90:] == -7.).all())
    C = net.num_labels
    for m, r in zip(methods, rows):
        assert into[m].data_ptr() == buf[r, 20:].data_ptr() and into[m].shape == (70,)
        if m in BIT_IDENTICAL:
            assert same_bits(into[m], plain[m]), m
            continue
        base = m[:-3] if m.endswith('-2s') else m
        if base in ROW_KIND:                                           # the bar of section 1, on this evaluation's losses
            src = losses['iws' if base == 'iws' else 'total'].cpu().double()
            exact = reference_row(ROW_KIND[base], src, float(np.float32(math.log(C))) if base == 'iws' else 0.)
            bar = 2 * float((plain[m].cpu().double() - exact).abs().max()) + ulp32(exact)
        else:       # softmax rows, 1 / sum_c exp <= 1, against the plain call: twice the bound (C - 1) + 2 half-ulps of an fp32
            # sum of C rounded exponentials and a division, once for either side
            exact, bar = plain[m].cpu().double(), torch.full((70,), 2 * (C + 1) * 2. ** -24, dtype=torch.float64)
        err = (into[m].cpu().double() - exact).abs()
        print(m, 'out= vs reference', float(err.max()), 'bar', float(bar.max()))
        assert bool((err <= bar).all()), (m, float(err.max()))
    # the fall-backs: a non-fp32 source and more classes than the kernel stages go through the torch expressions
    monkeypatch.setattr(ops, 'misclass_scores', real)
    wide = {'total': make_source(130, 9, 30., 1)[:, :6].contiguous().to(DEV)}
    half = {'total': losses['total'].double()}
    for lo, n in ((wide, 6), (half, 70)):
        buf = torch.zeros((2, n), device=DEV)
        got = net.batch_dist_measures(None, lo, ['max', 'sum'], out=buf)
        want = net.batch_dist_measures(None, lo, ['max', 'sum'])
        assert same_bits(got['max'], want['max'].float()) and same_bits(got['sum'], want['sum'].float())


def test_score_set_rows_are_those_of_the_plain_call():
    """ood_detection_rates fills its buffers through batch_dist_measures(out=...); the rows it stores are, bit for bit, what
    the plain call gives on the same batches for every method of the cvae table (SCORE_SET_TORCH_ROWS - `iws`, `elbo`, the
    softmax rows - by their torch expressions, the others by the kernel)."""
    net = build_net('e2_n8_L3')
    net.eval()
    dset = synth(137, 'ind', 2)
    methods = net._ood_methods('all') + ['max', 'kl', 'wmse']
    torch.manual_seed(9)
    buf = net._score_set(dset, methods, 64, 3, False, None, [])
    torch.manual_seed(9)
    rows, measures = {m: [] for m in methods}, None
    with torch.no_grad():
        for i, (x, _) in enumerate(torch.utils.data.DataLoader(dset, batch_size=64, shuffle=False)):
            _, logits, losses, measures = net.evaluate(x.to(DEV), batch=i, current_measures=measures)
            for m, v in net.batch_dist_measures(logits, losses, methods).items():
                rows[m].append(v)
    assert buf.shape == (len(methods), 137)
    for r, m in enumerate(methods):
        assert same_bits(buf[r], torch.cat(rows[m])), m


# ---------------------------------------------------------------------------------------------- 4. train_model
class Sig:
    sig = 0


def run_training(tmp_path, caplog, monkeypatch, on):
    from cvae import ClassificationVariationalNetwork as Net
    torch.manual_seed(5)
    net = Net(**dict(get_case('c2_n8')['net'])).to(DEV)
    assert Net.TRAIN_OOD_PHASE is False
    if on:
        net.TRAIN_OOD_PHASE = True
    trainset, testset = synth(160, 'synth', 31), synth(70, 'synth', 32)
    oodsets = [synth(50, 'ood-a', 33, .3), synth(33, 'ood-b', 34, -.2)]
    calls = []
    real = net.evaluate
    monkeypatch.setattr(net, 'evaluate', lambda x, *a, **k: calls.append((net.trained, len(a) + ('y' in k), x.shape[0]))
                        or real(x, *a, **k))
    save_dir = str(tmp_path / 'job')
    with caplog.at_level(logging.WARNING):
        net.train_model(trainset, epochs=2, batch_size=32, test_batch_size=32, full_test_every=1, ood_detection_every=1,
                        validation=32, device=DEV, testset=testset, oodsets=oodsets, save_dir=save_dir, signal_handler=Sig())
    return net, save_dir, testset, oodsets, calls


def test_train_model_runs_the_ood_phase(tmp_path, caplog, monkeypatch):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.recorders import LossRecorder
    net, save_dir, testset, oodsets, calls = run_training(tmp_path, caplog, monkeypatch, on=True)
    assert not [r for r in caplog.records if 'OOD' in r.getMessage() or 'phase skipped' in r.getMessage()]
    methods = net._ood_methods('all')
    assert set(net.ood_results) >= {1, 2}
    for epoch in (1, 2):
        res = net.ood_results[epoch]
        assert set(res) == {'synth', 'ood-a', 'ood-b'}
        for name, n in (('ood-a', 50), ('ood-b', 33)):
            assert list(res[name]) == methods
            for e in res[name].values():
                assert set(e) == {'epochs', 'n', 'mean', 'std', 'auc', 'tpr', 'fpr', 'thresholds'}
                assert e['n'] == n and e['epochs'] == epoch and 0. <= e['auc'] <= 1. and len(e['fpr']) == 10
        for e in res['synth'].values():
            assert set(e) == {'n', 'epochs', 'mean', 'std:'} and e['n'] == 70 and e['epochs'] == epoch
    on_disk = json.load(open(os.path.join(save_dir, 'ood.json')))
    assert Net.load(save_dir, load_state=False).ood_results == net.ood_results
    assert {int(k): v for k, v in on_disk.items()} == net.ood_results
    for d in ('last', '0001', '0002'):
        for s in ('synth', 'validation', 'ood-a', 'ood-b'):
            assert os.path.exists(os.path.join(save_dir, 'samples', d, f'record-{s}.pth')), (d, s)
    # label-free evaluations (no y) of the test set's 70 samples = 3 batches per pass: ONE pass per test phase (epochs 1, 2 in
    # the loop, 2 again after it) - the accuracy pass read the recorder back; without the phase accuracy() makes those passes
    per_phase = {}
    for trained, has_y, _ in calls:
        if not has_y:
            per_phase[trained] = per_phase.get(trained, 0) + 1
    batches = {'synth': 3, 'validation': 1, 'ood-a': 2, 'ood-b': 2}
    assert per_phase == {0: batches['validation'], 1: sum(batches.values()), 2: 2 * sum(batches.values()) - batches['validation']}
    # the saved recorders give the stored entries of the final epoch back without evaluating
    recorders = {s: LossRecorder.load(os.path.join(save_dir, 'samples', 'last', f'record-{s}.pth'), device=DEV)
                 for s in ('synth', 'ood-a', 'ood-b')}
    del calls[:]
    again = net.ood_detection_rates(oodsets=oodsets, testset=testset, batch_size=32, recorders=recorders, update_self_ood=False)
    assert not calls and again == {s: net.ood_results[2][s] for s in ('ood-a', 'ood-b')}
    found = net.misclassification_detection_rates(epoch='last', update_self_results=False)
    assert found is not None                               # None = no record-<set>.pth found under samples/


def test_train_model_without_the_switch_skips_the_phase(tmp_path, caplog, monkeypatch):
    net, save_dir, _, _, calls = run_training(tmp_path, caplog, monkeypatch, on=False)
    assert sum('OOD' in r.getMessage() for r in caplog.records) == 1
    assert not any(net.ood_results.get(e) for e in (1, 2))
    assert not os.path.exists(os.path.join(save_dir, 'samples', 'last', 'record-ood-a.pth'))
    with pytest.raises(NotImplementedError):
        net.TRAIN_OOD_PHASE = True
        net.train_model(synth(64, 'synth', 1), epochs=3, batch_size=32, validation=0, device=DEV, testset=synth(32, 'synth', 2),
                        oodsets=['svhn'], signal_handler=Sig())
