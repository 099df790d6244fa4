"""Device-side ROC (csrc/roc.hip, ops.roc_curve, jvae_compat.roc_curves) and ClassificationVariationalNetwork.ood_detection_rates.

The goldens under tests/golden/roc hold what the reference's utils/roc_curves.py::roc_curve returns (tools/gen_roc_golden.py);
where a case has no golden the checker is the numpy restatement of tests/test_roc_restatement.py, which reproduces every golden.
Rates and thresholds are compared bit for bit (the same fp64 expressions over integer counts and exactly widened scores), the
AUC to (n_in + 2) * 2^-50 (test_roc_restatement.auc_bound: the reference's own summation error)."""
import logging
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_roc_restatement import auc_bound, golden_cases, roc_restatement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = golden_cases(GOLDEN)
KEPT = [pc / 100 for pc in range(90, 100)]


def grid(rng, n, mean=0.):
    """fp32 multiples of 2^-10 below 16: their fp64 sum is exact in any order (the centre of the around-mean mode)."""
    return np.clip(np.round((rng.standard_normal(n) + mean) * 1024) / 1024, -15.5, 15.5).astype(np.float32)


def device_roc(ins, outs, kept, modes):
    from jvae_hip import ops
    r = ops.roc_curve(torch.as_tensor(ins).to(DEV), torch.as_tensor(outs).to(DEV), list(kept), modes)
    return {k: v.cpu().numpy() for k, v in r.items()}


def same(got, want, what):
    assert got.dtype == np.float64 and np.array_equal(got, np.asarray(want, np.float64)), (what, got, want)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_roc_curve_matches_the_reference_golden(case):
    cid, ins, outs, kept, mode, (auc, fpr, tpr, low, up) = case
    r = device_roc(ins, outs, kept, 'around-mean' if mode else False)
    assert int(r['status']) == 0
    print(cid, 'auc', float(r['auc']), 'ref', float(auc), 'diff', abs(float(r['auc']) - float(auc)), 'bound', auc_bound(len(ins)))
    same(r['fpr'], fpr, 'fpr'), same(r['tpr'], tpr, 'tpr'), same(r['low'], low, 'low'), same(r['up'], up, 'up')
    assert abs(float(r['auc']) - float(auc)) <= auc_bound(len(ins))


def test_batched_rows_equal_single_rows_and_runs_repeat():
    rng = np.random.default_rng(3)
    M, n_in, n_out = 11, 3000, 2500
    ins = np.stack([grid(rng, n_in, m * .1) for m in range(M)])
    outs = rng.standard_normal((M, n_out)).astype(np.float32)
    modes = ['around-mean' if m % 3 == 1 else bool(m % 2) for m in range(M)]
    a, b = device_roc(ins, outs, KEPT, modes), device_roc(ins, outs, KEPT, modes)
    for k in a:
        assert a[k].shape[0] == M and a[k].tobytes() == b[k].tobytes(), k
    for m in range(M):
        one = device_roc(ins[m], outs[m], KEPT, modes[m])
        for k in a:
            assert one[k].tobytes() == a[k][m].tobytes(), (m, k)
        auc, fpr, tpr, low, up = roc_restatement(ins[m], outs[m], KEPT, around_mean=modes[m] == 'around-mean')
        same(a['fpr'][m], fpr, 'fpr'), same(a['tpr'][m], tpr, 'tpr'), same(a['low'][m], low, 'low'), same(a['up'][m], up, 'up')
        assert abs(a['auc'][m] - auc) <= auc_bound(n_in)


@pytest.mark.parametrize('n_in', [1, 2, 63, 65, 1025])
@pytest.mark.parametrize('n_out', [1, 2, 63, 65, 1025])
def test_sizes_that_are_not_multiples_of_the_sort_tile(n_in, n_out):
    rng = np.random.default_rng(1000 * n_in + n_out)
    ins, outs = grid(rng, n_in, .5), rng.standard_normal(n_out).astype(np.float32)
    for mode in (False, 'around-mean'):
        r = device_roc(ins, outs, KEPT, mode)
        auc, fpr, tpr, low, up = roc_restatement(ins, outs, KEPT, around_mean=bool(mode))
        same(r['fpr'], fpr, 'fpr'), same(r['tpr'], tpr, 'tpr'), same(r['low'], low, 'low'), same(r['up'], up, 'up')
        assert abs(float(r['auc']) - auc) <= auc_bound(n_in)


def test_a_row_longer_than_every_golden():
    """131 073 scores: one more than a power of two, the padded row is 2^18 keys (seven merge stages above the tile)."""
    rng = np.random.default_rng(5)
    ins, outs = grid(rng, 131073, 1.), rng.standard_normal(40000).astype(np.float32)
    for mode in (False, 'around-mean'):
        r = device_roc(ins, outs, KEPT, mode)
        auc, fpr, tpr, low, up = roc_restatement(ins, outs, KEPT, around_mean=bool(mode))
        same(r['fpr'], fpr, 'fpr'), same(r['tpr'], tpr, 'tpr'), same(r['low'], low, 'low'), same(r['up'], up, 'up')
        assert abs(float(r['auc']) - auc) <= auc_bound(len(ins))


def test_nan_and_non_finite_scores_raise_in_python_not_on_the_gpu():
    from jvae_hip import ops
    from jvae_compat import roc_curves
    rng = np.random.default_rng(9)
    ins, outs = grid(rng, 500), rng.standard_normal(300).astype(np.float32)
    bad_in, bad_out, inf_in = ins.copy(), outs.copy(), ins.copy()
    bad_in[17], bad_out[299], inf_in[3] = np.nan, np.nan, np.inf
    rows = device_roc(np.stack([ins, bad_in, ins, inf_in, inf_in]), np.stack([outs, outs, bad_out, outs, outs]), KEPT,
                      [False, 'around-mean', False, 'around-mean', False])
    assert rows['status'].tolist() == [0, 3, 1, 2, 0]           # a NaN in-score of an around-mean row is non-finite too
    with pytest.raises(ValueError):
        ops.roc_check_status(rows['status'])
    for i, o, mode in ((bad_in, outs, False), (ins, bad_out, 'around-mean'), (inf_in, outs, 'around-mean')):
        with pytest.raises(ValueError):
            roc_curves.roc_curve(i, o, *KEPT, two_sided=mode)
    torch.cuda.synchronize()                                   # the device is still healthy
    auc, fpr, tpr, thr = roc_curves.roc_curve(ins, outs, *KEPT[::-1])          # kept TPRs in any order, as the reference sorts them
    ref = roc_restatement(ins, outs, KEPT)
    assert isinstance(auc, float) and abs(auc - ref[0]) <= auc_bound(len(ins))
    same(fpr, ref[1], 'fpr'), same(tpr, ref[2], 'tpr'), same(thr['low'], ref[3], 'low'), same(thr['up'], ref[4], 'up')
    assert roc_curves.fpr_at_tpr(fpr, tpr, 0.95) == fpr[5]
    for kw in (dict(two_sided=(4, 1)), dict(validation=100), dict(ins_are_higher=False)):
        with pytest.raises(NotImplementedError):
            roc_curves.roc_curve(ins, outs, *KEPT, **kw)


def test_roc_curve_off_the_gpu_is_an_error():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    with pytest.raises(JvaeHipError):
        ops.roc_curve(torch.zeros(8), torch.zeros(8), KEPT)


# ---------------------------------------------------------------------------------------------- ood_detection_rates
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


def scores_by_hand(net, dset, methods, batch_size):
    """What per-batch evaluate + batch_dist_measures give, as the reference's loop collects them."""
    rows, measures = {m: [] for m in methods}, None
    net.eval()
    with torch.no_grad():
        for i, (x, _) in enumerate(torch.utils.data.DataLoader(dset, batch_size=batch_size, num_workers=0, shuffle=False)):
            _, logits, losses, measures = net.evaluate(net._device_batch(x.to(DEV)), batch=i, current_measures=measures)
            sc = net.batch_dist_measures(logits, losses, methods)
            for m in methods:
                rows[m].append(sc[m].float().cpu().numpy())
    return {m: np.concatenate(rows[m]) for m in methods}


def check_stats(mean, std, scores, what):
    """fp64 mean / population deviation against numpy on the same scores at n * 2^-52 relative: the rounding of an fp64 sum of
    n terms in any order.  Rows of one sign only, so that the sum has no cancellation."""
    x = scores.astype(np.float64)
    if not (np.all(x > 0) or np.all(x < 0)):
        return
    tol = len(x) * 2.0 ** -52
    print(what, 'mean', mean, x.mean(), 'std', std, x.std(), 'rel tol', tol)
    assert abs(mean - x.mean()) <= tol * abs(x.mean()), what
    assert abs(std - x.std()) <= tol * x.std(), what


def check_against_restatement(net, res, sets, methods, batch_size, seed):
    torch.manual_seed(seed)
    by_hand = [scores_by_hand(net, d, methods, batch_size) for d in sets]
    ind = by_hand[0]
    for d, sc in zip(sets[1:], by_hand[1:]):
        assert set(res[d.name]) == set(methods)
        for m in methods:
            r = res[d.name][m]
            assert set(r) == {'epochs', 'n', 'mean', 'std', 'auc', 'tpr', 'fpr', 'thresholds'}
            assert r['n'] == len(d) and r['epochs'] == net.trained and r['tpr'] == KEPT
            assert isinstance(r['auc'], float) and isinstance(r['fpr'], list) and isinstance(r['thresholds'], list)
            auc, fpr, tpr, low, up = roc_restatement(ind[m], sc[m], KEPT, around_mean=m.endswith('-2s'))
            print(d.name, m, 'auc', r['auc'], 'restated', auc, 'fpr', r['fpr'][5], fpr[5])
            assert r['fpr'] == fpr.tolist(), (d.name, m)
            assert [t[0] for t in r['thresholds']] == low.tolist() and [t[1] for t in r['thresholds']] == up.tolist()
            assert abs(r['auc'] - auc) <= auc_bound(len(ind[m]))
            check_stats(r['mean'], r['std'], sc[m], (d.name, m))
    return ind


def test_ood_detection_rates_of_a_cvae(tmp_path, caplog, monkeypatch):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.recorders import LossRecorder
    net = build_net('e2_n8_L3')
    sets = [synth(300, 'ind', 1), synth(200, 'ood-a', 2, .3), synth(137, 'ood-b', 3, -.2)]
    with caplog.at_level(logging.INFO):
        methods = net._ood_methods('all')
    said = [r for r in caplog.records if 'iws-a-4-1' in r.getMessage()]
    assert len(said) == 1 and all(m in said[0].getMessage() for m in ('iws-a-1-1', 'elbo-a-1-1', 'elbo-a-4-1'))
    assert methods == ['iws-2s', 'iws', 'mse', 'elbo', 'soft', 'elbo-2s', 'zdist']
    caplog.clear()

    torch.manual_seed(11)
    with caplog.at_level(logging.INFO):
        res = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64)
    assert len([r for r in caplog.records if 'iws-a-4-1' in r.getMessage()]) == 1
    assert set(res) == {'ood-a', 'ood-b'}
    ind = check_against_restatement(net, res, sets, methods, 64, seed=11)

    mine = net.ood_results[net.trained]
    assert mine['ood-a'] == res['ood-a'] and mine['ood-b'] == res['ood-b']
    for m in methods:
        e = mine['ind'][m]
        assert set(e) == {'n', 'epochs', 'mean', 'std:'} and e['n'] == 300
        check_stats(e['mean'], e['std:'], ind[m], ('ind', m))
    assert set(net.test_losses) >= {'total', 'kl', 'iws'} and net.test_measures

    saved = net.save(str(tmp_path / 'job'))
    back = Net.load(saved, load_state=False)
    assert back.ood_results == net.ood_results and back.ood_results[0]['ood-b'] == res['ood-b']

    # recorders: a recording pass (the LossRecorder re-seeds torch, so its draws are its own), the reference's record files,
    # then a pass over the full recorders that evaluates nothing and returns the same numbers
    recorders = {}
    first = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64, recorders=recorders,
                                    sample_dirs=[str(tmp_path)], update_self_ood=False)
    for d in sets:
        rec = LossRecorder.load(os.path.join(tmp_path, f'record-{d.name}.pth'), device=DEV)
        assert rec.recorded_samples == len(d) and len(recorders[d.name]) == int(np.ceil(len(d) / 64))
    calls = []
    real = net.evaluate
    monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append(1) or real(*a, **k))
    again = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64, recorders=recorders, update_self_ood=False)
    assert not calls and again == first
    assert net.ood_detection_rates(oodsets=sets[1:2], testset=sets[0], batch_size=64, update_self_ood=False) and calls

    for m in ('iws-a-4-1', 'odin-1-0.0040'):
        with pytest.raises(NotImplementedError):
            net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], method=m)
    with pytest.raises(NotImplementedError):
        net.ood_detection_rates(oodsets=sets[1:], testset=None)
    one = net.ood_detection_rates(oodsets=sets[1:2], testset=sets[0], batch_size=64, method='zdist', update_self_ood=False)
    assert list(one['ood-a']) == ['zdist']


def test_ood_detection_rates_of_a_vae():
    net = build_net('ea2_n8_vae_L3')
    sets = [synth(300, 'ind', 4), synth(137, 'ood', 5, .3)]
    methods = net._ood_methods('all')
    assert methods == ['iws', 'iws-2s', 'elbo', 'elbo-2s', 'zdist']
    torch.manual_seed(21)
    res = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64)
    check_against_restatement(net, res, sets, methods, 64, seed=21)


def test_no_host_copy_per_batch(monkeypatch):
    """Host copies (Tensor.cpu / item / tolist / numpy) of a whole ood_detection_rates call with outputs=None: a fixed handful
    (losses and measures of the in-distribution pass, its row statistics, the one ROC result), whatever the number of batches
    and of methods; with a progress sink, one more per ROC point (every 100 batches and the last one)."""
    net = build_net('e2_n8_L3')
    count = {'n': 0}
    for name in ('cpu', 'item', 'tolist', 'numpy'):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, **k):
            count['n'] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)

    def run(n_ind, n_ood, method, outputs=None):
        count['n'] = 0
        net.ood_detection_rates(oodsets=[synth(n_ood, 'ood', 7, .3)], testset=synth(n_ind, 'ind', 6), batch_size=2,
                                method=method, update_self_ood=False, outputs=outputs)
        return count['n']

    few = run(20, 12, 'zdist')                                 # 10 + 6 batches, 1 method
    many = run(64, 210, 'all')                                 # 32 + 105 batches, 7 methods
    print('host copies:', few, many)
    assert many == few and few <= 12

    class Sink:
        lines = 0

        def results(self, *a, **k):
            Sink.lines += 1
    with_sink = run(64, 210, 'all', outputs=Sink())            # lines at batches 0, 31 of 32 and 0, 100, 104 of 105
    print('host copies with a sink:', with_sink, 'lines', Sink.lines)
    assert Sink.lines == 2 + 3 and with_sink <= few + 5 * 3    # at most three copies per progress line
