"""The strided-quantile mode of the device ROC (csrc/roc.hip mode 2, ops.roc_curve(two_sided=('quantile', f_low, f_up)),
jvae_compat.roc_curves.roc_curve_quantile) and the '-a-x-y' OOD methods behind ClassificationVariationalNetwork.OOD_QUANTILE_METHODS.

The goldens under tests/golden/rocq hold, as record (a), what the reference's roc_curve returns in its tuple mode when only
its spline is replaced by the values at its knots (tools/gen_rocq_golden.py); where a case has no golden the checker is the
numpy restatement of tests/test_rocq_restatement.py, which reproduces every golden.  Rates and thresholds are compared bit
for bit, the AUC to (n_in + 2) * 2^-50 (test_roc_restatement.auc_bound: the reference's own summation error)."""
import logging
import os

import numpy as np
import pytest
import torch

from test_4_roc_gpu import DEV, KEPT, build_net, check_stats, device_roc, grid, same, scores_by_hand, synth
from test_roc_restatement import auc_bound, roc_restatement
from test_rocq_restatement import golden_cases, roc_restatement_quantile

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = golden_cases(GOLDEN)
ALL_CVAE = ['iws-2s', 'iws-a-1-1', 'iws-a-4-1', 'iws', 'mse', 'elbo', 'soft', 'elbo-2s', 'elbo-a-1-1', 'elbo-a-4-1', 'zdist']


def restated(ins, outs, kept, mode):
    if isinstance(mode, tuple):
        return roc_restatement_quantile(ins, outs, kept, mode[1:])
    return roc_restatement(ins, outs, kept, around_mean=mode == 'around-mean')


def check_row(r, m, ins, outs, kept, mode, what):
    auc, fpr, tpr, low, up = restated(ins, outs, kept, mode)
    pick = (lambda v: v) if m is None else (lambda v: v[m])
    print(what, mode, 'auc', float(pick(r['auc'])), 'restated', auc, 'bound', auc_bound(len(ins)))
    same(pick(r['fpr']), fpr, (what, 'fpr')), same(pick(r['tpr']), tpr, (what, 'tpr'))
    same(pick(r['low']), low, (what, 'low')), same(pick(r['up']), up, (what, 'up'))
    assert abs(float(pick(r['auc'])) - auc) <= auc_bound(len(ins)), what


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_quantile_rows_match_the_reference_golden(case):
    cid, ins, outs, kept, pair, (auc, fpr, tpr, low, up) = case
    r = device_roc(ins, outs, kept, ('quantile',) + pair)
    assert int(r['status']) == 0
    print(cid, 'auc', float(r['auc']), 'ref', float(auc), 'diff', abs(float(r['auc']) - float(auc)), 'bound', auc_bound(len(ins)))
    same(r['fpr'], fpr, 'fpr'), same(r['tpr'], tpr, 'tpr'), same(r['low'], low, 'low'), same(r['up'], up, 'up')
    assert abs(float(r['auc']) - float(auc)) <= auc_bound(len(ins))


@pytest.mark.parametrize('n_in', [1, 2, 4, 63, 65, 1025, 4099, 70001])
def test_sizes_across_the_regimes_of_the_sort(n_in):
    rng = np.random.default_rng(77 + n_in)
    ins, outs = rng.standard_normal(n_in).astype(np.float32) + .5, rng.standard_normal(777).astype(np.float32)
    for pair in ((1, 1), (4, 1), (1, 4), (7, 7), (255, 3)):
        mode = ('quantile',) + pair
        r = device_roc(ins, outs, KEPT, mode)
        assert int(r['status']) == 0
        check_row(r, None, ins, outs, KEPT, mode, n_in)


def test_mixed_modes_in_one_call():
    rng = np.random.default_rng(8)
    M, n_in, n_out = 7, 3001, 2500
    ins = np.stack([grid(rng, n_in, m * .1) for m in range(M)])
    outs = rng.standard_normal((M, n_out)).astype(np.float32)
    modes = [False, 'around-mean', ('quantile', 1, 1), ('quantile', 4, 1), True, ('quantile', 2, 3), 'around-mean']
    a, b = device_roc(ins, outs, KEPT, modes), device_roc(ins, outs, KEPT, modes)
    assert a['status'].tolist() == [0] * M
    for k in a:
        assert a[k].shape[0] == M and a[k].tobytes() == b[k].tobytes(), k
    for m in range(M):
        check_row(a, m, ins[m], outs[m], KEPT, modes[m], m)
        one = device_roc(ins[m], outs[m], KEPT, modes[m])
        for k in a:
            assert one[k].tobytes() == a[k][m].tobytes(), (m, k)
    old = [m for m in range(M) if not isinstance(modes[m], tuple)]          # the rows a call without quantile rows can hold
    alone = device_roc(ins[old], outs[old], KEPT, [modes[m] for m in old])
    for k in a:
        assert alone[k].tobytes() == a[k][old].tobytes(), k
    as_words = torch.tensor([0, 1, 2 | 1 << 8 | 1 << 16, 2 | 4 << 8 | 1 << 16, 0, 2 | 2 << 8 | 3 << 16, 1], dtype=torch.int32, device=DEV)
    c = device_roc(ins, outs, KEPT, as_words)
    for k in a:
        assert c[k].tobytes() == a[k].tobytes(), k
    for_all = device_roc(ins, outs, KEPT, ('quantile', 4, 1))               # one tuple for all rows
    same(for_all['fpr'][3], a['fpr'][3], 'fpr'), same(for_all['low'][0], restated(ins[0], outs[0], KEPT, ('quantile', 4, 1))[3], 'low')


def test_workspace_bytes_are_those_of_the_parent_build():
    """jvae_roc_workspace_bytes as the build before this mode returned it (recorded from that build)."""
    from jvae_hip import lib
    fn = lib.load().jvae_roc_workspace_bytes
    for args, nbytes in (((1, 1, 1), 34048), ((1, 4, 50), 34048), ((7, 4099, 1000), 976128), ((11, 10000, 26032), 4485888),
                         ((3, 70001, 5), 6424320), ((2, 1 << 24, 1), 671106304), ((1, (1 << 24) + 1, 1), 0)):
        assert fn(*args) == nbytes, args


def test_nan_and_malformed_modes_are_reported_not_faulted():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    from jvae_compat import roc_curves
    rng = np.random.default_rng(9)
    ins, outs = grid(rng, 500), rng.standard_normal(300).astype(np.float32)
    bad_in, bad_out = ins.copy(), outs.copy()
    bad_in[17], bad_out[299] = np.nan, np.nan
    q = ('quantile', 4, 1)
    rows = device_roc(np.stack([ins, bad_in, ins]), np.stack([outs, outs, bad_out]), KEPT, [q, q, q])
    assert rows['status'].tolist() == [0, 1, 1]
    with pytest.raises(ValueError):
        ops.roc_check_status(rows['status'])
    with pytest.raises(ValueError):
        roc_curves.roc_curve_quantile(bad_in, outs, *KEPT, factors=(4, 1))
    torch.cuda.synchronize()                                   # the device is still healthy
    check_row(rows, 0, ins, outs, KEPT, q, 'beside the NaN rows')

    for t in (('quantile', 0, 1), ('quantile', 1, 256), ('quantile', 1.5, 1), ('quantile', 1), ('quantile', True, 1)):
        with pytest.raises(JvaeHipError):
            device_roc(ins, outs, KEPT, t)
        with pytest.raises(JvaeHipError):
            device_roc(ins[None], outs[None], KEPT, [t])
    for t in ((4, 1), [(4, 1)]):                               # a bare tuple stays what it was: per-row values, not built
        with pytest.raises(NotImplementedError):
            device_roc(ins[None], outs[None], KEPT, t)
    with pytest.raises(NotImplementedError):
        roc_curves.roc_curve(ins, outs, *KEPT, two_sided=(4, 1))
    words = torch.tensor([3, 2, 2 | 1 << 8, 2 | 1 << 8 | 1 << 16 | 1 << 24, -1, 2 | 1 << 8 | 1 << 16, 0], dtype=torch.int32, device=DEV)
    r = device_roc(np.stack([ins] * 7), np.stack([outs] * 7), KEPT, words)
    assert r['status'].tolist() == [4, 4, 4, 4, 4, 0, 0]
    with pytest.raises(JvaeHipError):
        ops.roc_check_status(r['status'])
    torch.cuda.synchronize()
    check_row(r, 5, ins, outs, KEPT, ('quantile', 1, 1), 'beside the malformed rows')
    check_row(r, 6, ins, outs, KEPT, False, 'beside the malformed rows')


def test_roc_curve_quantile_is_the_op_on_one_row():
    from jvae_compat import roc_curves
    rng = np.random.default_rng(10)
    ins, outs = rng.standard_normal(900).astype(np.float32) + 1, rng.standard_normal(600).astype(np.float32)
    for pair in ((1, 1), (4, 1), (2, 3)):
        auc, fpr, tpr, thr = roc_curves.roc_curve_quantile(ins, outs, *KEPT[::-1], factors=pair)
        r = device_roc(ins, outs, KEPT, ('quantile',) + pair)
        assert isinstance(auc, float) and auc == float(r['auc'])
        same(fpr, r['fpr'], 'fpr'), same(tpr, r['tpr'], 'tpr'), same(thr['low'], r['low'], 'low'), same(thr['up'], r['up'], 'up')
        check_row(r, None, ins, outs, KEPT, ('quantile',) + pair, pair)
    auc, fpr, tpr, thr = roc_curves.roc_curve_quantile(torch.as_tensor(ins), list(outs), *KEPT)          # factors=(1, 1)
    same(fpr, device_roc(ins, outs, KEPT, ('quantile', 1, 1))['fpr'], 'fpr')
    roc_curves.roc_curve_quantile(ins[:4], outs, *KEPT)
    for n in (1, 3):
        with pytest.raises(ValueError):
            roc_curves.roc_curve_quantile(ins[:n], outs, *KEPT)


# ---------------------------------------------------------------------------------------------- ood_detection_rates
def mode_of(m):
    if '-a-' in m:
        return ('quantile',) + tuple(int(f) for f in m.split('-a-')[1].split('-'))
    return 'around-mean' if m.endswith('-2s') else False


def check_against_restatement(net, res, sets, methods, batch_size, seed):
    torch.manual_seed(seed)
    by_hand = [scores_by_hand(net, d, methods, batch_size) for d in sets]
    ind = by_hand[0]
    for d, sc in zip(sets[1:], by_hand[1:]):
        assert list(res[d.name]) == methods
        for m in methods:
            r = res[d.name][m]
            assert set(r) == {'epochs', 'n', 'mean', 'std', 'auc', 'tpr', 'fpr', 'thresholds'}
            assert r['n'] == len(d) and r['epochs'] == net.trained and r['tpr'] == KEPT
            assert isinstance(r['auc'], float) and isinstance(r['fpr'], list) and isinstance(r['thresholds'], list)
            auc, fpr, tpr, low, up = restated(ind[m], sc[m], KEPT, mode_of(m))
            print(d.name, m, 'auc', r['auc'], 'restated', auc, 'fpr', r['fpr'][5], fpr[5])
            assert r['fpr'] == fpr.tolist(), (d.name, m)
            assert [t[0] for t in r['thresholds']] == low.tolist() and [t[1] for t in r['thresholds']] == up.tolist()
            assert abs(r['auc'] - auc) <= auc_bound(len(ind[m]))
            check_stats(r['mean'], r['std'], sc[m], (d.name, m))
    for m in methods:                                          # a '-a-x-y' row holds the scores of its base method
        if '-a-' in m:
            assert np.array_equal(ind[m], ind[m.split('-')[0]]), m
    return ind


def test_switch_off_keeps_the_refusals(caplog):
    from cvae import ClassificationVariationalNetwork as Net
    assert Net.OOD_QUANTILE_METHODS is False
    net = build_net('e2_n8_L3')
    sets = [synth(40, 'ind', 1), synth(30, 'ood', 2, .3)]
    with caplog.at_level(logging.INFO):
        assert net._ood_methods('all') == ['iws-2s', 'iws', 'mse', 'elbo', 'soft', 'elbo-2s', 'zdist']
    assert len([r for r in caplog.records if 'iws-a-4-1' in r.getMessage()]) == 1
    with pytest.raises(NotImplementedError):
        net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], method='iws-a-4-1')


def test_ood_detection_rates_with_the_quantile_methods(tmp_path, caplog, monkeypatch):
    from jvae_compat.recorders import LossRecorder
    net = build_net('e2_n8_L3')
    net.OOD_QUANTILE_METHODS = True
    sets = [synth(300, 'ind', 1), synth(200, 'ood-a', 2, .3), synth(137, 'ood-b', 3, -.2)]
    with caplog.at_level(logging.INFO):
        methods = net._ood_methods('all')
    assert methods == ALL_CVAE and not [r for r in caplog.records if 'left out' in r.getMessage()]
    assert net._ood_methods('iws-a-4-1') == ['iws-a-4-1'] and net._ood_methods(['elbo-a-2-3', 'zdist']) == ['elbo-a-2-3', 'zdist']
    for m in ('iws-a-0-1', 'iws-a-1-256', 'iws-a-4', 'iws-a-x-1'):
        with pytest.raises(ValueError):
            net._ood_methods(m)
    with pytest.raises(NotImplementedError):
        net._ood_methods('odin-1-0.0040')

    torch.manual_seed(11)
    res = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64)
    assert set(res) == {'ood-a', 'ood-b'}
    ind = check_against_restatement(net, res, sets, methods, 64, seed=11)
    torch.manual_seed(11)
    assert net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64, update_self_ood=False) == res   # runs repeat
    mine = net.ood_results[net.trained]
    assert mine['ood-a'] == res['ood-a'] and mine['ood-b'] == res['ood-b']
    for m in methods:
        e = mine['ind'][m]
        assert set(e) == {'n', 'epochs', 'mean', 'std:'} and e['n'] == 300
        check_stats(e['mean'], e['std:'], ind[m], ('ind', m))

    # recorders: a recording pass, then a pass over the full recorders that evaluates nothing and returns the same numbers
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
    assert not calls and again == first and list(again['ood-b']) == ALL_CVAE

    one = net.ood_detection_rates(oodsets=sets[1:2], testset=sets[0], batch_size=64, method='elbo-a-4-1', update_self_ood=False)
    assert list(one['ood-a']) == ['elbo-a-4-1'] and calls
    tiny = synth(3, 'tiny', 4)
    with pytest.raises(ValueError):
        net.ood_detection_rates(oodsets=sets[1:2], testset=tiny, batch_size=64, method='iws-a-1-1', update_self_ood=False)
    assert net.ood_detection_rates(oodsets=sets[1:2], testset=tiny, batch_size=64, method='iws', update_self_ood=False)


def test_the_quantile_methods_of_a_vae():
    from cvae import ClassificationVariationalNetwork as Net
    net = build_net('ea2_n8_vae_L3')
    sets = [synth(300, 'ind', 4), synth(137, 'ood', 5, .3)]
    assert net._ood_methods('all') == ['iws', 'iws-2s', 'elbo', 'elbo-2s', 'zdist']
    net.OOD_QUANTILE_METHODS = True
    methods = net._ood_methods('all')
    assert methods == Net.ood_methods_per_type['vae'] and len(methods) == 9
    torch.manual_seed(21)
    res = net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=64)
    check_against_restatement(net, res, sets, methods, 64, seed=21)
