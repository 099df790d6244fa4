"""SCOD risk curves on the device (csrc/scod.hip, ops.scod_scores / ops.scod_curve, jvae_compat.scod, ScoringMixin.scod_rates).

The goldens under tests/golden/scod hold what the reference's tests/scod.py computes (tools/gen_scod_golden.py); the numpy
restatement of tests/test_scod_restatement.py reproduces every one of them and is the checker where the reference leaves a
result unspecified (inside a group of equal scores).  Curves, kept figures and score rows are compared bit for bit; the areas
with the fp64 trapezoid of the reference's own curves at test_scod_restatement.area_bound (the order of at most n fp64 additions:
a relative n * 2^-52 plus an absolute term of the same size)."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from test_scod_restatement import (F32, FIGURES, check_figures, e2e_record, row_records, scod_restatement, tie_group_ends)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CURVE_FILES = sorted(os.path.basename(f)[6:-4] for f in glob.glob(os.path.join(GOLDEN, 'scod', 'curve-*.npz')))
TIE_FREE = [f for f in CURVE_FILES if not f.startswith('ties')]
TIES = [f for f in CURVE_FILES if f.startswith('ties')]
CURVES = ('tpr', 'selective_risk', 'fpr')


def load(name):
    return np.load(os.path.join(GOLDEN, 'scod', f'curve-{name}.npz'))


def device_curve(scores, y_true, y_est, **kw):
    from jvae_hip import ops
    r = ops.scod_curve(torch.as_tensor(scores).to(DEV), torch.as_tensor(y_true).to(DEV), torch.as_tensor(y_est).to(DEV), **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_the_cases_the_curves_are_checked_on():
    assert TIE_FREE == ['all_correct_700_300', 'all_wrong_300_700', 'ood_head_400_250', 'rows3_2500_1700', 'small_5_3', 'tile',
                        'tile_minus_1', 'tile_plus_1', 'tiles_3000_2000'] and TIES == ['ties_2600_1900', 'ties_300_200']


@pytest.mark.parametrize('name', TIE_FREE)
def test_curves_and_figures_match_the_reference_golden(name):
    """All rows of a golden in ONE call (rows3: M = 3 rows in different orders - no row leaks into another)."""
    g = load(name)
    M, n = g['scores'].shape
    r = device_curve(g['scores'], g['y_true'], g['y_est'], n_in=int((g['y_true'] >= 0).sum()))
    assert r['status'].tolist() == [0] * M and r['figures'].shape == (M, 5) and r['figures'].dtype == np.float64
    for k in CURVES:
        assert r[k].dtype == F32 and r[k].shape == (M, n) and r[k].tobytes() == g[k].tobytes(), (name, k)
    for m in range(M):
        check_figures(f'{name}-{m}', r['figures'][m].tolist(), g['figures'][m], g['trapz'][m], n)
    if M > 1:
        assert len({g['scores'][m].tobytes() for m in range(M)}) == M
        for m in range(M):
            one = device_curve(g['scores'][m], g['y_true'], g['y_est'])           # n_in counted by the call
            for k in CURVES + ('figures', 'status'):
                assert one[k].tobytes() == r[k][m].tobytes(), (name, m, k)


@pytest.mark.parametrize('name', TIES)
def test_equal_scores_are_taken_in_the_order_of_their_positions(name):
    """Scores drawn from 8 values per side: the device curves are the stable-by-position ones, and agree with the reference's
    at every position that ends a group of equal scores.  No other claim is made for ties."""
    g = load(name)
    M, n = g['scores'].shape
    r = device_curve(g['scores'], g['y_true'], g['y_est'])
    for m in range(M):
        assert len(np.unique(g['scores'][m])) <= 16
        curves, figures = scod_restatement(g['scores'][m], g['y_true'], g['y_est'])
        ends = tie_group_ends(g['scores'][m])
        assert ends.sum() <= 16
        for k, want in zip(CURVES, curves):
            assert r[k][m].tobytes() == want.tobytes(), (name, m, k)
            assert np.array_equal(r[k][m][ends], g[k][m][ends]), (name, m, k)
        assert r['figures'][m, 0] == figures[0] and r['figures'][m, 1] == figures[1]


def test_two_calls_return_the_same_bits():
    g = load('rows3_2500_1700')
    a = device_curve(g['scores'], g['y_true'], g['y_est'])
    b = device_curve(g['scores'], g['y_true'], g['y_est'])
    assert set(a) == {'tpr', 'selective_risk', 'fpr', 'figures', 'status'}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    only = device_curve(g['scores'], g['y_true'], g['y_est'], curves=False)
    assert set(only) == {'figures', 'status'} and only['figures'].tobytes() == a['figures'].tobytes()


def test_refusals_come_before_any_launch():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    n = 16
    s = torch.arange(n, dtype=torch.float32, device=DEV)
    y = torch.zeros(n, dtype=torch.int64, device=DEV)
    mixed = torch.cat((y[:8], y[8:] - 1))
    for bad in (dict(y_true=y), dict(y_true=y - 1), dict(y_true=mixed, n_in=0), dict(y_true=mixed, n_in=n),       # an empty side
                dict(scores=s.double(), y_true=mixed), dict(scores=s.cpu(), y_true=mixed.cpu(), y_est=y.cpu()),
                dict(scores=s.cpu(), y_true=mixed), dict(y_true=mixed.int()), dict(y_true=mixed, curves=False, figures=False)):
        kw = dict(dict(scores=s, y_true=mixed, y_est=y), **bad)
        with pytest.raises(JvaeHipError):
            ops.scod_curve(kw.pop('scores'), kw.pop('y_true'), kw.pop('y_est'), **kw)
    # n above ROC_MAX_N: the size is refused from the shape alone (an expanded view: no 64 MiB buffer is made)
    big = torch.zeros(1, dtype=torch.float32, device=DEV).expand(ops.SCOD_MAX_N + 1)
    bigy = torch.zeros(1, dtype=torch.int64, device=DEV).expand(ops.SCOD_MAX_N + 1)
    assert ops.L.load().jvae_scod_workspace_bytes(1, ops.SCOD_MAX_N + 1) == 0 and ops.L.load().jvae_scod_workspace_bytes(1, ops.SCOD_MAX_N) > 0
    assert ops.L.load().jvae_scod_curve_f32(s.data_ptr(), mixed.data_ptr(), y.data_ptr(), s.data_ptr(), None, y.data_ptr(), 1,
                                            ops.SCOD_MAX_N + 1, 8, s.data_ptr(), 1 << 40, None) == -1
    with pytest.raises(JvaeHipError):
        ops.scod_curve(big, bigy, bigy, n_in=5)
    # a wrong n_in and a NaN score are reported through the status word, and raise in Python
    r = ops.scod_curve(s, mixed, y, n_in=7)
    with pytest.raises(JvaeHipError):
        ops.scod_check_status(r['status'].cpu())
    s2 = s.clone()
    s2[3] = float('nan')
    r = ops.scod_curve(s2, mixed, y)
    assert int(r['status']) == 1
    with pytest.raises(ValueError):
        ops.scod_check_status(r['status'].cpu())
    torch.cuda.synchronize()                                   # the device is still healthy
    assert int(ops.scod_curve(s, mixed, y)['status']) == 0


# ------------------------------------------------------------------------------------------------------------ score rows
def on_device(t):
    return {k: torch.as_tensor(v).to(DEV) for k, v in t.items()}


def recorder_on_device(which):
    from jvae_compat import scod
    t, mtype, rows = row_records(GOLDEN, which)
    d = on_device(t)
    if 'y_est_already' not in d:
        with pytest.raises(KeyError):
            scod.scoring(d, mtype=mtype)
        d['y_est_already'] = d['cross_y'].argmin(0)             # as scod_rates fills it
    return t, d, mtype, rows


def same_row(got, want, what):
    if want.ndim == 0:
        assert not torch.is_tensor(got) and float(got) == float(want), what
    else:
        assert got.dtype == torch.float32 and got.is_cuda and got.cpu().numpy().tobytes() == want.tobytes(), what


@pytest.mark.parametrize('which', ['wim', 'vib'])
def test_score_rows_match_the_reference_golden(which):
    """Every r kind and g kind, weights 0, 1 and 0.3 (0.3 tells a fused multiply-add from two rounded operations), the `zdist`
    -> 0 default of a wim, a 2-D `zdist@`; the vib recorder has an `odin-1-0.0040` row and no `y_est_already`.  The log-sum-exp
    row of `logmsp` is torch's on the host, as in the reference: how far the device's torch.logsumexp is from it is printed."""
    from jvae_compat import scod
    t, d, mtype, rows = recorder_on_device(which)
    assert {r for (r, _, _), _ in rows} >= ({None, 'zdist', 'dist', 'predist', 'logmsp', 'odin-1-0.0040'} if which == 'wim'
                                             else {None, 'odin-1-0.0040', 'logmsp'})
    lse_host, lse_dev = scod._host_lse(d['zdist']).cpu().numpy(), (-0.5 * d['zdist']).logsumexp(0).cpu().numpy()
    ulp = np.abs(lse_host.view(np.int32).astype(np.int64) - lse_dev.view(np.int32).astype(np.int64))
    print(which, 'torch.logsumexp, device against host:', int((ulp > 0).sum()), 'of', len(ulp), 'samples differ, at most', int(ulp.max()),
          'ulp,', float(np.abs(lse_host - lse_dev).max()), 'absolute')
    for (r, g, w), want in rows:
        same_row(scod.scoring(d, r=r, g=g, weight=w, mtype=mtype), want, (which, r, g, w))
    by = dict(rows)
    y = d['y_est_already']
    for r in sorted({r for (r, _, _), _ in rows} & {'dist', 'predist', 'logmsp', 'odin-1-0.0040'}):      # r on its own
        got = scod.scoring_r(d, r, y_est=y, mtype=mtype)       # = r + 0 * g: these rows hold no -0.
        assert got.cpu().numpy().tobytes() == by[(r, 'elbo', 0)].tobytes(), (which, r)
    assert scod.scoring_r(d, 'zdist', y_est=y) == 0. and scod.scoring_r(d, None, mtype='wim') == 0.
    if which == 'wim':
        assert scod.scoring_g(d, 'elbo', y_est=y).cpu().numpy().tobytes() == by[('zdist', 'elbo', 1)].tobytes()
        assert scod.scoring_g(d, None).cpu().numpy().tobytes() == by[(None, None, 1)].tobytes()
        assert scod.scoring_g(d, 'iws').cpu().numpy().tobytes() == by[('msp', 'iws', 1)].tobytes()
        assert scod.scoring_g(d, 'kl', mtype='cvae') == 0.
    else:
        assert scod.scoring_g(d, 'elbo', mtype='vib') == 0.
    assert scod.default_scores == {'wim': {'r': 'zdist', 'g': 'elbo'}, 'vib': {'r': 'odin-1-0.0040', 'g': 'none'}}


def test_a_label_outside_the_classes_raises_through_the_status_word():
    from jvae_compat import scod
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    t, mtype, rows = row_records(GOLDEN, 'wim')
    d = on_device(t)
    C = t['zdist'].shape[0]
    d['y_est_already'] = d['y_est_already'].clone()
    d['y_est_already'][5] = C
    row = scod.scoring(d, r='dist', g='elbo', mtype='wim')
    with pytest.raises(JvaeHipError):
        ops.wim_check_status()
    row = row.cpu().numpy()
    assert np.isnan(row[5]) and not np.isnan(np.delete(row, 5)).any()
    ops.wim_check_status()                                     # cleared
    with pytest.raises(JvaeHipError):                          # and through scod_rates
        scod.scod_rates({'a': d, 'b': on_device(t)}, 'a', mtype='wim')


# ------------------------------------------------------------------------------------------------------------ end to end
def write_records(directory, sets, batch_size=64):
    """record-<set>.pth in the layout tests/golden/record_ref pins (jvae_compat/recorders.py), with torch.save."""
    os.makedirs(directory, exist_ok=True)
    for s, t in sets.items():
        n = len(t['y_true'])
        nb = -(-n // batch_size)
        torch.save({'batch_size': batch_size, 'last_batch_size': n - (nb - 1) * batch_size, 'device': torch.device('cpu'), '_seed': 1,
                    '_num_batch': nb, '_samples': n, '_recorded_batches': nb,
                    '_tensors': {k: torch.as_tensor(v) for k, v in t.items()}}, os.path.join(directory, f'record-{s}.pth'))


def check_e2e(got, want, n):
    figures, trapz = want
    assert list(got) == list(FIGURES) and all(isinstance(v, float) for v in got.values())
    check_figures('e2e', [got[k] for k in FIGURES], figures, trapz, n)


def test_scod_rates_of_a_recorder_directory(tmp_path):
    from jvae_compat import scod
    from jvae_compat.recorders import LossRecorder
    from jvae_compat.wim import WIMJob
    from cvae import ClassificationVariationalNetwork as Net
    sets, figs = e2e_record(GOLDEN)
    n = sum(len(t['y_true']) for t in sets.values())
    job = WIMJob(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))
    job.to(DEV)
    job.training_parameters['set'] = 'ind'
    job.trained = 3
    saved = job.save(str(tmp_path / 'job'))
    write_records(os.path.join(saved, 'samples', '0003'), sets)
    recorders = LossRecorder.loadall(os.path.join(saved, 'samples', '0003'), map_location=DEV)
    assert list(recorders) == list(sets) and 'y_est_already' not in recorders['ood-b']

    default = scod.scod_rates(recorders, 'ind', mtype='wim')
    check_e2e(default, figs[(None, None, 1.)], n)
    rs, gs, ws = [None, 'dist'], [None, 'elbo', 'iws'], [1., 0.3]
    many = scod.scod_rates(recorders, 'ind', mtype='wim', r=rs, g=gs, weight=ws)
    assert list(many) == [(r, g, w) for r in rs for g in gs for w in ws] and set(many) == set(figs)
    for v in many:
        check_e2e(many[v], figs[v], n)
        assert scod.scod_rates(recorders, 'ind', mtype='wim', r=v[0], g=v[1], weight=v[2]) == many[v], v
    assert many[(None, None, 1.)] == default
    with_curves = scod.scod_rates(recorders, 'ind', mtype='wim', r='dist', weight=0.3, curves=True)
    assert {k: with_curves[k] for k in FIGURES} == many[('dist', None, 0.3)]
    assert all(with_curves[k].shape == (n,) and with_curves[k].is_cuda for k in ('tpr', 'selective_risk', 'fpr'))
    assert float(with_curves['fpr'][with_curves['tpr'] >= 0.95].min()) == with_curves['fpr95']

    # the job finds its own directory, set and type
    assert job.scod_rates() == default
    assert job.scod_rates(r=rs, g=gs, weight=ws) == many
    assert job.scod_rates(sample_dir=os.path.join(saved, 'samples', '0003'), epoch=None) == default
    assert job.scod_rates(epoch=3) == default
    plain = Net(**get_case('c1_n16_mlp')['net'])
    plain.to(DEV)
    plain.training_parameters['set'] = 'ind'
    where = plain.save(str(tmp_path / 'plain'))
    with pytest.raises(FileNotFoundError):
        plain.scod_rates()
    write_records(os.path.join(where, 'samples', 'last'), sets)
    with pytest.raises(KeyError):                              # a cvae has no default scores in the reference either
        plain.scod_rates()
    assert plain.scod_rates(mtype='wim') == default
    from jvae_hip.lib import JvaeHipError
    with pytest.raises(JvaeHipError):                          # no in-distribution set among the recorders
        scod.scod_rates(recorders, 'cifar10', mtype='wim')


def test_scrisk_returns_the_curves_on_the_device_of_its_inputs():
    from jvae_compat import scod
    g = load('small_5_3')
    tpr, sr, fpr = scod.scrisk(torch.as_tensor(g['y_true']).to(DEV), torch.as_tensor(g['y_est']).to(DEV),
                               torch.as_tensor(g['scores'][0]).to(DEV))
    for got, k in ((tpr, 'tpr'), (sr, 'selective_risk'), (fpr, 'fpr')):
        assert got.is_cuda and got.dtype == torch.float32 and got.cpu().numpy().tobytes() == g[k][0].tobytes()
