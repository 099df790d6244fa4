"""Device-side precision-recall figures (csrc/prc.hip, ops.pr_metrics, jvae_compat.roc_curves.pr_metrics) and the
`DETECTION_PR_METRICS` switch of ood_detection_rates / misclassification_detection_rates.

The goldens under tests/golden/pr hold scikit-learn's figures (tools/gen_pr_golden.py); where scikit-learn gives none (infinite
scores) the checker is the numpy restatement of tests/test_pr_restatement.py, which reproduces every golden.  Bounds
(test_pr_restatement.pr_bounds, derived): (n_in + n_out + 3) * 2^-52 absolute for the four areas, 2^-50 for the detection
error; status words and NaN placement exactly."""
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_mdr_restatement import load_case
from test_pr_restatement import CASES, PR_FIGURES, golden_cases, pr_bounds, pr_restatement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDENS = golden_cases(GOLDEN)
QUANTILE = 2 | 4 << 8 | 1 << 16


def device_pr(ins, outs, modes):
    """-> (M, 5) figures and (M,) status on the host"""
    from jvae_hip import ops
    r = ops.pr_metrics(torch.as_tensor(np.ascontiguousarray(ins)).to(DEV), torch.as_tensor(np.ascontiguousarray(outs)).to(DEV),
                       torch.as_tensor(np.asarray(modes, np.int32)).to(DEV))
    assert all(r[k].dtype == torch.float64 and r[k].is_cuda for k in PR_FIGURES) and r['status'].dtype == torch.int32
    return np.stack([r[k].cpu().numpy() for k in PR_FIGURES], -1), r['status'].cpu().numpy()


def check(got, want, n_in, n_out, what):
    for k, g, w, b in zip(PR_FIGURES, got, want, pr_bounds(n_in, n_out)):
        print(what, k, 'device', g, 'want', w, 'error / bound', abs(g - w) / b)
        assert abs(g - w) <= b, (what, k, g, w, abs(g - w) / b)


@pytest.mark.parametrize('name', CASES)
def test_pr_metrics_match_scikit_learn_and_the_restatement(name):
    c = GOLDENS[name]
    n_in, n_out = c['ins'].shape[1], c['outs'].shape[1]
    got, status = device_pr(c['ins'], c['outs'], c['modes'])
    assert got.shape == (len(c['modes']), 5) and not status.any()
    for m, mode in enumerate(c['modes']):
        if not c['refused'][m]:
            check(got[m], c['figures'][m], n_in, n_out, (name, m, 'scikit-learn'))
        check(got[m], pr_restatement(c['ins'][m], c['outs'][m], int(mode)), n_in, n_out, (name, m, 'restatement'))
    if name == 'identical_400':
        assert got[0, 4] == 0.5
    if name == 'separated_500_300':
        assert got[0, 4] == 0.
    if name == 'zeros_pm':                                     # the two zeros are one tie group
        one_sign, _ = device_pr(np.abs(c['ins']), np.abs(c['outs']), c['modes'])
        assert one_sign.tobytes() == got.tobytes()
    if name == 'rows3':                                        # no row leaks into another
        for m, mode in enumerate(c['modes']):
            alone, _ = device_pr(c['ins'][m:m + 1], c['outs'][m:m + 1], [mode])
            assert alone[0].tobytes() == got[m].tobytes(), m
        assert got[0].tobytes() == got[2].tobytes()            # one data set in another order


def test_single_rows_mode_values_and_the_compat_function():
    from jvae_compat import roc_curves
    from jvae_hip import ops
    c = GOLDENS['rows3']
    ins, outs = torch.as_tensor(c['ins']).to(DEV), torch.as_tensor(c['outs']).to(DEV)
    batched, _ = device_pr(c['ins'], c['outs'], c['modes'])
    by_value = ops.pr_metrics(ins, outs, [False, 'around-mean', False])
    assert np.stack([by_value[k].cpu().numpy() for k in PR_FIGURES], -1).tobytes() == batched.tobytes()
    one = ops.pr_metrics(ins[1], outs[1], 'around-mean')
    assert all(one[k].shape == () for k in PR_FIGURES) and one['status'].shape == ()
    assert [float(one[k]) for k in PR_FIGURES] == batched[1].tolist()
    host = roc_curves.pr_metrics(c['ins'][1], list(c['outs'][1]), two_sided='around-mean')
    assert list(host) == list(PR_FIGURES) and all(type(v) is float for v in host.values())
    assert list(host.values()) == batched[1].tolist()
    assert list(roc_curves.pr_metrics(torch.as_tensor(c['ins'][0]), c['outs'][0]).values()) == batched[0].tolist()
    with pytest.raises(NotImplementedError):
        roc_curves.pr_metrics(c['ins'][0], c['outs'][0], two_sided=(4, 1))


def test_a_quantile_row_has_nan_figures_and_status_0():
    c = GOLDENS['small_5_3']
    ins, outs = np.repeat(c['ins'], 3, 0), np.repeat(c['outs'], 3, 0)
    got, status = device_pr(ins, outs, [0, QUANTILE, 0])
    assert np.isnan(got[1]).all() and not np.isnan(got[[0, 2]]).any() and status.tolist() == [0, 0, 0]
    assert got[0].tobytes() == got[2].tobytes()
    ins[1, 2] = np.nan                                         # a quantile row has no scalar score: nothing to flag
    got, status = device_pr(ins, outs, [0, QUANTILE, 0])
    assert np.isnan(got[1]).all() and status.tolist() == [0, 0, 0]


def test_status_words_and_what_the_compat_function_raises():
    from jvae_compat import roc_curves
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    rng = np.random.default_rng(5)
    ins, outs = rng.standard_normal((5, 40)).astype(np.float32), rng.standard_normal((5, 30)).astype(np.float32)
    ins = np.round(ins * 1024) / 1024                          # multiples of 2^-10: the centre is the same in every summation order
    ins[0, 7] = np.nan                                        # NaN in-score
    outs[1, 3] = np.nan                                        # NaN out-score
    ins[2, 1] = np.inf                                         # around-mean row with a non-finite in-score
    outs[3, 0] = -np.inf                                       # around-mean row with a non-finite OUT-score: legal
    got, status = device_pr(ins, outs, [0, 1, 1, 1, 7])
    assert status.tolist() == [1, 1, 2, 0, 4]
    check(got[3], pr_restatement(ins[3], outs[3], 1), 40, 30, 'infinite out-score around the mean')
    check(got[4], pr_restatement(ins[4], outs[4], 0), 40, 30, 'a malformed word runs as a one-sided row')
    for s, err in ((status[:1], ValueError), (status[2:3], ValueError), (status[4:], JvaeHipError)):
        with pytest.raises(err):
            ops.roc_check_status(s)
    with pytest.raises(ValueError):
        roc_curves.pr_metrics(ins[0], outs[0])
    with pytest.raises(ValueError):
        roc_curves.pr_metrics(ins[2], outs[2], two_sided='around-mean')


def test_two_calls_return_identical_bytes():
    c = GOLDENS['tiles_5000_3000']
    ins, outs = np.concatenate([c['ins'], c['ins'][:, ::-1]]), np.concatenate([c['outs'], c['outs'][:, ::-1]])
    a, _ = device_pr(ins, outs, [0, 1])
    b, _ = device_pr(ins, outs, [0, 1])
    assert a.tobytes() == b.tobytes() and not np.isnan(a).any()
    check(a[1], pr_restatement(ins[1], outs[1], 1), 5000, 3000, 'around the mean over the HBM merge passes')


def test_sizes_out_of_range_and_wrong_shapes_raise():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    z = torch.zeros(2, 8, device=DEV)
    for bad in (lambda: ops.pr_metrics(z, torch.zeros(3, 8, device=DEV)), lambda: ops.pr_metrics(z, z[:, :0]),
                lambda: ops.pr_metrics(z, z, [False]), lambda: ops.pr_metrics(z.double(), z)):
        with pytest.raises(JvaeHipError):
            bad()


# ---------------------------------------------------------------------------------------------- the evaluation loops
def synth(n, name, seed, shift=0.):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset((torch.rand(n, 3, 32, 32, generator=g) + shift).clamp(0, 1),
                                       torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


def without(entry, keys):
    return {k: v for k, v in entry.items() if k not in keys}


def test_ood_detection_rates_with_the_switch(monkeypatch):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    net = Net(**dict(get_case('e2_n8_L3')['net']))
    load_det_state(net, seed=0)
    net.to(DEV)
    net.OOD_QUANTILE_METHODS = True
    sets = [synth(24, 'ind', 1), synth(16, 'ood', 2, .3)]
    kw = dict(oodsets=sets[1:], testset=sets[0], batch_size=8, update_self_ood=False)
    recorders = {}
    torch.manual_seed(3)
    first = net.ood_detection_rates(recorders=recorders, **kw)
    assert Net.DETECTION_PR_METRICS is False and not any(k in e for e in first['ood'].values() for k in PR_FIGURES)
    calls, rows, real_roc, real_pr = [], [], ops.roc_curve, ops.pr_metrics
    monkeypatch.setattr(net, 'evaluate', lambda *a, **k: pytest.fail('the recorders are full: nothing is evaluated'))
    monkeypatch.setattr(ops, 'roc_curve', lambda *a, **k: rows.append((a[0].clone(), a[1].clone(), a[3])) or real_roc(*a, **k))
    monkeypatch.setattr(ops, 'pr_metrics', lambda *a, **k: calls.append(a[0].shape) or real_pr(*a, **k))
    off = net.ood_detection_rates(recorders=recorders, **kw)
    assert off == first and not calls
    net.DETECTION_PR_METRICS = True
    on = net.ood_detection_rates(recorders=recorders, **kw)
    methods = list(off['ood'])
    assert len(calls) == 1 and calls[0] == (len(methods), 24)             # ONE call for all methods of the set
    assert any('-a-' in m for m in methods) and any(m.endswith('-2s') for m in methods)
    ins, outs, modes = rows[-1]
    want = real_pr(ins, outs, modes)
    assert not want['status'].cpu().numpy().any()
    for i, m in enumerate(methods):
        assert without(on['ood'][m], PR_FIGURES) == off['ood'][m], m       # key for key, float for float
        if '-a-' in m:
            assert on['ood'][m] == off['ood'][m], m                        # a quantile method gains nothing
            continue
        assert list(on['ood'][m]) == list(off['ood'][m]) + list(PR_FIGURES)
        for j, k in enumerate(PR_FIGURES):
            assert type(on['ood'][m][k]) is float and on['ood'][m][k] == float(want[k][i]), (m, k)
        if not m.endswith('-2s'):              # around the mean the order of near-equal distances hangs on the centre's last bit
            check([on['ood'][m][k] for k in PR_FIGURES], pr_restatement(ins[i].cpu().numpy(), outs[i].cpu().numpy()), 24, 16, m)
    net.DETECTION_PR_METRICS = False
    assert net.ood_detection_rates(recorders=recorders, **kw) == first


def test_misclassification_detection_rates_with_the_switch(monkeypatch):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.recorders import LossRecorder
    from jvae_hip import ops
    c = load_case(GOLDEN, 'cvae_257')
    net = Net(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))
    net.to(DEV)
    rec = LossRecorder(100)
    t = {k: torch.as_tensor(np.ascontiguousarray(v)).to(DEV) for k, v in c['recorder'].items()}
    for i in range(0, t['y_true'].shape[0], 100):
        rec.append_batch(**{k: v[..., i:i + 100] for k, v in t.items()})
    kw = dict(recorder=rec, epoch=7, update_self_results=False)
    first = net.misclassification_detection_rates(**kw)
    seen, real = [], ops.misclass_rates
    monkeypatch.setattr(ops, 'misclass_rates', lambda *a, **k: seen.append((a[0].clone(), a[1].clone())) or real(*a, **k))
    off = net.misclassification_detection_rates(**kw)
    assert off == first and list(first) == list(c['predict'])
    assert 'pr' not in real(*seen[0], [0.9, 0.95])
    net.DETECTION_PR_METRICS = True
    del seen[:]
    on = net.misclassification_detection_rates(**kw)
    keys = Net.MISCLASS_PR_KEYS
    assert list(on) == list(off) and len(seen) == len(off)
    for pm, (scores, mask) in zip(off, seen):
        ins, outs, nc = ops.misclass_split(scores, mask)
        want = ops.pr_metrics(ins, outs)
        assert list(on[pm]) == list(off[pm])
        for i, m in enumerate(off[pm]):
            assert without(on[pm][m], keys) == off[pm][m], (pm, m)
            assert list(on[pm][m]) == list(off[pm][m]) + list(keys)
            for key, k in zip(keys, PR_FIGURES):
                assert type(on[pm][m][key]) is float and on[pm][m][key] == float(want[k][i]), (pm, m, key)
            correct = mask.cpu().numpy().astype(bool)
            row = scores[i].cpu().numpy()
            check([on[pm][m][k] for k in keys], pr_restatement(row[correct], row[~correct]), nc, len(row) - nc, (pm, m))
    net.DETECTION_PR_METRICS = False
    assert net.misclassification_detection_rates(**kw) == first
