"""Misclassification detection on the device (csrc/misclass.hip, ops.misclass_*, ClassificationVariationalNetwork
.misclassification_detection_rates) against the goldens the reference's own method wrote (tools/gen_mdr_golden.py ->
tests/golden/mdr) and the numpy restatement of tests/test_mdr_restatement.py, which reproduces every golden.

Rates, thresholds, confusion counts and precision are compared bit for bit (fp64 expressions over integer counts and exactly widened
scores); the AUC to auc_bound(n_correct) (test_roc_restatement: the reference's own summation error).  The fused score kernel is
held to 4x the reference's own fp32 error against the fp64 formulas (stored per method family in the golden): the margin covers a
different but equally valid fp32 evaluation order of exp and sum.  Measured on the MI355X, maximum error against fp64 (and its
ratio to the reference's own error for the same family):
    cvae_1500: baseline 2.42e-07 (1.00x), softkl 2.45e-07 (1.00x), softzdist 2.41e-07 (1.00x), hyz 3.21e-07 (1.12x)
    cvae_257:  baseline 1.96e-07 (1.00x), softkl 1.14e-07 (1.00x), softzdist 2.14e-07 (1.00x), hyz 3.63e-07 (1.11x)
    vib_1200:  baseline 2.26e-07 (1.00x), hyz 2.98e-07 (1.08x)
kl / zdist / max / logits rows are bit-identical to the reference's (error 0 on both sides).
"""
import logging
import math
import os

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_mdr_restatement import CASES, EXACT_FAMILIES, family, fp64_rows, load_case, mdr_restatement
from test_odin_restatement import odin_cases
from test_roc_restatement import auc_bound

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEPT = [pc / 100 for pc in range(90, 100)]
EPOCH = 7                                                    # not 0: a new model's `testing` already holds an (empty) epoch 0
PAIRS = [(name, pm) for name in CASES for pm in load_case(GOLDEN, name)['predict']]
MODEL_CASES = ('cvae_1500', 'cvae_257', 'vib_1200')


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want.astype(got.dtype), equal_nan=True), (what, got, want)


def check_rows(r, want, n_correct, what):
    """r: host results of ops.misclass_rates; want: per-row dicts as mdr_restatement returns them."""
    for i, w in enumerate(want):
        assert int(r['status'][i]) == 0, what
        for k in ('fpr', 'tpr', 'low', 'tp', 'fp'):
            same(r[k][i], w[k], (what, i, k))
        with np.errstate(invalid='ignore', divide='ignore'):
            same(r['tp'][i] / (r['tp'][i] + r['fp'][i]).astype(np.float64), w['precision'], (what, i, 'precision'))
        assert abs(float(r['auc'][i]) - float(w['auc'])) <= auc_bound(n_correct), (what, i, float(r['auc'][i]), float(w['auc']))


def golden_rows(c, pm):
    return [{k: c[f'{k}_{pm}'][i] for k in ('auc', 'fpr', 'tpr', 'low', 'tp', 'fp', 'precision')} for i in range(len(c['methods']))]


# ---------------------------------------------------------------------------------------------- 1. split + ROC + confusion
@pytest.mark.parametrize('name,pm', PAIRS, ids=[f'{n}-{p}' for n, p in PAIRS])
def test_misclass_rates_match_the_reference_golden(name, pm):
    from jvae_hip import ops
    c = load_case(GOLDEN, name)
    mask = c[f'mask_{pm}']
    r = ops.misclass_rates(dev(c['scores']), dev(mask), KEPT)
    assert r['n_correct'] == int(mask.sum()) and r['tp'].dtype == torch.int32 and r['low'].dtype == torch.float64
    r = host(r)
    print(name, pm, 'n_correct', r['n_correct'], 'auc[0]', r['auc'][0], 'ref', c[f'auc_{pm}'][0])
    check_rows(r, golden_rows(c, pm), int(mask.sum()), (name, pm))


def test_split_keeps_every_score_on_its_side():
    from jvae_hip import ops
    rng = np.random.default_rng(11)
    for M, N in ((1, 1), (3, 63), (2, 1025), (5, 4099)):
        scores, mask = rng.standard_normal((M, N)).astype(np.float32), rng.random(N) < .6
        ins, outs, nc = ops.misclass_split(dev(scores), dev(mask))
        assert nc == int(mask.sum()) and ins.shape == (M, nc) and outs.shape == (M, N - nc)
        same(ins.cpu().numpy(), scores[:, mask], ('ins', M, N))      # the scatter keeps the order of each side
        same(outs.cpu().numpy(), scores[:, ~mask], ('outs', M, N))


def test_batched_rows_equal_single_rows_and_runs_repeat():
    from jvae_hip import ops
    c = load_case(GOLDEN, 'cvae_257')
    scores, mask = dev(c['scores']), dev(c['mask_iws'])
    a, b = host(ops.misclass_rates(scores, mask, KEPT)), host(ops.misclass_rates(scores, mask, KEPT))
    for k in ('auc', 'fpr', 'tpr', 'low', 'up', 'tp', 'fp', 'status'):
        assert a[k].tobytes() == b[k].tobytes(), k
    for i in range(0, len(c['methods']), 6):
        one = host(ops.misclass_rates(scores[i], mask, KEPT))
        assert one['n_correct'] == a['n_correct']
        for k in ('auc', 'fpr', 'tpr', 'low', 'up', 'tp', 'fp', 'status'):
            assert one[k].tobytes() == a[k][i].tobytes(), (i, k)


def test_confusion_counts_of_plain_thresholds():
    """Thresholds that are not scores of the row, +-inf and NaN among them; N not a multiple of the 2048 samples of a block."""
    from jvae_hip import ops
    rng = np.random.default_rng(5)
    M, N, K = 3, 5000, 16
    scores, mask = rng.standard_normal((M, N)).astype(np.float32), rng.random(N) < .7
    thr = rng.standard_normal((M, K))
    thr[0, 0], thr[1, 3], thr[2, 5], thr[2, 6] = -np.inf, np.inf, np.nan, float(scores[2, 17])
    tp, fp = ops.misclass_confusion(dev(scores), dev(mask), dev(thr))
    wide = scores.astype(np.float64)
    with np.errstate(invalid='ignore'):
        ge = wide[:, None, :] >= thr[:, :, None]
    same(tp.cpu().numpy(), (ge & mask).sum(-1), 'tp'), same(fp.cpu().numpy(), (ge & ~mask).sum(-1), 'fp')


# ---------------------------------------------------------------------------------------------- 2. + 3. score rows
def fused_rows(c):
    """Every fused method of a golden case through ops.misclass_scores, one launch per source tensor -> {method: fp32 row}."""
    from jvae_hip import ops
    from module import score_rows
    traits = score_rows.Traits(losses_might_be_computed_for_each_class=True, is_vae=False, is_jvae=False, num_labels=10)
    by_source = {}
    for m in c['methods']:
        row = score_rows.parse(m, traits, misclass=True)       # none of these rows depends on the model type
        if m != 'iws' and row.kind is not None:                 # the misclassification pass keeps `iws` on its torch row
            by_source.setdefault(row.source, []).append((m, (row.kind, row.const)))
    out = {}
    for key, rows in by_source.items():
        got = ops.misclass_scores(dev(c['recorder'][key]), [spec for _, spec in rows]).cpu().numpy()
        out.update({m: got[i] for i, (m, _) in enumerate(rows)})
    return out


@pytest.mark.parametrize('name', MODEL_CASES)
def test_fused_scores_against_the_fp64_formulas(name):
    c = load_case(GOLDEN, name)
    exact, got = fp64_rows(c['recorder'], c['methods']), fused_rows(c)
    assert set(got) == {m for m in c['methods'] if m != 'iws' and not m.startswith('odin')}
    worst = {}
    for m, row in got.items():
        err = float(np.abs(row.astype(np.float64) - exact[m]).max())
        worst[family(m)] = max(worst.get(family(m), 0.), err)
        if family(m) in EXACT_FAMILIES:
            assert row.tobytes() == c['scores'][c['methods'].index(m)].tobytes(), m      # pure max / negation: the reference's bits
    for fam, err in sorted(worst.items()):
        ref = c['referr'][fam]
        print(name, fam, 'device error', err, 'reference error', ref, 'ratio', err / ref if ref else 0.)
        assert err <= 4 * ref, (name, fam, err, ref)


def cvae_net(**kw):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case('c1_n16_mlp')['net'], gamma=0., **kw))      # gamma = 0: predict methods ('iws', 'closest')
    net.to(DEV)
    return net


def device_recorder_tensors(c):
    t = {k: dev(v) for k, v in c['recorder'].items()}
    logits, y = t.pop('logits').T, t.pop('y_true')
    return logits, t, y


def test_batch_dist_measures_new_branches_and_old_ones_bit_for_bit():
    from jvae_hip import ops
    from module import score_rows
    c = load_case(GOLDEN, 'cvae_1500')
    net = cvae_net()
    logits, losses, _ = device_recorder_tensors(c)
    losses['wmse'] = losses['cross_x'][0] * .5
    losses['cross_x'] = losses['cross_x'][0]
    new = {'softiws': ('iws', 'soft+', 1.), 'softiws-5': ('iws', 'soft-', 5.), 'softzdist-1': ('zdist', 'soft-', 1.),
           'softzdist-100': ('zdist', 'soft-', 100.), 'hyz': ('logits', 'hyz', 1.)}
    got = net.batch_dist_measures(logits, losses, list(new))
    rec = dict(c['recorder'])
    exact = fp64_rows(rec, list(new))
    soft_bar, hyz_bar = 4 * max(c['referr'][f] for f in ('softkl', 'softzdist', 'baseline')), 4 * c['referr']['hyz']
    for m, (key, kind, T) in new.items():
        row = score_rows.parse(m, score_rows.traits_of(net), misclass=True)
        assert (row.source, (row.kind, row.const)) == (key, (kind, T))
        fused = ops.misclass_scores(dev(rec[key]), [(kind, T)])[0].cpu().numpy().astype(np.float64)
        torch_row = got[m].cpu().numpy().astype(np.float64)
        bar = hyz_bar if m == 'hyz' else soft_bar
        print(m, 'torch vs fp64', np.abs(torch_row - exact[m]).max(), 'fused vs fp64', np.abs(fused - exact[m]).max(), 'bar', bar)
        assert np.abs(torch_row - exact[m]).max() <= bar and np.abs(fused - exact[m]).max() <= bar, m
        assert np.abs(torch_row - fused).max() <= bar, m
    C = 10
    top = losses['iws'].max(0)[0]
    old = {'elbo': (-losses['total']).max(0)[0], 'max': (-losses['total']).max(0)[0],
           'iws': (losses['iws'] - top).exp().sum(0).log() + top + math.log(C),
           'iws-2s': (losses['iws'] - top).exp().sum(0).log() + top + math.log(C),
           'soft': (-losses['kl']).softmax(0).max(0)[0], 'softkl': (-losses['kl']).softmax(0).max(0)[0],
           'softkl-10': (-losses['kl'] / 10.).softmax(0).max(0)[0], 'zdist': (-losses['zdist']).max(0)[0],
           'kl': (-losses['kl']).max(0)[0], 'mse': -losses['cross_x'], 'wmse': -losses['wmse'], 'logits': logits.max(-1)[0],
           'baseline': (logits / 1.).softmax(-1).max(-1)[0], 'baseline-5': (logits / 5.).softmax(-1).max(-1)[0]}
    got = net.batch_dist_measures(logits, losses, list(old))
    for m, want in old.items():
        assert torch.equal(got[m], want), m


# ---------------------------------------------------------------------------------------------- 4. end to end, cvae
def capture_scores(monkeypatch):
    """Record the (M, N) score rows and the mask of every ops.misclass_rates call."""
    from jvae_hip import ops
    seen, real = [], ops.misclass_rates

    def spy(scores, mask, kept):
        seen.append((scores.detach().cpu().numpy().copy(), mask.detach().cpu().numpy().astype(bool)))
        return real(scores, mask, kept)
    monkeypatch.setattr(ops, 'misclass_rates', spy)
    return seen


def recorder_of(c, batch=100, device=DEV):
    from jvae_compat.recorders import LossRecorder
    rec = LossRecorder(batch)
    t = {k: torch.as_tensor(np.ascontiguousarray(v)).to(device) for k, v in c['recorder'].items()}
    for i in range(0, t['y_true'].shape[0], batch):
        rec.append_batch(**{k: v[..., i:i + batch] for k, v in t.items()})
    return rec


def check_entries(res, seen, methods, predict, n, c=None):
    assert list(res) == list(predict) and len(seen) == len(predict)
    for pm, (scores, mask) in zip(predict, seen):
        assert list(res[pm]) == list(methods) and scores.shape == (len(methods), n)
        for i, m in enumerate(methods):
            e, w = res[pm][m], mdr_restatement(scores[i], mask, KEPT)
            assert set(e) == {'n', 'epochs', 'sampling', 'tpr', 'fpr', 'auc', 'precision'}
            assert e['n'] == n and e['epochs'] == EPOCH and type(e['auc']) is float
            assert all(type(v) is float for k in ('tpr', 'fpr', 'precision') for v in e[k]) and len(e['tpr']) == 10
            same(e['tpr'], w['tpr'], (pm, m, 'tpr')), same(e['fpr'], w['fpr'], (pm, m, 'fpr'))
            same(e['precision'], w['precision'], (pm, m, 'precision'))
            assert abs(e['auc'] - w['auc']) <= auc_bound(int(mask.sum())), (pm, m)
            if c is not None:
                ref = float(c[f'auc_{pm}'][c['methods'].index(m)])
                assert abs(e['auc'] - ref) <= 1e-3, (pm, m, e['auc'], ref)


@pytest.mark.parametrize('name', ['cvae_1500', 'cvae_257'])
def test_misclassification_detection_rates_of_a_cvae(name, tmp_path, monkeypatch):
    from cvae import ClassificationVariationalNetwork as Net
    c = load_case(GOLDEN, name)
    n = c['scores'].shape[1]
    net = cvae_net()
    net.train()
    seen = capture_scores(monkeypatch)
    res = net.misclassification_detection_rates(recorder=recorder_of(c), epoch=EPOCH)
    assert net.training                                        # left as found
    assert net.misclass_methods == Net.misclass_methods_per_type['cvae']          # the starred names are not expanded in place
    check_entries(res, seen, c['methods'], c['predict'], n, c)
    for pm, (_, mask) in zip(c['predict'], seen):
        same(mask, c[f'mask_{pm}'], pm)
        head = net.testing[EPOCH][pm]
        assert head['n'] == n and head['accuracy'] == float(c[f'accuracy_{pm}']) and head['sampling'] == 1
        assert type(head['accuracy']) is float
        for m in c['methods']:
            assert head[m] is res[pm][m]
    saved = net.save(str(tmp_path / 'job'))
    back = Net.load(saved, load_state=False)
    assert back.testing[EPOCH] == net.testing[EPOCH]            # through test.json (no NaN among the kept precisions here)

    # the same from saved_dir/samples/<epoch>/record-<set>.pth, found as the last epoch
    sdir = os.path.join(saved, 'samples', '{:04d}'.format(EPOCH))
    os.makedirs(sdir)
    os.makedirs(os.path.join(saved, 'samples', '0009'))       # an epoch directory without the file is not the last one
    recorder_of(c, device='cpu').save(os.path.join(sdir, 'record-synth.pth'))
    net.training_parameters['set'] = 'synth'
    assert net.saved_dir == saved
    again = net.misclassification_detection_rates(update_self_results=False)
    assert again == res
    assert net.misclassification_detection_rates(epoch=9, update_self_results=False) is None
    assert net.misclassification_detection_rates(from_where=('json',), update_self_results=False) is None
    few = net.misclassification_detection_rates(predict_methods='closest', misclass_methods=['kl', 'softzdist*'], epoch=EPOCH,
                                                update_self_results=False)
    assert list(few) == ['closest'] and list(few['closest']) == ['kl'] + [f'softzdist-{T}' for T in (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000)]
    assert few['closest']['kl'] == res['closest']['kl']


def test_a_method_whose_loss_is_not_recorded_is_skipped():
    c = load_case(GOLDEN, 'cvae_257')
    del c['recorder']['iws']
    net = cvae_net()
    res = net.misclassification_detection_rates(predict_methods='closest', recorder=recorder_of(c), epoch=EPOCH)
    assert list(res['closest']) == [m for m in c['methods'] if m != 'iws']


# ---------------------------------------------------------------------------------------------- 5. end to end, vib
def synth(n, name, seed, shift=0.):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset((torch.rand(n, 1, 28, 28, generator=g) + shift).clamp(0, 1),
                                       torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


def test_misclassification_detection_rates_of_a_vib_with_the_odin_grid(monkeypatch):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    net = Net(**dict(odin_cases()['mb2_n8_vib_L2_mlp']))
    load_det_state(net, seed=0)
    net.to(DEV)
    sets = [synth(96, 'ind', 1), synth(48, 'ood', 2, .3)]
    recorders = {}
    torch.manual_seed(3)
    net.ood_detection_rates(oodsets=sets[1:], testset=sets[0], batch_size=48, recorders=recorders, update_self_ood=False)
    rec = recorders['ind']
    assert rec.recorded_samples == 96 and 'logits' in rec.keys() and len([k for k in rec.keys() if k.startswith('odin-')]) == 210
    assert float(net.accuracy(sets[0], batch_size=48, recorder=rec, update_self_testing=False)['esty']) not in (0., 1.)
    rocs, real = [], ops.roc_curve
    monkeypatch.setattr(ops, 'roc_curve', lambda *a, **k: rocs.append(a[0].shape) or real(*a, **k))
    seen = capture_scores(monkeypatch)
    res = net.misclassification_detection_rates(recorder=rec, epoch=EPOCH)
    methods = ['baseline', 'logits', 'hyz'] + net._odin_names()
    assert len(methods) == 213 and len(rocs) == 1 and rocs[0][0] == 213     # ONE ROC call for the one prediction method
    check_entries(res, seen, methods, ['esty'], 96)
    scores, mask = seen[0]
    same(scores[3:], torch.stack([rec[m] for m in methods[3:]]).cpu().numpy(), 'odin rows are the recorded ones')
    y_est = rec['logits'].argmax(0)
    same(mask, (y_est == rec['y_true']).cpu().numpy(), 'mask')
    assert net.testing[EPOCH]['esty']['accuracy'] == float(mask.sum()) / 96
    one = net.misclassification_detection_rates(misclass_methods='odin-10-0.0012', recorder=rec, epoch=EPOCH, update_self_results=False)
    assert one['esty']['odin-10-0.0012'] == res['esty']['odin-10-0.0012']


# ---------------------------------------------------------------------------------------------- 6. host copies
def test_no_host_copy_per_row(monkeypatch):
    """Host copies (Tensor.cpu / item / tolist / numpy) per prediction method: n_correct and the one result block, whatever the
    number of methods M and of samples N."""
    small, big = load_case(GOLDEN, 'cvae_257'), load_case(GOLDEN, 'cvae_1500')
    net = cvae_net()
    recs = recorder_of(small), recorder_of(big)
    count = {'n': 0}
    for name in ('cpu', 'item', 'tolist', 'numpy'):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, **k):
            count['n'] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    count['n'] = 0
    net.misclassification_detection_rates(predict_methods='iws', misclass_methods='kl', recorder=recs[0], epoch=EPOCH)
    few = count['n']
    count['n'] = 0
    res = net.misclassification_detection_rates(recorder=recs[1], epoch=EPOCH)
    many = count['n']
    print('host copies: 1 method x 1 prediction', few, '35 methods x 2 predictions', many)
    assert len(res) == 2 and len(res['iws']) == 35
    assert few <= 4 and many == 2 * few


# ---------------------------------------------------------------------------------------------- 7. decided failure modes
def test_decided_failure_modes(caplog):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    c = load_case(GOLDEN, 'cvae_257')
    net = cvae_net()
    closest = c['recorder']['zdist'].argmin(0)

    right = dict(c, recorder=dict(c['recorder'], y_true=closest))               # 'closest' gets every sample right
    with caplog.at_level(logging.WARNING):
        res = net.misclassification_detection_rates(recorder=recorder_of(right), epoch=EPOCH)
    assert list(res) == ['iws'] and len(res['iws']) == 35
    assert [r for r in caplog.records if r.levelno == logging.WARNING and 'closest' in r.getMessage()]
    assert 'closest' not in net.testing[EPOCH]
    caplog.clear()
    wrong = dict(c, recorder=dict(c['recorder'], y_true=(closest + 1) % 10))   # ... and none
    with caplog.at_level(logging.WARNING):
        res = net.misclassification_detection_rates(predict_methods='closest', recorder=recorder_of(wrong), epoch=EPOCH)
    assert res == {} and [r for r in caplog.records if 'closest' in r.getMessage()]
    caplog.clear()

    logits = c['recorder']['logits'].copy()
    logits[0, 5], logits[1, 5] = 150., -150.                                     # a softmax term underflows to 0: hyz is NaN there
    nan = dict(c, recorder=dict(c['recorder'], logits=logits))
    with caplog.at_level(logging.WARNING):
        res = net.misclassification_detection_rates(recorder=recorder_of(nan), epoch=EPOCH, update_self_results=False)
    for pm in ('iws', 'closest'):
        assert list(res[pm]) == [m for m in c['methods'] if m != 'hyz']
        assert [r for r in caplog.records if f'{pm}-hyz' in r.getMessage()]

    for bad in (dict(misclass_methods='softmax'), dict(misclass_methods=['kl', 'odin-1-0.0000']), dict(predict_methods='esty')):
        with pytest.raises(ValueError):
            net.misclassification_detection_rates(recorder=recorder_of(c), epoch=EPOCH, **bad)
    vae = Net(**dict(get_case('ea2_n8_vae_L3')['net']))
    assert vae.misclassification_detection_rates(recorder=recorder_of(c, device='cpu')) is None      # no methods for a vae

    with pytest.raises(ValueError):
        ops.misclass_rates(torch.zeros(2, 8, device=DEV), torch.ones(8, dtype=torch.bool, device=DEV), KEPT)
    with pytest.raises(JvaeHipError):                                              # C beyond the kernel's bound
        ops.misclass_scores(torch.zeros(129, 8, device=DEV), [('max-', 1.)])
    # there is no CPU path
    for call in (lambda: ops.misclass_scores(torch.zeros(10, 8), [('max-', 1.)]),
                 lambda: ops.misclass_split(torch.zeros(2, 8), torch.ones(8, dtype=torch.bool)),
                 lambda: ops.misclass_confusion(torch.zeros(2, 8), torch.ones(8, dtype=torch.bool), torch.zeros(2, 3, dtype=torch.float64)),
                 lambda: ops.misclass_rates(torch.zeros(2, 8), torch.ones(8, dtype=torch.bool), KEPT)):
        with pytest.raises(JvaeHipError):
            call()
    on_cpu = Net(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))
    with pytest.raises(JvaeHipError):
        on_cpu.misclassification_detection_rates(recorder=recorder_of(c, device='cpu'), epoch=EPOCH)
    torch.cuda.synchronize()
