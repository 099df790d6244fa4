"""Mahalanobis OOD scores on the MI355X (ops.maha_moments / maha_fit / maha_scores, csrc/maha.hip, cvae.fit_latent_gaussians /
maha_scores) against the fp64 restatement and the bars of tests/test_maha_restatement.py.

Inputs are fp32 values and the reference is computed in fp64 from those same values.  Moments: counts exact, a mean within
M 2^-52 mean_i |b_ik|, a scatter entry within (M + 4) 2^-52 sqrt(S_ii S_jj) (Cauchy-Schwarz on the fp64 accumulation), the bits
of a second call.  Scores: d within max_c bar_c, rel within max_c bar_c + bar_0, a per-class entry within its own bar_c, cls a
class within 2 max_c bar_c of the fp64 minimum (test_maha_restatement.check_scores); the bits of a second call, of a call with the
per-class output and of N split into two calls.  Every figure is printed before its assertion.

Worst error / bar measured on the MI355X, per shape (K, N, M, C, offset, shrinkage): see DESIGN.md section 7q."""
import numpy as np
import pytest
import torch

from test_28_knn_gpu import build, stacked_posterior, synth
from test_maha_restatement import (SHAPES, bars, case, check_scores, maha_case, moments_restatement, scores_restatement)
from test_roc_restatement import auc_bound, roc_restatement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEPT = [pc / 100 for pc in range(90, 100)]
EPS = 2. ** -52


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_moments(bank, labels, C):
    """-> ({name: numpy array}, status) from a status word of the call's own."""
    from jvae_hip import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.maha_moments(dev(bank), dev(labels), C, status=status)
    K = bank.shape[1]
    assert got['counts'].dtype == torch.int64 and all(got[k].dtype == torch.float64 for k in ('means', 'mean0', 'Sw', 'St'))
    assert {k: tuple(v.shape) for k, v in got.items()} == {'counts': (C,), 'means': (C, K), 'mean0': (K,), 'Sw': (K, K), 'St': (K, K)}
    return {k: v.cpu().numpy() for k, v in got.items()}, int(status)


def check_moments(got, bank, labels, C, tag):
    """The device moments against the fp64 restatement on the same rows."""
    want = moments_restatement(bank, labels, C)
    M = bank.shape[0]
    assert np.array_equal(got['counts'], want['counts'])
    scale = np.abs(bank.astype(np.float64)).mean(0)
    ratios = {'means': np.abs(got['means'] - want['means']) / (M * EPS * scale), 'mean0': np.abs(got['mean0'] - want['mean0']) / (M * EPS * scale)}
    for k in ('Sw', 'St'):
        diag = np.sqrt(np.outer(np.diag(want[k]), np.diag(want[k])))
        with np.errstate(invalid='ignore', divide='ignore'):
            r = np.abs(got[k] - want[k]) / ((M + 4) * EPS * diag)
        ratios[k] = np.where((diag == 0) & (got[k] == want[k]), 0., r)
        assert np.array_equal(got[k], got[k].T), (tag, k)                    # symmetric to the bit
    worst = {k: float(v.max()) for k, v in ratios.items()}
    print(tag, 'moments: worst error / bar', worst)
    assert all(v <= 1. for v in worst.values()), (tag, worst)
    assert (got['means'][want['counts'] == 0] == 0).all()


_FITS = {}


def device_fit(shape):
    """The fit of one shape from the device's own moments, computed once and never modified."""
    from jvae_hip import ops
    if shape not in _FITS:
        c = case(shape)
        _FITS[shape] = ops.maha_fit(ops.maha_moments(dev(c['bank']), dev(c['labels']), shape[3]), shape[5])
    return _FITS[shape]


def run_scores(q, fit, per_class=False):
    """-> ({'d', 'cls', 'rel', 'dc'} as numpy, status)."""
    from jvae_hip import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.maha_scores(dev(q), fit, per_class=per_class, status=status)
    N, C = q.shape[0], fit['counts'].shape[0]
    assert len(got) == 3 + per_class and got[0].dtype == got[2].dtype == torch.float32 and got[1].dtype == torch.int32
    assert got[0].shape == got[1].shape == got[2].shape == (N,) and (not per_class or (got[3].shape == (N, C) and got[3].dtype == torch.float32))
    host = [t.cpu().numpy() for t in got]
    return dict(d=host[0], cls=host[1], rel=host[2], dc=host[3] if per_class else None), int(status)


def same_bits(a, b, keys=('d', 'cls', 'rel', 'dc')):
    return all((a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]).view(np.int32), np.asarray(b[k]).view(np.int32))
               for k in keys)


# ------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize('shape', SHAPES)
def test_moments_shapes(shape):
    c = case(shape)
    got, status = run_moments(c['bank'], c['labels'], shape[3])
    assert status == 0
    check_moments(got, c['bank'], c['labels'], shape[3], f'{shape}')
    again, _ = run_moments(c['bank'], c['labels'], shape[3])
    assert all(np.array_equal(got[k].view(np.int64), again[k].view(np.int64)) for k in got)          # no atomics on a float


def test_moments_over_several_slabs():
    """More rows than one slab holds (2048), and a count that is no multiple of the slab or of the workgroup."""
    _, bank, labels = maha_case(20, 2, 7001, 7, 30.)
    got, status = run_moments(bank, labels, 7)
    assert status == 0
    check_moments(got, bank, labels, 7, 'four slabs')
    again, _ = run_moments(bank, labels, 7)
    assert all(np.array_equal(got[k].view(np.int64), again[k].view(np.int64)) for k in got)


def test_moments_with_an_empty_class():
    _, bank, labels = maha_case(16, 2, 300, 5, 0.)
    keep = labels != 2
    got, status = run_moments(bank[keep], labels[keep], 5)
    assert status == 0 and got['counts'][2] == 0 and (got['means'][2] == 0).all()
    check_moments(got, bank[keep], labels[keep], 5, 'class 2 empty')


def test_moments_flag_and_leave_out_bad_rows():
    from jvae_hip import ops
    _, bank, labels = maha_case(16, 2, 300, 5, 0.)
    bank, labels = bank.copy(), labels.copy()
    labels[7], labels[150] = -1, 5
    bank[33, 4], bank[299, 15] = np.nan, np.inf
    got, status = run_moments(bank, labels, 5)
    assert status == ops.MAHA_STATUS_LABEL | ops.MAHA_STATUS_BANK
    keep = np.ones(300, bool)
    keep[[7, 150, 33, 299]] = False
    assert got['counts'].sum() == 296
    check_moments(got, bank[keep], labels[keep], 5, 'four rows left out')   # the other rows' sums: those of the bank without them
    only_label, status = run_moments(np.nan_to_num(bank, nan=0., posinf=0.), labels, 5)
    assert status == ops.MAHA_STATUS_LABEL and only_label['counts'].sum() == 298
    word = torch.tensor([status], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='label'):
        ops.maha_check_status(word)
    assert int(word) == 0                                                    # read and cleared


# ------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize('shape', SHAPES)
def test_scores_shapes(shape):
    c, fit = case(shape), device_fit(shape)
    got, status = run_scores(c['q'], fit, per_class=True)
    assert status == 0
    worst = check_scores(got, c['ref'], c['bars'], f'{shape}')
    assert worst <= 1.
    plain, _ = run_scores(c['q'], fit)
    assert same_bits(plain, got, ('d', 'cls', 'rel'))                        # the per-class output changes nothing
    again, _ = run_scores(c['q'], fit, per_class=True)
    assert same_bits(again, got)
    n1 = c['q'].shape[0] // 2 + 1                                            # no multiple of the 32 rows of a workgroup
    a, b = run_scores(c['q'][:n1], fit, per_class=True)[0], run_scores(c['q'][n1:], fit, per_class=True)[0]
    assert same_bits({k: np.concatenate([a[k], b[k]]) for k in a}, got)


def test_an_empty_class_is_never_the_argmin():
    from jvae_hip import ops
    q, bank, labels = maha_case(16, 70, 300, 5, 0.)
    keep = labels != 2
    mom = moments_restatement(bank[keep], labels[keep], 5)
    fit = ops.maha_fit(ops.maha_moments(dev(bank[keep]), dev(labels[keep]), 5))
    assert fit['cmap'].tolist() == [0, 1, 3, 4]
    got, status = run_scores(q, fit, per_class=True)
    assert status == 0 and (got['cls'] != 2).all() and (got['dc'][:, 2] == np.inf).all() and np.isfinite(got['dc'][:, [0, 1, 3, 4]]).all()
    check_scores(got, scores_restatement(q, mom, 0.), bars(q, mom, 0.), 'class 2 empty')


def test_a_non_finite_query_row():
    from jvae_hip import ops
    shape = SHAPES[2]                                                        # 130 rows: five workgroups
    c, fit = case(shape), device_fit(shape)
    clean, _ = run_scores(c['q'], fit, per_class=True)
    q = c['q'].copy()
    q[3, 5], q[64, 0], q[129, 15] = np.nan, np.inf, -np.inf
    got, status = run_scores(q, fit, per_class=True)
    assert status == ops.MAHA_STATUS_QUERY
    bad = np.zeros(130, bool)
    bad[[3, 64, 129]] = True
    check_scores(got, c['ref'], c['bars'], 'three rows not finite', bad=bad)
    assert same_bits({k: v[~bad] for k, v in got.items()}, {k: v[~bad] for k, v in clean.items()})   # the neighbours: unchanged
    word = torch.tensor([status], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='query'):
        ops.maha_check_status(word)
    assert int(word) == 0


def test_no_rows():
    fit = device_fit(SHAPES[2])
    got, status = run_scores(np.zeros((0, 16), np.float32), fit, per_class=True)
    assert status == 0 and got['d'].shape == (0,) and got['dc'].shape == (0, 10)


# ------------------------------------------------------------------------------------------- the model
_MODEL = {}


def fitted():
    """One model with its bank over a 96-image set and the Gaussians fitted on it, shared by the tests that read them."""
    if not _MODEL:
        net, train = build(), synth(96, 'train', 5)
        net.fit_latent_bank(train, batch_size=40)
        _MODEL.update(net=net, train=train, fit=net.fit_latent_gaussians())
    return _MODEL['net'], _MODEL['train'], _MODEL['fit']


def test_fit_latent_gaussians():
    from jvae_hip import ops
    net, train, fit = fitted()
    bank = net.latent_bank
    assert fit is net.latent_gaussians and fit['set'] == 'train' and fit['shrinkage'] == 0. and ops.maha_check_fit(fit) == (16, 10, 10)
    want = ops.maha_fit(ops.maha_moments(bank['bank'], bank['labels'], 10))
    assert all(torch.equal(fit[k], want[k]) and fit[k].device == bank['bank'].device for k in want if torch.is_tensor(want[k]))
    assert torch.equal(fit['counts'].cpu(), torch.bincount(train.tensors[1], minlength=10))
    other = build()
    other.latent_bank = dict(bank)
    assert other.fit_latent_gaussians(shrinkage=0.05)['shrinkage'] == 0.05 and not torch.equal(other.latent_gaussians['W'], fit['W'])
    other.latent_bank = dict(bank, labels=bank['labels'] + 5)               # labels outside the model's classes
    with pytest.raises(ValueError, match='label'):
        other.fit_latent_gaussians()


def test_maha_scores_against_the_restatement():
    net, train, fit = fitted()
    mu = net.latent_posterior(synth(37, 'q', 9).tensors[0].to(DEV))[0]
    scores = net.maha_scores(mu)
    assert list(scores) == ['maha', 'maha-rel']
    assert all(v.shape == (37,) and v.dtype == torch.float32 and v.is_cuda for v in scores.values())
    q, b, y = mu.cpu().numpy(), net.latent_bank['bank'].cpu().numpy(), net.latent_bank['labels'].cpu().numpy()
    mom = moments_restatement(b, y, 10)
    ref, bar = scores_restatement(q, mom, 0.), bars(q, mom, 0.)
    print('model: condition number of Sw', float(np.linalg.cond(mom['Sw'])), 'largest bar / d', float((bar['top'] / ref['d']).max()))
    got = dict(d=-scores['maha'].cpu().numpy(), rel=-scores['maha-rel'].cpu().numpy(), cls=ref['cls'], dc=None)
    check_scores(got, ref, bar, 'model')


def test_rates(monkeypatch):
    from module import score_rows
    net, train, fit = fitted()
    names = ['maha', 'maha-rel']
    sets = [synth(40, 'ind', 1), synth(40, 'ood', 2, .3)]
    call = dict(oodsets=sets[1:], testset=sets[0], batch_size=16, update_self_ood=False)
    for m in (['elbo'] + names, 'maha*', 'maha-rel'):
        with pytest.raises(NotImplementedError, match='OOD_MAHA_METHODS'):            # off: the names raise
            net.ood_detection_rates(method=m, **call)
    torch.manual_seed(11)
    plain = net.ood_detection_rates(method=['elbo'], **call)
    torch.manual_seed(11)
    off_all = net.ood_detection_rates(method='all', **call)
    families = score_rows.FAMILIES
    monkeypatch.setattr(score_rows, 'FAMILIES', tuple(f for f in families if f.prefix != 'maha'))      # the table without the family
    torch.manual_seed(11)
    assert net.ood_detection_rates(method='all', **call) == off_all                    # off: 'all' is bit for bit what it was
    monkeypatch.setattr(score_rows, 'FAMILIES', families)
    assert not any(m.startswith('maha') for m in off_all['ood'])
    net.OOD_MAHA_METHODS = True
    try:
        torch.manual_seed(11)
        bare = net.ood_detection_rates(method=['elbo', 'maha*'], **call)
        assert list(bare['ood']) == ['elbo'] + names
        assert bare['ood']['elbo'] == plain['ood']['elbo']                              # the other rows: the same bits
        torch.manual_seed(11)
        on_all = net.ood_detection_rates(method='all', **call)
        assert list(on_all['ood']) == list(off_all['ood']) + names and all(on_all['ood'][m] == off_all['ood'][m] for m in off_all['ood'])
        recorders = {}                                                                  # (a recorder seeds the noise by itself)
        first = net.ood_detection_rates(method=['elbo'] + names, recorders=recorders, **call)
        assert list(first['ood']) == ['elbo'] + names and all(first['ood'][m] == bare['ood'][m] for m in names)
        for s in sets:
            mu = stacked_posterior(net, s, 16)
            want = {}
            for i in range(0, 40, 16):                                                  # the batches of the pass
                for m, v in net.maha_scores(mu[i:i + 16]).items():
                    want.setdefault(m, []).append(v)
            for m in names:
                assert torch.equal(recorders[s.name][m].to(DEV), torch.cat(want[m])), (s.name, m)
        for m in names:
            ins, outs = (recorders[s][m].float().cpu().numpy() for s in ('ind', 'ood'))
            r = first['ood'][m]
            auc, fpr, tpr, low, up = roc_restatement(ins, outs, KEPT)
            print(m, 'auc', r['auc'], 'restated', auc, 'mean score in / out', ins.mean(), outs.mean())
            assert r['n'] == 40 and r['fpr'] == fpr.tolist() and abs(r['auc'] - auc) <= auc_bound(40)
        assert net.test_losses and not any(k.startswith('maha') for k in net.test_losses)     # test_losses: the loss components only
        calls = []
        real_eval, real_maha = net.evaluate, net.maha_scores
        monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append('e') or real_eval(*a, **k))
        monkeypatch.setattr(net, 'maha_scores', lambda *a, **k: calls.append('m') or real_maha(*a, **k))
        again = net.ood_detection_rates(method=['elbo'] + names, recorders=recorders, **call)
        assert not calls and again == first                                             # a full recorder is read back
        one = net.ood_detection_rates(method='maha-rel', **call)
        assert list(one['ood']) == ['maha-rel'] and one['ood']['maha-rel'] == first['ood']['maha-rel']
        assert calls.count('e') == 6 and calls.count('m') == 6                          # one pass and one maha call per batch
    finally:
        del net.OOD_MAHA_METHODS


def test_gaussians_file_round_trip(tmp_path):
    net, train, fit = fitted()
    path = net.save_latent_gaussians(str(tmp_path))
    assert path == str(tmp_path / 'latent-gaussians.pth')
    other = build()
    got = other.load_latent_gaussians(str(tmp_path))
    assert got['set'] == 'train' and got['shrinkage'] == fit['shrinkage']
    assert all(torch.equal(got[k], fit[k]) and got[k].device == fit[k].device for k in fit if torch.is_tensor(fit[k]))
    mu = net.latent_posterior(synth(9, 'q', 2).tensors[0].to(DEV))[0]
    a, b = net.maha_scores(mu), other.maha_scores(mu)
    assert list(a) == ['maha', 'maha-rel'] and all(torch.equal(a[m], b[m]) for m in a)
