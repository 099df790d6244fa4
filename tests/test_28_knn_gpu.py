"""Nearest-neighbour OOD scores on the MI355X (ops.knn, csrc/knn.hip, cvae.fit_latent_bank / knn_scores)
against the fp64 restatement of tests/test_knn_restatement.py.

Inputs are fp32 values and the reference is computed in fp64 from those same values.  Bars (test_knn_restatement.py, u = 2^-24):
plain bar_ij = 2 (K + 3) u (|q_i|^2 + |b_j|^2), normalised bar = 4 (K + 4) u; slot j of a row is held to the largest bar of the
row (an order statistic is 1-Lipschitz in the sup norm: near ties do not loosen anything, no element is left out).  On every
kernel case: values inside the bar and ascending; indices in [0, M), distinct; the fp64 distance of the row named in slot j within
twice the bar of the true j-th smallest (once for the value, once for a neighbour that took its place); +inf / -1 beyond the bank's
rows; a second call and splits in {1, 2, 5} return the bits of the first.  The workload-size case takes its fp64 reference from
one matrix product (2 - 2 cos on the fp64-normalised rows: the product form's own error there is K 2^-52, nothing beside the bar).
Model level: the square root carries a bar e on d2 to min(sqrt(e), e / sqrt(d2)) on the distance, plus the root's own rounding.
Every distance is printed before its assertion."""
import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_knn_restatement import (COPIES, NAN_BANK_ROW, NAN_QUERY_ROW, SHAPES, U, VARIANT_SHAPE, knn_case, knn_distances, knn_restatement,
                                  normalized_bar, plain_bar, row_bars, select)
from test_regret_restatement import regret_cases
from test_roc_restatement import auc_bound, roc_restatement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEPT = [pc / 100 for pc in range(90, 100)]
MODES = [False, True]


def run(q, bank, k, normalized, splits):
    """-> (d2 (N, k) fp32, idx (N, k) int32, status) as numpy / int, from a status word of the call's own."""
    from jvae_hip import ops
    b, sq = ops.knn_bank(torch.from_numpy(bank).to(DEV))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    d2, idx = ops.knn(torch.from_numpy(q).to(DEV), b, sq, k, normalized=normalized, splits=splits, status=status)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (q.shape[0], k)
    return d2.cpu().numpy(), idx.cpu().numpy(), int(status)


def same_bits(a, b):
    return np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def check_against(D, bad_q, bars, k, got, tag):
    """The checks every kernel case shares; D (N, M) the fp64 distances, bars (N,)."""
    d2, idx, _ = got
    N, M = D.shape
    ref, _ = select(D, k, bad_q)
    key = np.where(np.isfinite(D), D, np.inf)
    good = ~bad_q
    fin = np.isfinite(ref) & good[:, None]
    wide = np.broadcast_to(bars[:, None], ref.shape)
    assert (np.isfinite(d2) == fin).all(), tag
    with np.errstate(invalid='ignore'):                   # inf - inf in the padded slots, which `fin` leaves out
        err = np.abs(d2.astype(np.float64) - ref)
    ratio = float((err[fin] / wide[fin]).max()) if fin.any() else 0.
    print(tag, 'values: worst |d2 - ref|', float(err[fin].max()) if fin.any() else 0., 'largest bar', float(np.nanmax(bars)), 'worst error / bar', ratio)
    assert ratio <= 1.
    assert (d2[good][:, 1:] >= d2[good][:, :-1]).all()                                  # ascending (+inf at the end)
    assert ((idx >= 0) & (idx < M))[fin].all() and (idx[~fin] == -1).all()
    assert all(len(set(r[r >= 0].tolist())) == int((r >= 0).sum()) for r in idx)        # distinct within a row
    named = np.take_along_axis(key, np.clip(idx, 0, max(M - 1, 0)).astype(np.int64), 1) if M else np.full(ref.shape, np.inf)
    with np.errstate(invalid='ignore'):
        off = np.abs(named - ref)
    r2 = float((off[fin] / wide[fin]).max()) if fin.any() else 0.
    print(tag, 'rows named: worst |D[idx] - ref| / bar', r2, '(held to 2)')
    assert r2 <= 2.
    assert (d2[good[:, None] & ~fin] == np.inf).all()                                   # beyond the bank's rows: +inf (and -1 above)
    assert np.isnan(d2[bad_q]).all() and (idx[bad_q] == -1).all()
    return ratio


def check_kernel_case(q, bank, k, normalized, tag, status=0):
    D = knn_distances(q, bank, normalized)
    bad_q = ~np.isfinite(q).all(1)
    bars = row_bars(q, bank, normalized)
    first = run(q, bank, k, normalized, 1)
    assert first[2] == status, (tag, first[2])
    check_against(D, bad_q, bars, k, first, tag)
    assert same_bits(first, run(q, bank, k, normalized, 1)), tag                       # run to run
    for splits in (2, 5):
        assert same_bits(first, run(q, bank, k, normalized, splits)), (tag, splits)
    return first


@pytest.mark.parametrize('normalized', MODES)
@pytest.mark.parametrize('K,N,M,k', SHAPES)
def test_kernel_shapes(K, N, M, k, normalized):
    q, bank = knn_case(K, N, M)
    d2, idx, _ = check_kernel_case(q, bank, k, normalized, ((K, N, M, k), 'normalized' if normalized else 'plain'))
    if M < k:
        assert np.isinf(d2[:, M:]).all() and (idx[:, M:] == -1).all() and np.isfinite(d2[:, :M]).all()


@pytest.mark.parametrize('normalized', MODES)
def test_copied_rows_are_clamped_at_zero(normalized):
    K, N, M, k = VARIANT_SHAPE
    q, bank = knn_case(K, N, M, 'copies')
    d2, idx, _ = check_kernel_case(q, bank, k, normalized, ('copies', normalized))
    bars = row_bars(q, bank, normalized)
    for b, i in COPIES:
        print('copy of query row', i, 'at bank row', b, 'd2', float(d2[i, 0]), 'bar', float(bars[i]))
        assert idx[i, 0] == b and 0. <= d2[i, 0] <= bars[i]
    assert (d2 >= 0).all()


@pytest.mark.parametrize('normalized', MODES)
def test_duplicated_rows_share_bits_and_are_adjacent(normalized):
    K, N, M, k = VARIANT_SHAPE
    q, bank = knn_case(K, N, M, 'duplicates')
    d2, idx, _ = check_kernel_case(q, bank, k, normalized, ('duplicates', normalized))
    bits = d2.view(np.int32)
    pairs = cut = 0
    for i in range(N):
        pos = {int(b): j for j, b in enumerate(idx[i])}
        for b, j in pos.items():
            if b < 200:
                twin = b + M - 200
                if twin in pos:                           # equal bits, the lower row first; between them only rows at the same bits
                    j2 = pos[twin]
                    assert j2 > j and (bits[i, j:j2 + 1] == bits[i, j]).all() and (np.diff(idx[i, j:j2 + 1]) > 0).all()
                    pairs += 1
                else:                                     # the list ended between them
                    assert bits[i, k - 1] == bits[i, j]
                    cut += 1
            elif b >= M - 200:
                assert b - (M - 200) in pos
    print('duplicates', normalized, 'pairs met', pairs, 'cut by the end of the list', cut)
    assert pairs > 0


@pytest.mark.parametrize('normalized', MODES)
def test_offset_rows_cancel_inside_the_bar(normalized):
    K, N, M, k = VARIANT_SHAPE
    q, bank = knn_case(K, N, M, 'offset')
    check_kernel_case(q, bank, k, normalized, ('offset', normalized))


@pytest.mark.parametrize('normalized', MODES)
def test_non_finite_rows(normalized):
    from jvae_hip import ops
    K, N, M, k = VARIANT_SHAPE
    q, bank = knn_case(K, N, M, 'nan')
    d2, idx, status = check_kernel_case(q, bank, k, normalized, ('nan', normalized),
                                        status=ops.KNN_STATUS_BANK | ops.KNN_STATUS_QUERY)
    assert np.isnan(d2[NAN_QUERY_ROW]).all() and (idx[NAN_QUERY_ROW] == -1).all()
    assert not (idx == NAN_BANK_ROW).any() and np.isfinite(np.delete(d2, NAN_QUERY_ROW, 0)).all()
    word = torch.tensor([status], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='non-finite'):
        ops.knn_check_status(word)
    assert int(word) == 0                                 # read and cleared
    ops.knn_check_status(word)
    # an infinity behaves as a NaN does; a clean call leaves the word alone
    q2, bank2 = knn_case(K, 5, 300)
    bank2[7, 0] = np.inf
    got = run(q2, bank2, 4, normalized, 1)
    assert got[2] == ops.KNN_STATUS_BANK and not (got[1] == 7).any() and np.isfinite(got[0]).all()
    q2[3, 1] = -np.inf
    bank2[7, 0] = 0.
    got = run(q2, bank2, 4, normalized, 2)
    assert got[2] == ops.KNN_STATUS_QUERY and np.isnan(got[0][3]).all() and np.isfinite(np.delete(got[0], 3, 0)).all()


def test_workload_size():
    """K = 64, N = 512, M = 50 000, k = 50, normalised, the library's own choice of partitions."""
    K, N, M, k = 64, 512, 50000, 50
    q, bank = knn_case(K, N, M, seed=7)
    unit = lambda x: x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)
    D = np.maximum(2. - 2. * (unit(q.astype(np.float64)) @ unit(bank.astype(np.float64)).T), 0.)
    first = run(q, bank, k, True, 0)
    assert first[2] == 0
    check_against(D, np.zeros(N, bool), np.full(N, normalized_bar(K)), k, first, 'workload size')
    assert same_bits(first, run(q, bank, k, True, 0)) and same_bits(first, run(q, bank, k, True, 3))


def test_arguments():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    q, bank = (torch.from_numpy(t).to(DEV) for t in knn_case(8, 4, 20))
    b, sq = ops.knn_bank(bank)
    assert b.data_ptr() == bank.data_ptr() and sq.shape == (20,) and sq.dtype == torch.float32
    assert torch.equal(ops.knn_bank(bank.double())[1], sq)                              # widened / narrowed to the same fp32 rows
    print('norms against fp64', float((sq.double() - (bank.double() ** 2).sum(1)).abs().max()), 'bar', 8 * U * float(sq.max()))
    assert float((sq.double() - (bank.double() ** 2).sum(1)).abs().max()) <= 8 * U * float(sq.max())
    d2, idx = ops.knn(q[:0], b, sq, 3)
    assert d2.shape == idx.shape == (0, 3)                                              # N = 0: empties, nothing launched
    t = ops.knn(q.t().contiguous().t(), b, sq, 3, splits=1)                            # a strided q is made contiguous
    assert all(torch.equal(x, y) for x, y in zip(t, ops.knn(q, b, sq, 3, splits=1)))
    for bad in (lambda: ops.knn(q, b, sq, 0), lambda: ops.knn(q, b, sq, 65), lambda: ops.knn(q, b, sq[:5], 3),
                lambda: ops.knn(q[:, :4], b, sq, 3), lambda: ops.knn(q, b, sq, 3, splits=1025), lambda: ops.knn(q.double(), b, sq, 3),
                lambda: ops.knn(q, b, sq, 3, status=torch.zeros(1, device=DEV))):
        with pytest.raises(JvaeHipError):
            bad()
    ops.knn_check_status()                                                              # the default word: clean


# ------------------------------------------------------------------------------------------- the model
def build():
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(regret_cases()['rm2_n6_cvae_mlp'][0]))
    load_det_state(net, seed=0)
    net.to(DEV)
    net.eval()
    return net


def synth(n, name, seed, shift=0.):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset((torch.rand(n, 1, 28, 28, generator=g) + shift).clamp(0, 1), torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


_MODEL = {}


def fitted():
    """One model with its bank over a 96-image set, shared by the tests that read it (the bank is never modified)."""
    if not _MODEL:
        net, train = build(), synth(96, 'train', 5)
        _MODEL.update(net=net, train=train, bank=net.fit_latent_bank(train, batch_size=40))
    return _MODEL['net'], _MODEL['train'], _MODEL['bank']


def stacked_posterior(net, dset, batch_size):
    x = dset.tensors[0]
    return torch.cat([net.latent_posterior(x[i:i + batch_size].to(DEV))[0] for i in range(0, len(x), batch_size)])


def test_fit_latent_bank():
    from jvae_hip import ops
    net, train, bank = fitted()
    want = stacked_posterior(net, train, 40)
    assert bank is net.latent_bank and bank['set'] == 'train' and bank['bank'].dtype == torch.float32
    assert torch.equal(bank['bank'], want) and torch.equal(bank['labels'].cpu(), train.tensors[1])
    assert torch.equal(bank['sq'], ops.knn_bank(want)[1]) and not net.training
    other = build()
    half = other.fit_latent_bank(train, batch_size=40, ratio=0.5, seed=3)
    keep = torch.randperm(96, generator=torch.Generator().manual_seed(3))[:48].sort()[0]
    assert torch.equal(half['bank'], want[keep.to(DEV)]) and torch.equal(half['labels'].cpu(), train.tensors[1][keep])
    assert not torch.equal(other.fit_latent_bank(train, batch_size=40, ratio=0.5, seed=4)['bank'], half['bank'])
    other.train()
    assert torch.equal(other.fit_latent_bank(train, batch_size=40)['bank'], want)       # evaluation mode inside, whatever the flag
    assert other.training                                                               # the mode is put back
    other.eval()
    coded = type(net)(**dict(get_case('j2_n8_jvae')['net']))
    with pytest.raises(NotImplementedError, match='coded'):
        coded.fit_latent_bank(train)


@pytest.mark.parametrize('normalized', MODES)
def test_knn_scores_against_the_restatement(normalized):
    net, train, bank = fitted()
    net.KNN_NORMALIZE = normalized
    try:
        mu = net.latent_posterior(synth(37, 'q', 9).tensors[0].to(DEV))[0]
        scores = net.knn_scores(mu)
    finally:
        del net.KNN_NORMALIZE
    assert list(scores) == ['knn-1', 'knn-10', 'knn-50']
    q, b = mu.cpu().numpy(), bank['bank'].cpu().numpy()
    ref, _ = knn_restatement(q, b, 50, normalized)
    bars = row_bars(q, b, normalized)
    for name, k in (('knn-1', 1), ('knn-10', 10), ('knn-50', 50)):
        got = scores[name]
        assert got.shape == (37,) and got.dtype == torch.float32 and got.is_cuda
        root = np.sqrt(ref[:, k - 1])
        tol = np.minimum(np.sqrt(bars), bars / np.maximum(root, 1e-300)) + 2 * U * root
        d = np.abs(got.cpu().numpy().astype(np.float64) + root)
        print(name, 'normalized' if normalized else 'plain', 'worst |score + sqrt(ref)|', float(d.max()), 'worst distance / bar',
              float((d / tol).max()))
        assert (d <= tol).all()


def test_knn_scores_refusals():
    net = build()
    mu = torch.zeros(4, 16, device=DEV)
    with pytest.raises(ValueError, match='bank'):
        net.knn_scores(mu)
    net.fit_latent_bank(synth(20, 'few', 1), batch_size=20)
    with pytest.raises(ValueError, match='20 rows'):
        net.knn_scores(mu)
    net.KNN_K = (1, 20)
    assert list(net.knn_scores(mu)) == ['knn-1', 'knn-20']


def test_rates(monkeypatch):
    net, train, bank = fitted()
    names = ['knn-1', 'knn-10']
    sets = [synth(40, 'ind', 1), synth(40, 'ood', 2, .3)]
    call = dict(oodsets=sets[1:], testset=sets[0], batch_size=16, update_self_ood=False)
    with pytest.raises(NotImplementedError, match='OOD_KNN_METHODS'):                  # off: the same call raises
        net.ood_detection_rates(method=['elbo'] + names, **call)
    torch.manual_seed(11)
    plain = net.ood_detection_rates(method=['elbo'], **call)
    net.OOD_KNN_METHODS = True
    try:
        torch.manual_seed(11)
        bare = net.ood_detection_rates(method=['elbo'] + names, **call)
        assert bare['ood']['elbo'] == plain['ood']['elbo']                              # the other rows: the same bits
        recorders = {}                                                                  # (a recorder seeds the noise by itself)
        first = net.ood_detection_rates(method=['elbo'] + names, recorders=recorders, **call)
        assert list(first['ood']) == ['elbo'] + names and all(first['ood'][m] == bare['ood'][m] for m in names)
        for s in sets:
            mu = stacked_posterior(net, s, 16)
            want = {}
            for i in range(0, 40, 16):                                                  # the batches of the pass
                for m, v in net.knn_scores(mu[i:i + 16]).items():
                    want.setdefault(m, []).append(v)
            for m in names + ['knn-50']:                                                # one call fills every k of KNN_K
                assert torch.equal(recorders[s.name][m].to(DEV), torch.cat(want[m])), (s.name, m)
        for m in names:
            ins, outs = (recorders[s][m].float().cpu().numpy() for s in ('ind', 'ood'))
            r = first['ood'][m]
            auc, fpr, tpr, low, up = roc_restatement(ins, outs, KEPT)
            print(m, 'auc', r['auc'], 'restated', auc, 'mean distance in / out', -ins.mean(), -outs.mean())
            assert r['n'] == 40 and r['fpr'] == fpr.tolist() and abs(r['auc'] - auc) <= auc_bound(40)
        assert not any(k.startswith('knn') for k in net.test_losses)                    # test_losses: the loss components only
        calls = []
        real_eval, real_knn = net.evaluate, net.knn_scores
        monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append('e') or real_eval(*a, **k))
        monkeypatch.setattr(net, 'knn_scores', lambda *a, **k: calls.append('k') or real_knn(*a, **k))
        again = net.ood_detection_rates(method=['elbo'] + names, recorders=recorders, **call)
        assert not calls and again == first                                             # a full recorder is read back
        one = net.ood_detection_rates(method='knn-10', **call)
        assert list(one['ood']) == ['knn-10'] and one['ood']['knn-10'] == first['ood']['knn-10']
        assert calls.count('e') == 6 and calls.count('k') == 6                          # one pass and one knn call per batch
    finally:
        del net.OOD_KNN_METHODS


def test_two_families_in_one_pass(monkeypatch):
    """`regret*` and `knn*` together: each family's rows are those of a pass with that family alone, the per-batch calls run in
    the order evaluate, regret_scores, knn_scores, and a full recorder is read back without any of them."""
    net, train, bank = fitted()
    sets = [synth(40, 'ind', 1), synth(40, 'ood', 2, .3)]
    call = dict(oodsets=sets[1:], testset=sets[0], batch_size=16, update_self_ood=False)
    net.KNN_K, net.REGRET_PARAMS, net.OOD_KNN_METHODS, net.OOD_REGRET_METHODS = (1, 3), [(2, 0.05)], True, True
    try:
        knn, regret = net._knn_names(), net._regret_names()
        assert knn == ['knn-1', 'knn-3'] and regret == ['regret-2-0.0500']
        def rates(method, recorders):
            np.random.seed(28)                     # a new recorder takes its seed, and with it the noise of its pass, from numpy
            return net.ood_detection_rates(method=method, recorders=recorders, **call)
        alone = {m: rates(['elbo', m], {}) for m in ('knn*', 'regret*')}
        calls = []
        for name in ('evaluate', 'regret_scores', 'knn_scores'):
            real = getattr(net, name)
            monkeypatch.setattr(net, name, lambda *a, _real=real, _tag=name[0], **k: calls.append(_tag) or _real(*a, **k))
        recorders = {}
        both = rates(['elbo', 'regret*', 'knn*'], recorders)
        assert list(both['ood']) == ['elbo'] + regret + knn
        for m in knn:
            assert both['ood'][m] == alone['knn*']['ood'][m], m
        for m in regret:
            assert both['ood'][m] == alone['regret*']['ood'][m], m
        print('calls of the pass', ''.join(calls))
        assert calls == ['e', 'r', 'k'] * 6                                             # 3 batches of 2 sets, once each, in order
        assert all(m in recorders[s.name].keys() for s in sets for m in regret + knn)
        assert net.test_losses and not any(k.startswith(('knn', 'regret')) for k in net.test_losses)
        del calls[:]
        again = net.ood_detection_rates(method=['elbo', 'regret*', 'knn*'], recorders=recorders, **call)
        assert not calls and again == both                                              # full recorders: nothing is evaluated
    finally:
        del net.KNN_K, net.REGRET_PARAMS, net.OOD_KNN_METHODS, net.OOD_REGRET_METHODS


def test_bank_file_round_trip(tmp_path):
    net, train, bank = fitted()
    path = net.save_latent_bank(str(tmp_path))
    assert path == str(tmp_path / 'latent-bank.pth')
    other = build()
    got = other.load_latent_bank(str(tmp_path))
    assert got['set'] == 'train' and all(torch.equal(got[k], bank[k]) and got[k].device == bank[k].device for k in ('bank', 'sq', 'labels'))
    mu = net.latent_posterior(synth(9, 'q', 2).tensors[0].to(DEV))[0]
    a, b = net.knn_scores(mu), other.knn_scores(mu)
    assert all(torch.equal(a[m], b[m]) for m in a)
