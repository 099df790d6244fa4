"""Density-of-states OOD scores on the MI355X (ops.kde_fit / kde_logdensity, csrc/dose.hip, cvae.fit_score_bank / dose_scores;
DESIGN.md section 7s) against the fp64 restatement and the tolerance of tests/test_dose_restatement.py.

Inputs are fp32 values and the reference is computed in fp64 from those same values.  Fit: the centre within M 2^-52 mean |b|, the
deviation, the bandwidths and the normalisers within (M + 8) 2^-52 of their size (an fp64 sum of M terms in a fixed order, a
square root, a logarithm), z within its one fp32 rounding and what the centre's error adds.  Scores: |error| <= c 2^-24 (1 +
|ref|) with the c DERIVED for the case by test_dose_restatement.dose_c (asserted <= 64 on every case, the model's too), `dose`
within the sum of its marginals' tolerances AND within 64 x 2^-24 (1 + |dose|), the typicality rows within 2 x 2^-24 (1 +
|ref|); every output finite for finite input - an unshifted fp32 sum gives -inf on the far queries.  Every figure is printed before its assertion.

Derived / measured c on the MI355X, per shape (S, M, N): (1, 2, 1) 4.3 / 0.34, (1, 2, 3) 5.7 / 0.62, (5, 63, 1) 10.6 / 1.78,
(5, 64, 64) 14.5 / 3.80, (5, 65, 65) 28.4 / 5.87, (3, 257, 129) 13.0 / 4.18, (8, 4096, 257) 60.7 / 8.40, (5, 1023, 5) 13.6 / 3.07,
(5, 1024, 5) 13.3 / 3.61, (5, 1025, 5) 14.3 / 3.95, (5, 2051, 5) 37.7 / 6.24; the cvae's statistics 32.3 / 4.77, the vib's 55.4 /
5.65; `dose` over 2^-24 (1 + |dose|) at most 3.62 on the kernel shapes, 9.40 on the vib's statistics."""
import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_dose_restatement import C_LIMIT, SHAPES, U, dose_c, dose_case, dose_restatement, fit_restatement, tolerance

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2. ** -52
P = 1024                                               # ops.kde_partition(), asserted below
PIECE_SHAPES = [(5, P - 1, 5), (5, P, 5), (5, P + 1, 5), (5, 2 * P + 3, 5)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def run(stats, fit):
    """-> (scores (2 S + 2, N) on the device, status) from a status word of the call's own."""
    from jvae_hip import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.kde_logdensity(stats if torch.is_tensor(stats) else dev(stats), fit, status=status)
    assert out.dtype == torch.float32 and out.shape == (2 * fit['S'] + 2, stats.shape[1]) and out.is_cuda
    return out, int(status)


def check_fit(fit, bank, bandwidth, tag):
    from jvae_hip import ops
    S, M = bank.shape
    want = fit_restatement(bank, bandwidth)
    assert ops.kde_check_fit(fit) == (S, M) and fit['bandwidth'] == bandwidth and fit['z'].is_cuda
    got = {k: fit[k].cpu().numpy() for k in ('centre', 'sigma', 'h1', 'hS', 'lognorm', 'z')}
    scale = np.abs(bank.astype(np.float64)).mean(1)
    ratios = {'centre': np.abs(got['centre'] - want['centre']) / (M * EPS * scale)}
    for k in ('sigma', 'h1', 'hS'):
        ratios[k] = np.abs(got[k] - want[k]) / ((M + 8) * EPS * want[k])
    ratios['lognorm'] = np.abs(got['lognorm'] - want['lognorm']) / ((M + 8) * S * EPS * (1 + np.abs(want['lognorm'])))
    z = (bank.astype(np.float64) - want['centre'][:, None]) / want['h1'][:, None]
    ratios['z'] = np.abs(got['z'] - z) / (U * np.abs(z) + (M + 8) * EPS * (np.abs(z) + (scale / want['h1'])[:, None]))
    worst = {k: float(v.max()) for k, v in ratios.items()}
    print(tag, 'fit: worst error / bar', worst)
    assert all(v <= 1. for v in worst.values()), (tag, worst)


def check_scores(got, stats, bank, bandwidth, tag):
    ref = dose_restatement(stats, bank, bandwidth)
    c = dose_c(stats, bank, bandwidth, P)
    S = bank.shape[0]
    err = np.abs(got.astype(np.float64) - ref)
    rows = list(range(S)) + [S + 1]
    measured = float((err[rows] / (U * (1 + np.abs(ref[rows])))).max())
    print(tag, f'derived c {c:.1f} measured c {measured:.2f}  dose: measured c {float((err[S] / (U * (1 + np.abs(ref[S])))).max()):.2f},'
          f' error / tolerance {float((err[S] / tolerance(ref, c)[S]).max()):.3f}'
          f'  typicality: {float((err[S + 2:] / (U * (1 + np.abs(ref[S + 2:])))).max()):.2f} u')
    assert np.isfinite(got).all(), tag                  # an unshifted sum fails here
    assert c <= C_LIMIT, (tag, c)
    assert (err <= tolerance(ref, c)).all(), (tag, measured, c)
    return c, measured


_FITS = {}


def fitted(shape, bandwidth=1.0):
    from jvae_hip import ops
    if (shape, bandwidth) not in _FITS:
        stats, bank = dose_case(*shape)
        _FITS[shape, bandwidth] = (stats, bank, ops.kde_fit(dev(bank), bandwidth))
    return _FITS[shape, bandwidth]


@pytest.mark.parametrize('shape', SHAPES + PIECE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_against_the_restatement(shape):
    from jvae_hip import ops
    assert ops.kde_partition() == P
    stats, bank, fit = fitted(shape)
    check_fit(fit, bank, 1.0, f'shape {shape}')
    got, status = run(stats, fit)
    assert status == 0
    check_scores(got.cpu().numpy(), stats, bank, 1.0, f'shape {shape}')


def test_a_bandwidth_factor():
    stats, bank, fit = fitted((3, 257, 129), 0.4)
    check_fit(fit, bank, 0.4, 'bandwidth 0.4')
    check_scores(run(stats, fit)[0].cpu().numpy(), stats, bank, 0.4, 'bandwidth 0.4')


def test_a_bank_row_with_all_values_equal_but_one():
    from jvae_hip import ops
    stats, bank = dose_case(3, 70, 9)
    bank, stats = bank.copy(), stats.copy()
    bank[1] = 30.
    bank[1, 17] = 33.
    stats[1, :4] = (30., 33., 30.5, 27.)
    fit = ops.kde_fit(dev(bank))
    check_fit(fit, bank, 1.0, 'one value off')
    check_scores(run(stats, fit)[0].cpu().numpy(), stats, bank, 1.0, 'one value off')


def test_bits_do_not_depend_on_the_batch_or_the_run():
    stats, bank, fit = fitted((5, 2 * P + 3, 100))
    whole, status = run(stats, fit)
    assert status == 0 and same_bits(run(stats, fit)[0], whole)                         # two runs
    s = dev(stats)
    singly = torch.cat([run(s[:, i:i + 1].contiguous(), fit)[0] for i in range(100)], 1)
    sliced = torch.cat([run(s[:, i:i + 7].contiguous(), fit)[0] for i in range(0, 100, 7)], 1)
    assert same_bits(singly, whole) and same_bits(sliced, whole)
    twice = np.concatenate([stats[:, 3:70], stats[:, 3:70][:, ::-1]], 1)                # duplicate queries, other lanes and workgroups
    got = run(twice, fit)[0]
    assert same_bits(got[:, :67], whole[:, 3:70].contiguous()) and same_bits(got[:, 67:].flip(1).contiguous(), got[:, :67].contiguous())


def test_non_finite_queries():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    stats, bank, fit = fitted((5, 65, 65))
    clean = run(stats, fit)[0]
    bad = stats.copy()
    bad[1, 7], bad[3, 40], bad[0, 64], bad[2, 64] = np.inf, -np.inf, np.nan, np.inf
    got, status = run(bad, fit)
    assert status == ops.DOSE_STATUS_QUERY
    S = 5
    for col, s in ((7, 1), (40, 3)):                   # +-inf: -inf in the rows that read it, the others as they were
        reads = [s, S, S + 1, S + 2 + s]
        assert bool((got[reads, col] == -np.inf).all())
        others = [r for r in range(2 * S + 2) if r not in reads]
        assert same_bits(got[others, col], clean[others, col])
    reads = [0, S, S + 1, S + 2]                       # NaN (and an inf beside it: NaN wins where both are read)
    assert bool(torch.isnan(got[reads, 64]).all()) and bool((got[[2, S + 4], 64] == -np.inf).all())
    others = [1, 3, 4, S + 3, S + 5, S + 6]
    assert same_bits(got[others, 64], clean[others, 64])
    keep = [c for c in range(65) if c not in (7, 40, 64)]
    assert same_bits(got[:, keep], clean[:, keep])     # other columns are untouched
    word = torch.full((1,), ops.DOSE_STATUS_QUERY, dtype=torch.int32, device=DEV)
    with pytest.raises(JvaeHipError, match='non-finite'):
        ops.kde_check_status(word)
    assert int(word) == 0                              # read and cleared
    ops.kde_check_status(word)
    ops.kde_logdensity(dev(bad), fit)                  # the default word of the device
    with pytest.raises(JvaeHipError, match='non-finite'):
        ops.kde_check_status()
    ops.kde_check_status()


def test_a_finite_query_whose_square_overflows():
    """|t - z| above 2^63: no fp32 sum exists.  The rows that read the statistic get -inf and the status bit, as for an infinite
    one, instead of a silent NaN; where only the SUM of the squares overflows, the joint row alone."""
    from jvae_hip import ops
    stats, bank, fit = fitted((5, 65, 65))
    clean = run(stats, fit)[0]
    far = stats.copy()
    far[1, 9] = 1e30                                   # t = 1e30 / h: finite in fp32, its square is not
    f = fit_restatement(bank)
    far[:3, 33] = (f['centre'][:3] + 1.2e19 * f['h1'][:3]).astype(np.float32)          # three squares of 1.4e38: finite, their sum is not
    ref = dose_restatement(far, bank)
    assert np.isfinite(ref).all()
    got, status = run(far, fit)
    assert status == ops.DOSE_STATUS_QUERY and not bool(torch.isnan(got).any())
    assert bool((got[[1, 5, 6], 9] == -np.inf).all()) and bool(torch.isfinite(got[7 + 1, 9]))
    others = [0, 2, 3, 4, 7, 9, 10, 11]
    assert same_bits(got[others, 9], clean[others, 9])
    keep = [c for c in range(65) if c not in (9, 33)]
    assert same_bits(got[:, keep], clean[:, keep])
    # only the SUM of the squares overflows: the marginals, `dose` and the typicality rows hold, the joint row alone gives way
    rows = [r for r in range(12) if r != 6]
    assert float(got[6, 33]) == -np.inf and bool(torch.isfinite(got[rows, 33]).all())
    read = [0, 1, 2, 5, 7, 8, 9]                       # the rows that read a far statistic: the roundings of t, d^2, k (twice), the result
    err = np.abs(got[read, 33].cpu().numpy().astype(np.float64) - ref[read, 33])
    print('far query: error / (u |ref|)', (err / (U * np.abs(ref[read, 33]))).max())
    assert (err <= 8 * U * (1 + np.abs(ref[read, 33]))).all()
    assert same_bits(got[[3, 4, 10, 11], 33], clean[[3, 4, 10, 11], 33])


def test_no_queries():
    stats, bank, fit = fitted((5, 64, 64))
    got, status = run(np.zeros((5, 0), dtype=np.float32), fit)
    assert got.shape == (12, 0) and status == 0


def test_fit_refusals_and_bits():
    from jvae_hip import ops
    _, bank = dose_case(3, 5000, 1)                    # two slabs of the moment sums
    check_fit(ops.kde_fit(dev(bank)), bank, 1.0, 'two slabs')
    a, b = ops.kde_fit(dev(bank)), ops.kde_fit(dev(bank))
    assert all(same_bits(a[k], b[k]) if k == 'z' else torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    flat = bank.copy()
    flat[1] = 30.
    with pytest.raises(ValueError, match='row 1 .* no spread'):
        ops.kde_fit(dev(flat))
    for v in (np.inf, np.nan):
        broken = bank.copy()
        broken[2, 4999] = v
        with pytest.raises(ValueError, match='row 2 .* non-finite'):
            ops.kde_fit(dev(broken))
    with pytest.raises(ValueError, match='two samples'):
        ops.kde_fit(dev(bank[:, :1]))
    with pytest.raises(ops.L.JvaeHipError, match='unsupported configuration'):
        ops.kde_fit(torch.zeros(9, 10, device=DEV))


# ------------------------------------------------------------------------------------------------------------- the model
def synth(n, name, seed, shape=(1, 28, 28), shift=0.):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset((torch.rand(n, *shape, generator=g) + shift).clamp(0, 1), torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


def build(case='c1_n16_mlp'):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case(case)['net']))
    load_det_state(net, seed=0)
    net.to(DEV)
    net.eval()
    return net


def stacked_rows(net, dset, batch_size, seed):
    """The DOSE_STATS rows of a label-free pass by the plain batch_dist_measures call, stacked (S, n)."""
    torch.manual_seed(seed)
    rows, measures = [], None
    with torch.no_grad():
        for i in range(0, len(dset), batch_size):
            x = dset.tensors[0][i:i + batch_size].to(DEV)
            _, logits, losses, measures = net.evaluate(x, batch=i // batch_size, current_measures=measures)
            got = net.batch_dist_measures(logits, losses, list(net.DOSE_STATS))
            rows.append(torch.stack([got[m].float() for m in net.DOSE_STATS]))
    return torch.cat(rows, 1)


_MODEL = {}


def model():
    """One cvae with its score bank over a 96-image set, shared by the tests that read it (the bank is never modified)."""
    if not _MODEL:
        net, train = build(), synth(96, 'train', 5)
        torch.manual_seed(3)
        _MODEL.update(net=net, train=train, bank=net.fit_score_bank(train, batch_size=40))
    return _MODEL['net'], _MODEL['train'], _MODEL['bank']


def equal_fits(a, b):
    return all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype if torch.is_tensor(b[k]) else a[k] == b[k] for k in b)


def test_fit_score_bank():
    from jvae_hip import ops
    net, train, bank = model()
    rows = stacked_rows(net, train, 40, 3)
    assert bank is net.score_bank and bank['set'] == 'train' and bank['stats'] == net.DOSE_STATS == ('elbo', 'iws', 'kl', 'zdist', 'mse')
    assert (bank['S'], bank['M'], bank['bandwidth']) == (5, 96, 1.0) and not net.training
    assert equal_fits(bank, ops.kde_fit(rows))                                          # the rows of the same pass, bit for bit
    check_fit(bank, rows.cpu().numpy(), 1.0, 'model')
    other = build()
    other.DOSE_BANDWIDTH = 0.5
    torch.manual_seed(3)
    half = other.fit_score_bank(train, batch_size=40, ratio=0.5, seed=3)
    keep = torch.randperm(96, generator=torch.Generator().manual_seed(3))[:48].sort()[0]
    assert half['M'] == 48 and equal_fits(half, ops.kde_fit(rows[:, keep.to(DEV)].contiguous(), 0.5))      # the columns of the full pass
    torch.manual_seed(3)
    assert not torch.equal(other.fit_score_bank(train, batch_size=40, ratio=0.5, seed=4)['z'], half['z'])
    # a ratio so small that most batches keep no sample: they are evaluated all the same, the latent noise stays that of a full pass
    rows8 = stacked_rows(net, train, 8, 3)
    torch.manual_seed(3)
    few = other.fit_score_bank(train, batch_size=8, ratio=0.05, seed=6)
    keep = torch.randperm(96, generator=torch.Generator().manual_seed(6))[:5].sort()[0]
    assert len({int(k) // 8 for k in keep}) < 12 and few['M'] == 5
    assert equal_fits(few, ops.kde_fit(rows8[:, keep.to(DEV)].contiguous(), 0.5))
    other.train()
    other.DOSE_BANDWIDTH = 1.0
    torch.manual_seed(3)
    assert equal_fits(other.fit_score_bank(train, batch_size=40), bank) and other.training       # evaluation mode inside; put back
    other.eval()
    other.DOSE_STATS = ('kl', 'soft-2')
    with pytest.raises(ValueError, match='DOSE_STATS'):
        other.fit_score_bank(train)
    coded = type(net)(**dict(get_case('j2_n8_jvae')['net']))
    with pytest.raises(NotImplementedError, match='coded'):
        coded.fit_score_bank(synth(8, 'c', 1, (3, 32, 32)))


def test_dose_scores_against_the_restatement():
    net, train, bank = model()
    queries = synth(64, 'q', 9, shift=.2)
    rows = stacked_rows(net, queries, 64, 21)
    torch.manual_seed(21)
    with torch.no_grad():
        _, logits, losses, _ = net.evaluate(queries.tensors[0].to(DEV), batch=0, current_measures=None)
        scores = net.dose_scores(logits, losses)
    assert list(scores) == net._dose_names() and len(scores) == 12
    assert all(v.shape == (64,) and v.dtype == torch.float32 and v.is_cuda for v in scores.values())
    order = ['dose-' + s for s in net.DOSE_STATS] + ['dose', 'dose-joint'] + ['dose-typ-' + s for s in net.DOSE_STATS]
    got = torch.stack([scores[m] for m in order]).cpu().numpy()
    check_scores(got, rows.cpu().numpy(), stacked_rows(net, train, 40, 3).cpu().numpy(), 1.0, 'model')
    bare = build()
    with pytest.raises(ValueError, match='fit_score_bank'):
        bare.dose_scores(logits, losses)
    bare.OOD_DOSE_METHODS = True
    with pytest.raises(ValueError, match='fit_score_bank'):                             # no bank: the pass says so
        bare.ood_detection_rates(oodsets=[queries], testset=train, batch_size=32, method='dose', update_self_ood=False)


def test_score_bank_file_round_trip(tmp_path):
    net, train, bank = model()
    path = net.save_score_bank(str(tmp_path))
    assert path == str(tmp_path / 'score-bank.pth')
    other = build()
    got = other.load_score_bank(str(tmp_path))
    assert got['set'] == 'train' and set(got) == set(bank) and equal_fits(got, bank)
    assert all(got[k].device == bank[k].device for k in bank if torch.is_tensor(bank[k]))
    torch.manual_seed(2)
    with torch.no_grad():
        _, logits, losses, _ = net.evaluate(synth(9, 'q', 2).tensors[0].to(DEV))
        a, b = net.dose_scores(logits, losses), other.dose_scores(logits, losses)
    assert list(a) == list(b) and all(same_bits(a[m], b[m]) for m in a)


def vib_rows(net, dset, batch_size, seed):
    """A vib's statistics by hand: its `kl` and `zdist` have no class axis, the statistic is minus the loss; `logits`: the largest."""
    torch.manual_seed(seed)
    rows, measures = [], None
    with torch.no_grad():
        for i in range(0, len(dset), batch_size):
            x = dset.tensors[0][i:i + batch_size].to(DEV)
            _, logits, losses, measures = net.evaluate(x, batch=i // batch_size, current_measures=measures)
            assert losses['kl'].shape == losses['zdist'].shape == (x.shape[0],)
            rows.append(torch.stack([-losses['kl'], -losses['zdist'], logits.max(-1)[0]]).float())
    return torch.cat(rows, 1)


def test_the_vib_statistics():
    from jvae_hip import ops
    net = build('b2_n8_vib')
    train, queries = synth(64, 'train', 4, (3, 32, 32)), synth(64, 'q', 6, (3, 32, 32), .3)
    torch.manual_seed(1)
    bank = net.fit_score_bank(train, batch_size=32)
    assert bank['stats'] == ('kl', 'zdist', 'logits') and (bank['S'], bank['M']) == (3, 64)
    rows, bank_rows = vib_rows(net, queries, 64, 8), vib_rows(net, train, 32, 1)
    assert equal_fits(bank, ops.kde_fit(bank_rows))
    torch.manual_seed(8)
    with torch.no_grad():
        _, logits, losses, _ = net.evaluate(queries.tensors[0].to(DEV), batch=0, current_measures=None)
        scores = net.dose_scores(logits, losses)
    names = ['dose', 'dose-joint', 'dose-kl', 'dose-zdist', 'dose-logits', 'dose-typ-kl', 'dose-typ-zdist', 'dose-typ-logits']
    assert list(scores) == names
    order = names[2:5] + names[:2] + names[5:]
    check_scores(torch.stack([scores[m] for m in order]).cpu().numpy(), rows.cpu().numpy(), bank_rows.cpu().numpy(), 1.0, 'vib')


def test_rates(monkeypatch, tmp_path):
    from jvae_hip import ops
    from jvae_compat.recorders import LossRecorder
    from module import score_rows
    net, train, bank = model()
    names = net._dose_names()
    sets = [synth(64, 'ind', 1), synth(64, 'ood', 2, shift=.3)]
    call = dict(oodsets=sets[1:], testset=sets[0], batch_size=32, update_self_ood=False)

    def rates(**kw):
        torch.manual_seed(11)                          # the latent noise of a pass without a recorder
        np.random.seed(11)                             # ... and of a pass with one: a new recorder draws its seed here
        return net.ood_detection_rates(**kw, **call)
    for m in (['elbo'] + names, 'dose*', 'dose-typ-kl'):
        with pytest.raises(NotImplementedError, match='OOD_DOSE_METHODS'):              # off: the names raise
            net.ood_detection_rates(method=m, **call)
    plain = rates(method=['elbo'])
    off_rec = {}
    off_all = rates(method='all', recorders=off_rec, sample_dirs=[str(tmp_path / 'off')])
    monkeypatch.setattr(score_rows, 'FAMILIES', tuple(f for f in score_rows.FAMILIES if f.prefix != 'dose'))      # the table without the family
    was_rec = {}
    assert rates(method='all', recorders=was_rec) == off_all  # off: 'all' is bit for bit what it was
    monkeypatch.undo()
    assert not any(m.startswith('dose') for m in off_all['ood'])
    assert all(sorted(off_rec[s].keys()) == sorted(was_rec[s].keys()) and not any(k.startswith('dose') for k in off_rec[s].keys())
               for s in ('ind', 'ood'))
    saved = LossRecorder.load(str(tmp_path / 'off' / 'record-ood.pth'))
    assert sorted(saved.keys()) == sorted(was_rec['ood'].keys())                        # record-*.pth: the keys of today
    net.OOD_DOSE_METHODS = True
    try:
        bare = rates(method=['elbo', 'dose*'])
        assert list(bare['ood']) == ['elbo'] + names
        assert bare['ood']['elbo'] == plain['ood']['elbo']                              # the other rows: the same bits
        on_all = rates(method='all', recorders={})
        assert list(on_all['ood']) == list(off_all['ood']) + names and all(on_all['ood'][m] == off_all['ood'][m] for m in off_all['ood'])
        seen, calls = [], []
        real_eval, real_dose = net.evaluate, net.dose_scores
        monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append('e') or real_eval(*a, **k))
        monkeypatch.setattr(net, 'dose_scores', lambda *a, **k: calls.append('d') or seen.append(real_dose(*a, **k)) or seen[-1])
        recorders = {}
        first = rates(method=['elbo'] + names, recorders=recorders, sample_dirs=[str(tmp_path / 'on')])
        assert calls.count('e') == 4 and calls.count('d') == 4 and len(seen) == 4       # one pass and one dose call per batch
        assert list(first['ood']) == ['elbo'] + names and all(first['ood'][m] == on_all['ood'][m] for m in names)
        rows = {s: {m: torch.cat([b[m] for b in seen[2 * i:2 * i + 2]]) for m in names} for i, s in enumerate(('ind', 'ood'))}
        for s in ('ind', 'ood'):
            assert all(torch.equal(recorders[s][m].to(DEV), rows[s][m]) for m in names)         # recorded as computed
        saved = LossRecorder.load(str(tmp_path / 'on' / 'record-ood.pth'))
        assert set(names) <= set(saved.keys()) and torch.equal(saved['dose'].to(DEV), rows['ood']['dose'])
        roc = ops.roc_curve(torch.stack([rows['ind'][m] for m in names]), torch.stack([rows['ood'][m] for m in names]),
                            net.OOD_KEPT_TPR, False)
        roc = {k: v.cpu().numpy() for k, v in roc.items()}
        assert not roc['status'].any()
        for i, m in enumerate(names):
            r = first['ood'][m]
            print(m, 'auc', r['auc'], 'fpr@95', r['fpr'][5], 'mean score in / out', float(rows['ind'][m].mean()), float(rows['ood'][m].mean()))
            assert r['n'] == 64 and r['auc'] == float(roc['auc'][i]) and r['fpr'] == roc['fpr'][i].tolist()
        assert net.test_losses and not any(k.startswith('dose') for k in net.test_losses)       # test_losses: the loss components only
        del calls[:]
        again = rates(method=['elbo'] + names, recorders=recorders)
        assert not calls and again == first                                             # a full recorder is read back
        one = rates(method='dose-joint', recorders=recorders)
        assert not calls and list(one['ood']) == ['dose-joint'] and one['ood']['dose-joint'] == first['ood']['dose-joint']
        with pytest.raises(ValueError, match='density-of-states rows'):
            net.ood_detection_rates(method='dose-logits', **call)
        ops.kde_check_status()                                                          # nothing was flagged
    finally:
        del net.OOD_DOSE_METHODS
