"""The SSIM rows on the device: ops.ssim (csrc/ssim.hip) against the fp64 restatement of
tests/test_ssim_restatement.py within the derived bound c 2^-24 (1 + B^2 / C2) on every case, its exact and bitwise properties,
the non-finite rule, and the model: ssim_scores, ssim_map, and ood_detection_rates with the family on, off and read back.

Largest measured error / bound on an MI355X over the shapes below: 0.010, for maps and scores alike (every case prints its own)."""
import functools

import numpy as np
import pytest
import torch

from test_28_knn_gpu import build, synth
from test_roc_restatement import auc_bound, roc_restatement
from test_ssim_restatement import KINDS, batch, map_bound, score_bound, ssim_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ['ssim', 'ssim-mu', 'ssim-cs']
KEPT = [pc / 100 for pc in range(90, 100)]
# (N, R, C, H, W): one output pixel; a 2 x 3 map; the test model's image; the workload's; config 5's (several strips); N a
# multiple of nothing; C = 4, wide and short; then the kernel's own boundaries - one strip of 38 rows at W = 32 and the first
# shape with two; the widest staged row; the last width whose strip fits the smaller LDS budget and the first that takes the
# larger one; draws chunked by two (N R >= 2048) and by the most, 32
SHAPES = [(1, 1, 1, 11, 11), (2, 2, 1, 12, 13), (3, 3, 1, 28, 28), (5, 3, 3, 32, 32), (1, 2, 3, 64, 64), (67, 2, 3, 32, 32),
          (2, 9, 4, 17, 40), (1, 2, 1, 48, 32), (1, 2, 1, 49, 32), (1, 3, 1, 11, 128), (1, 2, 1, 30, 79), (1, 2, 1, 30, 80),
          (64, 33, 1, 11, 12), (128, 256, 1, 11, 11)]


@functools.lru_cache(maxsize=None)
def case(shape):
    """-> (x, y, the fp64 restatement); computed once per shape, shared and never modified."""
    x, y = batch(*shape, seed=len(SHAPES) - SHAPES.index(shape) if shape in SHAPES else 0)
    return x, y, ssim_batch(x, y)


def run(x, y, **kw):
    from jvae_hip import ops
    return ops.ssim(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(y)).to(DEV), **kw)


def same_bits(a, b):
    a, b = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_strips_are_where_the_shapes_assume():
    from jvae_hip import ops
    assert [ops.ssim_strip_rows(H, W) for H, W in ((48, 32), (49, 32), (64, 64), (30, 79), (30, 80), (11, 128))] == [38, 38, 12, 8, 16, 1]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_scores_and_maps_are_the_restatements(shape):
    from jvae_hip import ops
    x, y, want = case(shape)
    N, R, C, H, W = shape
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    s, cs, m = run(x, y, maps=True, status=status)
    assert s.shape == cs.shape == (R, N) and m.shape == (R, N, H - 10, W - 10) and s.dtype == cs.dtype == m.dtype == torch.float32
    assert int(status) == 0
    s, cs, m = s.cpu().numpy().astype(np.float64), cs.cpu().numpy().astype(np.float64), m.cpu().numpy().astype(np.float64)
    ratios = {'ssim': np.abs(s - want['ssim']) / score_bound(want['B']), 'cs': np.abs(cs - want['cs']) / score_bound(want['B']),
              'map': np.abs(m - want['map']).max((-2, -1)) / map_bound(want['B'])}
    print(shape, 'largest error / bound:', {k: float(v.max()) for k, v in ratios.items()}, 'largest B', float(want['B'].max()),
          'largest map error in units of 2^-24:', float(np.abs(m - want['map']).max() * 2 ** 24))
    for k, v in ratios.items():
        assert np.isfinite(v).all() and v.max() <= 1., (k, float(v.max()))
    if R > 1:                                                  # draw 1 is x itself
        assert (s[1] == 1.).all() and (cs[1] == 1.).all() and (m[1] == 1.).all()
        assert (s[0] < 1.).all()
    # without the maps: the same bits; a second run: the same bits
    s2, cs2 = run(x, y, status=status)
    s3, cs3, m3 = run(x, y, maps=True, status=status)
    assert same_bits(s2.cpu().numpy().astype(np.float64), s) and same_bits(cs2.cpu().numpy().astype(np.float64), cs)
    assert same_bits(s3, s2) and same_bits(cs3, cs2) and same_bits(m3.cpu().numpy().astype(np.float64), m)
    assert ops.ssim_check_status(status) == 0


def test_every_kind_of_image_is_in_the_batches():
    x, y, want = case((5, 3, 3, 32, 32))
    assert len(KINDS) == 5                                       # five samples: every kind once
    B = want['B']
    near = [i for i in range(5) if 0 < B[0, i].max() < 7e-3]     # the near-constant bright plane against itself plus 10^-3 noise
    assert len(near) == 1 and x[near[0]].min() > 0.98 and np.abs(y[0, near[0]] - x[near[0]]).max() < 6e-3
    assert B[0, near[0]].max() ** 2 / 9e-4 < 0.06                # ... where the bound is within 6 % of c units of 2^-24
    assert any((x[i] == x[i].flat[0]).all() for i in range(5))   # a constant
    assert y[2].min() < 0 and y[2].max() > 1                     # values outside [0, 1]
    assert np.array_equal(y[1], x)                               # a draw equal to x


def test_splits_and_orders_give_the_same_bits():
    x, y, _ = case((67, 2, 3, 32, 32))
    s, cs, m = run(x, y, maps=True)
    for lo, hi in ((0, 1), (1, 30), (30, 67)):                   # N split
        a = run(x[lo:hi], y[:, lo:hi], maps=True)
        assert all(same_bits(g, w[:, lo:hi]) for g, w in zip(a, (s, cs, m))), (lo, hi)
    b = run(x, y[1:], maps=True)                                 # R split
    assert all(same_bits(g, w[1:]) for g, w in zip(b, (s, cs, m)))
    perm = np.random.default_rng(3).permutation(67)              # samples reordered, draws reversed
    c = run(x[perm], y[::-1][:, perm], maps=True)
    assert all(same_bits(g, w.cpu().numpy()[::-1][:, perm]) for g, w in zip(c, (s, cs, m)))
    # another chunking of the draws: 33 draws in chunks of two, then five of them alone in chunks of one
    x, y, _ = case((64, 33, 1, 11, 12))
    s, cs = run(x, y)
    a = run(x[:9], y[7:12, :9])
    assert same_bits(a[0], s[7:12, :9]) and same_bits(a[1], cs[7:12, :9])


def test_strided_inputs_and_empty_batches():
    from jvae_hip import ops
    x, y, _ = case((5, 3, 3, 32, 32))
    s, cs, m = run(x, y, maps=True)
    xt, yt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    wide_x = torch.zeros(5, 3, 32, 40, device=DEV)
    wide_y = torch.zeros(3, 5, 3, 32, 40, device=DEV)
    wide_x[..., 4:36], wide_y[..., 4:36] = xt, yt
    got = ops.ssim(wide_x[..., 4:36], wide_y[..., 4:36], maps=True)
    assert not wide_x[..., 4:36].is_contiguous() and all(same_bits(g, w) for g, w in zip(got, (s, cs, m)))
    got = ops.ssim(xt, yt.transpose(0, 1).contiguous().transpose(0, 1))           # draws strided over samples
    assert same_bits(got[0], s) and same_bits(got[1], cs)
    for n, r in ((0, 3), (5, 0), (0, 0)):
        e = ops.ssim(xt[:n], yt[:r, :n], maps=True)
        assert e[0].shape == e[1].shape == (r, n) and e[2].shape == (r, n, 22, 22) and e[0].dtype == torch.float32


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')], ids=['nan', 'inf', '-inf'])
@pytest.mark.parametrize('shape', [(5, 3, 3, 32, 32), (1, 2, 3, 64, 64)], ids=['one-strip', 'strips'])
def test_non_finite_pixels(shape, bad):
    from jvae_hip import ops
    x, y, _ = case(shape)
    N, R = shape[:2]
    clean = run(x, y, maps=True)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    n = N - 1
    xb = x.copy()
    xb[n, 1, -1, -1] = bad                                       # the last pixel of a middle channel: in the last strip only
    got = run(xb, y, maps=True, status=status)
    assert int(status) == ops.SSIM_STATUS_X
    keep = np.ones((R, N), dtype=bool)
    keep[:, n] = False
    for g, w in zip(got, clean):
        g, w = g.cpu().numpy(), w.cpu().numpy()
        assert np.isnan(g[~keep]).all() and same_bits(g[keep], w[keep])
    with pytest.raises(ValueError, match='image with a non-finite'):
        ops.ssim_check_status(status)
    assert int(status) == 0                                      # read and cleared
    yb = y.copy()
    yb[R - 1, 0, 0, 0, 0] = bad                                  # the first pixel of one draw
    got = run(x, yb, maps=True, status=status)
    assert int(status) == ops.SSIM_STATUS_Y
    keep = np.ones((R, N), dtype=bool)
    keep[R - 1, 0] = False
    for g, w in zip(got, clean):
        g, w = g.cpu().numpy(), w.cpu().numpy()
        assert np.isnan(g[~keep]).all() and same_bits(g[keep], w[keep])
    with pytest.raises(ValueError, match='reconstruction with a non-finite'):
        ops.ssim_check_status(status)
    assert ops.ssim_check_status(status) == 0
    # the default word of the device
    ops.ssim_check_status()
    run(x, yb)
    assert int(ops.ssim_status(torch.device(DEV))) == ops.SSIM_STATUS_Y
    with pytest.raises(ValueError):
        ops.ssim_check_status()
    assert ops.ssim_check_status() == 0


def test_arguments_on_the_device():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    x, y = torch.zeros(2, 1, 16, 16, device=DEV), torch.zeros(3, 2, 1, 16, 16, device=DEV)
    with pytest.raises(JvaeHipError, match='status word'):
        ops.ssim(x, y, status=torch.zeros(1, dtype=torch.int64, device=DEV))
    with pytest.raises(JvaeHipError, match='status word'):
        ops.ssim(x, y, status=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(JvaeHipError, match='unsupported configuration'):
        ops.ssim(x[..., :10], y[..., :10])
    s, cs = ops.ssim(x, y)                                       # zeros against zeros
    assert (s == 1).all() and (cs == 1).all()


# ------------------------------------------------------------------------------------------- the model
_MODEL = {}


def model():
    if not _MODEL:
        _MODEL['net'] = build()
    return _MODEL['net']


def formula(s, cs):
    """The stated rows on ops.ssim's (L + 1, N) outputs: fp64 means over the sampled draws, rounded once."""
    return {'ssim': s[1:].double().mean(0).float(), 'ssim-mu': s[0], 'ssim-cs': cs[1:].double().mean(0).float()}


def test_ssim_scores_and_map_of_a_batch():
    from jvae_hip import ops
    net = model()
    x = synth(9, 'q', 4).tensors[0].to(DEV)
    got = {}
    for seed in (3, 4):
        torch.manual_seed(seed)
        with torch.no_grad():
            x_reco = net.evaluate(x)[0]
        assert x_reco.shape == (3, 9, 1, 28, 28)                 # L = 2 draws behind the mean row
        s, cs, m = ops.ssim(x, x_reco, maps=True)
        got[seed] = net.ssim_scores(x, x_reco)
        want = formula(s, cs)
        assert list(got[seed]) == NAMES
        for k in NAMES:
            assert got[seed][k].dtype == torch.float32 and got[seed][k].shape == (9,) and torch.equal(got[seed][k], want[k]), k
        net.train()
        torch.manual_seed(seed + 10)
        pix = net.ssim_map(x)
        assert net.training
        net.eval()
        assert pix.shape == (9, 18, 18) and torch.equal(pix, m[0])           # row 0 draws no noise
        assert torch.equal(net.ssim_map(x), pix) and not net.training
    assert torch.equal(got[3]['ssim-mu'], got[4]['ssim-mu'])     # the same bits under any seed ...
    assert not torch.equal(got[3]['ssim'], got[4]['ssim']) and not torch.equal(got[3]['ssim-cs'], got[4]['ssim-cs'])
    assert ops.ssim_check_status() == 0


def test_rates(monkeypatch, tmp_path):
    from jvae_hip import ops
    from module import score_rows
    net = model()
    sets = [synth(40, 'ind', 1), synth(40, 'ood', 2, .3)]
    call = dict(oodsets=sets[1:], testset=sets[0], batch_size=16, update_self_ood=False)
    for m in (['elbo'] + NAMES, 'ssim*', 'ssim-mu'):
        with pytest.raises(NotImplementedError, match='OOD_SSIM_METHODS'):            # off: the names raise
            net.ood_detection_rates(method=m, **call)
    torch.manual_seed(11)
    plain = net.ood_detection_rates(method=['elbo', 'mse'], **call)
    torch.manual_seed(11)
    off_all = net.ood_detection_rates(method='all', **call)
    families = score_rows.FAMILIES
    monkeypatch.setattr(score_rows, 'FAMILIES', tuple(f for f in families if f.prefix != 'ssim'))      # the table without the family
    torch.manual_seed(11)
    assert net.ood_detection_rates(method='all', **call) == off_all                    # off: 'all' is bit for bit what it was
    monkeypatch.setattr(score_rows, 'FAMILIES', families)
    assert not any(m.startswith('ssim') for m in off_all['ood'])

    def record_keys(where, method=('elbo', 'mse')):
        # (a new recorder seeds the noise of its pass by itself: the keys are compared, the results above)
        net.ood_detection_rates(method=list(method), recorders={}, sample_dirs=[str(tmp_path / where)], **call)
        return {s.name: sorted(torch.load(tmp_path / where / f'record-{s.name}.pth', map_location='cpu',
                                               weights_only=False)['_tensors']) for s in sets}
    monkeypatch.setattr(score_rows, 'FAMILIES', tuple(f for f in families if f.prefix != 'ssim'))
    without = record_keys('without')                                                   # a pass without the family
    monkeypatch.setattr(score_rows, 'FAMILIES', families)
    assert record_keys('off') == without and not any(k.startswith('ssim') for k in without['ind'])
    net.OOD_SSIM_METHODS = True
    try:
        torch.manual_seed(11)
        bare = net.ood_detection_rates(method=['elbo', 'mse', 'ssim*'], **call)
        assert list(bare['ood']) == ['elbo', 'mse'] + NAMES
        assert all(bare['ood'][m] == plain['ood'][m] for m in ('elbo', 'mse'))         # the other rows: the same bits
        torch.manual_seed(11)
        on_all = net.ood_detection_rates(method='all', **call)
        assert list(on_all['ood']) == list(off_all['ood']) + NAMES and all(on_all['ood'][m] == off_all['ood'][m] for m in off_all['ood'])
        # on, but no row of the family asked for: the pass and its file are those of a model without it
        torch.manual_seed(11)
        assert net.ood_detection_rates(method=['elbo', 'mse'], **call) == plain
        assert record_keys('on') == without
        assert record_keys('asked', ['elbo', 'mse', 'ssim-mu']) == {k: sorted(v + NAMES) for k, v in without.items()}
        recorders = {}                                                                  # (a recorder seeds the noise by itself)
        seen = []
        real_scores = net.ssim_scores
        monkeypatch.setattr(net, 'ssim_scores', lambda x, x_reco: seen.append((x, x_reco)) or real_scores(x, x_reco))
        first = net.ood_detection_rates(method=['elbo', 'mse', 'ssim*'], recorders=recorders, **call)
        monkeypatch.setattr(net, 'ssim_scores', real_scores)
        assert list(first['ood']) == ['elbo', 'mse'] + NAMES and len(seen) == 6
        for j, s in enumerate(sets):
            rec = recorders[s.name]
            for i in range(3):                                                          # the batches of the pass
                x, x_reco = seen[3 * j + i]
                assert torch.equal(x, s.tensors[0][16 * i:16 * i + 16].to(DEV)) and x_reco.shape == (3,) + x.shape
                # the x_reco of the SAME pass: its squared error over the sampled draws is the recorded `wmse` of every sample,
                # up to the model's one constant sigma
                ratio = rec.get_batch(i, 'wmse').to(DEV).double() / ((x_reco[1:] - x).double() ** 2).mean((-3, -2, -1)).mean(0)
                assert float(ratio.max() / ratio.min()) - 1 < 1e-4 and float(ratio.min()) > 0
                want = formula(*ops.ssim(x, x_reco))
                for m in NAMES:
                    got = rec.get_batch(i, m).to(DEV)
                    assert got.dtype == torch.float32 and torch.equal(got, want[m]), (s.name, i, m)
        for m in NAMES:
            ins, outs = (recorders[s][m].float().cpu().numpy() for s in ('ind', 'ood'))
            r = first['ood'][m]
            auc, fpr, tpr, low, up = roc_restatement(ins, outs, KEPT)
            print(m, 'auc', r['auc'], 'restated', auc, 'mean score in / out', ins.mean(), outs.mean())
            assert r['n'] == 40 and r['fpr'] == fpr.tolist() and abs(r['auc'] - auc) <= auc_bound(40)
            roc = ops.roc_curve(torch.from_numpy(ins).to(DEV), torch.from_numpy(outs).to(DEV), KEPT)
            assert float(roc['auc']) == r['auc'] and [float(f) for f in roc['fpr']] == r['fpr']
        assert net.test_losses and not any(k.startswith('ssim') for k in net.test_losses)     # test_losses: the loss components only
        calls = []
        real_eval, real_op = net.evaluate, ops.ssim
        monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append('e') or real_eval(*a, **k))
        monkeypatch.setattr(net, 'ssim_scores', lambda *a, **k: calls.append('s') or real_scores(*a, **k))
        monkeypatch.setattr(ops, 'ssim', lambda *a, **k: calls.append('S') or real_op(*a, **k))
        again = net.ood_detection_rates(method=['elbo', 'mse', 'ssim*'], recorders=recorders, **call)
        assert not calls and again == first                                             # a full recorder is read back: no launch
        one = net.ood_detection_rates(method='ssim-cs', **call)
        assert list(one['ood']) == ['ssim-cs']
        assert calls.count('e') == 6 and calls.count('s') == 6 and calls.count('S') == 6       # one pass, one launch per batch
    finally:
        del net.OOD_SSIM_METHODS
    assert ops.ssim_check_status() == 0


def test_rates_through_a_wim_job_with_estimated_labels(monkeypatch):
    """The override of jvae_compat/wim.py: with estimated labels on, the items are ((x, y_est), y) pairs and the evaluation runs
    under both priors; its `with_reco` hands the reconstructions of that pass to the family."""
    from jvae_compat.wim import EstimatedLabelsDataset
    from jvae_hip import ops
    from test_14_wim_gpu import _Images, model_job
    job, kw = model_job()
    g = torch.Generator().manual_seed(9)
    sets = [EstimatedLabelsDataset(_Images(32, 1, 'in'), torch.randint(0, 10, (32,), generator=g)),
            EstimatedLabelsDataset(_Images(32, 2, 'out', shift=.6), torch.randint(0, 10, (32,), generator=g))]
    call = dict(oodsets=[sets[1]], testset=sets[0], batch_size=16, update_self_ood=False)
    torch.manual_seed(5)
    plain = job.ood_detection_rates(method=['zdist~@', 'elbo@'], **call)
    job.OOD_SSIM_METHODS = True
    seen = []
    real_scores, real_eval = job.ssim_scores, job._evaluate_for_scores

    def evaluated(*a, **k):
        out = real_eval(*a, **k)
        assert job._with_estimated_labels and k.get('with_reco') is True and len(out) == 5
        return out
    monkeypatch.setattr(job, '_evaluate_for_scores', evaluated)
    monkeypatch.setattr(job, 'ssim_scores', lambda x, x_reco: seen.append((x, x_reco)) or real_scores(x, x_reco))
    recorders = {}
    torch.manual_seed(5)
    got = job.ood_detection_rates(method=['zdist~@', 'elbo@', 'ssim*'], **call)
    assert list(got['out']) == ['zdist~@', 'elbo@'] + NAMES and all(got['out'][m] == plain['out'][m] for m in plain['out'])
    assert len(seen) == 4
    first = job.ood_detection_rates(method=['ssim*'], recorders=recorders, **call)
    for j, s in enumerate(sets):
        for i in range(2):
            x, x_reco = seen[4 + 2 * j + i]
            assert x.shape == (16, 3, 32, 32) and x_reco.shape[1:] == x.shape and x_reco.shape[0] >= 2
            want = formula(*ops.ssim(x, x_reco))
            for m in NAMES:
                assert torch.equal(recorders[s.name].get_batch(i, m).to(DEV), want[m]), (s.name, i, m)
    for m in NAMES:
        r = first['out'][m]
        assert r['n'] == 32 and 0. <= r['auc'] <= 1. and len(r['fpr']) == len(job.OOD_KEPT_TPR)
    assert ops.ssim_check_status() == 0
