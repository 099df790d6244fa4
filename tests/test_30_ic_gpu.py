"""Input-complexity OOD scores on the MI355X (ops.image_code_length, csrc/ic.hip, net.input_complexity / ic_scores and the `ic-*`
rows) against the numpy restatement of tests/test_ic_restatement.py.

The kernel's histograms are integers and the one floating-point sum of a histogram runs over the symbols ascending in fp64 over
the table the restatement reads too, so `bits` is held to the restatement BIT FOR BIT, `choice` is identical and bits32 is
float32(bits) - no tolerance anywhere.  Shapes: each is there for one way the kernel can go wrong (below); the images of a batch
cycle through constant images at 0, 77 and 255, uniform noise, smooth fields with noise of three strengths, a 0 / 255
checkerboard (the mod-256 wrap of every predictor) and a grey image replicated over the channels."""
import math

import numpy as np
import pytest
import torch

from test_28_knn_gpu import build, synth
from test_ic_restatement import (KINDS, STATUS_INEXACT, STATUS_NONFINITE, batch, batch_code_length, constant, uniform_noise)
from test_roc_restatement import auc_bound, roc_restatement

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEPT = [pc / 100 for pc in range(90, 100)]

SHAPES = [(1, 1, 1, 1),             # the smallest input: the stored mode
          (3, 1, 2, 3),
          (5, 3, 7, 5),             # odd sizes, borders
          (67, 3, 32, 32),          # N a multiple of nothing, the workload's image
          (2, 3, 64, 64),
          (1, 1, 300, 300),         # n > 65535: the counters' width, and the planes are read from global memory
          (2, 4, 9, 9),             # C = 4: no colour transform
          (2, 2, 8, 8),             # C = 2
          (1, 1, 181, 181),         # 32 761 bytes of planes: the largest image staged in LDS at C = 1 ...
          (1, 1, 182, 181),         # ... and the first one that is not
          (1, 3, 80, 81),           # 5 x 6 480 bytes: staged at C = 3 ...
          (1, 3, 81, 81)]           # ... 5 x 6 561: not staged
_CASES = {}


def case(shape):
    """(x, bits, choice) of a shape: the batch and its restatement, computed once and never modified.  The seed makes the first
    image of every batch a smooth field with noise, the next ones stronger noise, the checkerboard, the grey image, ..."""
    if shape not in _CASES:
        x = batch(*shape, seed=KINDS.index('smooth4') + len(KINDS) * SHAPES.index(shape))
        bits, choice, status = batch_code_length(x)
        assert status == 0
        _CASES[shape] = (x, bits, choice)
    return _CASES[shape]


def run(x):
    """-> (bits fp64, bits32 fp32, choice int32, status) as numpy / int, with a status word of the call's own."""
    from jvae_hip import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    bits, bits32, choice = ops.image_code_length(t, status=status)
    assert bits.dtype == torch.float64 and bits32.dtype == torch.float32 and choice.dtype == torch.int32
    assert bits.shape == bits32.shape == choice.shape == (x.shape[0],)
    return bits.cpu().numpy(), bits32.cpu().numpy(), choice.cpu().numpy(), int(status)


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bits_are_the_restatements(shape):
    x, want, want_choice = case(shape)
    bits, bits32, choice, status = run(x)
    n_dim = shape[1] * shape[2] * shape[3]
    print(shape, 'bits per dim: min', float(want.min()) / n_dim, 'max', float(want.max()) / n_dim, 'largest |difference|',
          float(np.abs(bits - want).max()), 'choices that differ', int((choice != want_choice).sum()))
    assert status == 0
    assert same_bits(bits, want)
    assert np.array_equal(choice, want_choice)
    assert np.array_equal(bits32.view(np.int32), want.astype(np.float32).view(np.int32))


def test_every_kind_of_image_is_in_the_workload_batch():
    x, want, want_choice = case((67, 3, 32, 32))
    assert len(KINDS) == 9 and 67 > 7 * len(KINDS)              # every kind at least seven times
    from jvae_hip import ops
    spaces = {ops.ic_choice(w)[0] for w in want_choice}
    modes = {m for w in want_choice for m in ops.ic_choice(w)[1]}
    print('spaces chosen', spaces, 'modes chosen', sorted(modes))
    assert spaces == {0, 1} and {0, 6} <= modes and len(modes) >= 4


def test_calls_repeat_and_split():
    x, want, _ = case((67, 3, 32, 32))
    first, second = run(x), run(x)
    assert same_bits(first[0], second[0]) and np.array_equal(first[2], second[2])
    a, b = run(x[:29]), run(x[29:])
    assert same_bits(np.concatenate([a[0], b[0]]), first[0]) and np.array_equal(np.concatenate([a[2], b[2]]), first[2])
    t = torch.from_numpy(x).to(DEV)
    from jvae_hip import ops
    strided = t.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)                    # made contiguous by the op
    assert torch.equal(ops.image_code_length(strided)[0], torch.from_numpy(first[0]).to(DEV))
    assert ops.ic_check_status() == 0                                                   # the default word: clean


def test_an_empty_batch():
    from jvae_hip import ops
    bits, bits32, choice = ops.image_code_length(torch.zeros((0, 3, 32, 32), device=DEV))
    assert bits.shape == bits32.shape == choice.shape == (0,) and bits.dtype == torch.float64
    torch.cuda.synchronize()


def test_pixels_off_the_grid_are_rounded_and_flagged():
    x, want, want_choice = case((5, 3, 7, 5))
    bits, _, choice, status = run(x + np.float32(0.3 / 255))
    assert status == STATUS_INEXACT and same_bits(bits, want) and np.array_equal(choice, want_choice)
    bits, _, choice, status = run(x + np.float32(0.005 / 255))                          # inside 1 / 64: exact
    assert status == 0 and same_bits(bits, want)
    from jvae_hip import ops
    word = torch.tensor([status | STATUS_INEXACT], dtype=torch.int32, device=DEV)
    assert ops.ic_check_status(word) == STATUS_INEXACT and int(word) == 0              # read and cleared, not an error


@pytest.mark.parametrize('shape', [(5, 3, 7, 5), (3, 1, 200, 200)], ids=['staged', 'global'])
def test_a_non_finite_pixel_refuses_its_image_alone(shape):
    from jvae_hip import ops
    x = batch(*shape, seed=2)
    want, want_choice, _ = batch_code_length(x)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, -1, shape[2] // 2, 1] = bad
        bits, bits32, choice, status = run(y)
        assert status == STATUS_NONFINITE
        assert np.isnan(bits[1]) and np.isnan(bits32[1]) and choice[1] == -1
        keep = [i for i in range(shape[0]) if i != 1]
        assert same_bits(bits[keep], want[keep]) and np.array_equal(choice[keep], want_choice[keep])
    word = torch.tensor([STATUS_NONFINITE], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match='non-finite'):
        ops.ic_check_status(word)
    assert int(word) == 0


def test_arguments():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    x = torch.zeros((2, 3, 8, 8), device=DEV)
    for bad in (lambda: ops.image_code_length(x.double()), lambda: ops.image_code_length(x[0]),
                lambda: ops.image_code_length(torch.zeros((2, 5, 8, 8), device=DEV)),
                lambda: ops.image_code_length(x, status=torch.zeros(1, device=DEV)),
                lambda: ops.image_code_length(x, status=torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(JvaeHipError):
            bad()
    assert ops.ic_table(64, x.device) is ops.ic_table(64, x.device) and ops.ic_table(64, x.device).is_cuda


# ------------------------------------------------------------------------------------------- the model
_MODEL = {}


def model():
    if not _MODEL:
        _MODEL['net'] = build()
    return _MODEL['net']


def formula(net, rows, L):
    """The stated fp64 formula on the `elbo` / `iws` rows of a batch (nats) and its code lengths L (bits)."""
    D = float(np.prod(tuple(net.input_shape)))
    return {'ic-bits': (-L).float(),
            **{'ic-' + k: (v.double() / math.log(2) - D * math.log2(255) + L).float() for k, v in rows.items()}}


def test_input_complexity_of_a_batch():
    from jvae_hip import ops
    net = model()
    x = synth(9, 'q', 4).tensors[0]
    ops.ic_check_status()                                                               # whatever earlier calls left: cleared
    got = net.input_complexity(x.to(DEV))
    want, want_choice, status = batch_code_length(x.numpy())
    assert list(got) == ['bits', 'bits_per_dim', 'choice'] and status == STATUS_INEXACT   # torch.rand: off the 8-bit grid
    assert same_bits(got['bits'].cpu().numpy(), want) and np.array_equal(got['choice'].cpu().numpy(), want_choice)
    assert torch.equal(got['bits_per_dim'], got['bits'] / 784.)
    assert ops.ic_check_status() == STATUS_INEXACT and ops.ic_check_status() == 0


def test_rates(monkeypatch):
    from jvae_hip import ops
    from module import score_rows
    net = model()
    names = ['ic-bits', 'ic-elbo', 'ic-iws']
    sets = [synth(40, 'ind', 1), synth(40, 'ood', 2, .3)]
    call = dict(oodsets=sets[1:], testset=sets[0], batch_size=16, update_self_ood=False)
    for m in (['elbo'] + names, 'ic*', 'ic-iws'):
        with pytest.raises(NotImplementedError, match='OOD_IC_METHODS'):              # off: the names raise
            net.ood_detection_rates(method=m, **call)
    torch.manual_seed(11)
    plain = net.ood_detection_rates(method=['elbo', 'iws'], **call)
    torch.manual_seed(11)
    off_all = net.ood_detection_rates(method='all', **call)
    families = score_rows.FAMILIES
    monkeypatch.setattr(score_rows, 'FAMILIES', tuple(f for f in families if f.prefix != 'ic-'))       # the table without the family
    torch.manual_seed(11)
    assert net.ood_detection_rates(method='all', **call) == off_all                    # off: 'all' is bit for bit what it was
    monkeypatch.setattr(score_rows, 'FAMILIES', families)
    assert not any(m.startswith('ic') for m in off_all['ood'])
    net.OOD_IC_METHODS = True
    try:
        torch.manual_seed(11)
        bare = net.ood_detection_rates(method=['elbo', 'iws', 'ic*'], **call)
        assert list(bare['ood']) == ['elbo', 'iws'] + names
        assert all(bare['ood'][m] == plain['ood'][m] for m in ('elbo', 'iws'))         # the other rows: the same bits
        torch.manual_seed(11)
        on_all = net.ood_detection_rates(method='all', **call)
        assert list(on_all['ood']) == list(off_all['ood']) + names and all(on_all['ood'][m] == off_all['ood'][m] for m in off_all['ood'])
        recorders = {}                                                                  # (a recorder seeds the noise by itself)
        first = net.ood_detection_rates(method=['elbo', 'iws', 'ic*'], recorders=recorders, **call)
        assert list(first['ood']) == ['elbo', 'iws'] + names
        traits = score_rows.traits_of(net)
        for s in sets:
            rec = recorders[s.name]
            for i in range(3):                                                          # the batches of the pass
                losses = rec.get_batch(i, 'total', 'iws', force_dict=True)
                rows = {k: score_rows.parse(k, traits).torch_row({k2: v.to(DEV) for k2, v in losses.items()}) for k in ('elbo', 'iws')}
                L = net.input_complexity(s.tensors[0][16 * i:16 * i + 16].to(DEV))['bits']
                want = formula(net, rows, L)
                for m in names:
                    got = rec.get_batch(i, m).to(DEV)
                    assert got.dtype == torch.float32 and torch.equal(got, want[m]), (s.name, i, m)
        for m in names:
            ins, outs = (recorders[s][m].float().cpu().numpy() for s in ('ind', 'ood'))
            r = first['ood'][m]
            auc, fpr, tpr, low, up = roc_restatement(ins, outs, KEPT)
            print(m, 'auc', r['auc'], 'restated', auc, 'mean score in / out', ins.mean(), outs.mean())
            assert r['n'] == 40 and r['fpr'] == fpr.tolist() and abs(r['auc'] - auc) <= auc_bound(40)
        assert net.test_losses and not any(k.startswith('ic') for k in net.test_losses)       # test_losses: the loss components only
        calls = []
        real_eval, real_ic, real_op = net.evaluate, net.ic_scores, ops.image_code_length
        monkeypatch.setattr(net, 'evaluate', lambda *a, **k: calls.append('e') or real_eval(*a, **k))
        monkeypatch.setattr(net, 'ic_scores', lambda *a, **k: calls.append('i') or real_ic(*a, **k))
        monkeypatch.setattr(ops, 'image_code_length', lambda *a, **k: calls.append('L') or real_op(*a, **k))
        again = net.ood_detection_rates(method=['elbo', 'iws', 'ic*'], recorders=recorders, **call)
        assert not calls and again == first                                             # a full recorder is read back: no launch
        one = net.ood_detection_rates(method='ic-elbo', **call)
        assert list(one['ood']) == ['ic-elbo']
        assert calls.count('e') == 6 and calls.count('i') == 6 and calls.count('L') == 6       # one pass, one launch per batch
    finally:
        del net.OOD_IC_METHODS
    assert ops.ic_check_status() == STATUS_INEXACT                                      # torch.rand images: flagged, not refused


def test_ic_bits_separates_constant_from_uniform_images():
    net = model()
    rng = np.random.default_rng(8)

    def dset(images, name):
        d = torch.utils.data.TensorDataset(torch.from_numpy(np.stack(images)), torch.zeros(len(images), dtype=torch.int64))
        d.name = name
        return d
    const = dset([constant(1, 28, 28, int(v)) for v in rng.integers(0, 256, 24)], 'const')
    noise = dset([uniform_noise(1, 28, 28, 50 + i) for i in range(24)], 'uniform')
    net.OOD_IC_METHODS = True
    recorders = {}
    try:
        got = net.ood_detection_rates(method='ic-bits', oodsets=[noise], testset=const, batch_size=24, update_self_ood=False,
                                      recorders=recorders)
    finally:
        del net.OOD_IC_METHODS
    r = got['uniform']['ic-bits']
    ins, outs = (recorders[k]['ic-bits'].cpu().numpy() for k in ('const', 'uniform'))
    rank_auc = float((ins[:, None] > outs[None, :]).mean() + .5 * (ins[:, None] == outs[None, :]).mean())
    curve_auc, curve_fpr = roc_restatement(ins, outs, KEPT)[:2]
    print('ic-bits, constant against uniform: rank auc', rank_auc, 'auc of the ROC', r['auc'], 'restated', curve_auc,
          'scores', set(ins.tolist()), set(outs.tolist()))
    # the coder's property: every constant image scores above every uniform one, the AUC of the ranks is 1.  The figure of
    # ood_detection_rates is the reference's curve, whose thresholds are the in-scores and whose pointer loops stop one short of
    # the end: on 24 TIED in-scores it reads 1 - 1 / 48 for two perfectly separated sets, and is held to its restatement.
    assert rank_auc == 1. and ins.min() > outs.max()
    assert set(ins.tolist()) == {-19.} and set(outs.tolist()) == {-(8. * 784 + 3)}        # 8 + 8 + 3 bits; stored: 8 n + 3
    assert abs(r['auc'] - curve_auc) <= auc_bound(24) and r['fpr'] == curve_fpr.tolist()
    assert r['mean'] == -(8 * 784 + 3)
    from jvae_hip import ops
    assert ops.ic_check_status() == 0
