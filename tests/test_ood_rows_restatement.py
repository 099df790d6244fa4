"""The class-axis score rows of csrc/misclass.hip (kinds 5 .. 13 of ops.misclass_scores), restated: the reference's expressions
(cvae.py:985-1068) as torch code that runs in any dtype - in float64 on the CPU it is the checker of tests/test_13_ood_phase_gpu.py,
in float32 it is what batch_dist_measures computes without `out=` - the inputs those tests share, and the rank count the kernel
finds the median with.  Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

from oracle.cases import get_case

# kind -> what the row reads its constant from (None: the kind takes none)
NEW_KINDS = ('lse-', 'lse+', 'mean', 'std', 'nstd', 'mag', 'IYx')
FLAT_KINDS = ('neg', 'id')
EXACT_KINDS = ('mag', 'neg', 'id')                      # no rounding beyond one subtraction: bit-equal to torch
CLASSES = (1, 2, 3, 10, 128)
SAMPLES = (1, 63, 64, 70, 193)
# standard deviation of the losses across the classes: 1 (softmax-sized differences), 30 (most exp underflow to denormals or 0),
# 3000 (the all-class ELBO of a 3x32x32 image: every exp but the largest is 0)
SPREADS = (1., 30., 3000.)


def reference_row(kind, v, const=0.):
    """The reference's expression for one kind on a (C, N) source `v` (any float dtype), cvae.py:985-1068."""
    C = v.shape[0]
    if kind == 'neg':
        return -v[0]
    if kind == 'id':
        return v[0]
    lp = v if kind == 'lse+' else -v
    top = lp.max(0)[0]
    d = lp - top
    if kind in ('lse-', 'lse+'):
        return d.exp().sum(0).log() + top + const
    if kind == 'mean':
        return d.exp().mean(0).log() + top
    if kind == 'std':
        return lp.std(0)
    if kind == 'nstd':
        return (d.exp().std(0).log() - d.exp().mean(0).log()).exp().pow(2)
    if kind == 'mag':
        return top - lp.median(0)[0]
    if kind == 'IYx':
        d_x = d.exp().mean(0).log()
        return (d * d.exp()).sum(0) / (C * d_x.exp()) - d_x
    raise ValueError(kind)


def make_source(C, N, spread, seed):
    """(C, N) fp32 losses: 2 * spread + spread * normal.  From N = 3 on, the last column holds one NaN and the one before it C
    equal values."""
    g = torch.Generator().manual_seed(seed)
    v = (2 * spread + spread * torch.randn(C, N, generator=g, dtype=torch.float64)).float()
    if N >= 3:
        v[C // 2, N - 1] = float('nan')
        v[:, N - 2] = v[0, N - 2]
    return v


def ulp32(x):
    """One fp32 unit in the last place of |x| (fp64 tensor in, fp64 out); that of the smallest normal number below it."""
    a = x.abs().clamp_min(2. ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def rank_median(column):
    """torch.median of a NaN-free column as the kernel finds it: the value whose rank interval holds index (C - 1) // 2."""
    k = (len(column) - 1) // 2
    for x in column:
        lt, eq = int((column < x).sum()), int((column == x).sum())
        if lt <= k < lt + eq:
            return x
    raise AssertionError('no element holds the middle rank')


@pytest.mark.parametrize('C', CLASSES)
def test_rank_count_finds_torch_median(C):
    for seed, N in enumerate((5, 8)):
        v = make_source(C, N, 30., seed)[:, :N - 2]
        v[:, 0] = v[:, 0].round()                          # ties
        want = (-v).median(0)[0].numpy()
        got = np.array([rank_median((-v[:, n]).numpy()) for n in range(v.shape[1])], np.float32)
        assert got.tobytes() == want.tobytes()


def cpu_cvae():
    from cvae import ClassificationVariationalNetwork as Net
    return Net(**dict(get_case('c1_n16_mlp')['net'], gamma=0.))


def test_the_six_class_axis_names_are_scores_of_batch_dist_measures():
    """`sum`, `mean`, `std`, `nstd`, `mag`, `IYx` (cvae.py:1020-1068) raised NotImplementedError before; the plain call is the
    reference's fp32 torch expression, so on the CPU it equals `reference_row` on the same tensor bit for bit."""
    net = cpu_cvae()
    total = make_source(net.num_labels, 70, 30., 3)
    names = {'sum': 'lse-', 'mean': 'mean', 'std': 'std', 'nstd': 'nstd', 'mag': 'mag', 'IYx': 'IYx'}
    got = net.batch_dist_measures(None, {'total': total}, list(names) + ['std-2s'])
    assert list(got) == list(names) + ['std-2s']
    for name, kind in names.items():
        want = reference_row(kind, total)
        assert got[name].shape == (70,) and got[name].numpy().tobytes() == want.numpy().tobytes(), name
    assert got['std-2s'].numpy().tobytes() == got['std'].numpy().tobytes()
    with pytest.raises(NotImplementedError):
        net.batch_dist_measures(None, {'total': total}, ['fisher_rao'])


def test_row_tables():
    """The kind numbers are the header's (include/jvae_hip.h); every class-axis name has a kernel row on `total`; the rows whose
    form depends on the model type."""
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    assert ops.MISCLASS_KINDS == {'soft-': 0, 'soft+': 1, 'max-': 2, 'max+': 3, 'hyz': 4, 'lse-': 5, 'lse+': 6, 'mean': 7,
                                  'std': 8, 'nstd': 9, 'mag': 10, 'IYx': 11, 'neg': 12, 'id': 13}
    from module import score_rows

    def fused_row(net, m, **kw):
        row = score_rows.parse(m, score_rows.traits_of(net), **kw)
        return row.source, None if row.kind is None else (row.kind, row.const)
    net = cpu_cvae()
    assert fused_row(net, 'sum', misclass=True) == ('total', ('lse-', 0.))
    for m in ('mean', 'std', 'nstd', 'mag', 'IYx'):
        assert fused_row(net, m, misclass=True) == ('total', (m, 0.))
    # the misclassification pass keeps `iws` on its torch row: no launch is tried (there is no CPU path), the row is torch's
    iws, row = {'iws': make_source(10, 5, 1., 0)}, score_rows.parse('iws', score_rows.traits_of(net), misclass=True)
    kept, = score_rows.write_rows([row], [0], None, iws, torch.zeros(1, 5), torch_rows=Net.MISCLASS_TORCH_ROWS)
    assert row.source == 'iws' and kept.numpy().tobytes() == row.torch_row(iws).numpy().tobytes()
    with pytest.raises(ValueError):
        score_rows.parse('softmax', score_rows.traits_of(net), misclass=True)
    assert fused_row(net, 'iws') == ('iws', ('lse+', math.log(net.num_labels)))
    assert fused_row(net, 'elbo') == ('total', ('max-', 1.)) and fused_row(net, 'zdist') == ('zdist', ('max-', 1.))
    assert fused_row(net, 'mse') == ('cross_x', ('neg', 0.)) and fused_row(net, 'wmse') == ('wmse', ('neg', 0.))
    assert fused_row(net, 'odin-1-0.0040') == ('odin-1-0.0040', None)
    with pytest.raises(NotImplementedError):
        score_rows.parse('fisher_rao', score_rows.traits_of(net))
    base = {m: score_rows.parse(m, score_rows.traits_of(net)).base for m in ('iws-2s', 'elbo-a-4-1', 'softkl-10')}
    assert base == {'iws-2s': 'iws', 'elbo-a-4-1': 'elbo', 'softkl-10': 'softkl-10'}
    vae = Net(**dict(get_case('ea2_n8_vae_L3')['net']))
    assert fused_row(vae, 'iws') == ('iws', ('id', 0.)) and fused_row(vae, 'elbo') == ('total', ('neg', 0.))
    assert fused_row(vae, 'zdist') == ('zdist', ('neg', 0.))
    assert Net.TRAIN_OOD_PHASE is False and set(Net.SCORE_SET_TORCH_ROWS) >= {'iws', 'elbo'}
