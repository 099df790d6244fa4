"""Host side of the Mahalanobis OOD rows (module/scoring.py, module/score_rows.py, ops.maha_fit and the argument checks of
ops.maha_moments / ops.maha_scores and csrc/maha.hip).  No GPU: the model is built on the CPU, nothing is
launched - the library's refusals and its workspace size are host-only calls, and the factorisation runs in numpy."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from test_maha_restatement import maha_case, moments_restatement, operands, whitener


def make_net(case='c1_n16_mlp'):
    from cvae import ClassificationVariationalNetwork as Net
    return Net(**dict(get_case(case)['net']))


def host_fit(K=6, M=80, C=3, shrinkage=0., drop=None):
    """ops.maha_fit on the fp64 restatement's moments, on the host -> (fit, moments)."""
    from jvae_hip import ops
    _, bank, labels = maha_case(K, 4, M, C, 0.)
    if drop is not None:
        bank, labels = bank[labels != drop], labels[labels != drop]
    mom = moments_restatement(bank, labels, C)
    return ops.maha_fit({k: torch.from_numpy(v) for k, v in mom.items()}, shrinkage), mom


def test_the_switch_is_off_by_default():
    net = make_net()
    assert net.OOD_MAHA_METHODS is False and net.latent_gaussians is None and net.LATENT_GAUSSIANS_FILE == 'latent-gaussians.pth'
    table = net._ood_methods('all')
    assert not any(m.startswith('maha') for m in table)
    for m in ('maha*', 'maha', 'maha-rel', 'maha-2s', 'mahalanobis', ['elbo', 'maha']):
        with pytest.raises(NotImplementedError, match='OOD_MAHA_METHODS'):
            net._ood_methods(m)


def test_all_with_the_switch_off_is_the_table_without_the_family():
    """'all' with the switch off is what it was before the family existed: the table of a model whose family list ends before it."""
    from module import score_rows
    net = make_net()
    assert [f.prefix for f in score_rows.FAMILIES] == ['odin', 'regret', 'knn', 'maha', 'ic-', 'dose', 'ssim']
    maha = score_rows.FAMILIES[3]
    assert (maha.starred, maha.names, maha.scores, maha.args) == ('maha*', '_maha_names', 'maha_scores', ('mu',))
    assert maha.is_row('maha') and maha.is_row('maha-rel') and not maha.is_row('maha-') and not maha.is_row('maha-3')
    with_family = net._ood_methods('all')
    families = score_rows.FAMILIES
    try:
        score_rows.FAMILIES = tuple(f for f in families if f is not maha)
        assert net._ood_methods('all') == with_family
    finally:
        score_rows.FAMILIES = families
    net.OOD_KNN_METHODS = True
    assert net._ood_methods('all') == with_family + net._knn_names()


def test_the_switch_on_expands_the_names():
    net = make_net()
    before = net._ood_methods('all')
    net.OOD_MAHA_METHODS = True                      # per instance: the class stays off
    assert type(net).OOD_MAHA_METHODS is False
    names = ['maha', 'maha-rel']
    assert net._maha_names() == names
    assert net._ood_methods('all') == before + names
    assert net._ood_methods('maha*') == names
    assert net._ood_methods(['elbo', 'maha*']) == ['elbo'] + names
    assert net._ood_methods('maha-rel') == ['maha-rel'] and net._ood_methods('maha') == ['maha']
    for unlisted in ('mahalanobis', 'maha-2s'):      # a suffix on the hyphenated name: out of scope, as for `knn-<k>`
        with pytest.raises(ValueError, match='Mahalanobis rows'):
            net._ood_methods(unlisted)
    net.OOD_KNN_METHODS = True
    assert net._ood_methods('all') == before + net._knn_names() + names


def test_maha_rel_is_refused_at_one_class():
    net = make_net()
    net.OOD_MAHA_METHODS = True
    fit, _ = host_fit(K=4, M=30, C=1)
    assert fit['cmap'].tolist() == [0]
    net.latent_gaussians = dict(fit, set='one')
    assert net._maha_names() == ['maha'] and net._ood_methods('maha*') == ['maha'] and net._ood_methods('maha') == ['maha']
    with pytest.raises(ValueError, match='maha-rel'):
        net._ood_methods('maha-rel')
    with pytest.raises(ValueError, match='maha-rel'):
        net._ood_methods(['elbo', 'maha-rel'])
    fit, _ = host_fit(K=4, M=40, C=3, drop=1)        # three labels, two of them seen: the row is back
    net.latent_gaussians = dict(fit, set='two')
    assert fit['cmap'].tolist() == [0, 2] and net._maha_names() == ['maha', 'maha-rel']


def test_score_rows_know_the_names_with_the_trait_only():
    from module import score_rows
    off = score_rows.Traits(True, False, False, 10)
    assert off.OOD_MAHA_METHODS is False and off.OOD_KNN_METHODS is False and off.OOD_REGRET_METHODS is False
    assert score_rows.Traits._fields[-1] == 'OOD_MAHA_METHODS' and score_rows.Traits._field_defaults['OOD_MAHA_METHODS'] is False
    for name in ('maha', 'maha-rel'):
        with pytest.raises(NotImplementedError):
            score_rows.parse(name, off)
    on = off._replace(OOD_MAHA_METHODS=True)
    row = score_rows.parse('maha-rel', on)
    assert (row.name, row.base, row.source, row.kind, row.const, row.roc_mode) == ('maha-rel', 'maha-rel', 'maha-rel', None, None, False)
    two = score_rows.parse('maha-2s', on)
    assert (two.base, two.source, two.roc_mode) == ('maha', 'maha', 'around-mean')
    v = torch.arange(4.)
    assert row.torch_row({'maha-rel': v}) is v       # a recorded row: read as it is
    with pytest.raises(NotImplementedError):
        score_rows.parse('maha-x', on)
    net = make_net()
    assert score_rows.traits_of(net).OOD_MAHA_METHODS is False
    net.OOD_MAHA_METHODS = True
    assert score_rows.traits_of(net).OOD_MAHA_METHODS is True
    assert score_rows.recorded_by('maha').prefix == 'maha' and score_rows.recorded_by('mag') is None


def test_fitting_and_scoring_need_their_inputs():
    net = make_net()
    with pytest.raises(ValueError, match='bank'):
        net.fit_latent_gaussians()
    net.latent_bank = {'bank': torch.zeros(1, 16), 'sq': torch.zeros(1), 'labels': torch.zeros(1, dtype=torch.int64), 'set': 's'}
    with pytest.raises(ValueError, match='two'):
        net.fit_latent_gaussians()
    with pytest.raises(ValueError, match='fit_latent_gaussians'):
        net.maha_scores(torch.zeros(4, 16))
    with pytest.raises(ValueError, match='fit_latent_gaussians'):
        net.save_latent_gaussians('nowhere')


def test_the_fit_is_the_restatement_s():
    from jvae_hip import ops
    fit, mom = host_fit(K=6, M=80, C=4, shrinkage=1e-2, drop=2)
    mu0, W, W0, m, m0, kept = operands(mom, 1e-2)
    assert ops.maha_check_fit(fit) == (6, 3, 4) and fit['shrinkage'] == 1e-2
    assert fit['cmap'].tolist() == kept.tolist() == [0, 1, 3] and fit['cmap'].dtype == torch.int32
    assert torch.equal(fit['counts'], torch.from_numpy(mom['counts'])) and fit['counts'][2] == 0
    assert np.array_equal(fit['means'].numpy(), mom['means']) and np.array_equal(fit['mean0'].numpy(), mom['mean0'])
    assert np.array_equal(fit['mu0_32'].numpy(), mu0) and np.array_equal(fit['W32'].numpy(), np.concatenate([W, W0]))
    assert np.array_equal(fit['m32'].numpy(), m) and np.array_equal(fit['m0_32'].numpy(), m0)
    Wf = fit['W'].numpy()
    assert np.array_equal(Wf, np.tril(Wf)) and np.allclose(Wf, whitener(mom['Sw'], 1e-2), rtol=1e-12, atol=1e-14)
    S = mom['Sw'] + 1e-2 * np.trace(mom['Sw']) / 6 * np.eye(6)
    assert np.allclose(Wf @ S @ Wf.T, np.eye(6), atol=1e-12)                 # it whitens the regularised matrix


def test_a_matrix_that_is_not_positive_definite_names_shrinkage():
    from jvae_hip import ops
    _, bank, labels = maha_case(8, 4, 5, 2, 0.)      # M < K: neither scatter matrix has full rank
    mom = {k: torch.from_numpy(v) for k, v in moments_restatement(bank, labels, 2).items()}
    with pytest.raises(ValueError, match='shrinkage'):
        ops.maha_fit(mom, 0.)
    fit = ops.maha_fit(mom, 1e-2)                    # regularised: it factors
    assert ops.maha_check_fit(fit) == (8, 2, 2)
    with pytest.raises(ValueError, match='shrinkage'):
        ops.maha_fit(mom, -1.)
    empty = dict(mom, counts=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='empty'):
        ops.maha_fit(empty, 1e-2)


def test_gaussians_file_round_trip_on_the_host(tmp_path):
    net = make_net()
    fit, _ = host_fit(K=16, M=200, C=10)
    net.latent_gaussians = dict(fit, set='demo')
    path = net.save_latent_gaussians(str(tmp_path / 'job'))
    assert path.endswith('latent-gaussians.pth') and [p.name for p in (tmp_path / 'job').iterdir()] == ['latent-gaussians.pth']
    other = make_net()
    got = other.load_latent_gaussians(str(tmp_path / 'job'))
    assert got is other.latent_gaussians and got['set'] == 'demo' and got['shrinkage'] == 0. and set(got) == set(fit) | {'set'}
    assert all(torch.equal(got[k], fit[k]) and got[k].dtype == fit[k].dtype for k in fit if torch.is_tensor(fit[k]))
    # the load validates keys, dtypes and shapes
    for broken in ({k: v for k, v in net.latent_gaussians.items() if k != 'cmap'}, dict(net.latent_gaussians, extra=1),
                   dict(net.latent_gaussians, W32=fit['W32'].double()), dict(net.latent_gaussians, m32=fit['m32'][:, :5]),
                   dict(net.latent_gaussians, cmap=fit['cmap'].long()), dict(net.latent_gaussians, mean0=fit['mean0'][:3]),
                   dict(net.latent_gaussians, shrinkage='0'), [1, 2]):
        torch.save(broken, str(tmp_path / 'job' / 'latent-gaussians.pth'))
        with pytest.raises(ValueError, match='load_latent_gaussians'):
            other.load_latent_gaussians(str(tmp_path / 'job'))


def test_library_exports_and_host_only_refusals():
    from jvae_hip import lib
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('jvae_maha_moments_workspace_bytes', 'jvae_maha_moments_f32', 'jvae_maha_scores_f32'):
        assert hasattr(handle, name) and name in lib.exported_symbols()
    L = lib.load()
    ws = L.jvae_maha_moments_workspace_bytes
    # the rows' classes, one count, then one slab of class sums and of scatter entries per 2048 rows, 32 at the most
    assert ws(5, 1, 1) == 24 + 8 + 8 + 8 and ws(2048, 64, 10) == 2048 * 4 + 8 + 8 * 64 * (10 + 64)
    assert ws(50000, 64, 10) == 50000 * 4 + 8 + 25 * 8 * 64 * (10 + 64) and ws(1 << 20, 256, 128) == (1 << 22) + 8 + 32 * 8 * 256 * 384
    for M, K, C in ((0, 8, 2), (5, 0, 2), (5, 257, 2), (5, 8, 0), (5, 8, 129), (1 << 31, 8, 2), (-1, 8, 2)):
        assert ws(M, K, C) == 0, (M, K, C)

    def moments(M, K, C):
        return L.jvae_maha_moments_f32(None, None, M, K, C, None, None, None, None, None, None, None, 0, None)

    def scores(N, K, Cn, C):
        return L.jvae_maha_scores_f32(None, None, None, None, None, None, None, None, None, None, N, K, Cn, C, None, None)
    assert moments(5, 257, 2) == -2 and moments(5, 8, 129) == -2 and moments(1 << 31, 8, 2) == -2          # JVAE_ENOTSUP
    assert moments(0, 8, 2) == -1 and moments(5, 0, 2) == -1 and moments(5, 8, 0) == -1                    # JVAE_EINVAL
    assert moments(5, 8, 2) == -1                    # sizes in range, pointers missing: refused before any launch
    assert scores(4, 257, 2, 2) == -2 and scores(4, 8, 2, 129) == -2 and scores(1 << 31, 8, 2, 2) == -2
    assert scores(-1, 8, 2, 2) == -1 and scores(4, 0, 2, 2) == -1 and scores(4, 8, 0, 2) == -1 and scores(4, 8, 3, 2) == -1
    assert scores(4, 8, 2, 2) == -1 and scores(0, 8, 2, 2) == 0                                            # nothing to do


def test_ops_refuse_before_any_launch():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    assert ops.MAHA_MAX_DIM == 256 and (ops.MAHA_STATUS_LABEL, ops.MAHA_STATUS_BANK, ops.MAHA_STATUS_QUERY) == (1, 2, 4)
    bank, labels = torch.zeros(6, 8), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(JvaeHipError, match='GPU'):
        ops.maha_moments(bank, labels, 2)            # no CPU path
    with pytest.raises(JvaeHipError, match='int64'):
        ops.maha_moments(bank, labels.int(), 2)
    with pytest.raises(JvaeHipError, match='fp32'):
        ops.maha_moments(bank.double(), labels, 2)
    with pytest.raises(JvaeHipError, match=r'\(M, K\)'):
        ops.maha_moments(bank, labels[:5], 2)
    with pytest.raises(JvaeHipError, match=r'\(M, K\)'):
        ops.maha_moments(bank[0], labels, 2)
    for b, y, C in ((torch.zeros(6, 257), labels, 2), (bank, labels, 0), (bank, labels, ops.MISCLASS_MAX_CLASSES + 1),
                    (torch.zeros(0, 8), labels[:0], 2), (torch.zeros(6, 0), labels, 2)):
        with pytest.raises(JvaeHipError, match='unsupported configuration'):
            ops.maha_moments(b, y, C)
    fit, _ = host_fit(K=8, M=60, C=3)
    with pytest.raises(JvaeHipError, match='GPU'):
        ops.maha_scores(torch.zeros(4, 8), fit)      # no CPU path
    with pytest.raises(JvaeHipError, match=r'\(N, 8\)'):
        ops.maha_scores(torch.zeros(4, 7), fit)
    with pytest.raises(JvaeHipError, match='fp32'):
        ops.maha_scores(torch.zeros(4, 8, dtype=torch.float64), fit)
    with pytest.raises(ValueError, match='maha_fit'):
        ops.maha_scores(torch.zeros(4, 8), {k: v for k, v in fit.items() if k != 'W32'})
    with pytest.raises(ValueError, match='m32'):
        ops.maha_scores(torch.zeros(4, 8), dict(fit, m32=fit['m32'].double()))
    with pytest.raises(ValueError, match='query'):
        ops.maha_check_status(ops.MAHA_STATUS_QUERY)
    with pytest.raises(ValueError, match='label'):
        ops.maha_check_status(ops.MAHA_STATUS_LABEL)
    with pytest.raises(ValueError, match='non-finite'):
        ops.maha_check_status(ops.MAHA_STATUS_BANK)
    ops.maha_check_status(0)
