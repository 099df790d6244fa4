"""Host side of the nearest-neighbour OOD rows (module/scoring.py, module/score_rows.py, csrc/knn.hip's argument checks; DESIGN.md
section 7p).  No GPU: the model is built on the CPU, nothing is launched - the library's refusals and its workspace size are
host-only calls."""
import ctypes

import pytest
import torch

from oracle.cases import get_case


def make_net(case='c1_n16_mlp'):
    from cvae import ClassificationVariationalNetwork as Net
    return Net(**dict(get_case(case)['net']))


def test_the_switch_is_off_by_default():
    net = make_net()
    assert net.OOD_KNN_METHODS is False and tuple(net.KNN_K) == (1, 10, 50) and net.KNN_NORMALIZE is True
    assert net.latent_bank is None
    table = net._ood_methods('all')
    assert not any(m.startswith('knn') for m in table)
    for m in ('knn*', 'knn-10', ['elbo', 'knn-1']):
        with pytest.raises(NotImplementedError, match='OOD_KNN_METHODS'):
            net._ood_methods(m)


def test_the_switch_on_expands_the_names():
    net = make_net()
    before = net._ood_methods('all')
    net.OOD_KNN_METHODS = True                       # per instance: the class stays off
    assert type(net).OOD_KNN_METHODS is False
    names = ['knn-1', 'knn-10', 'knn-50']
    assert net._knn_names() == names
    assert net._ood_methods('all') == before + names
    assert net._ood_methods('knn*') == names
    assert net._ood_methods(['elbo', 'knn*']) == ['elbo'] + names
    assert net._ood_methods('knn-10') == ['knn-10']
    with pytest.raises(ValueError, match='KNN_K'):
        net._ood_methods('knn-7')
    net.KNN_K = (3, 7)
    assert net._ood_methods('all') == before + ['knn-3', 'knn-7']
    with pytest.raises(ValueError, match='KNN_K'):
        net._ood_methods('knn-10')


def test_score_rows_know_the_names_with_the_trait_only():
    from module import score_rows
    off = score_rows.Traits(True, False, False, 10)
    assert off.OOD_KNN_METHODS is False and off.OOD_REGRET_METHODS is False
    with pytest.raises(NotImplementedError):
        score_rows.parse('knn-10', off)
    on = off._replace(OOD_KNN_METHODS=True)
    row = score_rows.parse('knn-10', on)
    assert (row.name, row.base, row.source, row.kind, row.const, row.roc_mode) == ('knn-10', 'knn-10', 'knn-10', None, None, False)
    v = torch.arange(4.)
    assert row.torch_row({'knn-10': v}) is v          # a recorded row: read as it is
    with pytest.raises(NotImplementedError):
        score_rows.parse('knn-x', on)
    net = make_net()
    assert score_rows.traits_of(net).OOD_KNN_METHODS is False
    net.OOD_KNN_METHODS = True
    assert score_rows.traits_of(net).OOD_KNN_METHODS is True


def test_scores_need_a_bank():
    net = make_net()
    with pytest.raises(ValueError, match='bank'):
        net.knn_scores(torch.zeros(4, 16))
    net.latent_bank = {'bank': torch.zeros(20, 16), 'sq': torch.zeros(20), 'labels': torch.zeros(20, dtype=torch.int64), 'set': 's'}
    with pytest.raises(ValueError, match='20 rows'):
        net.knn_scores(torch.zeros(4, 16))           # max(KNN_K) = 50 > 20 rows: refused before anything is launched
    with pytest.raises(ValueError):
        net.fit_latent_bank(torch.utils.data.TensorDataset(torch.zeros(4, 1, 28, 28), torch.zeros(4)), ratio=0.)


def test_bank_file_round_trip_on_the_host(tmp_path):
    net = make_net()
    with pytest.raises(ValueError):
        net.save_latent_bank(str(tmp_path))
    g = torch.Generator().manual_seed(3)
    bank = {'bank': torch.randn(7, 16, generator=g), 'sq': torch.rand(7, generator=g), 'labels': torch.arange(7), 'set': 'demo'}
    net.latent_bank = dict(bank)
    path = net.save_latent_bank(str(tmp_path / 'job'))
    assert path.endswith('latent-bank.pth') and [p.name for p in (tmp_path / 'job').iterdir()] == ['latent-bank.pth']
    other = make_net()
    got = other.load_latent_bank(str(tmp_path / 'job'))
    assert got is other.latent_bank and got['set'] == 'demo'
    assert all(torch.equal(got[k], bank[k]) and got[k].dtype == bank[k].dtype for k in ('bank', 'sq', 'labels'))


def test_library_exports_and_host_only_refusals():
    from jvae_hip import lib
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('jvae_knn_sqnorms_f32', 'jvae_knn_workspace_bytes', 'jvae_knn_f32'):
        assert hasattr(handle, name) and name in lib.exported_symbols()
    L = lib.load()
    ws = L.jvae_knn_workspace_bytes
    # N lists of k (distance, index) pairs per partition
    assert ws(512, 50000, 64, 50, 8) == 512 * 8 * 50 * 8
    assert ws(1, 1, 1, 1, 1) == 8 and ws(0, 10, 4, 4, 1) == 0
    own = ws(512, 50000, 64, 50, 0)                  # the library's own choice: a whole number of partitions, at most 1024
    assert own % (512 * 50 * 8) == 0 and 1 <= own // (512 * 50 * 8) <= 1024
    assert ws(512, 100, 64, 50, 0) == 512 * 50 * 8   # a bank smaller than one partition's least: one partition
    for N, M, K, k, s in ((4, 10, 8, 0, 1), (4, 10, 8, 65, 1), (4, 10, 0, 4, 1), (4, 10, 4097, 4, 1), (4, 1 << 31, 8, 4, 1),
                          (-1, 10, 8, 4, 1), (4, 10, 8, 4, 1025), (4, 10, 8, 4, -1)):
        assert ws(N, M, K, k, s) == 0, (N, M, K, k, s)

    def call(N, M, K, k, splits=1):
        return L.jvae_knn_f32(None, None, None, None, None, None, N, M, K, k, 1, splits, None, None, 0, None)
    assert call(4, 10, 8, 0) == -2 and call(4, 10, 8, 65) == -2 and call(4, 10, 0, 4) == -2      # JVAE_ENOTSUP
    assert call(4, 10, 4097, 4) == -2 and call(4, 1 << 31, 8, 4) == -2
    assert call(-1, 10, 8, 4) == -1 and call(4, 10, 8, 4, 1025) == -1                             # JVAE_EINVAL
    assert call(4, 10, 8, 4) == -1                   # sizes in range, pointers missing: refused before any launch
    assert call(0, 10, 8, 4) == 0                    # nothing to do
    assert L.jvae_knn_sqnorms_f32(None, None, 5, 0, None) == -2 and L.jvae_knn_sqnorms_f32(None, None, 0, 8, None) == 0
    assert L.jvae_knn_sqnorms_f32(None, None, 5, 8, None) == -1


def test_ops_refuse_host_tensors_and_bad_sizes():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    x = torch.zeros(4, 8)
    with pytest.raises(JvaeHipError):
        ops.knn_bank(x)                               # no CPU path
    with pytest.raises(JvaeHipError):
        ops.knn(x, x, torch.zeros(4), 2)
    with pytest.raises(JvaeHipError):
        ops.knn_bank(torch.zeros(4, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match='query'):
        ops.knn_check_status(ops.KNN_STATUS_QUERY)
    with pytest.raises(ValueError, match='bank'):
        ops.knn_check_status(ops.KNN_STATUS_BANK)
    ops.knn_check_status(0)
