"""Host side of the input-complexity OOD rows (module/scoring.py, module/score_rows.py, ops.image_code_length's and csrc/ic.hip's
argument checks).  No GPU: the model is built on the CPU, nothing is launched - the library's refusals are
host-only calls."""
import ctypes

import pytest
import torch

from oracle.cases import get_case

NAMES = ['ic-bits', 'ic-elbo', 'ic-iws']


def make_net(case='c1_n16_mlp'):
    from cvae import ClassificationVariationalNetwork as Net
    return Net(**dict(get_case(case)['net']))


def test_the_switch_is_off_by_default():
    net = make_net()
    assert net.OOD_IC_METHODS is False and tuple(net.IC_TYPES) == ('cvae', 'vae', 'xvae') and net._ic_names() == NAMES
    assert not any(m.startswith('ic') for m in net._ood_methods('all'))
    for m in NAMES + ['ic*', 'ic-bits-2s', 'ic-x', ['elbo', 'ic-elbo']]:
        with pytest.raises(NotImplementedError, match='OOD_IC_METHODS'):
            net._ood_methods(m)


def test_all_with_the_switch_off_is_the_table_without_the_family():
    from module import score_rows
    net = make_net()
    assert [f.prefix for f in score_rows.FAMILIES] == ['odin', 'regret', 'knn', 'maha', 'ic-', 'dose', 'ssim']
    ic = score_rows.FAMILIES[4]
    assert (ic.starred, ic.names, ic.scores, ic.args) == ('ic*', '_ic_names', 'ic_scores', ('x', 'losses'))
    assert all(ic.is_row(m) for m in NAMES) and not ic.is_row('ic-') and not ic.is_row('ic*') and not ic.is_row('ic-bits-2s')
    assert score_rows.claimed_by('ic-elbo') is ic and score_rows.claimed_by('ic*') is ic and score_rows.claimed_by('iws') is None
    with_family = net._ood_methods('all')
    families = score_rows.FAMILIES
    try:
        score_rows.FAMILIES = tuple(f for f in families if f is not ic)      # the table as it was before the family existed
        assert net._ood_methods('all') == with_family
    finally:
        score_rows.FAMILIES = families
    net.OOD_MAHA_METHODS = True
    assert net._ood_methods('all') == with_family + net._maha_names()


def test_the_switch_on_expands_the_names():
    net = make_net()
    before = net._ood_methods('all')
    net.OOD_IC_METHODS = True                        # per instance: the class stays off
    assert type(net).OOD_IC_METHODS is False
    assert net._ood_methods('all') == before + NAMES
    assert net._ood_methods('ic*') == NAMES
    assert net._ood_methods(['elbo', 'ic*']) == ['elbo'] + NAMES
    assert net._ood_methods('ic-iws') == ['ic-iws'] and net._ood_methods(['ic-elbo', 'iws']) == ['ic-elbo', 'iws']
    for unlisted in ('ic-bits-2s', 'ic-x', 'ic-'):   # a suffix on the hyphenated name: out of scope, as for `knn-<k>`
        with pytest.raises(ValueError, match='input-complexity rows'):
            net._ood_methods(unlisted)
    net.OOD_KNN_METHODS = net.OOD_MAHA_METHODS = True
    assert net._ood_methods('all') == before + net._knn_names() + net._maha_names() + NAMES      # the families' order


def test_models_without_a_decoder_are_refused():
    vib = make_net('b2_n8_vib')
    assert vib.type == 'vib'
    vib.OOD_IC_METHODS = True
    assert not any(m.startswith('ic') for m in vib._ood_methods('all'))
    for m in NAMES + ['ic*']:
        with pytest.raises(NotImplementedError, match='IC_TYPES'):
            vib._ood_methods(m)
    with pytest.raises(NotImplementedError, match='vib'):
        vib.ic_scores(torch.zeros(2, *vib.input_shape), {})
    coded = make_net('j2_n8_jvae')
    assert coded.y_is_coded
    with pytest.raises(NotImplementedError, match='coded'):
        coded.ic_scores(torch.zeros(2, *coded.input_shape), {})


def test_score_rows_know_the_names_with_the_trait_only():
    from module import score_rows
    off = score_rows.Traits(True, False, False, 10)
    assert off.OOD_IC_METHODS is False and score_rows.Traits._field_defaults['OOD_IC_METHODS'] is False
    for name in NAMES:
        with pytest.raises(NotImplementedError):
            score_rows.parse(name, off)
    on = off._replace(OOD_IC_METHODS=True)
    row = score_rows.parse('ic-elbo', on)
    assert (row.name, row.base, row.source, row.kind, row.const, row.roc_mode) == ('ic-elbo', 'ic-elbo', 'ic-elbo', None, None, False)
    v = torch.arange(4.)
    assert row.torch_row({'ic-elbo': v}) is v        # a recorded row: read as it is
    with pytest.raises(NotImplementedError):
        score_rows.parse('ic-x', on)
    assert score_rows.recorded_by('ic-bits').prefix == 'ic-' and score_rows.recorded_by('ic') is None
    net = make_net()
    assert score_rows.traits_of(net).OOD_IC_METHODS is False
    net.OOD_IC_METHODS = True
    assert score_rows.traits_of(net).OOD_IC_METHODS is True


def test_library_exports_and_host_only_refusals():
    from jvae_hip import lib
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, 'jvae_image_code_length_f32') and 'jvae_image_code_length_f32' in lib.exported_symbols()
    L = lib.load()

    def call(N, C, H, W, table_len, pointers=False):
        buf = (ctypes.c_double * 8)()
        p = ctypes.cast(buf, ctypes.c_void_p) if pointers else None
        return L.jvae_image_code_length_f32(p, N, C, H, W, p, table_len, p, p, p, p, None)
    big = (1 << 20) + 257
    for args in ((4, 5, 8, 8), (4, 0, 8, 8), (4, 3, 0, 8), (4, 3, 8, 0), (4, 1, 1025, 1024), (4, 1, 1 << 20, 2), (1 << 31, 3, 8, 8)):
        assert call(*args, big) == -2 and call(*args, big, pointers=True) == -2, args       # JVAE_ENOTSUP, whatever else is wrong
    assert call(4, 3, 8, 8, 64 + 256) == -1 and call(4, 3, 8, 8, 64 + 256, pointers=True) == -1          # a short table: JVAE_EINVAL
    assert call(4, 1, 1024, 1024, big - 1, pointers=True) == -1
    assert call(-1, 3, 8, 8, big) == -1
    assert call(4, 3, 8, 8, 64 + 257) == -1          # sizes in range, pointers missing: refused before any launch
    assert call(4, 1, 1024, 1024, big) == -1
    assert call(0, 3, 8, 8, 64 + 257) == 0           # nothing to do


def test_ops_refuse_before_any_launch():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    assert (ops.IC_MAX_CHANNELS, ops.IC_MAX_PIXELS, ops.IC_STATUS_INEXACT, ops.IC_STATUS_NONFINITE) == (4, 1 << 20, 1, 2)
    with pytest.raises(JvaeHipError, match='GPU'):
        ops.image_code_length(torch.zeros(2, 3, 8, 8))           # no CPU path
    with pytest.raises(JvaeHipError, match='fp32'):
        ops.image_code_length(torch.zeros(2, 3, 8, 8, dtype=torch.float64))
    with pytest.raises(JvaeHipError, match=r'\(N, C, H, W\)'):
        ops.image_code_length(torch.zeros(3, 8, 8))
    for shape in ((2, 5, 8, 8), (2, 0, 8, 8), (2, 3, 0, 8), (2, 1, 1025, 1024)):
        with pytest.raises(JvaeHipError, match='unsupported configuration'):
            ops.image_code_length(torch.zeros(shape))
    with pytest.raises(ValueError, match='non-finite'):
        ops.ic_check_status(ops.IC_STATUS_NONFINITE)
    with pytest.raises(ValueError, match='non-finite'):
        ops.ic_check_status(ops.IC_STATUS_NONFINITE | ops.IC_STATUS_INEXACT)
    assert ops.ic_check_status(ops.IC_STATUS_INEXACT) == ops.IC_STATUS_INEXACT and ops.ic_check_status(0) == 0
    word = torch.tensor([ops.IC_STATUS_INEXACT], dtype=torch.int32)
    assert ops.ic_check_status(word) == 1 and int(word) == 0     # read and cleared
    table = ops.ic_table(64)
    assert table.dtype == torch.float64 and table.shape == (64 + 257,) and ops.ic_table(64) is table
