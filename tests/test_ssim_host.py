"""Host side of the SSIM OOD rows (module/scoring.py, module/score_rows.py, ops.ssim's and csrc/ssim.hip's argument checks;
DESIGN.md section 7t).  No GPU: the model is built on the CPU, nothing is launched - the library's refusals are host-only calls."""
import ctypes
import inspect
import os

import pytest
import torch

from oracle.cases import get_case

NAMES = ['ssim', 'ssim-mu', 'ssim-cs']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_net(case='c1_n16_mlp', **over):
    from cvae import ClassificationVariationalNetwork as Net
    return Net(**dict(get_case(case)['net'], **over))


def test_the_switch_is_off_by_default():
    net = make_net()
    assert net.OOD_SSIM_METHODS is False and tuple(net.SSIM_TYPES) == ('cvae', 'vae', 'xvae') and net._ssim_names() == NAMES
    assert not any(m.startswith('ssim') for m in net._ood_methods('all'))
    for m in NAMES + ['ssim*', 'ssim-2s', 'ssim-x', 'ssim-', ['elbo', 'ssim-mu']]:
        with pytest.raises(NotImplementedError, match='OOD_SSIM_METHODS'):
            net._ood_methods(m)


def test_the_tables():
    from module import score_rows
    assert [f.prefix for f in score_rows.FAMILIES] == ['odin', 'regret', 'knn', 'maha', 'ic-', 'dose', 'ssim']
    ssim = score_rows.FAMILIES[6]
    assert (ssim.starred, ssim.names, ssim.scores, ssim.args) == ('ssim*', '_ssim_names', 'ssim_scores', ('x', 'x_reco'))
    assert all(ssim.is_row(m) for m in NAMES) and not any(ssim.is_row(m) for m in ('ssim-', 'ssim*', 'ssim-2s', 'ssim-x', 'ssimx'))
    assert score_rows.claimed_by('ssim-mu') is ssim and score_rows.claimed_by('ssim*') is ssim and score_rows.claimed_by('mse') is None
    assert score_rows.recorded_by('ssim-cs') is ssim and score_rows.recorded_by('ssim-2s') is None
    table = score_rows.FAMILIES                                # the table is read at the call
    try:
        score_rows.FAMILIES = tuple(f for f in table if f is not ssim)
        assert score_rows.FAMILIES == table[:6] and score_rows.claimed_by('ssim') is None
    finally:
        score_rows.FAMILIES = table


def test_all_with_the_switch_off_is_the_table_without_the_family():
    from module import score_rows
    net = make_net()
    with_family = net._ood_methods('all')
    table = score_rows.FAMILIES
    try:
        score_rows.FAMILIES = tuple(f for f in table if f.prefix != 'ssim')      # the table as it was before the family existed
        assert net._ood_methods('all') == with_family
    finally:
        score_rows.FAMILIES = table


def test_the_switch_on_expands_the_names_behind_the_other_families():
    net = make_net()
    before = net._ood_methods('all')
    net.OOD_SSIM_METHODS = True                      # per instance: the class stays off
    assert type(net).OOD_SSIM_METHODS is False
    assert net._ood_methods('all') == before + NAMES
    assert net._ood_methods('ssim*') == NAMES
    assert net._ood_methods(['elbo', 'ssim*']) == ['elbo'] + NAMES
    assert net._ood_methods('ssim-mu') == ['ssim-mu'] and net._ood_methods(['ssim', 'iws']) == ['ssim', 'iws']
    for unlisted in ('ssim-2s', 'ssim-x', 'ssim-'):  # a suffix on these names: out of scope, as for `ic-bits-2s`
        with pytest.raises(ValueError, match='SSIM rows'):
            net._ood_methods(unlisted)
    net.OOD_KNN_METHODS = net.OOD_MAHA_METHODS = net.OOD_IC_METHODS = net.OOD_DOSE_METHODS = True
    assert net._ood_methods('all') == before + net._knn_names() + net._maha_names() + net._ic_names() + net._dose_names() + NAMES
    net.OOD_REGRET_METHODS = True
    assert net._ood_methods('all') == (before + net._regret_names() + net._knn_names() + net._maha_names() + net._ic_names()
                                       + net._dose_names() + NAMES)


def test_traits_default_field_order_and_parse():
    from module import score_rows
    off = score_rows.Traits(True, False, False, 10)  # the four-argument positional constructor
    assert off.OOD_SSIM_METHODS is False and score_rows.Traits._field_defaults['OOD_SSIM_METHODS'] is False
    assert score_rows.Traits._fields[:4] == ('losses_might_be_computed_for_each_class', 'is_vae', 'is_jvae', 'num_labels')
    assert score_rows.Traits._fields[-2:] == ('OOD_DOSE_METHODS', 'OOD_MAHA_METHODS')
    assert not any(off[4:])
    for name in NAMES:
        with pytest.raises(NotImplementedError):
            score_rows.parse(name, off)
    on = off._replace(OOD_SSIM_METHODS=True)
    row = score_rows.parse('ssim-cs', on)
    assert (row.name, row.base, row.source, row.kind, row.const, row.roc_mode) == ('ssim-cs', 'ssim-cs', 'ssim-cs', None, None, False)
    v = torch.arange(4.)
    assert row.torch_row({'ssim-cs': v}) is v        # a recorded row: read as it is
    with pytest.raises(NotImplementedError):
        score_rows.parse('ssim-x', on)
    net = make_net()
    assert score_rows.traits_of(net).OOD_SSIM_METHODS is False
    net.OOD_SSIM_METHODS = True
    assert score_rows.traits_of(net).OOD_SSIM_METHODS is True


def test_models_that_decode_no_image_are_refused():
    vib = make_net('b2_n8_vib')
    assert vib.type == 'vib'
    vib.OOD_SSIM_METHODS = True
    assert not any(m.startswith('ssim') for m in vib._ood_methods('all'))
    for m in NAMES + ['ssim*']:
        with pytest.raises(NotImplementedError, match='SSIM_TYPES'):
            vib._ood_methods(m)

    def refused(net, match):
        x = torch.zeros(2, *net.input_shape)
        with pytest.raises(NotImplementedError, match=match):
            net.ssim_scores(x, torch.zeros(3, *x.shape))
        with pytest.raises(NotImplementedError, match=match):
            net.ssim_map(x)
    refused(vib, 'vib')
    coded = make_net('j2_n8_jvae')
    assert coded.y_is_coded
    refused(coded, 'coded')
    categorical = make_net('g2_n4_categorical')
    assert categorical.output_distribution == 'categorical'
    refused(categorical, 'categorical')
    vector = make_net(input_shape=(784,))            # the MLP on a flat input
    assert tuple(vector.input_shape) == (784,)
    refused(vector, r'\(784,\)')
    small = make_net(input_shape=(1, 10, 28))        # an image below the window
    refused(small, r'\(1, 10, 28\)')
    with pytest.raises(Exception, match='GPU'):      # an image model passes the refusals and reaches the op: no CPU path
        make_net().ssim_scores(torch.zeros(2, 1, 28, 28), torch.zeros(3, 2, 1, 28, 28))


def test_with_reco_is_in_both_signatures():
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.wim import WIMJob
    for cls in (Net, WIMJob):
        p = inspect.signature(cls._evaluate_for_scores).parameters
        assert list(p)[-2:] == ['with_mu', 'with_reco'] and p['with_reco'].default is False and p['with_mu'].default is False


def test_library_exports_and_host_only_refusals():
    from jvae_hip import lib
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, 'jvae_ssim_f32') and 'jvae_ssim_f32' in lib.exported_symbols()
    with open(os.path.join(ROOT, 'include', 'jvae_hip.h')) as f:
        assert 'int jvae_ssim_f32(const float* x, const float* y, long N, long R, int C, int H, int W,' in f.read()
    L = lib.load()
    buf = (ctypes.c_double * 8)()
    there = ctypes.cast(buf, ctypes.c_void_p)

    def call(N, R, C, H, W, pointers=False, skip=None):
        p = [there if pointers and i != skip else None for i in range(6)]        # x, y, ssim, cs, map, status
        return L.jvae_ssim_f32(p[0], p[1], N, R, C, H, W, p[2], p[3], p[4], p[5], None)
    # JVAE_ENOTSUP whatever else is wrong: the window does not fit, no channel, beyond the staged width / the row count
    for args in ((4, 2, 3, 10, 32), (4, 2, 3, 32, 10), (4, 2, 3, 10, 10), (4, 2, 0, 32, 32), (4, 2, -1, 32, 32), (4, 2, 3, 32, 129),
                 (4, 2, 3, 32769, 32), (1 << 31, 2, 3, 32, 32), (4, 1 << 31, 3, 32, 32)):
        assert call(*args) == -2 and call(*args, pointers=True) == -2, args
    # the last supported sizes, pointers missing: JVAE_EINVAL, so the sizes passed
    for args in ((4, 2, 3, 11, 11), (4, 2, 1, 11, 128), (4, 2, 3, 32768, 11), (4, 2, 1000, 32, 32)):
        assert call(*args) == -1, args
    assert call(-1, 2, 3, 32, 32) == -1 and call(4, -1, 3, 32, 32) == -1 and call(-1, 2, 3, 32, 32, pointers=True) == -1
    for skip in (0, 1, 2, 3, 5):                     # every pointer but the map's is needed
        assert call(4, 2, 3, 32, 32, pointers=True, skip=skip) == -1, skip
    assert call(0, 2, 3, 32, 32) == 0 and call(4, 0, 3, 32, 32) == 0 and call(0, 0, 3, 32, 32) == 0     # nothing to do
    assert call(0, 2, 3, 10, 32) == -2               # ... but a refused shape is refused first
    # the strips: at W = 32 a strip holds 38 output rows, so H = 48 is one strip and H = 49 two
    assert L.jvae_ssim_strip_rows(48, 32) == 38 and L.jvae_ssim_strip_rows(49, 32) == 38 and L.jvae_ssim_strip_rows(32, 32) == 22
    assert L.jvae_ssim_strip_rows(11, 11) == 1 and L.jvae_ssim_strip_rows(64, 64) == 12 and L.jvae_ssim_strip_rows(4096, 128) == 7
    assert L.jvae_ssim_strip_rows(10, 32) == 0 and L.jvae_ssim_strip_rows(32, 129) == 0 and L.jvae_ssim_strip_rows(32769, 32) == 0


def test_ops_refuse_before_any_launch():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    assert (ops.SSIM_WINDOW, ops.SSIM_MAX_W, ops.SSIM_MAX_H, ops.SSIM_STATUS_X, ops.SSIM_STATUS_Y) == (11, 128, 32768, 1, 2)
    x, y = torch.zeros(2, 3, 16, 16), torch.zeros(4, 2, 3, 16, 16)
    with pytest.raises(JvaeHipError, match='GPU'):
        ops.ssim(x, y)                                           # no CPU path
    with pytest.raises(JvaeHipError, match='fp32'):
        ops.ssim(x.double(), y)
    with pytest.raises(JvaeHipError, match='fp32'):
        ops.ssim(x, y.double())
    for bad_x, bad_y in ((x[0], y), (x, y[0]), (x, y[:, :1]), (x, y[..., :15]), (x, None)):
        with pytest.raises(JvaeHipError, match=r'\(R, N, C, H, W\)'):
            ops.ssim(bad_x, bad_y)
    for shape in ((2, 3, 10, 16), (2, 3, 16, 10), (2, 0, 16, 16), (2, 1, 16, 129)):
        with pytest.raises(JvaeHipError, match='unsupported configuration'):
            ops.ssim(torch.zeros(shape), torch.zeros((3,) + shape))
    for ok in ((2, 1, 11, 128), (2, 1, 11, 11)):                 # the other side of the limits: refused for the device alone
        with pytest.raises(JvaeHipError, match='GPU'):
            ops.ssim(torch.zeros(ok), torch.zeros((3,) + ok))
    with pytest.raises(ValueError, match='image with a non-finite'):
        ops.ssim_check_status(ops.SSIM_STATUS_X)
    with pytest.raises(ValueError, match='image with a non-finite'):
        ops.ssim_check_status(ops.SSIM_STATUS_X | ops.SSIM_STATUS_Y)
    with pytest.raises(ValueError, match='reconstruction with a non-finite'):
        ops.ssim_check_status(ops.SSIM_STATUS_Y)
    assert ops.ssim_check_status(0) == 0
    word = torch.tensor([ops.SSIM_STATUS_Y], dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.ssim_check_status(word)
    assert int(word) == 0                                        # read and cleared
    assert ops.ssim_strip_rows(48, 32) == 38 and ops.ssim_strip_rows(10, 32) == 0
