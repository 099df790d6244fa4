"""Host side of the density-of-states OOD rows (module/scoring.py, module/score_rows.py, the argument checks of ops.kde_fit /
ops.kde_logdensity and of csrc/dose.hip).  No GPU: the model is built on the CPU, nothing is launched - the
library's refusals and its workspace sizes are host-only calls."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from test_dose_restatement import dose_case, fit_restatement


def make_net(case='c1_n16_mlp'):
    from cvae import ClassificationVariationalNetwork as Net
    return Net(**dict(get_case(case)['net']))


def host_fit(S=3, M=40, bandwidth=1.0):
    """A fit with ops.kde_fit's keys, dtypes and shapes from the fp64 restatement, on the host."""
    _, bank = dose_case(S, M, 4)
    f = fit_restatement(bank, bandwidth)
    z = ((bank.astype(np.float64) - f['centre'][:, None]) / f['h1'][:, None]).astype(np.float32)
    return dict({k: torch.from_numpy(f[k]) for k in ('centre', 'sigma', 'h1', 'hS', 'lognorm')}, z=torch.from_numpy(z), M=M, S=S,
                bandwidth=float(bandwidth))


DEFAULT_NAMES = ['dose', 'dose-joint', 'dose-elbo', 'dose-iws', 'dose-kl', 'dose-zdist', 'dose-mse', 'dose-typ-elbo',
                 'dose-typ-iws', 'dose-typ-kl', 'dose-typ-zdist', 'dose-typ-mse']


def test_the_switch_is_off_by_default():
    net = make_net()
    assert net.OOD_DOSE_METHODS is False and net.score_bank is None and net.SCORE_BANK_FILE == 'score-bank.pth'
    assert net.DOSE_BANDWIDTH == 1.0 and net.DOSE_TYPES == ('cvae', 'vae', 'xvae', 'vib')
    assert net.DOSE_STATS == ('elbo', 'iws', 'kl', 'zdist', 'mse') and make_net('b2_n8_vib').DOSE_STATS == ('kl', 'zdist', 'logits')
    table = net._ood_methods('all')
    assert not any(m.startswith('dose') for m in table)
    for m in ('dose*', 'dose', 'dose-joint', 'dose-elbo', 'dose-typ-kl', 'dose-2s', 'dosed', ['elbo', 'dose']):
        with pytest.raises(NotImplementedError, match='OOD_DOSE_METHODS'):
            net._ood_methods(m)


def test_the_family_in_the_table():
    from module import score_rows
    assert [f.prefix for f in score_rows.FAMILIES] == ['odin', 'regret', 'knn', 'maha', 'ic-', 'dose', 'ssim']
    dose = score_rows.FAMILIES[5]
    assert (dose.starred, dose.names, dose.scores, dose.args) == ('dose*', '_dose_names', 'dose_scores', ('logits', 'losses'))
    assert dose.is_row('dose') and dose.is_row('dose-joint') and dose.is_row('dose-typ-kl') and not dose.is_row('dosed')
    assert score_rows.claimed_by('dose*') is dose and score_rows.claimed_by('dose-kl') is dose
    assert score_rows.recorded_by('dose-kl') is dose and score_rows.recorded_by('elbo') is None
    # the table is read at the call
    table = score_rows.FAMILIES
    try:
        score_rows.FAMILIES = tuple(f for f in table if f is not dose)
        assert score_rows.FAMILIES == table[:5] + table[6:] and score_rows.claimed_by('dose') is None
    finally:
        score_rows.FAMILIES = table


def test_all_with_the_switch_off_is_the_table_without_the_family():
    from module import score_rows
    net = make_net()
    with_family = net._ood_methods('all')
    table = score_rows.FAMILIES
    try:
        score_rows.FAMILIES = tuple(f for f in table if f.prefix != 'dose')
        assert net._ood_methods('all') == with_family
    finally:
        score_rows.FAMILIES = table


def test_the_switch_on_expands_the_names_behind_the_other_families():
    net = make_net()
    before = net._ood_methods('all')
    net.OOD_DOSE_METHODS = True                      # per instance: the class stays off
    assert type(net).OOD_DOSE_METHODS is False
    assert net._dose_names() == DEFAULT_NAMES
    assert net._ood_methods('all') == before + DEFAULT_NAMES
    assert net._ood_methods('dose*') == DEFAULT_NAMES
    assert net._ood_methods(['elbo', 'dose*']) == ['elbo'] + DEFAULT_NAMES
    assert net._ood_methods('dose-typ-kl') == ['dose-typ-kl'] and net._ood_methods('dose') == ['dose']
    for unlisted in ('dose-logits', 'dose-typ', 'dosed', 'dose-2s', 'dose-typ-logits'):      # `-2s` on these names: out of scope
        with pytest.raises(ValueError, match='density-of-states rows'):
            net._ood_methods(unlisted)
    net.OOD_KNN_METHODS = net.OOD_MAHA_METHODS = net.OOD_IC_METHODS = True
    assert net._ood_methods('all') == before + net._knn_names() + net._maha_names() + net._ic_names() + DEFAULT_NAMES
    vib = make_net('b2_n8_vib')
    vib.OOD_DOSE_METHODS = True
    names = ['dose', 'dose-joint', 'dose-kl', 'dose-zdist', 'dose-logits', 'dose-typ-kl', 'dose-typ-zdist', 'dose-typ-logits']
    assert vib._ood_methods('dose*') == names and vib._ood_methods('all')[-len(names):] == names
    vib.DOSE_TYPES = ('cvae',)                       # a type outside DOSE_TYPES: the family is off
    with pytest.raises(NotImplementedError, match='OOD_DOSE_METHODS'):
        vib._ood_methods('dose')


def test_one_statistic_has_no_joint_row():
    net = make_net()
    net.OOD_DOSE_METHODS = True
    net.DOSE_STATS = ('kl',)
    assert net.DOSE_STATS == ('kl',) and make_net().DOSE_STATS == ('elbo', 'iws', 'kl', 'zdist', 'mse')
    assert net._dose_names() == ['dose', 'dose-kl', 'dose-typ-kl'] == net._ood_methods('dose*')
    with pytest.raises(ValueError, match='density-of-states rows'):
        net._ood_methods('dose-joint')
    net.DOSE_STATS = ['zdist', 'kl']                 # a list is taken as a tuple, in its order
    assert net._dose_names() == ['dose', 'dose-joint', 'dose-zdist', 'dose-kl', 'dose-typ-zdist', 'dose-typ-kl']
    net.DOSE_STATS = None                            # back to the type's default
    assert net._dose_names() == DEFAULT_NAMES


def test_traits_default_and_parse():
    from module import score_rows
    off = score_rows.Traits(True, False, False, 10)
    assert off.OOD_DOSE_METHODS is False and score_rows.Traits._field_defaults['OOD_DOSE_METHODS'] is False
    assert score_rows.Traits._fields[-2:] == ('OOD_DOSE_METHODS', 'OOD_MAHA_METHODS')
    for name in ('dose', 'dose-joint', 'dose-typ-kl'):
        with pytest.raises(NotImplementedError):
            score_rows.parse(name, off)
    on = off._replace(OOD_DOSE_METHODS=True)
    row = score_rows.parse('dose-typ-kl', on)
    assert (row.name, row.base, row.source, row.kind, row.const, row.roc_mode) == ('dose-typ-kl', 'dose-typ-kl', 'dose-typ-kl', None,
                                                                                   None, False)
    v = torch.arange(4.)
    assert row.torch_row({'dose-typ-kl': v}) is v    # a recorded row: read as it is
    net = make_net()
    assert score_rows.traits_of(net).OOD_DOSE_METHODS is False
    net.OOD_DOSE_METHODS = True
    assert score_rows.traits_of(net).OOD_DOSE_METHODS is True


@pytest.mark.parametrize('stats', [('elbo', 'soft-10'), ('kl', 'joint'), ('typ',), ('kl', 'knn-1'), ('dose',), ('kl', 'nonsense'),
                                   ('zdist~',), (), ('kl', 'kl'), ('odin',), tuple('elbo iws kl zdist mse max soft sum mean'.split()),
                                   ('kl', 3)])
def test_dose_stats_are_validated_at_fit(stats):
    net = make_net()
    net.DOSE_STATS = stats
    with pytest.raises(ValueError, match='DOSE_STATS'):
        net.fit_score_bank([])
    with pytest.raises(ValueError, match='DOSE_STATS'):
        net._dose_stat_rows()


def test_scoring_and_saving_need_a_bank():
    net = make_net()
    assert [r.name for r in net._dose_stat_rows()] == list(net.DOSE_STATS)
    assert [(r.source, r.kind) for r in net._dose_stat_rows()] == [('total', 'max-'), ('iws', 'lse+'), ('kl', 'max-'), ('zdist', 'max-'),
                                                                   ('cross_x', 'neg')]
    # a vib's kl and zdist have no class axis: minus the loss, as for a vae
    assert [(r.source, r.kind) for r in make_net('b2_n8_vib')._dose_stat_rows()] == [('kl', 'neg'), ('zdist', 'neg'), ('logits', 'max+')]
    with pytest.raises(ValueError, match='fit_score_bank'):
        net.dose_scores(None, {})
    with pytest.raises(ValueError, match='fit_score_bank'):
        net.save_score_bank('nowhere')
    with pytest.raises(ValueError, match='ratio'):
        net.fit_score_bank([], ratio=0.)
    net.score_bank = dict(host_fit(S=2), stats=('kl', 'zdist'), set='s')
    with pytest.raises(ValueError, match='DOSE_STATS'):
        net.dose_scores(None, {})


def test_score_bank_file_round_trip_on_the_host(tmp_path):
    net = make_net()
    fit = host_fit(S=5, M=60, bandwidth=0.5)
    net.score_bank = dict(fit, stats=net.DOSE_STATS, set='demo')
    path = net.save_score_bank(str(tmp_path / 'job'))
    assert path.endswith('score-bank.pth') and [p.name for p in (tmp_path / 'job').iterdir()] == ['score-bank.pth']
    other = make_net()
    got = other.load_score_bank(str(tmp_path / 'job'))
    assert got is other.score_bank and got['set'] == 'demo' and got['bandwidth'] == 0.5 and set(got) == set(fit) | {'stats', 'set'}
    assert got['stats'] == other.DOSE_STATS and (got['M'], got['S']) == (60, 5)
    assert all(torch.equal(got[k], fit[k]) and got[k].dtype == fit[k].dtype for k in fit if torch.is_tensor(fit[k]))
    third = make_net()
    third.DOSE_STATS = ('kl', 'zdist', 'mse', 'elbo', 'iws')
    with pytest.raises(ValueError, match='DOSE_STATS'):
        third.load_score_bank(str(tmp_path / 'job'))
    # the load validates keys, dtypes and shapes
    bank = net.score_bank
    for broken in ({k: v for k, v in bank.items() if k != 'hS'}, dict(bank, extra=1), dict(bank, z=fit['z'].double()),
                   dict(bank, z=fit['z'][:, :5]), dict(bank, lognorm=fit['lognorm'][:5]), dict(bank, centre=fit['centre'].float()),
                   dict(bank, bandwidth='1'), dict(bank, M=60.), dict(bank, S=9), dict(bank, stats=list(bank['stats'])),
                   dict(bank, stats=bank['stats'][:4]), [1, 2]):
        torch.save(broken, str(tmp_path / 'job' / 'score-bank.pth'))
        with pytest.raises(ValueError, match='load_score_bank'):
            other.load_score_bank(str(tmp_path / 'job'))


def test_library_exports_and_host_only_refusals():
    from jvae_hip import lib
    handle = ctypes.CDLL(lib.LIB_PATH)
    names = ('jvae_kde_partition', 'jvae_kde_fit_workspace_bytes', 'jvae_kde_fit_f32', 'jvae_kde_workspace_bytes',
             'jvae_kde_logdensity_f32')
    header = open(lib.LIB_PATH.rsplit('joint-vae_amd', 1)[0] + 'include/jvae_hip.h').read()
    for name in names:
        assert hasattr(handle, name) and name in lib.exported_symbols() and name + '(' in header
    L = lib.load()
    P = L.jvae_kde_partition()
    assert P == 1024
    fit_ws, ws = L.jvae_kde_fit_workspace_bytes, L.jvae_kde_workspace_bytes
    # one fp64 partial per statistic and slab of 4096 values; one (exponent, sum) pair per query, row and piece of the bank
    assert fit_ws(2, 1) == 8 and fit_ws(4096, 5) == 40 and fit_ws(4097, 5) == 80 and fit_ws(50000, 8) == 8 * 8 * 13
    assert ws(1, 2, 1) == 16 and ws(100, 50000, 5) == 49 * 6 * 100 * 8 and ws(7, P + 1, 8) == 2 * 9 * 7 * 8
    for M, S in ((1, 3), (0, 3), (5, 0), (5, 9), ((1 << 24) + 1, 3), (-1, 3)):
        assert fit_ws(M, S) == 0 and ws(4, M, S) == 0, (M, S)
    assert ws(0, 5, 3) == 0 and ws(1 << 31, 5, 3) == 0 and ws(-1, 5, 3) == 0

    def fit(M, S, bw=1., s1=0.5, sS=0.5):
        factors = (ctypes.c_double * 3)(bw, s1, sS)    # read on the host by the call
        return L.jvae_kde_fit_f32(None, M, S, factors, None, None, None, None, None, None, None, None, 0, None)

    def score(N, M, S, r2=1.):
        return L.jvae_kde_logdensity_f32(None, None, None, None, None, None, None, N, M, S, ctypes.byref(ctypes.c_double(r2)), None,
                                         None, 0, None)
    assert L.jvae_kde_fit_f32(None, 5, 3, None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert fit(5, 9) == -2 and fit((1 << 24) + 1, 3) == -2                                                  # JVAE_ENOTSUP
    assert fit(1, 3) == -1 and fit(5, 0) == -1 and fit(5, 3, bw=0.) == -1 and fit(5, 3, s1=float('nan')) == -1      # JVAE_EINVAL
    assert fit(5, 3) == -1                           # sizes in range, pointers missing: refused before any launch
    assert score(4, 5, 9) == -2 and score(4, (1 << 24) + 1, 3) == -2 and score(1 << 31, 5, 3) == -2
    assert score(-1, 5, 3) == -1 and score(4, 1, 3) == -1 and score(4, 5, 0) == -1 and score(4, 5, 3, r2=0.) == -1
    assert score(4, 5, 3) == -1 and score(0, 5, 3) == 0                                                     # nothing to do


def test_ops_refuse_before_any_launch():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    assert ops.DOSE_MAX_STATS == 8 and ops.DOSE_STATUS_QUERY == 1 << 16 and ops.kde_partition() == 1024
    assert ops.kde_scott(32, 1) == 0.5 and ops.kde_scott(4096, 8) == 0.5
    bank = torch.zeros(3, 6)
    with pytest.raises(JvaeHipError, match='GPU'):
        ops.kde_fit(bank)                            # no CPU path
    with pytest.raises(JvaeHipError, match='fp32'):
        ops.kde_fit(bank.double())
    with pytest.raises(JvaeHipError, match=r'\(S, M\)'):
        ops.kde_fit(bank[0])
    for b in (torch.zeros(9, 6), torch.zeros(0, 6)):
        with pytest.raises(JvaeHipError, match='unsupported configuration'):
            ops.kde_fit(b)
    with pytest.raises(ValueError, match='two samples'):
        ops.kde_fit(bank[:, :1])
    for bw in (0., -1., float('inf'), float('nan')):
        with pytest.raises(ValueError, match='bandwidth'):
            ops.kde_fit(bank, bw)
    fit = host_fit(S=3, M=40)
    assert ops.kde_check_fit(fit) == (3, 40) and set(fit) == set(ops.DOSE_FIT_KEYS)
    with pytest.raises(JvaeHipError, match='GPU'):
        ops.kde_logdensity(torch.zeros(3, 4), fit)   # no CPU path
    with pytest.raises(JvaeHipError, match=r'\(3, N\)'):
        ops.kde_logdensity(torch.zeros(4, 4), fit)
    with pytest.raises(JvaeHipError, match=r'\(3, N\)'):
        ops.kde_logdensity(torch.zeros(3), fit)
    with pytest.raises(JvaeHipError, match='fp32'):
        ops.kde_logdensity(torch.zeros(3, 4, dtype=torch.float64), fit)
    with pytest.raises(ValueError, match='kde_fit'):
        ops.kde_logdensity(torch.zeros(3, 4), {k: v for k, v in fit.items() if k != 'z'})
    with pytest.raises(ValueError, match='h1'):
        ops.kde_logdensity(torch.zeros(3, 4), dict(fit, h1=fit['h1'].float()))
    with pytest.raises(ValueError, match='who'):
        ops.kde_check_fit(dict(fit, M=41), 'who')
    with pytest.raises(JvaeHipError, match='non-finite'):
        ops.kde_check_status(ops.DOSE_STATUS_QUERY)
    ops.kde_check_status(0)
