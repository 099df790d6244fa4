"""Host side of the aggregate-posterior density and the ELBO decomposition (the argument checks of ops.aggpost_bank /
aggpost_logdensity and of csrc/aggpost.hip, the stores and refusals of module/scoring.py, jvae_compat.inspection's table; DESIGN.md
section 7u).  No GPU: the model is built on the CPU, nothing is launched - the library's refusals and its workspace sizes are
host-only calls."""
import math

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from test_aggpost_restatement import P, STD_PRIOR, elbo_restatement, gaussian_prior, identical_bank, noise


def make_net(case='c1_n16_mlp'):
    from cvae import ClassificationVariationalNetwork as Net
    return Net(**dict(get_case(case)['net']))


def host_bank(N=70, K=16, seed=0):
    """A bank with ops.aggpost_bank's keys, dtypes and shapes, on the host."""
    g = torch.Generator().manual_seed(seed)
    mu, lv = torch.randn(N, K, generator=g), -3 * torch.rand(N, K, generator=g)
    Np = -(-N // 64) * 64
    pad = lambda t: torch.cat([t, torch.zeros(Np - N, K)]).t().contiguous()          # noqa: E731
    return {'mu': mu, 'log_var': lv, 'group': torch.randint(0, 10, (N,), generator=g).to(torch.int32), 'muT': pad(mu),
            'wT': pad((-lv.double()).exp().float()), 'lvT': pad(lv), 'c': torch.cat([lv.double().sum(1).float(), torch.zeros(Np - N)])}


def test_constants_and_the_partition():
    from jvae_hip import lib, ops
    assert (ops.AGGPOST_STATUS_BANK, ops.AGGPOST_STATUS_QUERY, ops.AGGPOST_STATUS_EMPTY) == (1, 2, 4)
    assert (ops.AGGPOST_MAX_K, ops.AGGPOST_MAX_BANK, ops.AGGPOST_MAX_PIECES) == (1024, 1 << 24, 1 << 14)
    assert ops.aggpost_partition() == P and ops.AGGPOST_MAX_BANK // P == ops.AGGPOST_MAX_PIECES
    h = lib.load()
    assert [h.jvae_aggpost_padded_rows(n) for n in (0, 1, 64, 65, 1 << 24, (1 << 24) + 1)] == [0, 64, 64, 128, 1 << 24, 0]
    assert h.jvae_aggpost_workspace_bytes(100, 2 * P + 3, 64, 0) == 3 * 100 * 12
    assert h.jvae_aggpost_workspace_bytes(100, 2 * P + 3, 64, 1) == 3 * 100 * 12 + 3 * 100 * 64 * 8
    for args in ((0, 5, 5, 0), (5, 0, 5, 0), (5, 5, 0, 1), (5, 5, 1025, 0), (5, (1 << 24) + 1, 5, 0), (1 << 31, 5, 5, 0)):
        assert h.jvae_aggpost_workspace_bytes(*args) == 0
    # the entry points refuse before any launch (no device is touched: the pointers are never read)
    assert h.jvae_aggpost_prepare_f32(None, None, None, None, None, None, 5, 5, None) == -1
    assert h.jvae_aggpost_prepare_f32(None, None, None, None, None, None, 5, 1025, None) == -2
    assert h.jvae_aggpost_prepare_f32(None, None, None, None, None, None, 0, 5, None) == -1
    assert h.jvae_aggpost_logdensity_f32(*[None] * 9, 5, 5, 1025, 0, None, None, 0, None) == -2
    assert h.jvae_aggpost_logdensity_f32(*[None] * 9, 5, 5, 5, 0, None, None, 0, None) == -1
    assert h.jvae_aggpost_logdensity_f32(*[None] * 9, -1, 5, 5, 0, None, None, 0, None) == -1
    assert h.jvae_aggpost_logdensity_f32(*[None] * 9, 0, 5, 5, 0, None, None, 0, None) == 0          # no queries: nothing to do


def test_bank_refusals():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    z = torch.zeros(4, 3)
    for mu, lv, group, why in ((z[0], z, None, r'mu \(N, K\)'), (z, z[:, :2], None, 'one shape'), (z.double(), z.double(), None, 'fp32'),
                               (z, z, torch.zeros(4), 'group'), (z, z, torch.zeros(3, dtype=torch.int32), 'group'),
                               (torch.zeros(2, 1025), torch.zeros(2, 1025), None, 'unsupported configuration'),
                               (torch.zeros(0, 3), torch.zeros(0, 3), None, 'unsupported configuration'), (None, z, None, r'mu \(N, K\)')):
        with pytest.raises(JvaeHipError, match=why):
            ops.aggpost_bank(mu, lv, group)
    with pytest.raises(JvaeHipError, match='resident on the GPU'):                        # well-formed, but on the host: no fallback
        ops.aggpost_bank(z, z)


def test_check_bank():
    from jvae_hip import ops
    bank = host_bank()
    assert ops.aggpost_check_bank(bank) == (70, 16)
    assert ops.aggpost_check_bank(dict(bank, extra=1), 'x') == (70, 16)
    for broken, why in (({k: v for k, v in bank.items() if k != 'c'}, 'keys'), (dict(bank, mu=bank['mu'].double()), 'mu'),
                        (dict(bank, log_var=bank['log_var'][:, :5]), 'log_var'), (dict(bank, group=bank['group'].long()), 'group'),
                        (dict(bank, muT=bank['mu']), 'muT'), (dict(bank, c=bank['c'][:70]), 'c'), (dict(bank, wT=None), 'wT'),
                        (dict(bank, mu=torch.zeros(2, 1025)), 'K <= 1024'), ([], 'keys')):
        with pytest.raises(ValueError, match=f'who: not a bank of aggpost_bank .*{why}'):
            ops.aggpost_check_bank(broken, 'who')


def test_logdensity_refusals_before_any_launch():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    bank = host_bank()
    z, g = torch.zeros(5, 16), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match='not a bank'):
        ops.aggpost_logdensity(z, {'mu': z})
    for args, kw, why in (((z[:, :15], bank), {}, r'z \(M, 16\)'), ((z[0], bank), {}, r'z \(M, 16\)'), ((z.double(), bank), {}, 'fp32'),
                          ((z, bank), dict(conditional=True), 'needs zgroup'), ((z, bank), dict(zgroup=g), 'conditional form only'),
                          ((z, bank), dict(zgroup=g[:4], conditional=True), 'needs zgroup'),
                          ((z, bank), dict(zgroup=g.float(), conditional=True), 'needs zgroup'),
                          ((z, bank), {}, 'resident on the GPU')):
        with pytest.raises(JvaeHipError, match=why):
            ops.aggpost_logdensity(*args, **kw)
    ops.aggpost_check_status(0)
    for bit, why in ((1, 'bank holds'), (2, 'non-finite element'), (4, 'no bank row'), (7, 'bank holds')):
        with pytest.raises(JvaeHipError, match=why):
            ops.aggpost_check_status(bit)


def test_the_store_round_trip_and_a_foreign_file(tmp_path):
    net = make_net()
    assert net.posterior_bank is None and net.POSTERIOR_BANK_FILE == 'posterior-bank.pth'
    assert net.ELBO_TYPES == ('cvae', 'xvae', 'vae', 'vib', 'jvae')
    with pytest.raises(ValueError, match='no bank is fitted'):
        net.save_posterior_bank(str(tmp_path))
    bank = dict(host_bank(), labels=torch.arange(70) % 10, set='train')
    net.posterior_bank = bank
    path = net.save_posterior_bank(str(tmp_path / 'a'))
    assert path == str(tmp_path / 'a' / 'posterior-bank.pth')
    other = make_net()
    got = other.load_posterior_bank(str(tmp_path / 'a'))
    assert got is other.posterior_bank and set(got) == set(bank) and got['set'] == 'train'
    assert all(torch.equal(got[k], bank[k]) and got[k].dtype == bank[k].dtype for k in bank if torch.is_tensor(bank[k]))
    # the latent bank is another store: neither reads the other's file
    latent = {'bank': bank['mu'], 'sq': bank['mu'].square().sum(1), 'labels': bank['labels'], 'set': 'train'}
    torch.save(latent, str(tmp_path / 'a' / 'latent-bank.pth'))
    assert set(other.load_latent_bank(str(tmp_path / 'a'))) == {'bank', 'sq', 'labels', 'set'}         # its exact key set, untouched
    for name, foreign in (('b', latent), ('c', dict(bank, extra=1)), ('d', {k: v for k, v in bank.items() if k != 'labels'}),
                          ('e', dict(bank, labels=bank['labels'][:5])), ('f', dict(bank, muT=bank['mu'])), ('g', [1, 2])):
        (tmp_path / name).mkdir()
        torch.save(foreign, str(tmp_path / name / 'posterior-bank.pth'))
        with pytest.raises(ValueError, match='does not hold a posterior bank'):
            other.load_posterior_bank(str(tmp_path / name))
    assert other.posterior_bank is got                                                   # a refused file changes nothing


def test_the_model_methods_refuse():
    net = make_net()
    for call in (lambda: net.elbo_decomposition(), lambda: net.aggregate_logdensity(torch.zeros(2, 16))):
        with pytest.raises(ValueError, match='no posterior bank is fitted'):
            call()
    with pytest.raises(ValueError, match='ratio'):
        net.fit_posterior_bank([], ratio=0.)
    coded = make_net('j2_n8_jvae')
    coded.posterior_bank = dict(host_bank(), labels=torch.zeros(70, dtype=torch.int64), set='s')
    for call in (lambda: coded.elbo_decomposition(), lambda: coded.aggregate_logdensity(torch.zeros(2, 16)),
                 lambda: coded.fit_posterior_bank([])):
        with pytest.raises(NotImplementedError, match='coded labels'):
            call()
    net.posterior_bank = dict(host_bank(), labels=torch.zeros(70, dtype=torch.int64), set='s')
    with pytest.raises(ValueError, match='samples'):
        net.elbo_decomposition(samples=0)
    with pytest.raises(ValueError, match='samples'):
        net.elbo_decomposition(samples=71)
    with pytest.raises(ValueError, match=r'epsilon \(70, 16\)'):
        net.elbo_decomposition(epsilon=torch.zeros(70, 15))
    with pytest.raises(ValueError, match=r'epsilon \(5, 16\)'):
        net.elbo_decomposition(samples=5, epsilon=torch.zeros(70, 16))


def test_the_table_as_text():
    from jvae_compat.inspection import elbo_decomposition_text
    bank = identical_bank()
    res = elbo_restatement(*bank, STD_PRIOR, noise(40, 5))
    text = elbo_decomposition_text(res)
    lines = text.splitlines()
    assert lines[0].split() == ['which', 'nats'] and [ln.split()[0] for ln in lines[1:10]] == ['kl', 'kl_mc', 'mi', 'mi_bound',
                                                                                            'kl_marginal', 'tc', 'dwkl', 'n', 'm']
    assert float(lines[1].split()[1]) == float(f'{res["kl"]:.7e}') and lines[8].split() == ['n', '40'] and lines[9].split() == ['m', '40']
    assert lines[10].split() == ['dim', 'dwkl'] and len(lines) == 11 + 5 and float(lines[11].split()[1]) == float(f'{res["dwkl_per_dim"][0]:.7e}')
    rng = np.random.default_rng(2)
    prior = gaussian_prior(rng.normal(0., 1., (3, 4)), np.tril(rng.normal(0., .3, (3, 4, 4))) + np.eye(4), 'full', True)
    labels = np.array([0] * 20 + [2] * 10)
    res = elbo_restatement(rng.normal(0., 1., (30, 4)), rng.uniform(-3., 0., (30, 4)), labels, prior, noise(30, 4))
    lines = elbo_decomposition_text(res).splitlines()
    names = [ln.split()[0] for ln in lines]
    assert names == ['which', 'kl', 'kl_mc', 'mi', 'mi_unconditional', 'mi_bound', 'kl_marginal', 'tc', 'n', 'm', 'class', '0', '2']
    assert lines[11].split()[:2] == ['0', '20'] and lines[12].split()[:2] == ['2', '10'] and math.isfinite(float(lines[12].split()[3]))
