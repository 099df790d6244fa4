"""The aggregate-posterior density and the ELBO decomposition on the MI355X (ops.aggpost_bank / aggpost_logdensity,
csrc/aggpost.hip, net.fit_posterior_bank / aggregate_logdensity / elbo_decomposition) against the fp64
restatement and the DERIVED bound of tests/test_aggpost_restatement.py: |error| <= 2^-24 B(case) on every output of every case,
none excluded; every output finite for finite queries (an unshifted fp32 sum gives -inf at 10^4 sigma).  Every figure is printed
before its assertion.

Measured error / bound on the MI355X (worst output of a case, logq / logq_dims; whole bank | conditional): K1 N1 M1 0.010 / 0.007
| the same; K3 N2 M64 0.18 / 0.32 | the same; K64 N63 M65 0.19 / 0.56 | 0.19 / 0.63; K65 N64 M129 0.18 / 0.59 | 0.18 / 0.63; K200
N65 M64 0.24 / 0.58 | 0.24 / 0.57; K3 N1023 M65 0.14 / 0.52 | 0.31 / 0.67; K64 N1024 M64 0.19 / 0.76 | 0.19 / 0.74; K65 N1025 M129
0.14 / 0.71 | the same; K200 N2051 M65 0.24 / 0.69 | 0.24 / 0.75; K64 N2051 M129 with an empty group 0.17 / 0.71 | 0.17 / 0.67.  The
models' figures (cvae, vae, vib, cvae with a full-variance prior; 200 images): at most 0.007 of their bounds, per-class mi 0.058;
aggregate_logdensity 0.093 / 0.033."""
import math

import numpy as np
import pytest
import torch

from oracle.cases import get_case
from oracle.det_init import load_det_state
from test_aggpost_restatement import (CASES, P, SEED, U, V_DATA, V_MODEL, aggpost_case, aggpost_reference, assert_limit, case_id,
                                      case_reference, check_identical, check_identities, check_separated, elbo_restatement,
                                      gaussian_prior, identical_bank, lattice_bank, noise)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_BANKS = {}


def bank_of(case):
    from jvae_hip import ops
    if case not in _BANKS:
        mu, lv, group, _, _ = aggpost_case(*case)
        _BANKS[case] = ops.aggpost_bank(dev(mu), dev(lv), dev(group))
    return _BANKS[case]


def run(z, bank, zgroup=None, conditional=False, dims=True):
    """-> (logq, logq_dims, status) from a status word of the call's own."""
    from jvae_hip import ops
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    z = z if torch.is_tensor(z) else dev(z)
    if conditional and not torch.is_tensor(zgroup):
        zgroup = dev(zgroup)
    logq, logq_dims = ops.aggpost_logdensity(z, bank, zgroup=zgroup if conditional else None, conditional=conditional, dims=dims,
                                             status=status)
    assert logq.dtype == torch.float32 and logq.shape == (z.shape[0],) and logq.is_cuda
    assert (logq_dims is None) == (not dims) and (not dims or logq_dims.shape == tuple(z.shape))
    return logq, logq_dims, int(status)


def check(logq, logq_dims, ref, tag):
    """Every output against the restatement within u B; -inf exactly where the restatement has it."""
    worst = {}
    for name, got, want, B in (('logq', logq, ref['logq'], ref['B']), ('logq_dims', logq_dims, ref['logq_dims'], ref['B_dims'])):
        got = got.cpu().numpy().astype(np.float64)
        gone = np.isneginf(want)
        assert (np.isneginf(got) == gone).all() and np.isfinite(got[~gone]).all(), (tag, name)
        if (~gone).any():
            worst[name] = float((np.abs(got[~gone] - want[~gone]) / (U * B[~gone])).max())
    print(tag, 'error / bound', worst)
    assert all(v <= 1. for v in worst.values()), (tag, worst)
    return worst


@pytest.mark.parametrize('conditional', [False, True], ids=['whole', 'conditional'])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_kernel_against_the_restatement(case, conditional):
    from jvae_hip import ops
    assert ops.aggpost_partition() == P
    K, N, M, G, empty = case
    mu, lv, group, z, zgroup = aggpost_case(*case)
    ref = case_reference(case, conditional)
    assert_limit(ref, K, N, V_DATA)
    logq, logq_dims, status = run(z, bank_of(case), zgroup, conditional)
    assert status == (ops.AGGPOST_STATUS_EMPTY if empty and conditional else 0)         # nothing else is flagged
    check(logq, logq_dims, ref, f'{case_id(case)} {"conditional" if conditional else "whole bank"}')
    alone, none, status = run(z, bank_of(case), zgroup, conditional, dims=False)
    assert none is None and same_bits(alone, logq)


def test_non_finite_elements_set_their_own_bits():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    case = CASES[3]
    mu, lv, group, z, zgroup = aggpost_case(*case)
    clean_q, clean_d, status = run(z, bank_of(case))
    assert status == 0
    bad = z.copy()
    bad[7, 2], bad[40, 0], bad[64, 5] = np.nan, np.inf, -np.inf
    bad[9] = 1e25                                      # finite, every square overflows fp32
    logq, logq_dims, status = run(bad, bank_of(case))
    assert status == ops.AGGPOST_STATUS_QUERY
    assert math.isnan(float(logq[7])) and bool((logq[[40, 64, 9]] == -np.inf).all())
    assert math.isnan(float(logq_dims[7, 2])) and float(logq_dims[40, 0]) == float(logq_dims[64, 5]) == -np.inf
    assert bool((logq_dims[9] == -np.inf).all())
    keep = [m for m in range(len(z)) if m not in (7, 40, 64, 9)]
    assert same_bits(logq[keep], clean_q[keep]) and same_bits(logq_dims[keep], clean_d[keep])
    other = np.ones(z.shape[1], dtype=bool)
    other[2] = False
    assert same_bits(logq_dims[7][dev(other)], clean_d[7][dev(other)])                  # the other coordinates of the row are untouched
    for broken, what in ((mu, 'mu'), (lv, 'lv')):
        for v in (np.nan, np.inf):
            b = broken.copy()
            b[len(b) - 1, 3] = v
            bank = ops.aggpost_bank(dev(b if what == 'mu' else mu), dev(b if what == 'lv' else lv), dev(group))
            assert run(z, bank)[2] & ops.AGGPOST_STATUS_BANK
    word = torch.full((1,), ops.AGGPOST_STATUS_QUERY, dtype=torch.int32, device=DEV)
    with pytest.raises(JvaeHipError, match='non-finite element'):
        ops.aggpost_check_status(word)
    assert int(word) == 0                              # read and cleared
    ops.aggpost_check_status(word)
    for bit, what in ((ops.AGGPOST_STATUS_BANK, 'bank holds'), (ops.AGGPOST_STATUS_EMPTY, 'no bank row')):
        with pytest.raises(JvaeHipError, match=what):
            ops.aggpost_check_status(torch.full((1,), bit, dtype=torch.int32, device=DEV))
    ops.aggpost_logdensity(dev(bad), bank_of(case))     # the default word of the device
    assert int(ops.aggpost_status(torch.device(DEV))) == ops.AGGPOST_STATUS_QUERY
    with pytest.raises(JvaeHipError, match='non-finite element'):
        ops.aggpost_check_status()
    ops.aggpost_check_status()


def test_bits_do_not_depend_on_the_batch_or_the_run():
    case = CASES[9]                                    # three pieces, an empty group
    mu, lv, group, z, zgroup = aggpost_case(*case)
    bank, zd, gd = bank_of(case), dev(z), dev(zgroup)
    for conditional in (False, True):
        whole_q, whole_d, _ = run(zd, bank, gd, conditional)
        again_q, again_d, _ = run(zd, bank, gd, conditional)
        assert same_bits(again_q, whole_q) and same_bits(again_d, whole_d)                  # two runs
        for a, b in ((0, 64), (0, 65), (63, 128), (17, 18), (5, 129)):                     # M on both sides of the query tile
            q, d, _ = run(zd[a:b].contiguous(), bank, gd[a:b].contiguous(), conditional)
            assert same_bits(q, whole_q[a:b]) and same_bits(d, whole_d[a:b])
        rev_q, rev_d, _ = run(zd.flip(0).contiguous(), bank, gd.flip(0).contiguous(), conditional)      # other lanes and workgroups
        assert same_bits(rev_q.flip(0), whole_q) and same_bits(rev_d.flip(0), whole_d)


def test_runs_of_queries_give_the_same_bits(monkeypatch):
    """A workspace budget so small that the op scores the 129 queries in three runs of 64, 64 and 1."""
    from jvae_hip import ops
    case = CASES[9]
    mu, lv, group, z, zgroup = aggpost_case(*case)
    whole_q, whole_d, status = run(z, bank_of(case), zgroup, True)
    monkeypatch.setattr(ops, 'AGGPOST_WS_BYTES', 1)
    q, d, again = run(z, bank_of(case), zgroup, True)
    assert status == again == ops.AGGPOST_STATUS_EMPTY and same_bits(q, whole_q) and same_bits(d, whole_d)


def test_no_queries_and_refusals():
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    bank = bank_of(CASES[2])
    logq, logq_dims, status = run(np.zeros((0, 64), dtype=np.float32), bank)
    assert logq.shape == (0,) and logq_dims.shape == (0, 64) and status == 0
    with pytest.raises(JvaeHipError, match=r'z \(M, 64\)'):
        ops.aggpost_logdensity(torch.zeros(3, 63, device=DEV), bank)
    with pytest.raises(JvaeHipError, match='unsupported configuration'):
        ops.aggpost_bank(torch.zeros(2, 1025, device=DEV), torch.zeros(2, 1025, device=DEV))
    with pytest.raises(ValueError, match='groups >= 0'):
        ops.aggpost_bank(torch.zeros(2, 3, device=DEV), torch.zeros(2, 3, device=DEV), torch.tensor([0, -1], device=DEV))
    with pytest.raises(JvaeHipError, match='status word'):
        ops.aggpost_logdensity(torch.zeros(3, 64, device=DEV), bank, status=torch.zeros(1, dtype=torch.int64, device=DEV))


def test_memory_and_the_workspace_formula():
    """N = 8192, M = 2048, K = 64: the call's peak allocation stays below the 64 MB an (M, N) fp32 matrix would take, and the
    library's workspace size is pieces M 12 bytes, plus pieces M K 8 with the coordinates."""
    from jvae_hip import lib, ops
    N, M, K = 8192, 2048, 64
    g = torch.Generator(device=DEV).manual_seed(1)
    bank = ops.aggpost_bank(torch.randn(N, K, generator=g, device=DEV), -4 * torch.rand(N, K, generator=g, device=DEV))
    z = torch.randn(M, K, generator=g, device=DEV)
    ops.aggpost_logdensity(z[:64], bank)               # the stream's workspace exists
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    logq, _ = ops.aggpost_logdensity(z, bank)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print('peak allocation of the call', peak, 'bytes; an (M, N) fp32 matrix', 4 * M * N)
    assert peak < 4 * M * N and bool(torch.isfinite(logq).all())
    pieces = N // P
    h = lib.load()
    assert h.jvae_aggpost_workspace_bytes(M, N, K, 0) == pieces * M * 12
    assert h.jvae_aggpost_workspace_bytes(M, N, K, 1) == pieces * M * 12 + pieces * M * K * 8
    assert h.jvae_aggpost_workspace_bytes(M, N + 1, K, 0) == (pieces + 1) * M * 12
    for args in ((0, N, K, 0), (M, 0, K, 0), (M, N, 0, 0), (M, N, 1025, 0), (M, (1 << 24) + 1, K, 0), (1 << 31, N, K, 0)):
        assert h.jvae_aggpost_workspace_bytes(*args) == 0


# ------------------------------------------------------------------------------------------------------------- the model
def synth(n, name, seed, shape=(1, 28, 28)):
    g = torch.Generator().manual_seed(seed)
    d = torch.utils.data.TensorDataset(torch.rand(n, *shape, generator=g), torch.randint(0, 10, (n,), generator=g))
    d.name = name
    return d


def build(case='c1_n16_mlp', **kw):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case(case)['net'], **kw))
    load_det_state(net, seed=0)
    net.to(DEV)
    net.eval()
    return net


def prior_of(net):
    pr = net.encoder.prior
    return gaussian_prior(pr.mean.detach().cpu().numpy(), pr.inv_trans.detach().cpu().numpy(), pr.var_dim, bool(pr.conditional))


def set_bank(net, bank):
    from jvae_hip import ops
    mu, lv, labels = bank
    net.posterior_bank = dict(ops.aggpost_bank(dev(mu), dev(lv), dev(labels.astype(np.int64))), labels=dev(labels.astype(np.int64)),
                              set='synthetic')


def test_closed_forms_through_the_model():
    net = build()
    K = net.encoder.prior.dim
    prior = prior_of(net)
    bank = identical_bank(40, K)
    set_bank(net, bank)
    res = net.elbo_decomposition(epsilon=dev(noise(40, K)))
    assert res['rows'] is None and res['m'] == res['n'] == 40
    check_identical(res, bank, prior, z=res['z'].cpu().numpy())
    check_identities(res)
    bank = lattice_bank(27, K)
    set_bank(net, bank)
    res = net.elbo_decomposition(epsilon=dev(noise(27, K, clip=4.)))
    check_separated(res, bank, prior, z=res['z'].cpu().numpy())
    check_identities(res)


def figures_against_the_restatement(net, res, tag):
    """Every figure of a result against the restatement on the bank read back, the model's own codes and noise."""
    from jvae_hip import ops
    bank = net.posterior_bank
    mu, lv, labels = (bank[k].cpu().numpy() for k in ('mu', 'log_var', 'labels'))
    assert np.abs(lv).max() <= V_MODEL
    rows = None if res['rows'] is None else res['rows'].numpy()
    eps = res['eps']
    ref = elbo_restatement(mu, lv, labels, prior_of(net), eps, rows=rows, z=res['z'].cpu().numpy())
    assert_limit(ref['ref'], mu.shape[1], len(mu), V_MODEL)
    b = ref['bound']
    tol = {'kl': b['kl'], 'kl_mc': b['logp'], 'mi': b['mi'], 'kl_marginal': b['kl_marginal'] + b['logp'], 'tc': b['tc'],
           'dwkl': b['dwkl'] + b['logp']}
    ratios = {}
    for k, t in tol.items():
        if ref[k] is None:
            assert res[k] is None
            continue
        ratios[k] = abs(res[k] - ref[k]) / (U * t)
    if ref['dwkl_per_dim'] is not None:
        ratios['dwkl_per_dim'] = float((np.abs(res['dwkl_per_dim'] - ref['dwkl_per_dim']) / (U * b['dwkl_per_dim'] + 1e-12)).max())
    else:
        assert res['dwkl_per_dim'] is None
    if 'per_class' in ref:
        seen = ref['per_class']['count'] > 0
        assert (res['per_class']['count'] == ref['per_class']['count']).all() and res['per_class']['count'].sum() == res['m']
        assert np.isnan(res['per_class']['mi'][~seen]).all()
        ratios['per_class mi'] = float((np.abs(res['per_class']['mi'] - ref['per_class']['mi'])[seen] / (U * b['per_class'][seen])).max())
        ratios['mi_unconditional'] = abs(res['mi_unconditional'] - ref['mi_unconditional']) / (U * b['mi_unconditional'])
    else:
        assert 'per_class' not in res and 'mi_unconditional' not in res
    print(tag, {k: res[k] for k in tol}, 'error / bound', ratios)
    assert all(v <= 1. for v in ratios.values()), (tag, ratios)
    assert res['mi_bound'] == math.log(len(mu)) and res['n'] == len(mu)
    check_identities(res)
    ops.aggpost_check_status()                          # nothing was flagged
    return ref


@pytest.mark.parametrize('case,shape,kw', [('c1_n16_mlp', (1, 28, 28), {}), ('a2_n8_vae', (3, 32, 32), {}), ('b2_n8_vib', (3, 32, 32), {}),
                                           ('c1_n16_mlp', (1, 28, 28), {'var_dim': 'full'})],
                         ids=['cvae', 'vae', 'vib', 'cvae-full'])
def test_models_against_the_restatement(case, shape, kw, tmp_path):
    if kw:
        kw = dict(prior=dict(get_case(case)['net']['prior'], **kw))
    net = build(case, **kw)
    train = synth(200, 'train', 5, shape)
    bank = net.fit_posterior_bank(train, batch_size=64)
    K = net.encoder.prior.dim
    assert bank is net.posterior_bank and bank['set'] == 'train' and bank['mu'].shape == (200, K) and not net.training
    assert torch.equal(bank['labels'].cpu(), train.tensors[1])
    with torch.no_grad():
        mu, lv = net.latent_posterior(train.tensors[0][64:128].to(DEV))
    assert torch.equal(bank['mu'][64:128], mu) and torch.equal(bank['log_var'][64:128], lv)         # the rows of the pass, bit for bit
    eps = noise(200, K, seed=SEED + 1)
    res = dict(net.elbo_decomposition(epsilon=dev(eps)), eps=eps)
    ref = figures_against_the_restatement(net, res, case + str(kw))
    conditional = net.type in ('cvae', 'xvae')
    assert ('per_class' in res) == conditional and (res['dwkl'] is None) == bool(kw)
    d = ref['summand_kl_mc'] - ref['kl_rows']
    assert abs(res['kl_mc'] - res['kl']) <= 5 * d.std(ddof=1) / math.sqrt(200) + U * (ref['bound']['kl'] + ref['bound']['logp'])
    # a seeded subset with the method's own noise: the queries it reports are rows of the bank, and the figures are those of a call
    # that is handed the same noise
    sub = net.elbo_decomposition(samples=50, seed=3)
    assert sub['m'] == 50 and sub['n'] == 200 and torch.equal(sub['rows'], torch.randperm(200, generator=torch.Generator().manual_seed(3))[:50])
    drawn = torch.randn((50, K), generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    figures_against_the_restatement(net, dict(sub, eps=drawn.cpu().numpy()), case + ' subset')
    # aggregate_logdensity: the kernel on arbitrary codes, with and without classes
    z, y = res['z'][:33], bank['labels'][:33]
    want = aggpost_reference(*(bank[k].cpu().numpy() for k in ('mu', 'log_var', 'labels')), z.cpu().numpy(), y.cpu().numpy(), conditional)
    logq, logq_dims = net.aggregate_logdensity(z, y if conditional else None, dims=True)
    check(logq, logq_dims, want, case + ' aggregate_logdensity')
    # save / load: the figures are bit-identical
    path = net.save_posterior_bank(str(tmp_path))
    assert path == str(tmp_path / 'posterior-bank.pth')
    other = build(case, **kw)
    got = other.load_posterior_bank(str(tmp_path))
    assert set(got) == set(bank) and all(torch.equal(got[k], bank[k]) and got[k].device == bank[k].device if torch.is_tensor(bank[k])
                                         else got[k] == bank[k] for k in bank)
    again = other.elbo_decomposition(epsilon=dev(eps))
    for k, v in res.items():
        if k in ('eps', 'rows', 'z', 'per_class'):
            continue
        assert np.array_equal(v, again[k], equal_nan=True) if isinstance(v, np.ndarray) else v == again[k], k
    assert torch.equal(res['z'], again['z'])
    if conditional:
        assert all(np.array_equal(res['per_class'][k], again['per_class'][k], equal_nan=True) for k in res['per_class'])
    # a seeded subset: the kept rows of the full pass, bit for bit (a batch that keeps a row is encoded whole)
    part = other.fit_posterior_bank(train, batch_size=64, ratio=0.25, seed=2)
    keep = torch.randperm(200, generator=torch.Generator().manual_seed(2))[:50].sort()[0].to(DEV)
    assert all(torch.equal(part[k], bank[k][keep]) for k in ('mu', 'log_var', 'labels')) and part['muT'].shape == (K, 64)


def test_model_refusals():
    net = build()
    with pytest.raises(ValueError, match='fit_posterior_bank'):
        net.elbo_decomposition()
    with pytest.raises(ValueError, match='fit_posterior_bank'):
        net.aggregate_logdensity(torch.zeros(2, 16, device=DEV))
    set_bank(net, identical_bank(40, 16))
    with pytest.raises(ValueError, match='samples'):
        net.elbo_decomposition(samples=41)
    with pytest.raises(ValueError, match='epsilon'):
        net.elbo_decomposition(epsilon=torch.zeros(40, 15))
