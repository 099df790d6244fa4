"""Host side of the beta-TCVAE objective (csrc/tcvae.hip, ops.tc_objective, TRAIN_OBJECTIVE = 'tcvae').  No
GPU: the C ABI's size queries and refusals come back before any launch (the pointers handed over are host addresses that are
never read), the argument checks of ops.tc_objective raise before the library is reached, and the model's refusals are raised by
the first training-mode evaluate() before it touches a tensor."""
import ctypes

import pytest
import torch

import tc_cases as tcc

SCALAR, DIAG, FULL = 0, 1, 2


@pytest.fixture(scope='module')
def h():
    from jvae_hip import lib
    return lib.load()


@pytest.fixture(scope='module')
def somewhere():
    """A 16-byte aligned host address that stands for 'a pointer was given': every call below returns before it could be read."""
    buf = (ctypes.c_float * 32)()
    a = ctypes.addressof(buf)
    return a + (-a) % 16, buf


def fwd_args(p, **kw):
    a = dict(z=p, mu=p, lv=p, eps=p, y=p, means=p, T=p, log_n=None, var_dim=SCALAR, alpha=1., beta_tc=6., gamma=1., L=2, N=3, K=4, C=2,
             reg=p, mi=p, tc=p, dwkl=p, keep=p, keep_bytes=1 << 40, ws=p, ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return list(a.values())


def bwd_args(p, **kw):
    a = dict(g_reg=p, z=p, mu=p, lv=p, y=p, means=p, T=p, var_dim=SCALAR, alpha=1., beta_tc=6., gamma=1., L=2, N=3, K=4, C=2, keep=p,
             keep_bytes=1 << 40, g_z=p, g_mu=p, g_lv=p, g_means=None, g_T=None, ws=None, ws_bytes=0, stream=None)
    a.update(kw)
    return list(a.values())


def test_size_queries_and_the_limits(h):
    keep, ws = h.jvae_tc_keep_bytes, h.jvae_tc_fwd_workspace_bytes
    # L N rows of Np = 64 kept exponents, L N joint pairs, L N K coordinate pairs, N K values of e^(-lv), each rounded up to 16 bytes
    up = lambda n: (n + 15) // 16 * 16                                                    # noqa: E731
    assert keep(2, 3, 4) == 6 * 64 * 4 + 6 * 8 + 6 * 4 * 8 + 3 * 4 * 4
    assert keep(1, 65, 1) == 65 * 128 * 4 + up(65 * 8) + up(65 * 8) + up(65 * 4)
    assert ws(2, 3, 4) > 0
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (1, 8193, 4), (1, 3, 1025), (-1, 3, 4)):
        assert keep(*shape) == 0 and ws(*shape) == 0, shape
    assert keep(1, 8192, 1024) > 0 and keep(1, 8192, 1) > 0
    # the kept exponents: L N^2 <= 2^26, asked through the size query alone - nothing is allocated
    assert keep(1, 8192, 4) > 0 and keep(2, 8192, 4) == 0
    assert keep(1025, 256, 4) == 0 and keep(1024, 256, 4) > 0
    assert h.jvae_tc_bwd_workspace_bytes(3, 4) == 8 * 2 * 3 * 4
    assert h.jvae_tc_bwd_workspace_bytes(0, 4) == 0 and h.jvae_tc_bwd_workspace_bytes(3, 0) == 0


def test_forward_refuses_malformed_calls(h, somewhere):
    p, _ = somewhere
    f = h.jvae_tc_objective_fwd_f32
    assert f(*fwd_args(p, N=0)) == 0                                                      # an empty batch launches nothing
    assert f(*fwd_args(p, N=0, z=None, mu=None, lv=None, eps=None, y=None, reg=None, mi=None, tc=None, dwkl=None, keep=None,
                       ws=None)) == 0
    for name in ('z', 'mu', 'lv', 'eps', 'y', 'means', 'T', 'reg', 'mi', 'tc', 'dwkl', 'keep', 'ws'):
        assert f(*fwd_args(p, **{name: None})) == -1, name
    for kw in (dict(L=0), dict(L=-1), dict(K=0), dict(N=-1), dict(C=0), dict(var_dim=3), dict(var_dim=-1), dict(alpha=float('nan')),
               dict(beta_tc=float('nan')), dict(gamma=float('nan')), dict(keep=p + 4), dict(ws=p + 8)):
        assert f(*fwd_args(p, **kw)) == -1, kw
    assert f(*fwd_args(p, keep_bytes=h.jvae_tc_keep_bytes(2, 3, 4) - 1)) == -3
    assert f(*fwd_args(p, ws_bytes=h.jvae_tc_fwd_workspace_bytes(2, 3, 4) - 1)) == -3


def test_refuses_what_is_not_built_before_any_launch(h, somewhere):
    p, _ = somewhere
    f, b = h.jvae_tc_objective_fwd_f32, h.jvae_tc_objective_bwd_f32
    for kw in (dict(var_dim=FULL), dict(K=1025), dict(N=8193), dict(L=2, N=8192), dict(L=1025, N=256)):
        assert f(*fwd_args(p, **kw)) == -2, kw
        assert b(*bwd_args(p, **kw)) == -2, kw
    assert f(*fwd_args(p, var_dim=FULL, L=0)) == -1 and f(*fwd_args(p, K=1025, means=None)) == -1


def test_backward_refusals_and_workspace(h, somewhere):
    p, _ = somewhere
    b = h.jvae_tc_objective_bwd_f32
    for name in ('z', 'mu', 'lv', 'y', 'means', 'T', 'keep', 'g_z', 'g_mu', 'g_lv'):
        assert b(*bwd_args(p, **{name: None})) == -1, name
    for kw in (dict(L=0), dict(K=0), dict(N=-1), dict(C=0), dict(var_dim=5)):
        assert b(*bwd_args(p, **kw)) == -1, kw
    assert b(*bwd_args(p, g_T=p)) == -1                                                   # the scalar factor is not learned
    assert b(*bwd_args(p, keep_bytes=8)) == -3
    need = h.jvae_tc_bwd_workspace_bytes(3, 4)
    assert b(*bwd_args(p, g_means=p)) == -3
    assert b(*bwd_args(p, g_means=p, ws=p, ws_bytes=need - 1)) == -3
    assert b(*bwd_args(p, var_dim=DIAG, g_T=p, ws=p, ws_bytes=need - 1)) == -3


def test_ops_refuses_operands_before_the_library(h):
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    c = tcc.SHAPE_CASES[3]                                                                # K 65, L 3, N 64, diag
    d = tcc.make(c)

    def call(**kw):
        a = dict(d, **kw)
        return ops.tc_objective(a['z'], a['mu'], a['lv'], a['eps'], a['y'], a['means'], a['T'], kw.get('weights', c.weights),
                                a['log_n'], var_dim=kw.get('var_dim', c.var))
    with pytest.raises(JvaeHipError, match='resident on the GPU'):                        # well-formed, on the host: no fallback
        call()
    for kw, why in ((dict(z=d['z'].double()), 'z must be torch.float32'),
                    (dict(mu=d['mu'].half()), 'mu must be torch.float32'),
                    (dict(y=d['y'].int()), 'y must be torch.int64'),
                    (dict(z=d['z'][1:]), 'z must have the shape'),
                    (dict(lv=d['lv'][:, :5]), 'log_var must have the shape'),
                    (dict(T=d['T'][:, 0].contiguous()), 'T must have the shape'),
                    (dict(log_n=torch.zeros(c.C)), 'log_n must be torch.float64'),
                    (dict(log_n=torch.zeros(c.C + 1, dtype=torch.float64)), 'log_n must have the shape'),
                    (dict(var_dim='banded'), 'var_dim')):
        with pytest.raises(JvaeHipError, match=why):
            call(**kw)
    with pytest.raises((TypeError, ValueError)):
        call(weights=(1., 6.))

    # the limits, on meta tensors: shapes alone, nothing is allocated
    def meta(L, N, K):
        e = lambda *s: torch.empty(*s, device='meta')                                     # noqa: E731
        return ops.tc_objective(e(L + 1, N, K), e(N, K), e(N, K), e(L, N, K), torch.empty(N, device='meta', dtype=torch.int64),
                                e(1, K), e(1))
    with pytest.raises(JvaeHipError, match='256 MB'):
        meta(2, 8192, 2)
    with pytest.raises(JvaeHipError, match='N <= 8192'):
        meta(1, 8193, 2)
    with pytest.raises(JvaeHipError, match='K <= 1024'):
        meta(1, 4, 1025)


def test_objective_values_and_the_two_checks():
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    assert Net.TRAIN_OBJECTIVE == 'elbo' and Net.TC_WEIGHTS == (1., 6., 1.) and Net.TC_DATASET_SIZE is None
    m = Net(**get_case('c1_n16_mlp')['net'])
    m.train()
    assert m._check_tc_objective(1., {}) is False and m._check_iwae_objective(1., {}) is False
    m.TRAIN_OBJECTIVE = 'iwae'
    assert m._check_tc_objective(1., {}) is False and m._check_iwae_objective(1., {}) is True
    m.TRAIN_OBJECTIVE = 'tcvae'
    assert Net.TRAIN_OBJECTIVE == 'elbo'                                                  # set per instance
    assert m._check_tc_objective(1., {}) is True and m._check_iwae_objective(1., {}) is False
    m.TRAIN_OBJECTIVE = 'dreg'
    with pytest.raises(ValueError, match="'elbo' or 'iwae' or 'tcvae'"):
        m._check_iwae_objective(1., {})
    m.TRAIN_OBJECTIVE = 'tcvae'
    m.TC_WEIGHTS = (1., float('nan'), 1.)
    with pytest.raises(ValueError, match='TC_WEIGHTS'):
        m._check_tc_objective(1., {})
    m.TC_WEIGHTS = (1., 2.)
    with pytest.raises(ValueError, match='TC_WEIGHTS'):
        m._check_tc_objective(1., {})
    for who in (m.graph_train_step, m.capture_train_step):                                # the captured steps train on the ELBO
        with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'tcvae'.*" + who.__name__):
            who(torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64))


def test_dataset_size_operand():
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    m = Net(**get_case('c1_n16_mlp')['net'])
    C = m.encoder.prior.mean.shape[0]
    assert m._tc_log_n(C, 'cpu') is None
    m.TC_DATASET_SIZE = list(range(1, C + 1))
    t = m._tc_log_n(C, 'cpu')
    assert t.dtype == torch.float64 and torch.equal(t, torch.arange(1, C + 1, dtype=torch.float64).log())
    assert m._tc_log_n(C, 'cpu') is t                                                     # kept until the attribute changes
    m.TC_DATASET_SIZE = 50000
    assert torch.equal(m._tc_log_n(1, 'cpu'), torch.tensor([50000.], dtype=torch.float64).log())
    with pytest.raises(ValueError, match='class counts'):
        m._tc_log_n(C, 'cpu')
    m.TC_DATASET_SIZE = [3, 0]
    with pytest.raises(ValueError, match='>= 1'):
        m._tc_log_n(2, 'cpu')
    # what train_model() fills it with: the length for a single prior, one bincount of the labels for a conditional one -
    # through random_split's Subsets, from .targets where the dataset carries them and from the samples where it does not
    y = torch.tensor([0, 2, 2, 1, 2, 0, 2, 2])
    ds = torch.utils.data.TensorDataset(torch.rand(8, 2), y)
    assert Net._tc_dataset_size_of(ds, 1) == 8 and Net._tc_dataset_size_of(ds, 3) == (2, 1, 5)
    sub = torch.utils.data.Subset(torch.utils.data.Subset(ds, [0, 1, 2, 3, 4]), [1, 2, 4])
    assert Net._tc_dataset_size_of(sub, 3) == (1, 1, 3)                                   # class 0 has no sample: any count serves
    ds.targets = y.tolist()
    assert Net._tc_dataset_size_of(sub, 3) == (1, 1, 3) and Net._tc_dataset_size_of(ds, 4) == (2, 1, 5, 1)
    # a label outside [0, C) is in nobody's set in the kernels: it is not counted into a neighbouring class either
    assert Net._tc_dataset_size_of(ds, 2) == (2, 1)
    ds.targets = [0, -1, 2, 1, 7, 0, 2, 2]
    assert Net._tc_dataset_size_of(ds, 3) == (2, 1, 3)


@pytest.mark.parametrize('row', tcc.refusal_table(), ids=lambda r: r[0])
def test_model_refuses_by_name_at_the_first_training_evaluate(row):
    """On the host: the refusal comes before the first tensor is touched, so CPU tensors get as far as it."""
    name, kwargs, tweak, ev_kw, word = row
    m = tcc.refusal_model(kwargs, tweak)
    x, y = torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'tcvae'.*" + word):
        m.evaluate(x, y, **ev_kw)
    if name == 'world':
        with pytest.raises(NotImplementedError, match='whole batch.*shard'):
            m.evaluate(x, y, **ev_kw)
    if name == 'train_captured':
        for who in (m.graph_train_step, m.capture_train_step):
            with pytest.raises(NotImplementedError, match='TRAIN_OBJECTIVE.*' + who.__name__):
                who(x, y)


def test_an_encoder_that_does_not_sample_is_refused():
    from oracle.cases import get_case
    m = tcc.refusal_model(get_case('c1_n16_mlp')['net'], lambda m: setattr(m.encoder.sampling, 'is_sampled', False))
    with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'tcvae'.*does not sample"):
        m.evaluate(torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64))
