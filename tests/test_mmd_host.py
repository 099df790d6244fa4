"""Host side of the MMD objective (csrc/mmd.hip, ops.mmd_objective, TRAIN_OBJECTIVE = 'mmd').  No GPU: the
C ABI's size queries and refusals come back before any launch (the pointers handed over are host addresses that are never read),
the argument checks of ops.mmd_objective raise before the library is reached, and the model's refusals are raised by the first
training-mode evaluate() before it touches a tensor."""
import ctypes

import pytest
import torch

import mmd_cases as mc

SCALAR, DIAG, FULL = 0, 1, 2
IMQ, RBF = 0, 1


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


def scales(*v):
    return (ctypes.c_float * len(v))(*v)


def fwd_args(p, **kw):
    a = dict(z=p, eps_p=p, y=p, means=p, T=p, var_dim=SCALAR, kind=IMQ, scales=scales(1., 2.), n_scales=2, joint=1, L=2, N=3, K=4, C=2,
             m=p, ws=p, ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return list(a.values())


def bwd_args(p, **kw):
    a = dict(g_m=p, z=p, eps_p=p, y=p, means=p, T=p, var_dim=SCALAR, kind=IMQ, scales=scales(1., 2.), n_scales=2, joint=1, L=2, N=3,
             K=4, C=2, g_z=p, g_means=None, g_T=None, ws=p, ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return list(a.values())


def test_size_queries_the_tile_and_the_limits(h):
    fwd, bwd = h.jvae_mmd_fwd_workspace_bytes, h.jvae_mmd_bwd_workspace_bytes
    assert h.jvae_mmd_tile() == 64
    up = lambda n: (n + 15) // 16 * 16                                                    # noqa: E731
    # p (L, N, K) fp32, the groups (N,), then the fp64 partial sums of one piece: 3 per (l, i) forward, 2 per (l, i, k) backward and
    # the two (N, K) class contributions; N = 3 is one step of columns, so one piece
    assert fwd(2, 3, 4) == up(2 * 3 * 4 * 4) + up(3 * 4) + up(1 * 2 * 3 * 3 * 8)
    assert bwd(2, 3, 4) == up(2 * 3 * 4 * 4) + up(3 * 4) + up(1 * 2 * 3 * 4 * 2 * 8) + 2 * up(3 * 4 * 8)
    # the pieces are a function of the shape alone: N = 512, L = 1 is 16 steps of 32 columns, every one a piece of its own
    assert fwd(1, 512, 64) == up(512 * 64 * 4) + up(512 * 4) + up(16 * 512 * 3 * 8)
    for shape in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (1, 8193, 4), (1, 3, 1025), (-1, 3, 4), (65536, 3, 4)):
        assert fwd(*shape) == 0 and bwd(*shape) == 0, shape
    assert fwd(1, 8192, 1024) > 0 and bwd(1, 8192, 1024) > 0 and fwd(65535, 1, 1) > 0
    assert fwd(8, 8192, 4) > 0                                                            # no L N^2 limit: nothing of that size is kept


def test_forward_refuses_malformed_calls(h, somewhere):
    p, _ = somewhere
    f = h.jvae_mmd_objective_fwd_f32
    assert f(*fwd_args(p, N=0)) == 0                                                      # an empty batch launches nothing
    assert f(*fwd_args(p, N=0, z=None, eps_p=None, y=None, m=None, ws=None)) == 0
    for name in ('z', 'eps_p', 'y', 'means', 'T', 'scales', 'm', 'ws'):
        assert f(*fwd_args(p, **{name: None})) == -1, name
    for kw in (dict(L=0), dict(L=-1), dict(K=0), dict(N=-1), dict(C=0), dict(var_dim=3), dict(var_dim=-1), dict(kind=2), dict(kind=-1),
               dict(joint=2), dict(n_scales=0), dict(n_scales=9), dict(scales=scales(1., 0.)), dict(scales=scales(1., -3.)),
               dict(scales=scales(float('nan'), 1.)), dict(scales=scales(float('inf'), 1.)), dict(ws=p + 8)):
        assert f(*fwd_args(p, **kw)) == -1, kw
    assert f(*fwd_args(p, ws_bytes=h.jvae_mmd_fwd_workspace_bytes(2, 3, 4) - 1)) == -3


def test_refuses_what_is_not_built_before_any_launch(h, somewhere):
    p, _ = somewhere
    f, b = h.jvae_mmd_objective_fwd_f32, h.jvae_mmd_objective_bwd_f32
    for kw in (dict(var_dim=FULL), dict(K=1025), dict(N=8193), dict(L=65536)):
        assert f(*fwd_args(p, **kw)) == -2, kw
        assert b(*bwd_args(p, **kw)) == -2, kw
    assert f(*fwd_args(p, var_dim=FULL, L=0)) == -1 and f(*fwd_args(p, K=1025, means=None)) == -1


def test_backward_refusals_and_workspace(h, somewhere):
    p, _ = somewhere
    b = h.jvae_mmd_objective_bwd_f32
    for name in ('z', 'eps_p', 'y', 'means', 'T', 'scales', 'g_z', 'ws'):
        assert b(*bwd_args(p, **{name: None})) == -1, name
    for kw in (dict(L=0), dict(K=0), dict(N=-1), dict(C=0), dict(var_dim=5), dict(kind=7), dict(n_scales=9), dict(ws=p + 4)):
        assert b(*bwd_args(p, **kw)) == -1, kw
    need = h.jvae_mmd_bwd_workspace_bytes(2, 3, 4)
    assert b(*bwd_args(p, ws_bytes=need - 1)) == -3
    assert b(*bwd_args(p, g_means=p, g_T=p, ws_bytes=need - 1)) == -3
    assert b(*bwd_args(p, N=0, g_means=p, ws=None)) == -3                                 # the zeros of an empty class sum need a launch
    assert b(*bwd_args(p, N=0, g_z=None, ws=None)) == 0


def test_ops_refuses_operands_before_the_library(h):
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    c = mc.SHAPE_CASES[3]                                                                 # K 65, L 3, N 64, diag
    d = mc.make(c)

    def call(**kw):
        a = dict(d, **kw)
        return ops.mmd_objective(a['z'], a['eps_p'], a['y'], a['means'], a['T'], kernel=kw.get('kernel', mc.kernel_of(c)),
                                 joint=c.joint, var_dim=kw.get('var_dim', c.var))
    with pytest.raises(JvaeHipError, match='resident on the GPU'):                        # well-formed, on the host: no fallback
        call()
    for kw, why in ((dict(z=d['z'].double()), 'z must be torch.float32'),
                    (dict(eps_p=d['eps_p'].half()), 'eps_p must be torch.float32'),
                    (dict(y=d['y'].int()), 'y must be torch.int64'),
                    (dict(z=d['z'][1:]), 'z must have the shape'),
                    (dict(eps_p=d['eps_p'][0]), 'eps_p must have the shape'),
                    (dict(means=d['means'][:, :5]), 'means must have the shape'),
                    (dict(T=d['T'][:, 0].contiguous()), 'T must have the shape'),
                    (dict(var_dim='banded'), 'var_dim'),
                    (dict(kernel=('laplace', None)), 'kernel kind'),
                    (dict(kernel='imq'), 'kernel is'),
                    (dict(kernel=('imq', ())), 'positive finite scales'),
                    (dict(kernel=('imq', (1., 0.))), 'positive finite scales'),
                    (dict(kernel=('rbf', (1e-60,))), 'positive finite scales'),            # not positive as the fp32 the kernels read
                    (dict(kernel=('rbf', (float('nan'),))), 'positive finite scales'),
                    (dict(kernel=('rbf', tuple(range(1, 10)))), 'positive finite scales'),
                    (dict(kernel=('rbf', ('a',))), 'scales is')):
        with pytest.raises(JvaeHipError, match=why):
            call(**kw)
    assert ops.mmd_scales(('imq', None), 64) == ('imq', tuple(2. * 64 * s for s in (.1, .2, .5, 1., 2., 5., 10.)))
    assert ops.mmd_scales(('rbf', [3, 4.5]), 64) == ('rbf', (3., 4.5)) and ops.mmd_tile() == 64

    # the limits, on meta tensors: shapes alone, nothing is allocated
    def meta(L, N, K):
        e = lambda *s: torch.empty(*s, device='meta')                                     # noqa: E731
        return ops.mmd_objective(e(L + 1, N, K), e(L, N, K), torch.empty(N, device='meta', dtype=torch.int64), e(1, K), e(1))
    with pytest.raises(JvaeHipError, match='N <= 8192'):
        meta(1, 8193, 2)
    with pytest.raises(JvaeHipError, match='K <= 1024'):
        meta(1, 4, 1025)


def test_objective_values_and_the_checks():
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    assert Net.TRAIN_OBJECTIVE == 'elbo' and Net.MMD_WEIGHTS == (1., 1000.) and Net.MMD_KERNEL == ('imq', None) and Net.MMD_JOINT is True
    m = Net(**get_case('c1_n16_mlp')['net'])
    m.train()
    before = dict(m.training_parameters)
    assert m._check_mmd_objective(1., {}) is False and m._check_tc_objective(1., {}) is False and m._check_iwae_objective(1., {}) is False
    for other in ('iwae', 'tcvae'):
        m.TRAIN_OBJECTIVE = other
        assert m._check_mmd_objective(1., {}) is False
    m.TRAIN_OBJECTIVE = 'mmd'
    assert Net.TRAIN_OBJECTIVE == 'elbo'                                                  # set per instance
    assert m._check_mmd_objective(1., {}) is True and m._check_iwae_objective(1., {}) is False and m._check_tc_objective(1., {}) is False
    assert m._check_mmd_objective(0.5, {}) is True                                        # a warm-up of the KL is free here
    assert m._check_mmd_objective(torch.tensor([0.5]), {}) is True                        # ... as a device scalar too
    m.TRAIN_OBJECTIVE = 'dreg'
    with pytest.raises(ValueError, match="'elbo' or 'iwae' or 'tcvae' or 'mmd', got 'dreg'"):
        m._check_iwae_objective(1., {})
    m.TRAIN_OBJECTIVE = 'mmd'
    for attr, value in (('MMD_WEIGHTS', (1., float('nan'))), ('MMD_WEIGHTS', (1., 2., 3.)), ('MMD_WEIGHTS', 5.),
                        ('MMD_KERNEL', ('laplace', None)), ('MMD_KERNEL', ('imq', (0.,))), ('MMD_KERNEL', ('rbf', tuple(range(1, 10))))):
        good = getattr(m, attr)
        setattr(m, attr, value)
        with pytest.raises(ValueError, match=attr):
            m._check_mmd_objective(1., {})
        setattr(m, attr, good)
    assert m._mmd_settings() == (1., 1000., 'imq', tuple(2. * m.latent_dim * s for s in mc.WAE_SCALES))
    for who in (m.graph_train_step, m.capture_train_step):                                # the captured steps train on the ELBO
        with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'mmd'.*" + who.__name__):
            who(torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64))
    assert m.training_parameters == before                                                # nothing is recorded outside train_model()


def test_training_parameters_stay_untouched_on_a_default_model():
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    m = Net(**get_case('c1_n16_mlp')['net'])
    assert not ({'objective', 'mmd_weights', 'mmd_kernel'} & set(m.training_parameters))
    assert 'TRAIN_OBJECTIVE' not in m.__dict__ and not any(k.startswith('MMD_') for k in m.__dict__)
    assert not hasattr(m, '_last_prior_epsilon')


def test_prior_mmd_refuses_on_the_host():
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    from jvae_hip.lib import JvaeHipError
    m = Net(**get_case('c1_n16_mlp')['net'])
    K = m.latent_dim
    with pytest.raises(ValueError, match='labels'):
        m.prior_mmd(torch.zeros(4, K))
    with pytest.raises(ValueError, match='codes must be'):
        m.prior_mmd(torch.zeros(4, K + 1), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match='epsilon must be'):
        m.prior_mmd(torch.zeros(4, K), torch.zeros(4, dtype=torch.int64), epsilon=torch.zeros(3, K))
    with pytest.raises(JvaeHipError, match='resident on the GPU'):                        # well-formed, on the host: no fallback
        m.prior_mmd(torch.zeros(4, K), torch.zeros(4, dtype=torch.int64), epsilon=torch.zeros(4, K))
    m.MMD_KERNEL = ('imq', (-1.,))
    with pytest.raises(ValueError, match='MMD_KERNEL'):
        m.prior_mmd(torch.zeros(4, K), torch.zeros(4, dtype=torch.int64))


@pytest.mark.parametrize('row', mc.refusal_table(), ids=lambda r: r[0])
def test_model_refuses_by_name_at_the_first_training_evaluate(row):
    """On the host: the refusal comes before the first tensor is touched, so CPU tensors get as far as it."""
    name, kwargs, tweak, ev_kw, word = row
    m = mc.refusal_model(kwargs, tweak)
    x, y = torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'mmd'.*" + word):
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
    m = mc.refusal_model(get_case('c1_n16_mlp')['net'], lambda m: setattr(m.encoder.sampling, 'is_sampled', False))
    with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'mmd'.*does not sample"):
        m.evaluate(torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64))
