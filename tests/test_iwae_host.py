"""Host side of the importance-weighted bound (csrc/iwae.hip, ops.iw_bound, TRAIN_OBJECTIVE).  No GPU:
the C ABI's refusals come back before any launch (the pointers handed over are host addresses that are never read), the
argument checks of ops.iw_bound raise before the library is reached, and the model's refusals are raised by the first
training-mode evaluate() before it touches a tensor."""
import ctypes

import pytest
import torch

import iwae_cases as ic

SIG_VALUE, SIG_LOG, SIG_CODED, SIG_RMSE = 0, 1, 2, 3
GAUSS, TILTED, UNIFORM = 0, 1, 2
SCALAR, DIAG, FULL = 0, 1, 2


@pytest.fixture(scope='module')
def h():
    from jvae_hip import lib
    return lib.load()


@pytest.fixture(scope='module')
def somewhere():
    """A host address that stands for 'a pointer was given': every call below returns before anything could read it."""
    buf = (ctypes.c_float * 16)()
    return ctypes.addressof(buf), buf


def fwd_args(p, **kw):
    a = dict(wmse_s=p, z=p, lv=p, eps=p, y=p, means=p, T=p, sigma=p, sigma_is_log=SIG_VALUE, prior=GAUSS, var_dim=SCALAR, beta=1.,
             L=2, N=3, K=4, C=2, D=5, bound=p, wt=p, ess=p, state=None, stream=None)
    a.update(kw)
    return list(a.values())


def bwd_args(p, **kw):
    a = dict(g_bound=p, wt=p, z=p, y=p, means=p, T=p, sigma=p, sigma_is_log=SIG_VALUE, prior=GAUSS, var_dim=SCALAR, beta=1.,
             L=2, N=3, K=4, C=2, D=5, g_wmse_s=p, g_z=p, g_lv=p, g_means=None, g_T=None, g_sigma=None, ws=None, ws_bytes=0,
             stream=None)
    a.update(kw)
    return list(a.values())


def test_forward_refuses_malformed_calls(h, somewhere):
    p, _ = somewhere
    f = h.jvae_iw_bound_fwd_f32
    for name in ('wmse_s', 'z', 'lv', 'eps', 'y', 'means', 'T', 'sigma', 'bound', 'wt', 'ess'):
        assert f(*fwd_args(p, **{name: None})) == -1, name
    for kw in (dict(L=0), dict(L=-1), dict(K=0), dict(N=-1), dict(C=0), dict(D=0), dict(sigma_is_log=4), dict(sigma_is_log=-1),
               dict(prior=3), dict(prior=-1), dict(var_dim=3), dict(var_dim=-1), dict(beta=float('nan'))):
        assert f(*fwd_args(p, **kw)) == -1, kw


def test_forward_refuses_what_is_not_built_before_any_launch(h, somewhere):
    p, _ = somewhere
    f = h.jvae_iw_bound_fwd_f32
    for kw in (dict(var_dim=FULL), dict(prior=TILTED), dict(prior=UNIFORM), dict(sigma_is_log=SIG_RMSE),
               dict(var_dim=FULL, prior=TILTED, sigma_is_log=SIG_RMSE)):
        assert f(*fwd_args(p, **kw)) == -2, kw
    # a malformed call stays malformed whatever else it asks for
    assert f(*fwd_args(p, var_dim=FULL, L=0)) == -1 and f(*fwd_args(p, prior=TILTED, z=None)) == -1


def test_an_empty_batch_launches_nothing(h, somewhere):
    p, _ = somewhere
    # N = 0: no per-sample array exists, so none is asked for
    assert h.jvae_iw_bound_fwd_f32(*fwd_args(p, N=0, wmse_s=None, z=None, lv=None, eps=None, y=None, bound=None, wt=None,
                                             ess=None)) == 0
    assert h.jvae_iw_bound_fwd_f32(*fwd_args(p, N=0, sigma=None, sigma_is_log=SIG_CODED)) == 0
    assert h.jvae_iw_bound_fwd_f32(*fwd_args(p, N=0, sigma=None)) == -1                   # one value is still one value
    assert h.jvae_iw_bound_bwd_f32(*bwd_args(p, N=0, wt=None, z=None, y=None, g_wmse_s=None, g_z=None, g_lv=None)) == 0


def test_backward_refusals_and_workspace(h, somewhere):
    p, _ = somewhere
    b = h.jvae_iw_bound_bwd_f32
    for name in ('wt', 'z', 'y', 'means', 'T', 'sigma', 'g_wmse_s', 'g_z', 'g_lv'):
        assert b(*bwd_args(p, **{name: None})) == -1, name
    for kw in (dict(L=0), dict(K=0), dict(N=-1), dict(C=0), dict(D=0), dict(sigma_is_log=7), dict(prior=9), dict(var_dim=5)):
        assert b(*bwd_args(p, **kw)) == -1, kw
    for kw in (dict(var_dim=FULL), dict(prior=TILTED), dict(prior=UNIFORM), dict(sigma_is_log=SIG_RMSE)):
        assert b(*bwd_args(p, **kw)) == -2, kw
    assert b(*bwd_args(p, g_T=p)) == -1                                                   # the scalar factor is not learned
    need = h.jvae_iw_bound_bwd_workspace_bytes(3, 4)
    assert need == 8 * (2 * 3 * 4 + 3)                                                   # fp64 contributions
    assert h.jvae_iw_bound_bwd_workspace_bytes(0, 4) == 0 and h.jvae_iw_bound_bwd_workspace_bytes(3, 0) == 0
    assert h.jvae_iw_bound_bwd_workspace_bytes(-1, 4) == 0
    for out in ('g_means', 'g_sigma'):
        assert b(*bwd_args(p, **{out: p})) == -3                                          # asked for a class sum, gave no scratch
        assert b(*bwd_args(p, **{out: p}, ws=p, ws_bytes=need - 1)) == -3
    assert b(*bwd_args(p, var_dim=DIAG, g_T=p, ws=p, ws_bytes=need - 1)) == -3


def test_ops_refuses_operands_before_the_library(h):
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    c = ic.SHAPE_CASES[2]                                                                 # K 63, L 5, N 3, coded sigma
    d = ic.make(c)

    def call(**kw):
        a = dict(d, **kw)
        return ops.iw_bound(a['wmse_s'], a['z'], a['lv'], a['eps'], a['y'], a['means'], a['T'], a['sigma'], c.sig, c.D,
                            beta=c.beta, var_dim=kw.get('var_dim', c.var))
    with pytest.raises(JvaeHipError, match='resident on the GPU'):                        # well-formed, on the host: no fallback
        call()
    for kw, why in ((dict(wmse_s=d['wmse_s'].double()), 'wmse_s must be torch.float32'),
                    (dict(z=d['z'].half()), 'z must be torch.float32'),
                    (dict(y=d['y'].int()), 'y must be torch.int64'),
                    (dict(z=d['z'][1:]), 'z must have the shape'),
                    (dict(lv=d['lv'][:, :5]), 'lv must have the shape'),
                    (dict(T=d['T'].unsqueeze(-1).expand(c.C, c.K)), 'T must have the shape'),
                    (dict(sigma=d['sigma'][:2]), 'sigma must be'),
                    (dict(var_dim='banded'), 'var_dim')):
        with pytest.raises(JvaeHipError, match=why):
            call(**kw)
    with pytest.raises(JvaeHipError, match='contiguous|resident on the GPU'):
        call(eps=d['eps'].transpose(0, 1).contiguous().transpose(0, 1))


def test_default_objective_and_its_values():
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    assert Net.TRAIN_OBJECTIVE == 'elbo'
    m = Net(**get_case('c1_n16_mlp')['net'])
    assert 'objective' not in m.training_parameters
    m.train()
    assert m._check_iwae_objective(1., {}) is False
    m.TRAIN_OBJECTIVE = 'iwae'
    assert Net.TRAIN_OBJECTIVE == 'elbo' and m._check_iwae_objective(1., {}) is True     # set per instance
    m.TRAIN_OBJECTIVE = 'dreg'
    with pytest.raises(ValueError, match="'elbo' or 'iwae'"):
        m._check_iwae_objective(1., {})


@pytest.mark.parametrize('row', ic.refusal_table(), ids=lambda r: r[0])
def test_model_refuses_by_name_at_the_first_training_evaluate(row):
    """On the host: the refusal comes before the first tensor is touched, so CPU tensors get as far as it."""
    name, kwargs, tweak, ev_kw, word = row
    m = ic.refusal_model(kwargs, tweak)
    x, y = torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="TRAIN_OBJECTIVE = 'iwae'.*" + word):
        m.evaluate(x, y, **ev_kw)
    if name == 'train_captured':
        for who in (m.graph_train_step, m.capture_train_step):
            with pytest.raises(NotImplementedError, match='TRAIN_OBJECTIVE.*' + who.__name__):
                who(x, y)
