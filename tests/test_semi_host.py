"""Host side of semi-supervised training (csrc/semisup.hip, ops.class_marginal_kl, net.SEMI_SUPERVISED).  No
GPU: the C ABI's size queries and refusals come back before any launch (the pointers handed over are host addresses that are
never read), the argument checks of ops.class_marginal_kl raise before the library is reached, and the model's refusals are raised
by the first training-mode evaluate() before it touches a tensor."""
import ctypes

import pytest
import torch

import semi_cases as sc

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
    a = dict(mu=p, lv=p, y=p, means=p, T=p, log_pi=None, var_dim=SCALAR, w=1., N=3, K=4, C=2, kl_in=p, zd_in=p, vkl_in=p, kl=p, zd=p,
             vkl=p, r=p, r_bytes=1 << 40, ws=p, ws_bytes=1 << 40, stream=None)
    a.update(kw)
    return list(a.values())


def bwd_args(p, **kw):
    a = dict(g=p, mu=p, lv=p, y=p, means=p, T=p, var_dim=SCALAR, w=1., N=3, K=4, C=2, r=p, r_bytes=1 << 40, g_kl_in=p, g_mu=p, g_lv=p,
             g_means=None, g_T=None, stream=None)
    a.update(kw)
    return list(a.values())


def test_size_queries_and_the_limits(h):
    keep, ws = h.jvae_semi_keep_bytes, h.jvae_semi_fwd_workspace_bytes
    assert keep(3, 2) == 4 * 3 * 2 and ws(3, 2) == 8 * 3 * 2             # r (N, C) fp32; the parked exponents (N, C) fp64
    assert keep(0, 2) == 0 and ws(0, 2) == 0
    assert keep(1 << 20, 1024) == 4 << 30 and ws(1 << 20, 1024) == 8 << 30
    for shape in ((-1, 2), (3, 0), (3, 1025), ((1 << 20) + 1, 2)):
        assert keep(*shape) == 0 and ws(*shape) == 0, shape


def test_forward_refuses_malformed_calls(h, somewhere):
    p, _ = somewhere
    f = h.jvae_semi_class_marginal_fwd_f32
    assert f(*fwd_args(p, N=0)) == 0                                                      # an empty batch launches nothing
    assert f(*fwd_args(p, N=0, mu=None, lv=None, y=None, kl_in=None, zd_in=None, vkl_in=None, kl=None, zd=None, vkl=None, r=None,
                       ws=None)) == 0
    for name in ('mu', 'lv', 'y', 'means', 'T', 'kl_in', 'zd_in', 'vkl_in', 'kl', 'zd', 'vkl', 'r', 'ws'):
        assert f(*fwd_args(p, **{name: None})) == -1, name
    for name in ('mu', 'lv', 'means', 'T', 'kl_in', 'zd_in', 'vkl_in', 'kl', 'zd', 'vkl', 'r'):
        assert f(*fwd_args(p, **{name: p + 2})) == -1, name                               # fp32 operands: 4 bytes
    for name in ('y', 'log_pi', 'ws'):
        assert f(*fwd_args(p, **{name: p + 4})) == -1, name                               # int64 / fp64: 8 bytes
    for kw in (dict(K=0), dict(K=1025), dict(C=0), dict(C=1025), dict(N=-1), dict(N=(1 << 20) + 1), dict(var_dim=FULL), dict(var_dim=-1),
               dict(var_dim=3), dict(w=float('nan')), dict(w=float('inf')), dict(w=-float('inf'))):
        assert f(*fwd_args(p, **kw)) == -1, kw
    assert f(*fwd_args(p, N=0, means=None)) == -1 and f(*fwd_args(p, N=0, var_dim=FULL)) == -1
    assert f(*fwd_args(p, r_bytes=h.jvae_semi_keep_bytes(3, 2) - 1)) == -3
    assert f(*fwd_args(p, ws_bytes=h.jvae_semi_fwd_workspace_bytes(3, 2) - 1)) == -3


def test_backward_refuses_malformed_calls(h, somewhere):
    p, _ = somewhere
    b = h.jvae_semi_class_marginal_bwd_f32
    assert b(*bwd_args(p, N=0)) == 0                                                      # no class gradient asked for: nothing to do
    assert b(*bwd_args(p, N=0, g=None, mu=None, lv=None, y=None, r=None, g_kl_in=None, g_mu=None, g_lv=None)) == 0
    for name in ('mu', 'lv', 'y', 'means', 'T', 'r', 'g_kl_in', 'g_mu', 'g_lv'):
        assert b(*bwd_args(p, **{name: None})) == -1, name
    for name in ('g', 'mu', 'lv', 'means', 'T', 'r', 'g_kl_in', 'g_mu', 'g_lv', 'g_means'):
        assert b(*bwd_args(p, **{name: p + 2})) == -1, name
    assert b(*bwd_args(p, y=p + 4)) == -1
    for kw in (dict(K=0), dict(K=1025), dict(C=0), dict(C=1025), dict(N=-1), dict(N=(1 << 20) + 1), dict(var_dim=FULL), dict(var_dim=5),
               dict(w=float('nan')), dict(w=float('inf'))):
        assert b(*bwd_args(p, **kw)) == -1, kw
    assert b(*bwd_args(p, g_T=p)) == -1                                                   # the scalar factor is not learned
    assert b(*bwd_args(p, var_dim=DIAG, g_T=p + 2)) == -1
    assert b(*bwd_args(p, r_bytes=h.jvae_semi_keep_bytes(3, 2) - 1)) == -3


def test_ops_refuses_operands_before_the_library(h):
    from jvae_hip import ops
    from jvae_hip.lib import JvaeHipError
    c = sc.SHAPE_CASES[1]                                                                 # N 37, C 3, K 5, diag, non-uniform pi
    d = sc.make(c)

    def call(**kw):
        a = dict(d, **kw)
        return ops.class_marginal_kl(a['mu'], a['lv'], a['y'], a['means'], a['T'], a['kl_in'], a['zd_in'], a['vkl_in'],
                                     log_pi=a['log_pi'], w=kw.get('w', c.w), var_dim=kw.get('var_dim', c.var))
    with pytest.raises(JvaeHipError, match='resident on the GPU'):                        # well-formed, on the host: no fallback
        call()
    for kw, why in ((dict(mu=d['mu'].double()), 'mu must be torch.float32'),
                    (dict(lv=d['lv'].half()), 'log_var must be torch.float32'),
                    (dict(y=d['y'].int()), 'y must be torch.int64'),
                    (dict(y=d['y'][1:]), 'y must have the shape'),
                    (dict(lv=d['lv'][:, :4]), 'log_var must have the shape'),
                    (dict(means=d['means'][:, :4]), 'means must have the shape'),
                    (dict(T=d['T'][:, 0].contiguous()), 'T must have the shape'),
                    (dict(log_pi=torch.zeros(c.C)), 'log_pi must be torch.float64'),
                    (dict(log_pi=torch.zeros(c.C + 1, dtype=torch.float64)), 'log_pi must have the shape'),
                    (dict(kl_in=d['kl_in'][1:]), 'kl must have the shape'),
                    (dict(vkl_in=d['vkl_in'].double()), 'var_kl must be torch.float32'),
                    (dict(mu=d['mu'][0]), r'mu \(N, K\) and means \(C, K\)'),
                    (dict(w=float('nan')), 'finite w'),
                    (dict(w=torch.tensor(0.5)), 'host float'),
                    (dict(var_dim='full'), "'scalar' or 'diag'")):
        with pytest.raises(JvaeHipError, match=why):
            call(**kw)

    # the limits, on meta tensors: shapes alone, nothing is allocated
    def meta(N, K, C):
        e = lambda *s: torch.empty(*s, device='meta')                                     # noqa: E731
        return ops.class_marginal_kl(e(N, K), e(N, K), torch.empty(N, device='meta', dtype=torch.int64), e(C, K), e(C), e(N), e(N), e(N))
    with pytest.raises(JvaeHipError, match='K <= 1024'):
        meta(4, 1025, 2)
    with pytest.raises(JvaeHipError, match='C <= 1024'):
        meta(4, 8, 1025)
    with pytest.raises(JvaeHipError, match='at least one coordinate'):
        meta(4, 0, 2)


def test_the_switch_and_its_operands():
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    assert Net.SEMI_SUPERVISED is False and Net.UNLABELLED_CLASS_WEIGHTS is None
    m = Net(**get_case('c1_n16_mlp')['net'])
    m.train()
    C = m.encoder.prior.mean.shape[0]
    assert m._check_semi_supervised(1., {}) is False
    m.SEMI_SUPERVISED = True
    assert Net.SEMI_SUPERVISED is False                                                   # set per instance
    assert m._check_semi_supervised(1., {}) is True and m._check_semi_supervised(0.5, {}) is True       # a plain float weight is fine
    assert m._check_iwae_objective(1., {}) is False and m._check_tc_objective(1., {}) is False
    assert m._semi_log_pi(C, 'cpu') is None                                               # uniform weights: no operand
    m.UNLABELLED_CLASS_WEIGHTS = list(range(1, C + 1))
    t = m._semi_log_pi(C, 'cpu')
    w = torch.arange(1, C + 1, dtype=torch.float64)
    assert t.dtype == torch.float64 and torch.equal(t, (w / w.sum()).log())
    assert m._semi_log_pi(C, 'cpu') is t                                                  # kept until the attribute changes
    m.UNLABELLED_CLASS_WEIGHTS = torch.ones(C)
    assert float(m._semi_log_pi(C, 'cpu').exp().sum()) == pytest.approx(1.) and m._semi_log_pi(C, 'cpu') is not t
    for bad in ([1.] * (C + 1), [1.] * (C - 1) + [0.], [1.] * (C - 1) + [float('nan')], [1.] * (C - 1) + [-2.]):
        m.UNLABELLED_CLASS_WEIGHTS = bad
        with pytest.raises(ValueError, match='UNLABELLED_CLASS_WEIGHTS'):
            m._check_semi_supervised(1., {})
    m.UNLABELLED_CLASS_WEIGHTS = None
    for who in (m.graph_train_step, m.capture_train_step):                                # the captured steps take a label on every row
        with pytest.raises(NotImplementedError, match='SEMI_SUPERVISED.*' + who.__name__):
            who(torch.rand(4, *m.input_shape), torch.zeros(4, dtype=torch.int64))


@pytest.mark.parametrize('row', sc.refusal_table(), ids=lambda r: r[0])
def test_model_refuses_by_name_at_the_first_training_evaluate(row):
    """On the host: the refusal comes before the first tensor is touched, so CPU tensors get as far as it."""
    name, kwargs, tweak, ev_kw, word = row
    m = sc.refusal_model(kwargs, tweak)
    x, y = torch.rand(4, *m.input_shape), torch.tensor([0, -1, 1, -1])
    with pytest.raises(NotImplementedError, match='SEMI_SUPERVISED: .*' + word):
        m.evaluate(x, y, **ev_kw)
    if name == 'train_captured':
        for who in (m.graph_train_step, m.capture_train_step):
            with pytest.raises(NotImplementedError, match='SEMI_SUPERVISED.*' + who.__name__):
                who(x, y)


def test_class_marginal_refuses_what_the_switch_refuses_about_the_model():
    for name, kwargs, tweak, _, word in sc.refusal_table():
        if name not in ('jvae', 'coded_labels', 'tilted', 'full_variance', 'bf16', 'single_prior'):
            continue
        m = sc.refusal_model(kwargs, tweak)
        with pytest.raises(NotImplementedError, match='class_marginal: .*' + word):
            m.class_marginal(torch.rand(4, *m.input_shape))


def test_hidden_labels_over_a_resident_set_is_refused_by_name_through_train_model(monkeypatch):
    """train_model() hands its loaders the Subset of its own random_split, with and without a validation set: the refusal looks
    through it."""
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat import torch_load
    from jvae_compat.semi import HiddenLabels
    from oracle.cases import get_case
    m = Net(**get_case('c1_n16_mlp')['net'])
    m.SEMI_SUPERVISED = True
    ds = torch.utils.data.TensorDataset(torch.rand(8, *m.input_shape), torch.arange(8) % 2)
    ds.name = 'tiny'
    hidden = HiddenLabels(ds, keep_per_class=1)
    hidden.name = 'tiny'
    seen = []

    def fake_loader(dset, *a, **k):                          # stands for "the wrapped set is resident on the device"
        seen.append(dset)
        return object() if dset is ds else None
    monkeypatch.setattr(torch_load, 'device_loader', fake_loader)
    for validation in (0, 2):
        with pytest.raises(NotImplementedError, match='HiddenLabels over a device-resident image set'):
            m.train_model(trainset=hidden, epochs=0, batch_size=4, validation=validation, device='cpu', testset=None, save_dir=None)
    assert seen == [ds, ds]
    m.train_model(trainset=torch.utils.data.TensorDataset(*ds.tensors), epochs=0, batch_size=4, validation=0, device='cpu',
                  testset=None, save_dir=None)              # a host set without the wrapper goes its usual way
    assert len(seen) == 3 and isinstance(seen[2], torch.utils.data.Subset)


def test_the_switch_left_off_changes_nothing_in_training_parameters():
    """train_model() records the switch only when it is on: with no epoch to run it returns after its bookkeeping."""
    from cvae import ClassificationVariationalNetwork as Net
    from oracle.cases import get_case
    params = {}
    for on in (False, True):
        torch.manual_seed(0)
        m = Net(**get_case('c1_n16_mlp')['net'])
        m.SEMI_SUPERVISED = on
        ds = torch.utils.data.TensorDataset(torch.rand(8, *m.input_shape), torch.arange(8) % 2)
        ds.name = 'tiny'
        m.train_model(trainset=ds, epochs=0, batch_size=4, validation=0, device='cpu', testset=None, save_dir=None)
        params[on] = dict(m.training_parameters)
    assert 'semi_supervised' not in params[False]
    assert params[True].pop('semi_supervised') is True
    assert params[True].keys() == params[False].keys()
    assert all(params[True][k] == params[False][k] for k in params[False] if k not in ('sigma', 'validation_split_seed'))
