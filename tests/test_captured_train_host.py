"""CPU: the host side of train_model()'s captured step - the header, the library and the ctypes table agree on the new
entry points, their launchers refuse bad arguments before touching a device, and the capture key changes exactly when a
captured step stops being valid; the one decode of the measures block, CapturedStep driven by fakes, and the optimiser's
external-reduce flag."""
import ctypes
import gc
import os
import re
import types
import weakref

import pytest
import torch

from oracle.cases import full_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'jvae_latent_fwd_wdev_f32': 'jvae_latent_fwd_f32', 'jvae_latent_bwd_wdev_f32': 'jvae_latent_bwd_f32',
       'jvae_elbo_fwd_wdev_f32': 'jvae_elbo_fwd_f32', 'jvae_elbo_bwd_wdev_f32': 'jvae_elbo_bwd_f32',
       'jvae_measures_dev_f32': None, 'jvae_loss_sums_f32': None}


def _protos():
    src = open(os.path.join(REPO, 'include', 'jvae_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    found = dict(re.findall(r'\b(jvae_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S))
    return {k: [a.strip() for a in v.replace('\n', ' ').split(',')] for k, v in found.items()}


def _kind(decl):
    if '*' in decl:
        return 'ptr'
    for t in ('float', 'size_t', 'long'):
        if re.match(r'^(const\s+)?' + t + r'\b', decl):
            return t
    return 'int'


def _ckind(ct):
    return {ctypes.c_void_p: 'ptr', ctypes.c_float: 'float', ctypes.c_size_t: 'size_t', ctypes.c_long: 'long',
            ctypes.c_int: 'int'}[ct]


def test_new_entry_points_agree_between_header_library_and_ctypes():
    from jvae_hip import lib
    protos = _protos()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name, base in NEW.items():
        assert name in protos, name + ' is not declared in include/jvae_hip.h'
        assert hasattr(handle, name), name + ' is not exported by the library'
        res, args = lib._SIGS[name]
        assert res is ctypes.c_int
        assert [_kind(d) for d in protos[name]] == [_ckind(c) for c in args], name
        if base is not None:
            # the device-scalar form = the host-float form + ONE device pointer; the host float stays where it was
            extra = [d for d in protos[name] if d not in protos[base]]
            assert len(protos[name]) == len(protos[base]) + 1 and len(extra) == 1, (name, extra)
            assert _kind(extra[0]) == 'ptr' and extra[0].startswith('const float*')
            assert [d for d in protos[name] if d in protos[base]] == protos[base]


def test_loss_sums_launcher_checks_its_table_on_the_host():
    from jvae_hip import lib, ops
    h = lib.load()
    ptrs = (ctypes.c_void_p * 17)(*([0x1000] * 17))
    lens = (ctypes.c_long * 17)(*([4] * 17))
    assert h.jvae_loss_sums_f32(ptrs, lens, 0, None, None) == 0            # nothing to do: no launch
    assert h.jvae_loss_sums_f32(ptrs, lens, 17, 0x1000, None) == -1        # more rows than the kernel's table holds
    assert h.jvae_loss_sums_f32(ptrs, lens, -1, 0x1000, None) == -1
    assert h.jvae_loss_sums_f32(ptrs, lens, 2, None, None) == -1           # no accumulator
    lens[1] = 0
    assert h.jvae_loss_sums_f32(ptrs, lens, 2, 0x1000, None) == -1         # an empty row has no mean
    ptrs[0] = None
    lens[1] = 4
    assert h.jvae_loss_sums_f32(ptrs, lens, 2, 0x1000, None) == -1
    assert ops.LOSS_ROWS_MAX == 16
    with pytest.raises(lib.JvaeHipError):
        ops.loss_sums([torch.zeros(3)] * 17, torch.zeros(17))
    with pytest.raises(lib.JvaeHipError):                                   # no CPU fallback
        ops.loss_sums([torch.ones(3)], torch.zeros(1))


def test_device_entry_points_refuse_missing_device_words():
    from jvae_hip import lib
    h = lib.load()
    a = 0x1000
    # run / counter are what make the call capturable: both are required
    assert h.jvae_measures_dev_f32(a, 8, a, a, a, 2, 2, a, 0, None, 0, 0, None, None, a, None) == -1
    assert h.jvae_measures_dev_f32(a, 8, a, a, a, 2, 2, a, 0, None, 0, 0, None, a, None, None) == -1


def test_device_scalar_arguments_are_checked():
    from jvae_hip import lib, ops
    for bad in (torch.zeros(1), torch.zeros(2), torch.zeros(1, dtype=torch.float64)):      # CPU / two values / fp64
        with pytest.raises(lib.JvaeHipError):
            ops._device_scalar(bad, 'w')


def test_switch_and_hook_defaults():
    from cvae import ClassificationVariationalNetwork as Net
    assert Net.TRAIN_CAPTURED is False and Net._train_batch_hook is None and Net._captures_built == 0
    assert Net.CAPTURE_WARMUP_BATCHES >= 1      # at least one eager step builds the optimiser's flat buffers
    net = Net(**full_config(2, 32)['net'])
    net.TRAIN_CAPTURED = True                    # an instance may set it
    assert Net.TRAIN_CAPTURED is False


def test_capture_key_follows_shape_and_trainable_set_only():
    from cvae import ClassificationVariationalNetwork as Net
    kw = dict(full_config(2, 32)['net'])
    kw['prior'] = dict(kw['prior'], freeze_means=1)
    net = Net(**kw)
    x, y = torch.zeros(32, 3, 32, 32), torch.zeros(32, dtype=torch.int64)
    key = net._capture_key(x, y, False)
    assert key == net._capture_key(x.clone(), y.clone(), False)            # another batch of the same shape
    net.optimizer._lr *= 0.5                                                 # the learning rate is a device word of the step
    net.training_parameters['warmup'] = [0, 5]
    assert key == net._capture_key(x, y, False)
    assert key != net._capture_key(x[:7], y[:7], False)                     # a ragged batch is not served by the capture
    assert key != net._capture_key(x, y, True)                              # cross_y enters the loss
    net.encoder.prior.thaw_means(0)
    assert not net.encoder.prior.mean.requires_grad and key == net._capture_key(x, y, False)
    net.encoder.prior.thaw_means(1)                                         # epoch 1: the dictionary starts to train
    assert net.encoder.prior.mean.requires_grad and key != net._capture_key(x, y, False)
    key = net._capture_key(x, y, False)
    net.latent_sampling = 3
    assert key != net._capture_key(x, y, False)
    # whether cross_y is in the loss: gamma = 0 never, gamma > 0 whenever its warm-up weight is not zero
    assert net._cross_y_on(1.) is False
    g = Net(**dict(kw, gamma=2.0, classifier=[20]))
    assert g._cross_y_on(0.5) is True and g._cross_y_on(0.) is False


# ---- the 16-float measures block: the indices are written out here on purpose, as the second copy that guards the table
H = [100. + i for i in range(16)]


def test_decode_measures_without_dictionary():
    from cvae import decode_measures
    assert decode_measures(H, False) == {'sigma': 100., 'xpow': 110., 'mse': 111., 'rmse': 112., 'dB': 113., 'zdist': 114.,
                                         'var_kl': 115.}


def test_decode_measures_with_dictionary():
    from cvae import decode_measures
    assert decode_measures(H, True) == {'sigma': 100., 'ld-norm': 106., 'imut-zy': 107., 'd-mind': 108., 'xpow': 110.,
                                        'mse': 111., 'rmse': 112., 'dB': 113., 'zdist': 114., 'var_kl': 115.}


@pytest.mark.parametrize('has_dictionary', (False, True))
def test_decode_measures_only(has_dictionary):
    from cvae import decode_measures
    assert decode_measures(H, has_dictionary, only=('sigma', 'zdist', 'var_kl')) == {'sigma': 100., 'zdist': 114., 'var_kl': 115.}


def test_nonfinite_word_of_both_blocks():
    from cvae import measures_nonfinite
    for n in (16, 40):
        h = [0.] * n
        assert not measures_nonfinite(h)
        h[9] = 1.
        assert measures_nonfinite(h)
    h = [0.] * 40
    h[32] = 1e-45                       # the optimiser's int32 flag read as a float: a denormal, not zero
    assert measures_nonfinite(h)
    h = [1.] * 40                       # every other word is free to be anything
    h[9] = h[32] = 0.
    assert not measures_nonfinite(h)


# ---- CapturedStep driven by fakes: graphs that log their replay, an optimiser that logs its note, CPU buffers
class FakeGraph:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def replay(self):
        self.log.append(self.name)


def fake_net(log):
    optimizer = types.SimpleNamespace(note_replayed_step=lambda: log.append('noted'))
    return types.SimpleNamespace(optimizer=optimizer)


def test_two_graphs_replay_around_the_exchange():
    from cvae import CapturedStep
    log = []
    sx, sy = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    graphs = [FakeGraph(log, 'replay0'), FakeGraph(log, 'replay1')]
    losses = {'total': torch.ones(2)}
    step = CapturedStep(fake_net(log), sx, sy, graphs, lambda: log.append('between'), losses=losses)
    xb, yb = torch.arange(6.).reshape(2, 3), torch.tensor([4, 7])
    out = step(xb, yb)
    assert log == ['replay0', 'between', 'replay1', 'noted']
    assert torch.equal(sx, xb) and torch.equal(sy, yb) and step.x is sx and step.y is sy
    assert out is losses and step.losses is losses and step.keys == ['total']
    assert isinstance(step.graph, tuple) and len(step.graph) == 2
    assert step.graph[0] is graphs[0] and step.graph[1] is graphs[1]


def test_one_graph_needs_no_exchange():
    from cvae import CapturedStep
    log = []
    sx, sy = torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)
    graph = FakeGraph(log, 'replay0')
    step = CapturedStep(fake_net(log), sx, sy, [graph])
    xb, yb = torch.full((2, 3), 5.), torch.tensor([1, 0])
    step(xb, yb)
    assert log == ['replay0', 'noted']
    assert torch.equal(sx, xb) and torch.equal(sy, yb)
    assert step.graph is graph


def test_constants_live_as_long_as_the_step():
    from cvae import CapturedStep
    log = []
    constant = torch.ones(3)
    alive = weakref.ref(constant)
    step = CapturedStep(fake_net(log), torch.zeros(2, 3), torch.zeros(2), [FakeGraph(log, 'replay0')],
                        constants=(constant, [torch.zeros(1)]))
    del constant
    gc.collect()
    assert alive() is not None and step.constants[0] is alive()
    assert torch.equal(step.constants[0], torch.ones(3))
    del step
    gc.collect()
    assert alive() is None


# ---- the one flag for "the gradient exchange happens outside" (Optimizer.external_reduce)
def test_external_reduce_is_set_inside_and_cleared_after():
    from module.optimizers import Optimizer
    opt = Optimizer([])
    assert not getattr(opt, '_external_reduce', False)
    with opt.external_reduce():
        assert opt._external_reduce is True
    assert opt._external_reduce is False


def test_external_reduce_is_cleared_when_the_body_raises():
    from module.optimizers import Optimizer
    opt = Optimizer([])
    with pytest.raises(RuntimeError, match='in the body'):
        with opt.external_reduce():
            assert opt._external_reduce is True
            raise RuntimeError('in the body')
    assert opt._external_reduce is False
