"""CPU: the host side of train_model()'s captured step - the header, the library and the ctypes table agree on the new
entry points, their launchers refuse bad arguments before touching a device, and the capture key changes exactly when a
captured step stops being valid."""
import ctypes
import os
import re

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
