"""Device-resident named image sets on the MI355X: ops.imageset_batch (csrc/imageset.hip) against the torch-CPU composition of
tests/imageset_cases.py and against PIL's own resize (tests/golden/imagesets/pil_resize.npz), the refusals, and the loops
(accuracy, train_model, ood_detection_rates) fed from names through `DATA_ROOT`.  Everything is compared with torch.equal:
the kernel moves bytes and divides by 255, there is no tolerance to choose."""
import logging
import os

import numpy as np
import pytest
import torch

import imageset_cases as IC
from oracle.cases import get_case
from oracle.det_init import load_det_state

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
IDX = [8, 0, 3, 3, 5]                                          # out of order, one repeat


def run(data, idx, desc, targets=None, lut=None, **kw):
    from jvae_hip import ops
    targets = torch.arange(data.shape[0]) if targets is None else targets
    x, y = ops.imageset_batch(data.to(DEV), torch.as_tensor(idx).to(DEV), desc, targets.to(DEV),
                              None if lut is None else lut.to(DEV), **{k: v.to(DEV) for k, v in kw.items()})
    return x.cpu(), y.cpu()


# ---------------------------------------------------------------------------------------------- 5. resize against PIL
@pytest.fixture(scope='module')
def pil(golden_dir):
    return np.load(os.path.join(golden_dir, 'imagesets', 'pil_resize.npz'))


@pytest.mark.parametrize('key,Hr,Wr,A', [('28_32', 32, 32, 0), ('7x5_9x8', 9, 8, 0), ('32_28', 28, 28, 0), ('turn_7x5_8x9', 8, 9, 1)])
def test_resize_is_pils(pil, key, Hr, Wr, A):
    from jvae_hip import ops
    from jvae_compat.torch_load import pil_bilinear_tables
    src, want = torch.from_numpy(pil['src_' + key]), torch.from_numpy(pil['out_' + key])
    n, Hs, Ws = src.shape
    H1, W1 = (Ws, Hs) if A else (Hs, Ws)
    tables = (*pil_bilinear_tables(W1, Wr), *pil_bilinear_tables(H1, Hr))
    if key == '32_28':
        assert tables[0].shape[1] == 5                         # ksize 5: down-scaling
    idx = list(range(n - 1, -1, -1)) + [0]
    for g2c in (False, True):
        desc = ops.ImagesetDesc((Hs, Ws, 1), False, A=A, resize=(Hr, Wr, *tables), g2c=g2c, device=DEV)
        x, _ = run(src[:, None], idx, desc)
        expect = IC.expected_batch(src[idx][:, None], resized=want[idx][:, None], g2c=g2c)
        assert x.shape == expect.shape == (n + 1, 3 if g2c else 1, Hr, Wr) and torch.equal(x, expect), (key, g2c)
    # with the later stages behind it: zero padding, a transpose, the random part, the post padding
    desc = ops.ImagesetDesc((Hs, Ws, 1), True, A=A, resize=(Hr, Wr, *tables), p0=2, B=7, g2c=True, pa=1, post='pad', device=DEV)
    flip, dy, dx = torch.tensor([1, 0] * n)[:n + 1], torch.tensor([0, 2] * n)[:n + 1], torch.tensor([2, 1] * n)[:n + 1]
    x, _ = run(src[..., None], idx, desc, flip=flip, dy=dy, dx=dx)
    expect = IC.expected_batch(src[idx][:, None], resized=want[idx][:, None], p0=2, B=7, g2c=True, flip=flip, dy=dy, dx=dx, pa=1,
                               post='pad')
    assert torch.equal(x, expect), key


# ---------------------------------------------------------------------------------------------- 6. the chain
def sources():
    g = torch.Generator().manual_seed(11)
    return {'nhwc': (torch.randint(0, 256, (9, 6, 10, 3), generator=g, dtype=torch.uint8), True),
            'nchw': (torch.randint(0, 256, (9, 3, 6, 10), generator=g, dtype=torch.uint8), False),
            'grey': (torch.randint(0, 256, (9, 1, 7, 7), generator=g, dtype=torch.uint8), False)}


RANDOM = dict(flip=torch.tensor([1, 0, 1, 0, 0]), dy=torch.tensor([0, 4, 2, 4, 0]), dx=torch.tensor([4, 0, 1, 4, 0]))


def check_chain(data, nhwc, A, B, p0, g2c, post, random, crop_by=(3, 2)):
    from jvae_hip import ops
    nchw = data.permute(0, 3, 1, 2) if nhwc else data
    source = (nchw.shape[2], nchw.shape[3], nchw.shape[1])
    probe = ops.ImagesetDesc(source, nhwc, A=A, p0=p0, B=B, g2c=g2c, device=DEV)
    if post == 'crop':
        post = ('crop', probe.shape[1] - crop_by[0], probe.shape[2] - crop_by[1])
    desc = ops.ImagesetDesc(source, nhwc, A=A, p0=p0, B=B, g2c=g2c, pa=2 if random else 0, post=post, device=DEV)
    kw = RANDOM if random else {}
    x, y = run(data, IDX, desc, **kw)
    expect = IC.expected_batch(nchw[IDX], A=A, p0=p0, B=B, g2c=g2c, pa=2, post=post, **{k: v for k, v in kw.items()})
    assert tuple(x.shape) == (5, *desc.shape) == tuple(expect.shape), (A, B, p0, g2c, post, random)
    assert torch.equal(x, expect), (A, B, p0, g2c, post, random)
    assert y.tolist() == IDX
    return desc.shape


@pytest.mark.parametrize('name', ['nhwc', 'nchw', 'grey'])
def test_chain_every_turn_in_both_slots(name):
    data, nhwc = sources()[name]
    posts = [None, 'pad', 'crop']
    shapes = set()
    for A in range(8):
        for B in range(8):
            for p0 in (0, 2):
                shapes.add(check_chain(data, nhwc, A, B, p0, name == 'grey' and (A + B) % 2 == 1, posts[(A + B + p0 // 2) % 3], True))
    if name != 'grey':
        assert {s[1:] for s in shapes} >= {(6, 10), (10, 6), (14, 10), (10, 14)}       # H != W: both orientations were produced


@pytest.mark.parametrize('name', ['nhwc', 'nchw', 'grey'])
def test_chain_every_stage_on_and_off(name):
    data, nhwc = sources()[name]
    for A, B in ((0, 0), (1, 6), (7, 3)):
        for p0 in (0, 2):
            for post in (None, 'pad', 'crop'):
                for random in (False, True):
                    for g2c in ((False, True) if name == 'grey' else (False,)):
                        check_chain(data, nhwc, A, B, p0, g2c, post, random)
    for crop_by in ((1, 5), (5, 1), (2, 4), (0, 3)):           # centre-crop offsets at .5: torchvision rounds halves to even
        check_chain(data, nhwc, 0, 0, 2, False, 'crop', True, crop_by=crop_by)


@pytest.mark.parametrize('nhwc', [True, False])
def test_identity_chain_is_augment_batch(nhwc):
    from jvae_hip import ops
    g = torch.Generator().manual_seed(3)
    data = torch.randint(0, 256, (7, 12, 9, 3) if nhwc else (7, 3, 12, 9), generator=g, dtype=torch.uint8).to(DEV)
    flip, dy, dx = ops.draw_augmentation(7, 2, DEV, generator=torch.Generator(DEV).manual_seed(4))
    desc = ops.ImagesetDesc((12, 9, 3), nhwc, pa=2, device=DEV)
    x, y = ops.imageset_batch(data, torch.arange(7, device=DEV), desc, torch.arange(7, device=DEV), None, flip, dy, dx)
    assert torch.equal(x, ops.augment_batch(data, flip, dy, dx, pad=2, nhwc=nhwc)) and y.tolist() == list(range(7))
    x, _ = ops.imageset_batch(data, torch.arange(7, device=DEV), desc.with_pa(0), torch.arange(7, device=DEV))
    assert torch.equal(x, ops.augment_batch(data, nhwc=nhwc))
    x, _ = ops.imageset_batch(data, torch.arange(7, device=DEV), desc, torch.arange(7, device=DEV), flip=flip)
    assert torch.equal(x, ops.augment_batch(data, flip, pad=2, nhwc=nhwc))          # flip alone: the centred crop


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('sets'))
    return root, {'mnist': IC.write_idx_tree(root, 'MNIST', 40, 20, seed=21),
                  'letters': IC.write_idx_tree(root, 'EMNIST', 9, 9, seed=22, prefix='emnist-letters-', test_part='test',
                                               classes=26, first_label=1),
                  'cifar10': IC.write_cifar10_tree(root, per_file=9, seed=23)}


def test_registry_chains_at_their_real_sizes(trees):
    from jvae_hip import ops
    from jvae_compat import torch_load as T
    root, raw = trees
    idx = [8, 0, 3, 3, 5]
    mn = torch.from_numpy(raw['mnist']['test'][0])[:, None]
    s = T.get_dataset('mnist32p', splits=['test'], root=root, device=DEV)[1]
    x, y = s.batch(idx)
    assert tuple(x.shape) == (5, 3, 32, 32) and torch.equal(x.cpu(), IC.expected_batch(mn[idx], p0=2, g2c=True))
    assert y.tolist() == raw['mnist']['test'][1][idx].tolist()
    s = T.get_dataset('mnist', transformer='pad', splits=['test'], root=root, device=DEV)[1]
    x, _ = s.batch(torch.tensor(idx))
    assert tuple(x.shape) == (5, 1, 32, 32) and torch.equal(x.cpu(), IC.expected_batch(mn[idx], post='pad'))
    xi, yi = s[-1]
    assert torch.equal(xi.cpu(), IC.expected_batch(mn[-1:], post='pad')[0]) and yi == int(raw['mnist']['test'][1][-1])
    # letters: rotate-270 then hflip = a transpose; labels through the y-1 table
    le = torch.from_numpy(raw['letters']['test'][0])[:, None]
    s = T.get_dataset('letters', splits=['test'], root=root, device=DEV)[1]
    x, y = s.batch(idx)
    assert torch.equal(x.cpu(), IC.expected_batch(le[idx], A=3 + 4)) and torch.equal(x.cpu(), le[idx].transpose(-1, -2).float().div(255))
    assert y.tolist() == (raw['letters']['test'][1][idx] - 1).tolist()
    # cifar1090 with flip + crop (pa = 4): the draws are those of ops.draw_augmentation under the same generator
    ci = torch.from_numpy(raw['cifar10']['train'][0]).permute(0, 3, 1, 2)
    s = T.get_dataset('cifar1090', splits=['train'], root=root, device=DEV)[0]
    flip, dy, dx = ops.draw_augmentation(5, 4, DEV, generator=torch.Generator(DEV).manual_seed(8))
    x, y = s.batch(idx, ['flip', 'crop'], generator=torch.Generator(DEV).manual_seed(8))
    expect = IC.expected_batch(ci[idx], A=1, flip=flip.cpu(), dy=dy.cpu(), dx=dx.cpu(), pa=4)
    assert s.name == 'cifar1090' and torch.equal(x.cpu(), expect) and y.tolist() == raw['cifar10']['train'][1][idx].tolist()
    # held-out table: the stored targets keep their numbering, y is re-numbered
    s = T.get_dataset('cifar10-3', splits=['train'], root=root, device=DEV)[0]
    kept = raw['cifar10']['train'][1][raw['cifar10']['train'][1] != 3]
    x, y = s.batch(range(len(s)))
    assert len(s) == len(kept) < 45 and y.tolist() == [t - (t > 3) for t in kept.tolist()] and max(y.tolist()) <= 8
    assert torch.equal(x.cpu(), IC.expected_batch(ci[torch.from_numpy(raw['cifar10']['train'][1] != 3)]))
    # synthetic siblings: shape, range, one colour per channel and image
    c = T.get_dataset('const32', splits=['test'], device=DEV)[1]
    x, y = c.batch([0, 1, 9999])
    assert tuple(x.shape) == (3, 3, 32, 32) and bool((x == x[:, :, :1, :1]).all()) and y.tolist() == [0, 0, 0]
    u = T.get_dataset('uniform28', transformer='pad', splits=['test'], device=DEV)[1]
    x, _ = u.batch([5, 6])
    assert tuple(x.shape) == (2, 1, 32, 32) and float(x[:, :, :2].abs().max()) == 0. and 0. <= float(x.min()) and float(x.max()) < 1.


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_come_before_any_launch(trees, monkeypatch):
    from jvae_hip import ops, JvaeHipError
    from jvae_compat import torch_load as T
    s = T.get_dataset('mnist', splits=['test'], root=trees[0], device=DEV)[1]
    launches = []
    real = ops.imageset_batch
    monkeypatch.setattr(ops, 'imageset_batch', lambda *a, **k: launches.append(1) or real(*a, **k))
    for bad, error in (([0, len(s)], IndexError), ([-len(s) - 1], IndexError), (torch.tensor([0, 1], device=DEV), TypeError)):
        with pytest.raises(error):
            s.batch(bad)
    assert not launches
    assert s.batch([-len(s), len(s) - 1])[1].tolist() == raw_labels(trees, [0, -1]) and launches == [1]
    monkeypatch.setattr(ops, 'imageset_batch', real)
    tables = (*T.pil_bilinear_tables(32, 3), *T.pil_bilinear_tables(32, 3))
    assert tables[0].shape[1] > 8
    desc = ops.ImagesetDesc((32, 32, 1), False, resize=(3, 3, *tables), device=DEV)
    with pytest.raises(JvaeHipError, match='unsupported'):
        ops.imageset_batch(torch.zeros((2, 1, 32, 32), dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                           desc, torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):                            # tables that would read past the image never reach the device
        ops.ImagesetDesc((30, 30, 1), False, resize=(3, 3, *tables), device=DEV)


def raw_labels(trees, where):
    return trees[1]['mnist']['test'][1][where].tolist()


# ---------------------------------------------------------------------------------------------- 8. the loops
class Plain(torch.utils.data.Dataset):
    """The same raw images as a plain map-style data set: the DataLoader path of the loops."""

    def __init__(self, images, labels, name='mnist'):
        self.x, self.y, self.name, self.transformer = torch.from_numpy(images)[:, None], labels.tolist(), name, ''

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


@pytest.fixture
def mnist_root(tmp_path):
    root = str(tmp_path / 'data')
    return root, {'mnist': IC.write_idx_tree(root, 'MNIST', 40, 20, seed=21)}


def build_net(root=None):
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case('c1_n16_mlp')['net']))
    load_det_state(net, seed=0)
    net.to(DEV)
    net.DATA_ROOT = root
    return net


def test_accuracy_by_name_is_accuracy_of_the_plain_set(mnist_root, tmp_path):
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_compat.recorders import LossRecorder
    root, raw = mnist_root
    assert Net.DATA_ROOT is None
    net = build_net(root)
    net.training_parameters.update(set='mnist', transformer='')
    plain = Plain(*raw['mnist']['test'])
    for num_batch in ('all', 1):
        got = {}
        for tag, testset in (('named', None), ('plain', plain)):
            np.random.seed(12)                                 # a recorder draws the seed of its pass from numpy when it is made
            rec = LossRecorder(8)
            torch.manual_seed(12)
            acc = net.accuracy(testset, batch_size=8, num_batch=num_batch, recorder=rec, sample_dirs=[str(tmp_path / tag)],
                               update_self_testing=False)
            got[tag] = (acc, torch.load(str(tmp_path / tag / 'record-mnist.pth'), weights_only=False)['_tensors'], dict(net.test_losses))
        assert got['named'][0] == got['plain'][0] and set(got['named'][0]) == set(net.predict_methods)
        assert got['named'][2] == got['plain'][2]
        a, b = got['named'][1], got['plain'][1]
        assert list(a) == list(b) and 'y_true' in a
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (num_batch, k)
    by_name = []
    for testset in ('mnist', plain):                           # a name given outright, no recorder
        torch.manual_seed(12)
        by_name.append(net.accuracy(testset, batch_size=8, update_self_testing=False))
    assert by_name[0] == by_name[1]
    net.DATA_ROOT = None
    for testset in (None, 'mnist'):
        with pytest.raises(NotImplementedError, match='named torchvision datasets are outside this build'):
            net.accuracy(testset)


def test_train_model_by_name_is_train_model_of_the_plain_set(mnist_root, monkeypatch):
    root, raw = mnist_root
    real_seed = np.random.seed
    monkeypatch.setattr(np.random, 'seed', lambda *a: real_seed(77))     # the validation split is drawn anew in every call
    # a recorded accuracy pass leaves torch on the seed torch.seed() gave it, a fresh random one: pinned, so that the two
    # trainings draw the same noise
    monkeypatch.setattr(torch, 'seed', lambda: torch.manual_seed(99).initial_seed())
    states, nets = [], []
    for named in (True, False):
        net = build_net(root if named else None)
        net.augmentation_generator = torch.Generator(DEV).manual_seed(3)
        torch.manual_seed(6)
        trainset = 'mnist' if named else Plain(*raw['mnist']['train'])
        testset = None if named else Plain(*raw['mnist']['test'])
        hist = net.train_model(trainset, epochs=1, batch_size=10, test_batch_size=10, validation=8, data_augmentation=['flip'],
                               device=DEV, testset=testset, full_test_every=1)
        assert hist['epochs'] == 1 and 'test_accuracy' in hist[1] and 'validation_accuracy' in hist[0]
        states.append({k: v.clone() for k, v in net.state_dict().items()})
        nets.append(net)
    assert nets[0].training_parameters['set'] == 'mnist' and nets[0].training_parameters['transformer'] == ''
    assert nets[0].training_parameters['data_augmentation'] == ['flip']
    assert nets[0].train_history[1]['test_accuracy'] == nets[1].train_history[1]['test_accuracy']
    assert nets[0].train_history[0]['train_loss'] == nets[1].train_history[0]['train_loss']
    moved = 0
    fresh = build_net().state_dict()
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
        moved += int(not torch.equal(states[0][k], fresh[k]))
    assert moved > 0
    nets[1].DATA_ROOT = None
    with pytest.raises(NotImplementedError, match='named torchvision datasets are host-side plumbing outside this build'):
        nets[1].train_model('mnist', epochs=2, batch_size=10, validation=8, device=DEV)


def test_ood_rates_score_the_siblings_that_are_there(mnist_root, caplog):
    root, raw = mnist_root
    net = build_net(root)
    net.training_parameters.update(set='mnist', transformer='')

    def rates():
        caplog.clear()
        torch.manual_seed(2)
        with caplog.at_level(logging.WARNING):
            res = net.ood_detection_rates(batch_size=10, num_batch=2, method=['kl', 'max'], update_self_ood=False)
        return res, [r.getMessage() for r in caplog.records if 'is left out' in r.getMessage()]
    res, left = rates()
    assert list(res) == ['const28', 'uniform28', 'mnist90'] and len(left) == 2
    assert 'fashion' in left[0] and 'FashionMNIST' in left[0] and 'letters' in left[1]
    for name, entry in res.items():
        assert list(entry) == ['kl', 'max'] and entry['kl']['n'] == 20 and 0. <= entry['kl']['auc'] <= 1., name
    IC.write_idx_tree(root, 'FashionMNIST', 4, 13, seed=24)
    res, left = rates()
    assert list(res) == ['const28', 'uniform28', 'fashion', 'mnist90'] and len(left) == 1 and res['fashion']['max']['n'] == 13
    only = net.ood_detection_rates(oodsets=['fashion'], testset='mnist', batch_size=10, method='kl', update_self_ood=False)
    assert list(only) == ['fashion']
    with pytest.raises(FileNotFoundError, match='EMNIST'):
        net.ood_detection_rates(oodsets=['letters'], batch_size=10, method='kl', update_self_ood=False)
    net.DATA_ROOT = None
    for kw in (dict(), dict(testset='mnist', oodsets=['fashion'])):
        with pytest.raises(NotImplementedError, match='named torchvision datasets are outside this build'):
            net.ood_detection_rates(batch_size=10, method='kl', **kw)
