"""Host side of the named, device-resident image sets (jvae_compat/torch_load.py), no GPU: the pure name functions against what
the reference's returned (tests/golden/torch_load/names.json, tools/gen_sets_golden.py), the PIL resize tables against PIL,
the readers on tiny trees in every on-disk format, and the sample order / generator use of device_loader()."""
import json
import os

import numpy as np
import pytest
import torch

import imageset_cases as IC
from jvae_compat import torch_load as T


def _plain(v):
    return json.loads(json.dumps(v))


def test_name_functions_match_the_reference(golden_dir):
    g = json.load(open(os.path.join(golden_dir, 'torch_load', 'names.json')))
    assert len(g['names']) == 15
    for name, want in g['names'].items():
        assert _plain(T.get_shape_by_name(name)) == want['shape_default'], name
        assert _plain(T.get_shape_by_name(name, 'pad')) == want['shape_pad'], name
        assert T.get_same_size_by_name(name) == want['same_size'], name
        assert _plain(T.get_heldout_classes_by_name(name)) == want['heldout'], name
        assert T.get_classes_by_name(name) == want['classes'], name
    for call in g['name_by_heldout']:
        assert T.get_name_by_heldout_classes(*call['args']) == call['name'], call
    assert T.get_same_size_by_name('cifar10-?') == g['same_size_question'] == ['cifar10+?']
    # what the issue spells out
    assert T.get_shape_by_name('cifar10-3')[1] == 9 and T.get_same_size_by_name('cifar10-3') == ['cifar10+3']
    assert T.get_name_by_heldout_classes('cifar10', 0, 1, 2, 3, 4, 5) == 'cifar10+6+7+8+9'
    assert T.get_shape_by_name('mnist90')[0] == (1, 28, 28) and T.get_same_size_by_name('mnist')[-1] == 'mnist90'
    assert T.get_shape_by_name('nosuchset') == (None, None)


SIZE_PAIRS = [((28, 28), (32, 32)), ((7, 5), (9, 8)), ((32, 32), (28, 28)), ((28, 28), (64, 64))]


def _images(rng, H, W, n=20):
    a = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    a[1] = 255
    a[2] = (rng.random((H, W)) < 0.5) * np.uint8(255)
    return a


@pytest.mark.parametrize('src,dst', SIZE_PAIRS)
def test_pil_bilinear_tables_against_pil(src, dst):
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(7)
    th, tv = T.pil_bilinear_tables(src[1], dst[1]), T.pil_bilinear_tables(src[0], dst[0])
    for t, size, out in ((th, src[1], dst[1]), (tv, src[0], dst[0])):
        assert t[0].dtype == t[1].dtype == np.int32 and t[0].shape[0] == out and t[1].shape == (out, 2)
        assert (t[1][:, 0] >= 0).all() and (t[1].sum(1) <= size).all() and (t[1][:, 1] <= t[0].shape[1]).all()
        assert (t[0] >= 0).all() and (np.abs(t[0].sum(1) - (1 << 22)) <= t[0].shape[1]).all()
    for a in _images(rng, *src):
        want = np.asarray(Image.fromarray(a, mode='L').resize((dst[1], dst[0]), Image.BILINEAR))
        assert np.array_equal(IC.apply_pil_tables(a, th, tv), want)


def test_pil_bilinear_tables_tap_counts_and_fixture(golden_dir):
    c, b = T.pil_bilinear_tables(28, 32)
    assert c.shape == (32, 3) and b[:, 1].max() == 2           # upscaling: at most 2 taps per axis
    assert T.pil_bilinear_tables(32, 28)[0].shape == (28, 5)
    fx = np.load(os.path.join(golden_dir, 'imagesets', 'pil_resize.npz'))
    for key, (Hr, Wr) in (('28_32', (32, 32)), ('7x5_9x8', (9, 8)), ('32_28', (28, 28))):
        src, out = fx['src_' + key], fx['out_' + key]
        th, tv = T.pil_bilinear_tables(src.shape[2], Wr), T.pil_bilinear_tables(src.shape[1], Hr)
        for a, want in zip(src, out):
            assert np.array_equal(IC.apply_pil_tables(a, th, tv), want), key
    src, out = fx['src_turn_7x5_8x9'], fx['out_turn_7x5_8x9']
    th, tv = T.pil_bilinear_tables(7, 9), T.pil_bilinear_tables(5, 8)
    for a, want in zip(src, out):
        assert np.array_equal(IC.apply_pil_tables(np.rot90(a, 1), th, tv), want)


@pytest.mark.parametrize('gz', [False, True])
def test_idx_reader_plain_and_gzipped(tmp_path, gz):
    want = IC.write_idx_tree(str(tmp_path), 'MNIST', 12, 12, seed=3, gz=gz)
    train, test = T.get_dataset('mnist', root=str(tmp_path), device='cpu')
    for s, split in ((train, 'train'), (test, 'test')):
        assert len(s) == 12 and s.data.dtype == torch.uint8 and tuple(s.data.shape) == (12, 1, 28, 28)
        assert np.array_equal(s.data[:, 0].numpy(), want[split][0]) and np.array_equal(s.targets.numpy(), want[split][1])
        assert s.name == 'mnist' and s.transformer == '' and s.heldout == [] and s.lut is None
        assert s.classes == [str(d) for d in range(10)] and s.same_size == ['const28', 'uniform28', 'fashion', 'letters', 'mnist90']
        assert s.desc.shape == (1, 28, 28)
    only = T.get_dataset('mnist', splits=['test'], root=str(tmp_path), device='cpu')
    assert only[0] is None and len(only[1]) == 12
    padded = T.get_dataset('mnist', transformer='pad', splits=['test'], root=str(tmp_path), device='cpu')[1]
    assert padded.transformer == 'pad' and padded.desc.shape == (1, 32, 32)
    assert T.get_dataset('mnist32p', splits=['test'], root=str(tmp_path), device='cpu')[1].desc.shape == (3, 32, 32)
    assert T.get_dataset('mnist32r', splits=['test'], root=str(tmp_path), device='cpu')[1].desc.shape == (3, 32, 32)
    assert T.get_dataset('mnist90', splits=['test'], root=str(tmp_path), device='cpu')[1].name == 'mnist90'


def test_letters_labels_are_shifted_by_the_table(tmp_path):
    want = IC.write_idx_tree(str(tmp_path), 'EMNIST', 12, 12, seed=4, prefix='emnist-letters-', test_part='test', classes=26,
                             first_label=1)
    s = T.get_dataset('letters', splits=['test'], root=str(tmp_path), device='cpu')[1]
    assert np.array_equal(s.targets.numpy(), want['test'][1]) and s.targets.min() >= 1
    assert s.lut.tolist() == list(range(-1, 26)) and len(s.classes) == 26 and s.classes[0] == 'a'


def test_truncated_and_missing_files_raise(tmp_path):
    with pytest.raises(FileNotFoundError) as e:
        T.get_dataset('mnist', root=str(tmp_path), device='cpu')
    assert os.path.join(str(tmp_path), 'MNIST', 'raw', 'train-images-idx3-ubyte') in str(e.value)
    IC.write_idx_tree(str(tmp_path), 'MNIST', 12, 12, seed=3)
    path = os.path.join(str(tmp_path), 'MNIST', 'raw', 't10k-images-idx3-ubyte')
    raw = open(path, 'rb').read()
    with open(path, 'wb') as f:
        f.write(raw[:-5])
    with pytest.raises(ValueError, match='bytes of data'):
        T.get_dataset('mnist', splits=['test'], root=str(tmp_path), device='cpu')
    os.remove(os.path.join(str(tmp_path), 'MNIST', 'raw', 't10k-labels-idx1-ubyte'))
    with open(path, 'wb') as f:
        f.write(raw)
    with pytest.raises(FileNotFoundError, match='t10k-labels-idx1-ubyte'):
        T.get_dataset('mnist', splits=['test'], root=str(tmp_path), device='cpu')
    with pytest.raises(FileNotFoundError, match='cifar-10-batches-py'):
        T.get_dataset('cifar10', root=str(tmp_path), device='cpu')


def test_cifar_readers_and_heldout(tmp_path):
    want = IC.write_cifar10_tree(str(tmp_path))
    train, test = T.get_dataset('cifar10', root=str(tmp_path), device='cpu')
    assert tuple(train.data.shape) == (20, 32, 32, 3) and tuple(test.data.shape) == (4, 32, 32, 3) and train.nhwc
    assert np.array_equal(train.data.numpy(), want['train'][0]) and np.array_equal(train.targets.numpy(), want['train'][1])
    assert np.array_equal(test.data.numpy(), want['test'][0]) and train.classes[3] == 'cat' and train.lut is None
    held = T.get_dataset('cifar10-3', splits=['train'], root=str(tmp_path), device='cpu', data_augmentation=['flip'])[0]
    keep = want['train'][1] != 3
    assert 0 < keep.sum() < 20 and len(held) == keep.sum()
    assert np.array_equal(held.targets.numpy(), want['train'][1][keep])         # the stored targets keep their numbering
    assert np.array_equal(held.data.numpy(), want['train'][0][keep])
    assert held.lut.tolist() == [0, 1, 2, -1, 3, 4, 5, 6, 7, 8]
    assert held.name == 'cifar10-3' and held.heldout == [3] and held.same_size == ['cifar10+3'] and 'cat' not in held.classes
    assert len(held.classes) == 9 and held.data_augmentation == ('flip',)
    plus = T.get_dataset('cifar10+3', splits=['test'], root=str(tmp_path), device='cpu')[1]
    assert plus.name == 'cifar10+3' and plus.classes == ['cat'] and len(plus) == int((want['test'][1] == 3).sum())
    want = IC.write_cifar100_tree(str(tmp_path))
    train, test = T.get_dataset('cifar100', root=str(tmp_path), device='cpu')
    for s, split in ((train, 'train'), (test, 'test')):
        assert np.array_equal(s.data.numpy(), want[split][0]) and np.array_equal(s.targets.numpy(), want[split][1])
        assert len(s.classes) == 100 and s.classes[1] == 'aquarium fish'


def test_svhn_reader(tmp_path):
    pytest.importorskip('scipy')
    want = IC.write_svhn_tree(str(tmp_path))
    train, test = T.get_dataset('svhn', root=str(tmp_path), device='cpu')
    for s, split in ((train, 'train'), (test, 'test')):
        assert tuple(s.data.shape) == (5, 3, 32, 32) and not s.nhwc
        assert np.array_equal(s.data.numpy(), want[split][0]) and np.array_equal(s.targets.numpy(), want[split][1])
        assert s.targets[1] == 0 and s.targets.max() <= 9


def test_sets_outside_the_build_are_refused_by_name(tmp_path):
    for name in ('lsunc', 'lsunr', 'dtd', 'random300k', 'imagenet1k'):
        with pytest.raises(NotImplementedError, match=name):
            T.get_dataset(name, root=str(tmp_path), device='cpu')
    T.REGISTRY['_probe'] = dict(T.REGISTRY['mnist'], pre_transform='center-crop-20')
    try:
        with pytest.raises(NotImplementedError, match='_probe'):
            T.chain_of('_probe', (28, 28, 1), False, '')
        T.REGISTRY['_probe']['pre_transform'] = 'pad-2 hflip pad-2'
        with pytest.raises(NotImplementedError, match='_probe'):
            T.chain_of('_probe', (28, 28, 1), False, '')
    finally:
        del T.REGISTRY['_probe']
    const = T.get_dataset('const32', splits=['test'], device='cpu')[1]
    assert len(const) == 10000 and const.name == 'const32' and const.same_size[-1] == 'const3290'


def test_device_loader_index_order_and_generator_use(monkeypatch):
    """The index batches of device_loader(shuffle=True) over a Subset chain are those of DataLoader(shuffle=True,
    num_workers=0) over range(n), and the global generator ends in the same state.  The production of x is stubbed."""
    n = 23
    base = T.DeviceImageSet('probe', torch.zeros((n, 1, 2, 2), dtype=torch.uint8), False, torch.arange(n), None, None, (1, 2, 2),
                            classes=['0'])
    seen = []
    monkeypatch.setattr(T.DeviceImageSet, 'batch', lambda self, idx, aug=(), gen=None: (seen.append(idx.clone()), idx)[1:] * 2)
    first = torch.utils.data.Subset(base, [22, 0, 5, 7, 9, 11, 13, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 1, 3])
    chain = torch.utils.data.Subset(first, [18, 3, 4, 0, 1, 2, 17, 16, 9, 8, 7, 12, 11])
    composed = torch.as_tensor(first.indices)[torch.as_tensor(chain.indices)]
    assert T.device_loader(torch.utils.data.TensorDataset(torch.zeros(4)), 5, True) is None
    assert T.device_loader([1, 2, 3], 5, True) is None
    for dset, indices in ((base, None), (first, torch.as_tensor(first.indices)), (chain, composed)):
        for s in (0, 5):
            torch.manual_seed(s)
            want = [b.clone() for b in torch.utils.data.DataLoader(range(len(dset)), batch_size=5, shuffle=True, num_workers=0)]
            state = torch.get_rng_state()
            torch.manual_seed(s)
            del seen[:]
            loader = T.device_loader(dset, 5, True)
            assert len(loader) == len(want)
            got = [b[0] for b in loader]
            assert torch.equal(torch.get_rng_state(), state)
            assert len(got) == len(want) and sorted(torch.cat(want).tolist()) == list(range(len(dset)))
            for a, b in zip(got, want):
                assert torch.equal(a, b if indices is None else indices[b])
            again = [b[0] for b in loader]                     # re-iterable: a new epoch, a new order
            assert len(again) == len(want)
    plain = [b[0] for b in T.device_loader(chain, 5, False)]
    assert torch.equal(torch.cat(plain), composed)


def test_batch_refuses_bad_indices_on_the_host():
    base = T.DeviceImageSet('probe', torch.zeros((9, 1, 2, 2), dtype=torch.uint8), False, torch.arange(9), None, None, (1, 2, 2),
                            classes=['0'])
    for bad in ([9], [0, -10], torch.tensor([3, 9])):
        with pytest.raises(IndexError):
            base.batch(bad)
    assert base._indices([-1, 0, -9]).tolist() == [8, 0, 0]
    with pytest.raises(ValueError):
        base.batch([0], data_augmentation=['rotate'])
