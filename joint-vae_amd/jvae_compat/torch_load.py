"""Named image sets, resident on the device (the reference's utils/torch_load.py:312-523 and data/sets.ini, without
torchvision): `get_dataset('cifar10-3')` reads the raw files torchvision leaves on disk, keeps the uint8 images and labels
on the GPU and hands out `DeviceImageSet`s whose batches come from ONE kernel launch (`ops.imageset_batch`,
csrc/imageset.hip) - gather by sample index, the set's static transform chain, the random flip / crop when asked, /255.
`mixed_loader` does the same for a moving set of jvae_compat/ft_datasets.py, whose batches mix several resident sets:
`ops.imageset_mixed_batch`, one launch per batch as well.

The static chain has eight fixed slots, in the reference's order (utils/torch_load.py:347-426):
    A (quarter turns / flip) -> resize (PIL 8-bit bilinear) -> zero padding -> B (quarter turns / flip) -> g2c
    -> [random flip, edge-padded random crop] -> post transform ('pad' | 'crop' | nothing) -> / 255
A `pre_transform` these slots cannot express is refused by name (NotImplementedError); so are the folder / JPEG sets.
Nothing is ever downloaded: a missing file raises FileNotFoundError with the path that was looked for."""
import gzip
import logging
import os
import pickle
import string
import struct

import numpy as np
import torch
import torch.nn.functional as F

from jvae_hip import ops

SYNTHETIC_LENGTH = 10000

_FASHION = 't-shirt/top trouser pullover dress coat sandal shirt sneaker bag ankle_boot'
_LSUN = 'bedroom bridge church class conference dining kitchen living restaurant tower'
_DTD = ('banded blotchy braided bubbly bumpy chequered cobwebbed cracked crosshatched crystalline dotted fibrous flecked '
        'freckled frilly gauzy grid grooved honeycombed interlaced knitted lacelike lined marbled matted meshed paisley '
        'perforated pitted pleated polka-dotted porous potholed scaly smeared spiralled sprinkled stained stratified striped '
        'studded swirly veined waffled woven wrinkled zigzagged')
_CIFAR100 = ('apple aquarium_fish baby bear beaver bed bee beetle bicycle bottle bowl boy bridge bus butterfly camel can castle '
             'caterpillar cattle chair chimpanzee clock cloud cockroach couch crab crocodile cup dinosaur dolphin elephant '
             'flatfish forest fox girl hamster house kangaroo keyboard lamp lawn_mower leopard lion lizard lobster man '
             'maple_tree motorcycle mountain mouse mushroom oak_tree orange orchid otter palm_tree pear pickup_truck pine_tree '
             'plain plate poppy porcupine possum rabbit raccoon ray road rocket rose sea seal shark shrew skunk skyscraper '
             'snail snake spider squirrel streetcar sunflower sweet_pepper table tank telephone television tiger tractor train '
             'trout tulip turtle wardrobe whale willow_tree wolf woman worm')
_DIGITS = ' '.join(str(d) for d in range(10))


def _entry(shape, classes=None, pre='', target=None, default='', files=None, labels=None):
    names = [c.replace('_', ' ') for c in classes.split()] if classes else None
    return dict(shape=tuple(shape), classes=names, labels=len(names) if names else (labels or 0), pre_transform=pre,
                target_transform=target, default_transform=default, files=files)


# The sets, in the order their same-size siblings are listed.  `files`: which reader and where under the root (None: no raw
# files this build reads).  Class names are the data sets' own; an underscore stands for a blank.
REGISTRY = {
    'const28': _entry((1, 28, 28), pre='already_tensor', files=('const',)),
    'const32': _entry((3, 32, 32), pre='already_tensor', files=('const',)),
    'uniform28': _entry((1, 28, 28), pre='already_tensor', files=('uniform',)),
    'uniform32': _entry((3, 32, 32), pre='already_tensor', files=('uniform',)),
    'mnist': _entry((1, 28, 28), _DIGITS, files=('idx', 'MNIST', '{}-images-idx3-ubyte', '{}-labels-idx1-ubyte', 'train', 't10k')),
    'mnist32p': _entry((3, 32, 32), _DIGITS, pre='tensor g2c pad-2',
                       files=('idx', 'MNIST', '{}-images-idx3-ubyte', '{}-labels-idx1-ubyte', 'train', 't10k')),
    'mnist32r': _entry((3, 32, 32), _DIGITS, pre='resize tensor g2c',
                       files=('idx', 'MNIST', '{}-images-idx3-ubyte', '{}-labels-idx1-ubyte', 'train', 't10k')),
    'fashion': _entry((1, 28, 28), _FASHION,
                      files=('idx', 'FashionMNIST', '{}-images-idx3-ubyte', '{}-labels-idx1-ubyte', 'train', 't10k')),
    'fashion32p': _entry((3, 32, 32), _FASHION, pre='tensor g2c pad-2',
                         files=('idx', 'FashionMNIST', '{}-images-idx3-ubyte', '{}-labels-idx1-ubyte', 'train', 't10k')),
    'fashion32r': _entry((3, 32, 32), _FASHION, pre='resize tensor g2c',
                         files=('idx', 'FashionMNIST', '{}-images-idx3-ubyte', '{}-labels-idx1-ubyte', 'train', 't10k')),
    'letters': _entry((1, 28, 28), ' '.join(string.ascii_lowercase), pre='rotate-270 hflip', target='y-1',
                      files=('idx', 'EMNIST', 'emnist-letters-{}-images-idx3-ubyte', 'emnist-letters-{}-labels-idx1-ubyte',
                             'train', 'test')),
    'cifar10': _entry((3, 32, 32), 'airplane automobile bird cat deer dog frog horse ship truck', files=('cifar10', 'cifar10')),
    'cifar100': _entry((3, 32, 32), _CIFAR100, files=('cifar100', 'cifar100')),
    'svhn': _entry((3, 32, 32), _DIGITS, files=('svhn', 'svhn')),
    'lsunc': _entry((3, 32, 32), _LSUN, pre='crop'),
    'lsunr': _entry((3, 32, 32), _LSUN, pre='tensor center-crop-256 resize'),
    'dtd': _entry((3, 32, 32), _DTD, pre='center-crop-256 resize-32 crop'),
    'random300k': _entry((3, 32, 32)),
    'imagenet1k': _entry((3, 224, 224), pre='resize-256', default='crop', labels=1000),
    'imagenet20': _entry((3, 224, 224), pre='resize-256', default='crop', labels=20),
    'imagenet2': _entry((3, 224, 224), pre='resize-256', default='crop', labels=2),
}


# ------------------------------------------------------------------------------------------------- names
def get_heldout_classes_by_name(dataset):
    """'cifar10-3-1' -> ('cifar10', [1, 3]); 'cifar10+7+9' -> ('cifar10', every class but 7 and 9); plain -> (name, [])."""
    if '-' in dataset:
        parent, *held = dataset.split('-')
        return parent, sorted(int(c) for c in held)
    if '+' in dataset:
        parent, *kept = dataset.split('+')
        C = get_shape_by_name(parent)[-1]
        return parent, [c for c in range(C) if str(c) not in kept]
    return dataset, []


def get_name_by_heldout_classes(dataset, *heldout):
    """The '-' form, or the '+' form once more than half of the classes are held out."""
    if not heldout:
        return dataset
    C = get_shape_by_name(dataset)[-1]
    heldout = sorted(heldout)
    if len(heldout) / C > 0.5:
        return dataset + '+' + '+'.join(str(c) for c in range(C) if c not in heldout)
    return dataset + '-' + '-'.join(str(c) for c in heldout)


def get_shape_by_name(set_name, transform='default'):
    """-> ((C, H, W), number of labels); a '...90' name swaps H and W (and ignores `transform`, as the reference does);
    'pad' adds 2 on every side; (None, None) for a name outside the registry."""
    if set_name.endswith('90'):
        shape, labels = get_shape_by_name(set_name[:-2])
        return (shape[0], shape[2], shape[1]), labels
    set_name, heldout = get_heldout_classes_by_name(set_name)
    if set_name not in REGISTRY:
        return None, None
    shape = REGISTRY[set_name]['shape']
    labels = REGISTRY[set_name]['labels'] - len(heldout)
    if transform != 'pad':
        return shape, labels
    return (shape[0], shape[1] + 4, shape[2] + 4), labels


def get_same_size_by_name(set_name, rotated=False):
    """The sets an OOD evaluation of `set_name` runs against: the held-out complement of a held-out name, else every registered
    set of the same shape, the quarter-turned set itself last."""
    if set_name.endswith('-?'):
        return [set_name[:-2] + '+?']
    if set_name.endswith('90'):
        return get_same_size_by_name(set_name[:-2], rotated=True)
    parent, heldout = get_heldout_classes_by_name(set_name)
    if heldout:
        C = get_shape_by_name(parent)[-1]
        return [get_name_by_heldout_classes(parent, *[c for c in range(C) if c not in heldout])]
    if set_name not in REGISTRY:
        return []
    shape = REGISTRY[set_name]['shape']
    same = [s for s, p in REGISTRY.items() if p['shape'] == shape]
    if not rotated:
        same.remove(set_name)
        same.append(set_name + '90')
    return same


def get_classes_by_name(dataset, texify=False):
    if dataset.endswith('90'):
        return get_classes_by_name(dataset[:-2])
    parent, heldout = get_heldout_classes_by_name(dataset)
    classes = REGISTRY[parent]['classes'] or [parent]
    return [str(c).replace('_', '-') if texify else c for i, c in enumerate(classes) if i not in heldout]


# ------------------------------------------------------------------------------------------------- PIL's bilinear resize
def pil_bilinear_tables(in_size, out_size):
    """-> (coeffs int32 (out, ksize), bounds int32 (out, 2) = first source index, count): the per-axis tables of PIL's 8-bit
    bilinear resampling (precompute_coeffs + normalize_coeffs_8bpc), 22-bit fixed point.  A pass is
    clip8((2^21 + sum_k coeffs[o, k] * src[bounds[o, 0] + k]) >> 22)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale                         # the bilinear filter's own support is 1
    ksize = 2 * int(np.ceil(support)) + 1
    coeffs = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = 1.0 - np.abs((np.arange(xmax - xmin) + xmin - center + 0.5) / filterscale)
        w = np.where(w > 0.0, w, 0.0)
        total = w.sum()
        if total != 0.0:
            w = w / total
        coeffs[xx, :xmax - xmin] = [int(0.5 + v * (1 << 22)) for v in w]
        bounds[xx] = (xmin, xmax - xmin)
    return coeffs, bounds


# ------------------------------------------------------------------------------------------------- the chain of a name
def _compose(element, turns=0, flip=False):
    """(k, f) = k counter-clockwise quarter turns then a flip when f; followed by `turns` more turns / one more flip."""
    k, f = element
    if turns:
        k = (k - turns) % 4 if f else (k + turns) % 4
    if flip:
        f = not f
    return k, f


def chain_of(name, source, nhwc, transformer, device=None):
    """The static chain of the set `name` (a '...90' name included, held-out suffixes already removed) over raw images of
    extents `source` = (Hs, Ws, Cs) -> ops.ImagesetDesc.  `transformer`: '' | 'pad' | 'crop' (already resolved)."""
    rotated = name.endswith('90')
    parent = name[:-2] if rotated else name
    props = REGISTRY[parent]
    tokens = (['rotate-90'] if rotated else []) + props['pre_transform'].split()
    A, B, stage, resize, p0, g2c, as_tensor = (0, False), (0, False), 0, None, 0, False, False

    def refuse(why):
        return NotImplementedError('{}: pre_transform {!r} {} (jvae_compat/torch_load.py builds quarter turns / flips, one '
                                   'PIL resize, one zero padding, quarter turns / flips, g2c)'.format(name, ' '.join(tokens), why))
    Hs, Ws, Cs = source
    H, W = Hs, Ws
    for t in tokens:
        if t.startswith('rotate') or t == 'hflip':
            turns = 0
            if t != 'hflip':
                angle = int(t.split('-')[-1])
                if angle % 90:
                    raise refuse('turns by an angle that is no multiple of 90')
                turns = (angle // 90) % 4
            if stage == 0:
                A = _compose(A, turns, t == 'hflip')
            else:
                stage = 3
                B = _compose(B, turns, t == 'hflip')
            if turns & 1:
                H, W = W, H
        elif t.startswith('resize'):
            if stage != 0 or as_tensor:
                raise refuse('resizes a tensor, or after another stage' if as_tensor else 'resizes after another stage')
            dims = [int(v) for v in t.split('-')[1:]]
            if len(dims) == 1:
                raise refuse('resizes the smaller edge')
            Hr, Wr = dims if dims else props['shape'][1:]
            resize = (Hr, Wr, *pil_bilinear_tables(W, Wr), *pil_bilinear_tables(H, Hr))
            H, W, stage = Hr, Wr, 1
        elif t.startswith('pad'):
            if stage > 1:
                raise refuse('pads after the second turn')
            p0, stage = 2, 2                      # the reference pads by 2 whatever the token says (utils/torch_load.py:381-386)
            H, W = H + 4, W + 4
        elif t == 'g2c':
            g2c = True
        elif t == 'tensor':
            as_tensor = True
        elif t == 'already_tensor':
            pass
        else:
            raise refuse('holds the token {!r}, which is outside this build'.format(t))
    post = None
    if transformer == 'pad':
        post = 'pad'
    elif transformer == 'crop':
        post = ('crop', *props['shape'][1:])
    elif transformer:
        raise ValueError('transformer {!r}: default, pad or crop'.format(transformer))
    return ops.ImagesetDesc(source, nhwc, A=A[0] + 4 * A[1], resize=resize, p0=p0, B=B[0] + 4 * B[1], g2c=g2c, post=post,
                            device=device)


# ------------------------------------------------------------------------------------------------- readers
def _existing(*paths):
    for p in paths:
        if os.path.exists(p):
            return p
    raise FileNotFoundError('no such data set file: ' + ' (nor '.join(paths) + ')' * (len(paths) - 1))


def read_idx(path):
    """An idx file (the MNIST format), plain or gzipped -> uint8 array of the dimensions its header states."""
    with (gzip.open if path.endswith('.gz') else open)(path, 'rb') as f:
        raw = f.read()
    if len(raw) < 4 or raw[:3] != b'\x00\x00\x08':
        raise ValueError('{}: not an unsigned-byte idx file'.format(path))
    ndim = raw[3]
    if len(raw) < 4 + 4 * ndim:
        raise ValueError('{}: truncated idx header'.format(path))
    dims = struct.unpack('>' + 'I' * ndim, raw[4:4 + 4 * ndim])
    count = int(np.prod(dims, dtype=np.int64))
    if len(raw) - 4 - 4 * ndim != count:
        raise ValueError('{}: {} bytes of data for dimensions {}'.format(path, len(raw) - 4 - 4 * ndim, dims))
    return np.frombuffer(raw, np.uint8, count, 4 + 4 * ndim).reshape(dims)


def _read_idx_pair(root, spec, split):
    _, folder, images, labels, train, test = spec
    part = train if split == 'train' else test
    found = []
    for pattern in (images, labels):
        base = os.path.join(root, folder, 'raw', pattern.format(part))
        found.append(read_idx(_existing(base, base + '.gz')))
    x, y = found
    if x.ndim != 3 or y.ndim != 1 or len(x) != len(y):
        raise ValueError('{} {}: images {} and labels {} do not belong together'.format(folder, split, x.shape, y.shape))
    return x[:, None], False, y


def _unpickle(path):
    with open(path, 'rb') as f:
        return pickle.load(f, encoding='latin1')


def _cifar_arrays(path, key, x, y):
    d = _unpickle(path)
    images, labels = np.asarray(d['data'], np.uint8), list(d[key])
    if images.ndim != 2 or images.shape[1] != 3072 or len(labels) != len(images):
        raise ValueError('{}: data {} with {} labels'.format(path, images.shape, len(labels)))
    x.append(images.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
    y.extend(labels)


def _read_cifar10(root, spec, split):
    files = ['data_batch_{}'.format(i) for i in range(1, 6)] if split == 'train' else ['test_batch']
    x, y = [], []
    for name in files:
        tail = os.path.join('cifar-10-batches-py', name)
        _cifar_arrays(_existing(os.path.join(root, spec[1], tail), os.path.join(root, tail)), 'labels', x, y)
    return np.concatenate(x), True, np.asarray(y)


def _read_cifar100(root, spec, split):
    tail = os.path.join('cifar-100-python', split)
    x, y = [], []
    _cifar_arrays(_existing(os.path.join(root, spec[1], tail), os.path.join(root, tail)), 'fine_labels', x, y)
    return x[0], True, np.asarray(y)


def _read_svhn(root, spec, split):
    tail = '{}_32x32.mat'.format(split)
    path = _existing(os.path.join(root, spec[1], tail), os.path.join(root, tail))
    from scipy.io import loadmat                  # only the SVHN reader needs scipy
    d = loadmat(path)
    x, y = np.asarray(d['X']), np.asarray(d['y']).astype(np.int64).reshape(-1)
    if x.ndim != 4 or x.shape[:3] != (32, 32, 3) or x.dtype != np.uint8 or x.shape[3] != len(y):
        raise ValueError('{}: X {} {} with {} labels'.format(path, x.shape, x.dtype, len(y)))
    y[y == 10] = 0
    return x.transpose(3, 2, 0, 1), False, y


_READERS = {'idx': _read_idx_pair, 'cifar10': _read_cifar10, 'cifar100': _read_cifar100, 'svhn': _read_svhn}


# ------------------------------------------------------------------------------------------------- the set object
def _augmentation_padding(name, tokens, height):
    unknown = [t for t in tokens if t not in ('flip', 'crop')]
    if unknown:
        raise ValueError('data_augmentation: only flip and crop exist (utils/torch_load.py:405-413), got {}'.format(unknown))
    if 'crop' not in tokens:
        return 0
    return 0 if 'imagenet' in name else height // 8


class DeviceImageSet(torch.utils.data.Dataset):
    """A named image set whose raw uint8 images (`.data`) and labels (`.targets`, original numbering) live on the device.
    `batch(indices)` is the fast path - one launch; `set[i]` goes through it with one index.  The held-out classes were
    removed at construction; `.lut` re-numbers the stored targets (held-out re-numbering, `y-1`), None = as they are."""

    def __init__(self, name, data, nhwc, targets, lut, desc, shape, classes, heldout=(), same_size=(), transformer='',
                 data_augmentation=()):
        self.name, self.same_size, self.transformer = name, list(same_size), transformer
        self.classes, self.heldout = list(classes), list(heldout)
        self.data, self.targets, self.lut, self.desc, self.nhwc = data, targets, lut, desc, nhwc
        self.shape = tuple(shape)                 # the registry's (C, H, W): the random crop's padding is H // 8
        self.data_augmentation = tuple(data_augmentation)
        _augmentation_padding(name, self.data_augmentation, self.shape[1])

    @property
    def device(self):
        return self.targets.device

    def to(self, device):
        device = torch.device(device)
        self.targets = self.targets.to(device)
        if self.data is not None:
            self.data = self.data.to(device)
            self.desc = ops.ImagesetDesc(**dict(self.desc._args, device=device))
        if self.lut is not None:
            self.lut = self.lut.to(device)
        return self

    def __len__(self):
        return int(self.targets.shape[0])

    def _indices(self, indices):
        if torch.is_tensor(indices):
            if indices.device.type != 'cpu':
                raise TypeError('DeviceImageSet.batch takes CPU indices (they are range-checked on the host before the upload), '
                                'not a tensor on ' + str(indices.device))
            idx = indices.to(torch.int64).reshape(-1)
        else:
            idx = torch.as_tensor([int(i) for i in indices], dtype=torch.int64)
        n = len(self)
        if idx.numel() and (int(idx.min()) < -n or int(idx.max()) >= n):
            raise IndexError('index out of range for the {} samples of {}'.format(n, self.name))
        return torch.where(idx < 0, idx + n, idx)

    def batch(self, indices, data_augmentation=(), generator=None):
        """-> (x float32 (N, C, H, W), y int64 (N,)) on the set's device, for CPU `indices` (sequence or tensor; checked here).
        `data_augmentation`: 'flip' / 'crop' tokens, drawn by ops.draw_augmentation in its order; empty = the set's own list."""
        idx = self._indices(indices)
        tokens = tuple(data_augmentation) or self.data_augmentation
        pa = _augmentation_padding(self.name, tokens, self.shape[1])
        return self._produce(idx, tokens, pa, generator)

    def _produce(self, idx, tokens, pa, generator):
        device = self.data.device
        flip, dy, dx = ops.draw_augmentation(idx.numel(), pa, device, generator=generator, flip='flip' in tokens, crop=pa > 0)
        return ops.imageset_batch(self.data, idx.to(device), self.desc.with_pa(pa), self.targets, self.lut, flip, dy, dx)

    def __getitem__(self, i):
        x, y = self.batch([i])
        return x[0], int(y[0])


class SyntheticImageSet(DeviceImageSet):
    """`const*` (one uniform colour per channel and image) and `uniform*` (uniform noise): drawn with torch.rand on the device,
    SYNTHETIC_LENGTH samples, label 0.  Only the distribution is that of utils/torch_load.py:150-186."""

    def __init__(self, name, kind, shape, device, **kw):
        super().__init__(name, None, False, torch.zeros(SYNTHETIC_LENGTH, dtype=torch.int64, device=device), None, None, shape,
                         **kw)
        self.kind, self.image_shape = kind, tuple(shape)

    def _produce(self, idx, tokens, pa, generator):
        if tokens:
            raise NotImplementedError('{}: synthetic sets are not augmented'.format(self.name))
        C, H, W = self.image_shape
        N, device = idx.numel(), self.targets.device
        if self.kind == 'const':
            x = torch.rand((N, C, 1, 1), device=device).expand(N, C, H, W).contiguous()
        else:
            x = torch.rand((N, C, H, W), device=device)
        if self.transformer == 'pad':
            x = F.pad(x, (2, 2, 2, 2))
        return x, torch.zeros(N, dtype=torch.int64, device=device)


def get_dataset(dataset='mnist', transformer='default', data_augmentation=[], splits=['train', 'test'], root=None, device=None):
    """-> (trainset, testset): DeviceImageSets of the named set read from the torchvision-style directory `root`, None for a
    split not asked for.  Names: the registry's, with '-c-d' / '+c+d' held-out suffixes and a trailing '90' (one
    counter-clockwise quarter turn first).  `data_augmentation` becomes the TRAIN set's own list."""
    dataset = dataset.lower()
    rotated = dataset.endswith('90')
    if rotated:
        dataset = dataset[:-2]
    parent, heldout = get_heldout_classes_by_name(dataset)
    if parent not in REGISTRY:
        raise KeyError(parent)
    props = REGISTRY[parent]
    if transformer == 'default':
        transformer = props['default_transform']
    if props['files'] is None:
        raise NotImplementedError('{}: folder / JPEG sets and their pre_transform {!r} are outside this build'.format(
            parent, props['pre_transform']))
    if device is None:
        device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    device = torch.device(device)
    C = props['labels']
    same_size = get_same_size_by_name(get_name_by_heldout_classes(parent, *heldout))
    classes = props['classes'] or [str(i) for i in range(C)]
    name = parent + ('90' if rotated else '')
    if heldout:
        classes = [c for i, c in enumerate(classes) if i not in heldout]
        if len(heldout) < C / 2:
            name += '-' + '-'.join(str(c) for c in heldout)
        else:
            name += '+' + '+'.join(str(c) for c in range(C) if c not in heldout)
    shape = props['shape']
    if rotated:
        shape = (shape[0], shape[2], shape[1])
    common = dict(classes=classes, heldout=heldout, same_size=same_size, transformer=transformer)
    out = []
    for split in ('train', 'test'):
        own = tuple(data_augmentation) if split == 'train' else ()
        if split not in splits:
            out.append(None)
        elif props['files'][0] in ('const', 'uniform'):
            if transformer not in ('', 'pad'):
                raise ValueError('{}: transformer {!r}'.format(name, transformer))
            out.append(SyntheticImageSet(name, props['files'][0], shape, device, data_augmentation=own, **common))
        else:
            if root is None:
                raise FileNotFoundError('{}: no data root given'.format(name))
            out.append(_load_split(parent, rotated, name, split, heldout, root, device, shape, transformer, own, common))
    return tuple(out)


def _load_split(parent, rotated, name, split, heldout, root, device, shape, transformer, own, common):
    props = REGISTRY[parent]
    chain_name = parent + ('90' if rotated else '')
    x, nhwc, y = _READERS[props['files'][0]](str(root), props['files'], split)
    y = np.asarray(y).astype(np.int64)
    C = props['labels']
    shift = 1 if props['target_transform'] == 'y-1' else 0
    if len(y) and (y.min() < 0 or y.max() >= C + shift):
        raise ValueError('{} {}: labels in [{}, {}] for {} classes'.format(parent, split, y.min(), y.max(), C))
    # the label table: the set's own target transform, then the held-out re-numbering; -1 = the sample is left out
    table = np.arange(C + shift, dtype=np.int64) - shift
    if heldout:
        renumber = {c: i for i, c in enumerate(c for c in range(C) if c not in heldout)}
        table = np.asarray([renumber.get(int(v), -1) for v in table], np.int64)
    keep = table[y] >= 0
    x, y = np.ascontiguousarray(x[keep]), y[keep]
    identity = len(table) == C and bool((table == np.arange(C)).all())
    source = (x.shape[1], x.shape[2], x.shape[3]) if nhwc else (x.shape[2], x.shape[3], x.shape[1])
    desc = chain_of(chain_name, source, nhwc, transformer, device=device)
    return DeviceImageSet(name, torch.from_numpy(x).to(device), nhwc, torch.from_numpy(y).to(device),
                          None if identity else torch.from_numpy(table).to(device), desc, shape, data_augmentation=own, **common)


# ------------------------------------------------------------------------------------------------- loaders
class _Indices(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class DeviceBatches:
    """Re-iterable of device batches of a DeviceImageSet (behind Subsets: `indices`).  The index batches come from a DataLoader
    run over the bare sample numbers, so the order of the samples and what the shuffling draws from the global generator are
    those of a DataLoader over the data set itself."""

    def __init__(self, base, indices, batch_size, shuffle, data_augmentation=(), generator=None):
        self.base, self.indices = base, indices
        self.data_augmentation, self.generator = tuple(data_augmentation), generator
        n = len(base) if indices is None else len(indices)
        self.loader = torch.utils.data.DataLoader(_Indices(n), batch_size=batch_size, shuffle=shuffle, num_workers=0)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for idx in self.loader:
            if self.indices is not None:
                idx = self.indices[idx]
            yield self.base.batch(idx, self.data_augmentation, self.generator)


def device_loader(dset, batch_size, shuffle, data_augmentation=(), generator=None):
    """DeviceBatches over `dset` if it is a DeviceImageSet behind any chain of torch Subsets (the seeded random_split of
    train_model), `SubSampledDataset`s over one set and `NamedView`s (the sub-sets the fine-tuning loop scores), the indices
    composed on the host; else None: the caller keeps its DataLoader."""
    from jvae_compat.ft_datasets import NamedView, SubSampledDataset
    base, indices = dset, None
    while True:
        if isinstance(base, torch.utils.data.Subset):
            idx, base = torch.as_tensor(base.indices, dtype=torch.int64), base.dataset
        elif isinstance(base, NamedView):
            base = base.dataset
            continue
        elif isinstance(base, SubSampledDataset):
            leaves, _, index, _ = base.resolve()
            if len(leaves) != 1 or hasattr(base._source, 'resolve'):     # over a mixture the items are (x, tag), not (x, y)
                return None
            idx, base = torch.tensor(index), leaves[0]
        else:
            break
        indices = idx if indices is None else idx[indices]
    if not isinstance(base, DeviceImageSet):
        return None
    return DeviceBatches(base, indices, batch_size, shuffle, data_augmentation, generator)


class MixedBatches:
    """Re-iterable of the (x, tag) device batches of a resolved moving set (`SubSampledDataset` / `MixtureDataset` of
    jvae_compat.ft_datasets) whose leaves are all resident on one device: ONE launch per batch (`ops.imageset_mixed_batch`)
    whatever the number of sets, layouts and chains in it, plus one torch.rand when a synthetic leaf is in the set.  The index
    batches come from a DataLoader over the bare positions, as in `DeviceBatches`.  The table on the device is built again when
    the set was shrunk, barred or moved since the last epoch."""

    def __init__(self, moving_set, device, batch_size, shuffle, drop_last):
        self.moving_set, self.device, self.table = moving_set, device, None
        self.loader = torch.utils.data.DataLoader(_Indices(len(moving_set)), batch_size=batch_size, shuffle=shuffle,
                                                  drop_last=drop_last, num_workers=0)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        resolved = self.moving_set.resolve()
        if self.table is None or not self.table.matches(*resolved):
            self.table = ops.ImagesetMixTable(*resolved, self.device)
            if self.table.n_items != self.loader.dataset.n:
                raise RuntimeError('{}: {} items, the loader was made for {}'.format(
                    getattr(self.moving_set, 'name', 'moving set'), self.table.n_items, self.loader.dataset.n))
        table = self.table
        C, H, W = table.shape
        for idx in self.loader:
            n = idx.numel()
            if n and (int(idx.min()) < 0 or int(idx.max()) >= table.n_items):
                raise IndexError('position out of range for the {} items of the moving set'.format(table.n_items))
            u = None
            if table.u_dims:
                u = torch.rand((n, C) if table.u_dims == 2 else (n, C, H, W), device=self.device)
            x, tag, _ = ops.imageset_mixed_batch(table, idx.to(self.device), u)
            yield x, tag


def mixed_loader(moving_set, batch_size, shuffle, drop_last):
    """MixedBatches over `moving_set` when it resolves (`resolve()`) to DeviceImageSets / SyntheticImageSets that are all on one
    device, else None: the caller keeps its DataLoader.  Sample order and use of the global generator are those of a DataLoader
    over the set itself; the images are too unless a synthetic leaf is in the set (its noise is drawn per batch, not per item)."""
    if not hasattr(moving_set, 'resolve'):
        return None
    leaves = moving_set.resolve()[0]
    if not leaves or not all(isinstance(l, DeviceImageSet) for l in leaves):
        return None
    devices = {l.device for l in leaves}
    if len(devices) != 1 or next(iter(devices)).type == 'cpu':
        return None
    return MixedBatches(moving_set, next(iter(devices)), batch_size, shuffle, drop_last)


def open_named(name, transformer, root, device, split='test', data_augmentation=()):
    """One split of a named set for the loops' `DATA_ROOT` opt-in."""
    sets = get_dataset(name, transformer=transformer, data_augmentation=list(data_augmentation), splits=[split], root=root,
                       device=device)
    return sets[0] if split == 'train' else sets[1]


def open_siblings(testset, root, device):
    """The same-size sets of `testset` that can be opened (utils/cvae.py's `oodsets=None`): one log line per sibling whose
    files are not under the root or whose transform is not built; none left raises."""
    found = []
    for name in testset.same_size:
        try:
            found.append(open_named(name, testset.transformer, root, device))
        except (FileNotFoundError, NotImplementedError) as e:
            logging.warning('OOD set %s of %s is left out: %s', name, testset.name, e)
    if not found:
        raise FileNotFoundError('none of the same-size sets of {} ({}) can be opened under {}'.format(
            testset.name, ', '.join(testset.same_size), root))
    return found
