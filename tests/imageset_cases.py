"""Expected values for the device-resident image sets (tests/test_21_imagesets_gpu.py, tests/test_torch_load_host.py), written
with the torch-CPU calls the torchvision chain of utils/torch_load.py:347-426 consists of: torch.rot90(x, k, (-2, -1)) for a
counter-clockwise quarter turn, x.flip(-1), F.pad(mode='constant'), F.pad(mode='replicate') + slicing for the edge-padded
crop, x.repeat(3, 1, 1) for g2c and x.to(float32).div(255) for ToTensor - as oracle/augment_oracle.py does for the two
transforms it covers.  The resize is never recomputed here: its expected bytes come from PIL itself
(tests/golden/imagesets/pil_resize.npz); `apply_pil_tables` is the numpy restatement the host test holds against PIL."""
import gzip
import os
import pickle
import struct

import numpy as np
import torch
import torch.nn.functional as F


def turn(x, e):
    """Element e = k + 4 f on (..., H, W): k counter-clockwise quarter turns, then a horizontal flip when f."""
    x = torch.rot90(x, e & 3, (-2, -1))
    return x.flip(-1) if e >> 2 else x


def centre_crop(x, th, tw):
    h, w = x.shape[-2:]
    i, j = int(round((h - th) / 2.)), int(round((w - tw) / 2.))
    return x[..., i:i + th, j:j + tw]


def expected_batch(images, A=0, resized=None, p0=0, B=0, g2c=False, flip=None, dy=None, dx=None, pa=0, post=None):
    """images: uint8 (N, C, H, W), already gathered -> float32 (N, C', H', W').  `resized`: the uint8 (N, C, Hr, Wr) images the
    resize makes of turn(images, A) (from the PIL fixture), or None.  post: None | 'pad' | ('crop', th, tw)."""
    out = []
    for n in range(images.shape[0]):
        x = turn(images[n], A) if resized is None else resized[n]
        x = x.to(torch.float32)                                # whole numbers: exact, and F.pad takes floats
        if p0:
            x = F.pad(x, (p0, p0, p0, p0), mode='constant', value=0.)
        x = turn(x, B)
        if g2c:
            x = x.repeat(3, 1, 1)
        if flip is not None and bool(flip[n]):
            x = x.flip(-1)
        if dy is not None:
            H, W = x.shape[-2:]
            x = F.pad(x.unsqueeze(0), (pa, pa, pa, pa), mode='replicate').squeeze(0)
            x = x[:, int(dy[n]):int(dy[n]) + H, int(dx[n]):int(dx[n]) + W]
        if post == 'pad':
            x = F.pad(x, (2, 2, 2, 2), mode='constant', value=0.)
        elif post:
            x = centre_crop(x, post[1], post[2])
        out.append(x.to(torch.float32).div(255))
    return torch.stack(out)


def apply_pil_tables(img, tables_h, tables_v):
    """PIL's two 8-bit passes on a (H, W) uint8 image with the (coeffs, bounds) tables of pil_bilinear_tables."""
    def one_pass(a, coeffs, bounds):                           # along the last axis
        out = np.empty(a.shape[:-1] + (len(coeffs),), np.uint8)
        for o, (first, count) in enumerate(bounds):
            s = (a[..., first:first + count].astype(np.int64) * coeffs[o, :count].astype(np.int64)).sum(-1)
            out[..., o] = np.clip((s + (1 << 21)) >> 22, 0, 255)
        return out
    return one_pass(one_pass(img, *tables_h).T, *tables_v).T


# ---- tiny data-set trees in the layouts torchvision leaves on disk
def write_idx(path, array):
    array = np.ascontiguousarray(array, np.uint8)
    raw = b'\x00\x00\x08' + bytes([array.ndim]) + struct.pack('>' + 'I' * array.ndim, *array.shape) + array.tobytes()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with (gzip.open if path.endswith('.gz') else open)(path, 'wb') as f:
        f.write(raw)


def write_idx_tree(root, folder, n_train, n_test, seed, prefix='', test_part='t10k', gz=False, classes=10, first_label=0):
    """-> {'train': (images (n, 28, 28), labels), 'test': ...} written under root/<folder>/raw."""
    rng = np.random.default_rng(seed)
    out = {}
    for split, part, n in (('train', 'train', n_train), ('test', test_part, n_test)):
        x = rng.integers(0, 256, (n, 28, 28), dtype=np.uint8)
        y = (np.arange(n) % classes + first_label).astype(np.uint8)
        rng.shuffle(y)
        ext = '.gz' if gz else ''
        write_idx(os.path.join(root, folder, 'raw', '{}{}-images-idx3-ubyte{}'.format(prefix, part, ext)), x)
        write_idx(os.path.join(root, folder, 'raw', '{}{}-labels-idx1-ubyte{}'.format(prefix, part, ext)), y)
        out[split] = (x, y.astype(np.int64))
    return out


def write_cifar10_tree(root, per_file=4, seed=0):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, 'cifar10', 'cifar-10-batches-py')
    os.makedirs(d, exist_ok=True)
    out = {'train': ([], []), 'test': ([], [])}
    for name in ['data_batch_{}'.format(i) for i in range(1, 6)] + ['test_batch']:
        x = rng.integers(0, 256, (per_file, 3072), dtype=np.uint8)
        y = [int(v) for v in rng.integers(0, 10, per_file)]
        if name == 'data_batch_2':
            y[0] = 3
        with open(os.path.join(d, name), 'wb') as f:
            pickle.dump({'data': x, 'labels': y, 'batch_label': name}, f)
        split = 'test' if name == 'test_batch' else 'train'
        out[split][0].append(x.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
        out[split][1].extend(y)
    return {k: (np.concatenate(v[0]), np.asarray(v[1], np.int64)) for k, v in out.items()}


def write_cifar100_tree(root, n=6, seed=1):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, 'cifar100', 'cifar-100-python')
    os.makedirs(d, exist_ok=True)
    out = {}
    for split in ('train', 'test'):
        x = rng.integers(0, 256, (n, 3072), dtype=np.uint8)
        y = [int(v) for v in rng.integers(0, 100, n)]
        with open(os.path.join(d, split), 'wb') as f:
            pickle.dump({'data': x, 'fine_labels': y, 'coarse_labels': [v // 5 for v in y]}, f)
        out[split] = (x.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1), np.asarray(y, np.int64))
    return out


def write_svhn_tree(root, n=5, seed=2):
    from scipy.io import savemat
    rng = np.random.default_rng(seed)
    d = os.path.join(root, 'svhn')
    os.makedirs(d, exist_ok=True)
    out = {}
    for split in ('train', 'test'):
        x = rng.integers(0, 256, (32, 32, 3, n), dtype=np.uint8)
        y = rng.integers(1, 10, (n, 1)).astype(np.uint8)
        y[1] = 10
        savemat(os.path.join(d, '{}_32x32.mat'.format(split)), {'X': x, 'y': y})
        lab = y.reshape(-1).astype(np.int64)
        lab[lab == 10] = 0
        out[split] = (x.transpose(3, 2, 0, 1), lab)
    return out
