"""Mixed batches of the seeded moving sets on the MI355X: ops.imageset_mixed_batch (csrc/imageset.hip) - one launch for a batch
whose images come from several resident sets with different layouts and chains and from the synthetic sets - against the
torch-CPU composition of tests/imageset_cases.py per leaf (PIL's own bytes for the resized leaf) and against the single-set
kernel, then the loaders and WIMJob.finetune(moving_size=...) fed both ways.  Everything is compared with torch.equal: bytes are
moved and divided by 255, there is no tolerance to choose."""
import os

import numpy as np
import pytest
import torch

import imageset_cases as IC
from oracle.cases import get_case
from oracle.det_init import load_det_state

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def image_set(name, data, nhwc, targets=None, lut=None, **chain):
    from jvae_hip import ops
    from jvae_compat.torch_load import DeviceImageSet
    n = data.shape[0]
    source = tuple(data.shape[1:]) if nhwc else (data.shape[2], data.shape[3], data.shape[1])
    desc = ops.ImagesetDesc(source, nhwc, device=DEV, **chain)
    targets = torch.arange(n) if targets is None else targets
    return DeviceImageSet(name, data.to(DEV), nhwc, targets.to(DEV), None if lut is None else lut.to(DEV), desc, desc.shape,
                          [str(i) for i in range(10)])


def table_of(leaves, tag_of=lambda l, i: 2 * l + i % 2):
    """Every sample of every leaf, leaf after leaf -> (ImagesetMixTable, leaf, index, tag as lists)."""
    from jvae_hip import ops
    leaf = [l for l, s in enumerate(leaves) for _ in range(len(s))]
    index = [i for s in leaves for i in range(len(s))]
    tag = [tag_of(l, i) for l, i in zip(leaf, index)]
    return ops.ImagesetMixTable(leaves, np.asarray(leaf), np.asarray(index), np.asarray(tag), DEV), leaf, index, tag


def mixed(table, pos, u=None, vec=0):
    from jvae_hip import ops
    assert 0 <= min(pos) and max(pos) < table.n_items         # the caller's check: the kernel has no trap
    x, tag, y = ops.imageset_mixed_batch(table, torch.as_tensor(pos, dtype=torch.int64).to(DEV), u, vec=vec)
    return x.cpu(), tag.cpu(), y.cpu()


# ---------------------------------------------------------------------------------------------- 1. mixed chains in one wave
@pytest.fixture(scope='module')
def four_leaves(golden_dir):
    pil = np.load(os.path.join(golden_dir, 'imagesets', 'pil_resize.npz'))
    g = torch.Generator().manual_seed(31)
    raw = [torch.randint(0, 256, (9, 8, 9, 3), generator=g, dtype=torch.uint8),
           torch.randint(0, 256, (6, 3, 9, 8), generator=g, dtype=torch.uint8),
           torch.from_numpy(pil['src_turn_7x5_8x9'])[:, None],
           torch.randint(0, 256, (5, 1, 4, 5), generator=g, dtype=torch.uint8)]
    from jvae_compat.torch_load import pil_bilinear_tables
    tables = (*pil_bilinear_tables(7, 9), *pil_bilinear_tables(5, 8))          # after the quarter turn: (5, 7) -> (8, 9)
    lut = torch.arange(9, -1, -1)
    labels = torch.tensor([3, 0, 9, 9, 1, 7])
    leaves = [image_set('nhwc', raw[0], True),
              image_set('nchw', raw[1], False, targets=labels, lut=lut, B=1),
              image_set('resized', raw[2], False, A=1, resize=(8, 9, *tables), g2c=True),
              image_set('padded', raw[3], False, p0=2, g2c=True)]
    # the expected images and labels of every item, once, from torch-CPU / PIL
    want = [IC.expected_batch(raw[0].permute(0, 3, 1, 2)), IC.expected_batch(raw[1], B=1),
            IC.expected_batch(raw[2], resized=torch.from_numpy(pil['out_turn_7x5_8x9'])[:, None], g2c=True),
            IC.expected_batch(raw[3], p0=2, g2c=True)]
    assert all(tuple(w.shape[1:]) == (3, 8, 9) == tuple(s.desc.shape) for w, s in zip(want, leaves))
    y = [torch.arange(9), lut[labels], torch.arange(3), torch.arange(5)]
    return leaves, torch.cat(want), torch.cat(y)


@pytest.mark.parametrize('pos', [[0], [22], [17], [8, 9, 15, 0, 8, 22, 14], [18, 3, 17, 12, 15, 17, 14], [22, 14, 18, 9, 15, 8, 0]])
def test_mixed_chains_in_one_wave(four_leaves, pos):
    from jvae_hip import JvaeHipError
    leaves, want_x, want_y = four_leaves
    table, leaf, index, tag = table_of(leaves)
    assert table.shape == (3, 8, 9) and table.n_items == 23 and 3 * 8 * 9 % 64 != 0 and table.u_dims == 0
    # items 0..8 nhwc, 9..14 nchw, 15..17 resized, 18..22 padded: the lists above interleave the leaves, repeat a position and
    # reach the first and the last sample of every leaf
    x, t, y = mixed(table, pos)
    assert tuple(x.shape) == (len(pos), 3, 8, 9) and x.dtype == torch.float32 and t.dtype == y.dtype == torch.int64
    for n, p in enumerate(pos):
        assert torch.equal(x[n], want_x[p]), (n, p, leaf[p], index[p])
    assert y.tolist() == want_y[pos].tolist() and t.tolist() == [tag[p] for p in pos]
    with pytest.raises(JvaeHipError, match='invalid argument'):                # W = 9: no four x per thread
        mixed(table, pos, vec=4)
    with pytest.raises(JvaeHipError, match='no synthetic leaf'):
        mixed(table, pos, u=torch.zeros((len(pos), 3), device=DEV))


def test_every_position_covers_first_and_last_of_each_leaf(four_leaves):
    leaves, want_x, want_y = four_leaves
    table, _, _, tag = table_of(leaves)
    x, t, y = mixed(table, list(range(22, -1, -1)))
    assert torch.equal(x, want_x.flip(0)) and torch.equal(y, want_y.flip(0)) and t.tolist() == tag[::-1]


# ---------------------------------------------------------------------------------------------- 2. the grid-stride path
@pytest.mark.parametrize('vec', [0, 1, 4])
def test_grid_stride_against_the_single_set_kernel(vec):
    from jvae_hip import ops
    g = torch.Generator().manual_seed(32)
    a = torch.randint(0, 256, (37, 32, 32, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (23, 3, 32, 32), generator=g, dtype=torch.uint8)
    leaves = [image_set('a', a, True), image_set('b', b, False, targets=torch.arange(23) % 10, lut=torch.arange(10) + 5)]
    table, leaf, index, tag = table_of(leaves)
    N = 400
    assert N * 3 * 32 * 32 > 4096 * 256
    pos = torch.randint(0, 60, (N,), generator=g)
    pos[0], pos[-1], pos[1], pos[-2] = 0, 59, 36, 37
    x, t, y = ops.imageset_mixed_batch(table, pos.to(DEV), vec=vec)
    leaf_of, index_of = torch.tensor(leaf)[pos], torch.tensor(index)[pos]
    for l, s in enumerate(leaves):                             # the single-set kernel on the rows of each leaf
        rows = (leaf_of == l).nonzero().reshape(-1)
        xs, ys = ops.imageset_batch(s.data, index_of[rows].to(DEV), s.desc, s.targets, s.lut)
        assert len(rows) > 100 and torch.equal(x[rows.to(DEV)], xs) and torch.equal(y[rows.to(DEV)], ys)
    assert t.cpu().tolist() == [tag[p] for p in pos.tolist()]
    x = x.cpu()
    for n in [0, N - 1] + torch.randint(0, N, (10,), generator=g).tolist():
        i = int(index_of[n])
        want = IC.expected_batch(a[i:i + 1].permute(0, 3, 1, 2)) if leaf_of[n] == 0 else IC.expected_batch(b[i:i + 1])
        assert torch.equal(x[n], want[0]), n


# ---------------------------------------------------------------------------------------------- 3. synthetic leaves
@pytest.mark.parametrize('pad', [False, True])
def test_synthetic_leaves_show_what_the_caller_drew(pad):
    from jvae_hip import ops, JvaeHipError
    from jvae_compat.torch_load import SyntheticImageSet
    g = torch.Generator().manual_seed(33)
    raw = torch.randint(0, 256, (5, 6, 8, 3), generator=g, dtype=torch.uint8)
    kw = dict(classes=['0'], transformer='pad' if pad else '')
    const = SyntheticImageSet('const', 'const', (3, 6, 8), DEV, **kw)
    uniform = SyntheticImageSet('uniform', 'uniform', (3, 6, 8), DEV, **kw)
    image = image_set('image', raw, True, post='pad' if pad else None)
    H, W = (10, 12) if pad else (6, 8)
    want_image = IC.expected_batch(raw.permute(0, 3, 1, 2), post='pad' if pad else None)

    def item(leaves, which, sample):                           # position of a sample in table_of's leaf-after-leaf order
        return sum(len(s) for s in leaves[:which]) + sample

    def inner(v):
        return v[..., 2:-2, 2:-2] if pad else v

    def border_is_zero(v):
        border = v.clone()
        border[:, 2:-2, 2:-2] = 0
        return float(border.abs().max()) == 0.

    # const + image: u is (N, C)
    leaves = [image, const]
    table = ops.ImagesetMixTable(leaves, np.array([0, 1, 0, 1, 1]), np.array([4, 0, 0, 9999, 17]), np.array([0, 1, 0, 1, 1]), DEV)
    assert table.shape == (3, H, W) and table.u_dims == 2
    u = torch.rand((6, 3), generator=g)
    pos = [1, 0, 3, 2, 4, 1]
    for vec in (1, 4):
        x, t, y = mixed(table, pos, u.to(DEV), vec=vec)
        for n, p in enumerate(pos):
            if p in (0, 2):
                assert torch.equal(x[n], want_image[4 if p == 0 else 0]) and y[n] == (4 if p == 0 else 0) and t[n] == 0
            else:
                assert torch.equal(inner(x[n]), u[n][:, None, None].expand(3, 6, 8)) and y[n] == 0 and t[n] == 1
                assert not pad or border_is_zero(x[n])
    with pytest.raises(JvaeHipError, match='u float32'):
        mixed(table, pos)
    with pytest.raises(JvaeHipError, match='u float32'):
        mixed(table, pos, torch.rand((6, 3, H, W)).to(DEV))
    # const + uniform + image: u is (N, C, H, W); a uniform row is u[n], a const row u[n, c, 0, 0] broadcast
    leaves = [const, image, uniform]
    table = ops.ImagesetMixTable(leaves, np.array([0, 1, 2, 2, 1]), np.array([5, 2, 0, 9999, 4]), np.array([2, 0, 1, 1, 0]), DEV)
    assert table.u_dims == 4
    u = torch.rand((7, 3, H, W), generator=g)
    pos = [2, 0, 1, 3, 4, 0, 2]
    for vec in (1, 4):
        x, t, y = mixed(table, pos, u.to(DEV), vec=vec)
        assert t.tolist() == [1, 2, 0, 1, 0, 2, 1] and y.tolist() == [0, 0, 2, 0, 4, 0, 0]
        for n, p in enumerate(pos):
            if p in (2, 3):
                assert torch.equal(inner(x[n]), inner(u[n]))
            elif p == 0:
                assert torch.equal(inner(x[n]), u[n, :, 0, 0][:, None, None].expand(3, 6, 8))
            else:
                assert torch.equal(x[n], want_image[2 if p == 1 else 4])
            assert not pad or border_is_zero(x[n])
    if not pad:
        assert torch.equal(x[0], u[0]) and torch.equal(x[3], u[3])


# ---------------------------------------------------------------------------------------------- 4. the loaders
@pytest.fixture(scope='module')
def named_sets(tmp_path_factory):
    from jvae_compat import torch_load as T
    root = str(tmp_path_factory.mktemp('moving'))
    IC.write_cifar10_tree(root, per_file=24, seed=41)
    IC.write_svhn_tree(root, n=16, seed=42)
    IC.write_idx_tree(root, 'MNIST', 4, 20, seed=43)
    return {n: T.get_dataset(n, splits=['test'], root=root, device=DEV)[1] for n in ('cifar10', 'svhn', 'mnist32r', 'mnist32p')}


def moving_of(sets, **kw):
    from jvae_compat.ft_datasets import create_moving_set
    return create_moving_set(sets['cifar10'], {'svhn': sets['svhn'], 'mnist32r': sets['mnist32r']}, {'mnist32p': sets['mnist32p']},
                             24, 0.5, padding=0.5, mix_padding=0.25, seed=3, task=1, **kw)


def test_mixed_loader_yields_the_batches_of_a_dataloader(named_sets, monkeypatch):
    from jvae_hip import ops
    from jvae_compat import torch_load as T
    moving = moving_of(named_sets)
    assert moving.classes == ('ood', 'ind', 'pad', 'padmix') and [len(d) for d in moving.subdatasets] == [12, 12, 12, 6]
    leaves = moving.resolve()[0]
    assert [l.name for l in leaves] == ['svhn', 'mnist32r', 'cifar10', 'mnist32p'] and [l.nhwc for l in leaves][::2] == [False, True]
    launches = []
    real = ops.imageset_mixed_batch
    monkeypatch.setattr(ops, 'imageset_mixed_batch', lambda *a, **k: launches.append(1) or real(*a, **k))
    for shuffle, drop_last in ((True, True), (False, False)):
        fast = T.mixed_loader(moving, 8, shuffle, drop_last)
        slow = torch.utils.data.DataLoader(moving, batch_size=8, shuffle=shuffle, drop_last=drop_last, num_workers=0)
        assert len(fast) == len(slow) == (5 if drop_last else 6)
        for epoch in range(2):                                 # re-iterable: the second epoch draws the next permutation
            del launches[:]
            torch.manual_seed(50)
            a = [(x.cpu(), t.cpu()) for x, t in fast]
            assert len(launches) == len(fast)
            state = torch.get_rng_state()
            torch.manual_seed(50)
            b = [(x.cpu(), t) for x, t in slow]
            assert torch.equal(state, torch.get_rng_state())   # the same draws from the global generator
            assert len(a) == len(b) == len(fast)
            for (xa, ta), (xb, tb) in zip(a, b):
                assert xa.shape == xb.shape and torch.equal(xa, xb) and torch.equal(ta, tb) and ta.dtype == tb.dtype
        assert fast.table is not None and fast.table.matches(*moving.resolve())
    # barred: re-resolved, and the loader made for the old length refuses; a new one follows the set
    table = fast.table
    moving.bar(True)
    assert not table.matches(*moving.resolve())
    with pytest.raises(RuntimeError, match='the loader was made for 42'):
        next(iter(fast))
    fast = T.mixed_loader(moving, 16, False, False)
    slow = torch.utils.data.DataLoader(moving, batch_size=16, shuffle=False, num_workers=0)
    for (xa, ta), (xb, tb) in zip(fast, slow):
        assert torch.equal(xa.cpu(), xb.cpu()) and torch.equal(ta.cpu(), tb)


def test_mixed_loader_draws_the_synthetic_leaves_per_batch(named_sets):
    from jvae_compat import torch_load as T
    from jvae_compat.ft_datasets import create_moving_set
    const = T.get_dataset('const32', splits=['test'], device=DEV)[1]
    moving = create_moving_set(named_sets['cifar10'], {'svhn': named_sets['svhn']}, {'const32': const}, 8, 0.5, padding=0.5, seed=1)
    fast = T.mixed_loader(moving, 12, False, False)
    (x, tag), = list(fast)
    assert fast.table.u_dims == 2 and tag.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    pad = x[8:]
    assert bool((pad == pad[:, :, :1, :1]).all()) and len(set(pad[:, :, 0, 0].reshape(-1).tolist())) == 12
    slow = torch.utils.data.DataLoader(moving, batch_size=12, num_workers=0)
    (xs, ts), = list(slow)
    assert torch.equal(x[:8], xs[:8]) and ts.tolist() == tag.tolist()          # the images of the resident sets either way


def test_device_loader_reads_the_extracted_subsets(named_sets):
    from jvae_compat import torch_load as T
    moving = moving_of(named_sets)
    ind = moving.extract_subdataset('ind', new_name='cifar-ind')
    ood = moving.extract_subdataset('ood')
    for dset in (ind, ood.extract_subdataset('svhn', new_name='svhn'), ood.extract_subdataset('mnist32r')):
        for shuffle in (False, True):
            fast = T.device_loader(dset, 5, shuffle)
            slow = torch.utils.data.DataLoader(dset, batch_size=5, shuffle=shuffle, num_workers=0)
            assert isinstance(fast, T.DeviceBatches) and len(fast) == len(slow)
            torch.manual_seed(51)
            a = [(x.cpu(), y.cpu()) for x, y in fast]
            torch.manual_seed(51)
            b = [(x.cpu(), y) for x, y in slow]
            for (xa, ya), (xb, yb) in zip(a, b):
                assert torch.equal(xa, xb) and torch.equal(ya, yb), dset.name
    assert ind.name == 'cifar-ind' and len(ind) == 12 and T.device_loader(moving, 5, False) is None


# ---------------------------------------------------------------------------------------------- 5. the loop
class Plain(torch.utils.data.Dataset):
    def __init__(self, x, y, name):
        self.x, self.y, self.name = x, [int(v) for v in y], name

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return self.x[i], self.y[i]


def wim_job():
    """WIMJob on the geometry and the weights of case w2_n8 (config 2: conv32 / deconv32), as tests/test_15 builds it."""
    from jvae_compat.wim import WIMJob
    from module.priors import build_prior
    case = get_case('w2_n8')
    K = case['net']['latent_dim']
    job = WIMJob(**case['net'], alternate_prior=dict(case['alternate_prior'], num_priors=1, dim=K))
    load_det_state(job, seed=0)
    job.to(DEV)
    with torch.no_grad():
        for k in ('mean', '_var_parameter'):
            getattr(job._alternate_prior, k).copy_(build_prior(dim=K, num_priors=1, **case['alternate_prior']).to(DEV).state_dict()[k])
    return job, case


def same(a, b):
    """Equal results, a nan equal to a nan."""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return bool(a == b)


def test_finetune_on_a_moving_set_both_ways(named_sets, monkeypatch):
    from jvae_hip import ops
    g = torch.Generator().manual_seed(60)
    trainset = Plain(torch.rand((21, 3, 32, 32), generator=g), torch.randint(0, 10, (21,), generator=g), 'train')
    resident = {n: named_sets[n] for n in ('cifar10', 'svhn', 'mnist32p')}
    plain = {}
    for n, s in resident.items():
        x, y = s.batch(range(len(s)))
        plain[n] = Plain(x.cpu(), y.cpu(), n)
    launches = []
    real = ops.imageset_mixed_batch
    monkeypatch.setattr(ops, 'imageset_mixed_batch', lambda *a, **k: launches.append(1) or real(*a, **k))
    out = {}
    for way, sets in (('resident', resident), ('plain', plain)):
        job, case = wim_job()
        seen = []
        del launches[:]
        np.random.seed(62)                                     # a loss recorder draws the seed of its pass from numpy when it is made
        torch.manual_seed(61)
        res = job.finetune(trainset, sets['cifar10'], {'svhn': sets['svhn']}, batch_size=7, epochs=2, test_batch_size=8,
                           alpha=case['alpha'], moving_size=16, padding=0.5, padding_sets={'mnist32p': sets['mnist32p']},
                           mix_padding=0.25, seed=3, task=1,
                           on_batch=lambda e, b, i, m, tags: seen.append((e, b, tags.cpu().clone(), m['zdist'].detach().cpu().clone())))
        torch.cuda.synchronize()
        out[way] = (res, dict(job.ft_params), {k: v.detach().cpu().clone() for k, v in job.state_dict().items()}, seen, len(launches))
    a, b = out['resident'], out['plain']
    assert a[4] == 8 and b[4] == 0                             # 2 epochs x 4 batches, one launch each; none on the DataLoader route
    assert same(a[0], b[0]) and set(a[0]) == {'svhn'} and a[1] == b[1]
    fp = a[1]
    # 16 wanted: 8 ood + 8 ind, 8 pad, 4 padmix (2 from the complement of each) = 28 items, 28 // 1.75 = 16
    assert fp['moving_size'] == 16 and fp['mix'] == 8 / 28 and fp['padding'] == 0.5 and fp['padding_sets'] == ['mnist32p']
    assert fp['mix_padding'] == 0.25 and fp['sets'] == ['svhn'] and fp['train_size'] == 2 * 28
    assert set(a[2]) == set(b[2])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    fresh, _ = wim_job()
    assert not torch.equal(fresh.state_dict()['features.0.weight'].cpu(), a[2]['features.0.weight'])      # the run did train
    assert [(e, i) for e, i, _, _ in a[3]] == [(e, i) for e in range(2) for i in range(4)] == [(e, i) for e, i, _, _ in b[3]]
    for (_, _, ta, za), (_, _, tb, zb) in zip(a[3], b[3]):
        assert torch.equal(ta, tb) and torch.equal(za, zb)
    for e in range(2):                                         # batches of 7 cover the 28 items: every class in full, per epoch
        tags = torch.cat([t for ep, _, t, _ in a[3] if ep == e])
        assert torch.bincount(tags, minlength=4).tolist() == [8, 8, 8, 4]
