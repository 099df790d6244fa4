"""Host side of the seeded moving sets (jvae_compat/ft_datasets.py: SubSampledDataset, MixtureDataset, create_moving_set) against
what the reference's ft/datasets.py gave for the same parameters (tests/golden/moving_sets/reference_indices.json, recorded by
tools/gen_moving_set_golden.py), the three places where this build does not follow the reference because it raises there, the
host checks of ops.ImagesetMixTable and the ft_params of WIMJob.finetune().  No GPU."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle.cases import get_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Stub(torch.utils.data.Dataset):
    """Items ((name, i), i % 7), as the recorded run's stub sets."""

    def __init__(self, name, n):
        self.name, self.n = name, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return (self.name, int(i)), int(i) % 7


@pytest.fixture(scope='module')
def recorded(golden_dir):
    with open(os.path.join(golden_dir, 'moving_sets', 'reference_indices.json')) as f:
        return json.load(f)


def stub(recorded, name):
    return Stub(name, recorded['sizes'][name]['test'])


def build(recorded, case, **over):
    from jvae_compat.ft_datasets import create_moving_set
    kw = dict(case, **over)
    return create_moving_set(stub(recorded, 'ind'), {n: stub(recorded, n) for n in recorded['ood_sets']},
                             {n: stub(recorded, n) for n in kw['padding_sets']}, kw['moving_size'], kw['ood_mix'],
                             padding=kw['padding'], mix_padding=kw['mix_padding'], seed=kw['seed'], task=kw['task'])


def resolved(dset):
    leaves, leaf, index, tag = dset.resolve()
    assert leaf.dtype == index.dtype == tag.dtype == np.int64 and len(leaf) == len(index) == len(tag) == len(dset)
    assert len({id(l) for l in leaves}) == len(leaves) and not any(hasattr(l, 'resolve') for l in leaves)
    return [[leaves[l].name, int(i), int(t)] for l, i, t in zip(leaf, index, tag)]


def through_getitem(dset):
    out = []
    for i in range(len(dset)):
        (name, sample), tag = dset[i]
        out.append([name, sample, tag])
    return out


def samples(rows):
    return {(r[0], r[1]) for r in rows}


# ---------------------------------------------------------------------------------------------- against the recorded lists
def test_the_fixture_covers_the_parameter_table(recorded):
    got = {(c['moving_size'], c['ood_mix'], c['padding'], tuple(c['padding_sets']), c['mix_padding'], c['seed'], c['task'])
           for c in recorded['cases']}
    assert got >= {(40, 0.5, 0.5, ('c32',), 0., 3, 0), (40, 0.5, 0.5, ('c32',), 0., 3, 1), (40, 0.5, 0.5, ('c32',), 0.25, 3, 0),
                   (40, 0.5, 0.5, ('c32',), 0.25, 3, 1), (40, 0.3, 0.5, ('c32',), 0.2, 7, 0), (40, 0.3, 0.5, ('c32',), 0.2, 7, 2),
                   (64, 0.5, 0.5, ('c32',), 0.2, 7, 5), (33, 0.5, 0.5, ('c32',), 0.2, 7, 1), (40, 0.5, 0.25, ('c32',), 0., 0, 0),
                   (40, 0.5, 1.0, ('c32', 'u32'), 0., 0, 0)}
    by = {(c['moving_size'], c['task']): c for c in recorded['cases'] if c['seed'] == 7}
    assert by[(40, 2)]['lengths'] == [12, 28, 20, 8] and len(by[(40, 2)]['items']) == 68
    assert by[(33, 1)]['lengths'] == [16, 17, 16, 6] and len(by[(33, 1)]['items']) == 55 and len(by[(64, 5)]['items']) == 108
    assert sum('bar' in c for c in recorded['cases']) == 1


@pytest.mark.parametrize('k', range(10))
def test_moving_set_is_the_recorded_one(recorded, k):
    case = recorded['cases'][k]
    m = build(recorded, case)
    assert list(m.classes) == case['classes'] and m.mix == case['mix'] and [len(d) for d in m.subdatasets] == case['lengths']
    assert len(m) == len(case['items']) and resolved(m) == case['items'] and through_getitem(m) == case['items']
    with pytest.raises(IndexError):
        m[len(m)]
    ood = m.extract_subdataset('ood')
    want = case['ood']
    assert ood.name == 'ood' and list(ood.classes) == want['classes'] and ood.mix == want['mix']
    assert [len(d) for d in ood.subdatasets] == want['lengths']
    assert resolved(ood) == want['items'] and through_getitem(ood) == want['items']
    for name in ood.classes:
        sub = ood.extract_subdataset(name, new_name='as-' + name)
        assert sub.name == 'as-' + name and sub.maxlength == recorded['sizes'][name]['test']
        assert through_getitem(sub) == want['subsets'][name]                # the leaf's own (x, y) items
        assert [r[:2] for r in resolved(sub)] == [r[:2] for r in want['subsets'][name]]
    assert list(m.which_subsets(0, 1, which='ind')) == [False, True] and list(m.which_subsets(0, 1)) == ['ood', 'ind']
    if 'bar' in case:
        before = resolved(m)
        m.bar(True)
        assert [len(d) for d in m.subdatasets] == case['bar']['lengths']
        assert resolved(m) == case['bar']['items'] and through_getitem(m) == case['bar']['items']       # re-resolved
        m.bar(False)                                           # 'padmix' was shrunk after it was barred: it comes back at the
        back = resolved(m)                                     # length it was barred at, as in the reference; the others as before
        assert [r for r in back if r[2] < 3] == [r for r in before if r[2] < 3]


def test_subsampled_and_its_complement(recorded):
    from jvae_compat.ft_datasets import SubSampledDataset
    want = recorded['subsampled']
    d = SubSampledDataset(stub(recorded, want['set']), length=want['length'], seed=want['seed'], task=want['task'])
    assert d.name == 'sub-b' and d.maxlength == 90 and len(d) == 20
    assert through_getitem(d) == want['items'] and [r[:2] for r in resolved(d)] == [r[:2] for r in want['items']]
    perm = np.random.default_rng(want['seed']).permutation(90)
    assert [r[1] for r in want['items']] == perm[20:40].tolist()
    d.bar()
    assert len(d) == want['bar_length'] == 70 and through_getitem(d) == want['bar_items']
    assert not samples(want['bar_items']) & samples(want['items'])
    d.bar(False)
    assert len(d) == 20 and through_getitem(d) == want['unbar_items'] == want['items']


def test_tasks_take_disjoint_slices(recorded):
    from jvae_compat.ft_datasets import SubSampledDataset
    seen = set()
    for task in range(4):
        rows = resolved(SubSampledDataset(stub(recorded, 'b'), length=20, seed=5, task=task))
        assert len(samples(rows)) == 20 and not samples(rows) & seen
        seen |= samples(rows)
    by_task = {c['task']: c for c in recorded['cases'] if c['seed'] == 3 and c['mix_padding'] == 0.}
    for cls in (0, 1):
        a, b = ([r for r in resolved(build(recorded, by_task[t])) if r[2] == cls] for t in (0, 1))
        assert len(a) == 20 and not samples(a) & samples(b)


@pytest.mark.parametrize('k', [2, 3, 4, 5, 6, 7])
def test_padmix_shares_no_sample_with_ind_or_ood(recorded, k):
    m = build(recorded, recorded['cases'][k])
    assert m.classes == ('ood', 'ind', 'pad', 'padmix')
    rows = resolved(m)
    padmix = [r for r in rows if r[2] == 3]
    rest = [r for r in rows if r[2] in (0, 1)]
    assert padmix and len(samples(padmix)) == len(padmix) and not samples(padmix) & samples(rest)
    assert {r[0] for r in padmix} <= {'ind', 'a', 'b'} and {r[0] for r in rows if r[2] == 2} == {'c32'}


def test_shrink_and_back(recorded):
    from jvae_compat.ft_datasets import MixtureDataset, SubSampledDataset
    d = SubSampledDataset(stub(recorded, 'b'), length=20, seed=5, task=1)
    before = resolved(d)
    d.shrink(7)
    assert len(d) == 7 and len(resolved(d)) == 7
    d.shrink(20)
    assert resolved(d) == before
    d.shrink(1000)
    assert len(d) == 90
    m = MixtureDataset(mix=1, seed=3, task=1, length=20, a=stub(recorded, 'a'), b=stub(recorded, 'b'))
    before = resolved(m)
    m.shrink(6)
    assert [len(s) for s in m.subdatasets] == [3, 3] and through_getitem(m) == resolved(m) != before
    m.shrink(20)
    assert resolved(m) == before and m.mix == [0.5, 0.5]
    m.rename('x', 'y')
    assert m.classes == ('x', 'y')
    m.rename(x='a')
    assert m.classes == ('a', 'y')


def test_resolve_refuses_an_index_past_its_leaf(recorded):
    from jvae_compat.ft_datasets import SubSampledDataset
    leaf = stub(recorded, 'a')
    d = SubSampledDataset(leaf, length=60, seed=1)
    leaf.n = 50                                                # the leaf lost samples after the permutation was sized
    d.shrink(59)
    with pytest.raises(IndexError, match='sub-a'):
        d.resolve()


# ---------------------------------------------------------------------------------------------- where the reference raises
def test_task_none_is_task_zero(recorded):
    from jvae_compat.ft_datasets import SubSampledDataset
    case = recorded['cases'][0]
    assert case['task'] == 0 and resolved(build(recorded, case, task=None)) == case['items']
    assert resolved(SubSampledDataset(stub(recorded, 'b'), length=20, seed=5, task=None)) == resolved(
        SubSampledDataset(stub(recorded, 'b'), length=20, seed=5, task=0))


@pytest.mark.parametrize('pads', [['c32'], []])
def test_no_padding_leaves_the_pad_class_out(recorded, pads):
    case = recorded['cases'][0]
    m = build(recorded, case, padding=0., padding_sets=pads)
    assert m.classes == ('ood', 'ind') and [len(d) for d in m.subdatasets] == [20, 20]
    assert resolved(m) == [r for r in case['items'] if r[2] < 2]
    m = build(recorded, recorded['cases'][2], padding=0., padding_sets=pads)
    assert m.classes == ('ood', 'ind', 'padmix') and [len(d) for d in m.subdatasets] == [20, 20, 10]
    assert [r[:2] for r in resolved(m)] == [r[:2] for r in recorded['cases'][2]['items'] if r[2] != 2]
    with pytest.raises(ValueError, match='padding set'):
        build(recorded, case, padding=0.5, padding_sets=[])


def test_a_size_the_sets_cannot_fill_names_the_set(recorded):
    # 300 from a 100-image test split: 'ind' takes all 100, so its complement - and that of `a` - is empty
    with pytest.raises(ValueError, match=r'no sample is left of .*sub-a.*sub-b'):
        build(recorded, recorded['cases'][2], moving_size=300)
    with pytest.raises(ValueError, match='a is an out-of-distribution set and a padding set'):
        build(recorded, recorded['cases'][0], padding_sets=['a'])       # an OOD set as a padding set, as the reference refuses


# ---------------------------------------------------------------------------------------------- the table's host checks
def resident(name, n, shape_hw=(8, 9), nhwc=True, augmentation=(), **chain):
    from jvae_hip import ops
    from jvae_compat.torch_load import DeviceImageSet
    H, W = shape_hw
    data = torch.zeros((n, H, W, 3) if nhwc else (n, 3, H, W), dtype=torch.uint8)
    desc = ops.ImagesetDesc((H, W, 3), nhwc, **chain)
    return DeviceImageSet(name, data, nhwc, torch.zeros(n, dtype=torch.int64), None, desc, desc.shape, [str(i) for i in range(10)],
                          data_augmentation=augmentation)


def test_mix_table_refuses_before_anything_reaches_the_device():
    from jvae_hip import ops
    from jvae_compat.ft_datasets import MixtureDataset
    from jvae_compat.torch_load import SyntheticImageSet, mixed_loader
    a, b = resident('a', 6), resident('b', 5, shape_hw=(9, 8))
    with pytest.raises(ValueError, match=r'one shape.*a \(3, 8, 9\).*b \(3, 9, 8\)'):
        ops.ImagesetMixTable(*MixtureDataset(a=a, b=b).resolve(), 'cpu')
    turned = resident('b', 5, shape_hw=(9, 8), A=1)
    assert turned.desc.shape == (3, 8, 9)
    flipped = resident('c', 4, augmentation=('flip',))
    with pytest.raises(ValueError, match=r"c carries its own data_augmentation \['flip'\]"):
        ops.ImagesetMixTable(*MixtureDataset(a=a, b=turned, c=flipped).resolve(), 'cpu')
    padded = SyntheticImageSet('const', 'const', (3, 8, 9), 'cpu', classes=['const'], transformer='pad')
    with pytest.raises(ValueError, match=r'one shape.*const \(3, 12, 13\)'):
        ops.ImagesetMixTable(*MixtureDataset(a=a, c=padded).resolve(), 'cpu')
    sliced = resident('d', 6)
    sliced.data = torch.zeros((6, 8, 9, 6), dtype=torch.uint8)[..., ::2]
    assert tuple(sliced.data.shape) == (6, 8, 9, 3) and not sliced.data.is_contiguous()
    with pytest.raises(ValueError, match='d holds a tensor that is not contiguous'):
        ops.ImagesetMixTable(*MixtureDataset(d=sliced, a=a).resolve(), 'cpu')
    leaves, leaf, index, tag = MixtureDataset(a=a, b=turned).resolve()
    for bad in ((leaf, np.where(leaf == 1, 5, index), tag), (leaf + 1, index, tag), (leaf, index, tag - 1), (leaf, -index - 1, tag)):
        with pytest.raises(IndexError):
            ops.ImagesetMixTable(leaves, *bad, 'cpu')
    # sets that are not resident on a GPU keep the DataLoader
    assert mixed_loader(MixtureDataset(a=a, b=turned), 4, True, True) is None
    assert mixed_loader(MixtureDataset(a=Stub('a', 6), b=Stub('b', 5)), 4, True, True) is None
    assert mixed_loader(torch.utils.data.TensorDataset(torch.zeros(4, 1)), 4, True, True) is None


def test_device_loader_looks_through_subsampled_sets_and_views():
    from jvae_compat.ft_datasets import MixtureDataset, NamedView, SubSampledDataset
    from jvae_compat.torch_load import DeviceBatches, device_loader
    a = resident('a', 9)
    sub = SubSampledDataset(a, length=5, seed=2, task=1)
    perm = np.random.default_rng(2).permutation(9)
    got = device_loader(NamedView(sub, 'other'), 4, False)
    assert isinstance(got, DeviceBatches) and got.base is a and got.indices.tolist() == perm[[5, 6, 7, 8, 0]].tolist() and len(got) == 2
    inner = torch.utils.data.Subset(a, [8, 7, 6, 5, 4, 3])
    nested = device_loader(SubSampledDataset(inner, length=3, seed=2), 4, False)
    assert nested.base is a and nested.indices.tolist() == [8 - int(p) for p in np.random.default_rng(2).permutation(6)[:3]]
    plain = device_loader(a, 4, False)
    assert plain.base is a and plain.indices is None
    assert device_loader(torch.utils.data.Subset(a, [3, 1]), 4, False).indices.tolist() == [3, 1]
    assert device_loader(SubSampledDataset(Stub('a', 9), length=5), 4, False) is None
    assert device_loader(MixtureDataset(a=a, b=resident('b', 4)), 4, False) is None
    # over a mixture of ONE set the items are (x, tag), not the leaf's (x, y): that stays with the DataLoader
    over = SubSampledDataset(MixtureDataset(a=a), length=4, seed=2)
    assert len(over.resolve()[0]) == 1 and device_loader(over, 4, False) is None


def test_new_symbols_are_declared_and_bound():
    from jvae_hip import lib, ops
    with open(os.path.join(REPO, 'include', 'jvae_hip.h')) as f:
        header = f.read()
    table = next(v for v in vars(lib).values() if isinstance(v, dict) and 'jvae_imageset_batch_u8_f32' in v)
    for name in ('jvae_imageset_mixed_u8_f32', 'jvae_imageset_mix_leaf_bytes'):
        decl = re.search(r'^int ' + name + r'\(([^;]*)\);', header, re.M | re.S)
        assert decl and name in table, name
        args = [a for a in decl.group(1).split(',') if a.strip() != 'void']
        assert len(table[name][1]) == len(args), name
    import ctypes
    assert ctypes.sizeof(ops._MixLeaf) == lib.load().jvae_imageset_mix_leaf_bytes() == 8 + 7 * 8 + 4 * lib.load().jvae_imageset_desc_words()


# ---------------------------------------------------------------------------------------------- ft_params
class _Reached(Exception):
    pass


def job_on_cpu(monkeypatch):
    from jvae_compat.wim import WIMJob
    case = get_case('w2_n8')
    K = case['net']['latent_dim']
    job = WIMJob(**case['net'], alternate_prior=dict(case['alternate_prior'], num_priors=1, dim=K))

    def stop(*a, **kw):                                        # the first device work of finetune(): ft_params are written by then
        raise _Reached
    monkeypatch.setattr(job, 'ood_detection_rates', stop)
    return job


def test_ft_params_without_moving_size_are_the_plain_moving_sets(monkeypatch):
    """A regression guard, not evidence for the feature: it passes before the seeded moving sets exist too - `moving_size=None`
    must go on recording exactly these keys, values and types."""
    job = job_on_cpu(monkeypatch)
    with pytest.raises(_Reached):
        job.finetune(Stub('train', 24), Stub('cifar', 8), {'svhn': Stub('a', 5), 'lsun': Stub('b', 3)}, batch_size=8, epochs=2,
                     train_size=77, alpha=0.25)
    run = {k: v for k, v in job.ft_params.items() if k in job.FT_RUN_KEYS}     # beside them: the alternate prior's own parameters
    assert run == dict(sets=['svhn', 'lsun'], train_size=77, moving_size=16, mix=0.5, padding=0, padding_sets=[], mix_padding=0,
                       alpha=0.25)
    assert list(run) == ['sets', 'train_size', 'moving_size', 'mix', 'padding', 'padding_sets', 'mix_padding', 'alpha']
    assert type(run['padding']) is int and type(run['mix_padding']) is int and type(run['moving_size']) is int


def test_ft_params_with_a_moving_size(recorded, monkeypatch):
    job = job_on_cpu(monkeypatch)
    sets = (Stub('train', 24), stub(recorded, 'ind'), {n: stub(recorded, n) for n in ('a', 'b')})
    with pytest.raises(_Reached):
        job.finetune(*sets, batch_size=8, epochs=1, moving_size=40, ood_mix=0.3, padding=0.5, mix_padding=0.2, seed=7, task=2,
                     padding_sets={'c32': stub(recorded, 'c32')})
    fp = job.ft_params
    assert fp['moving_size'] == 40 == int(68 // 1.7) and fp['mix'] == 12 / 68 and fp['padding'] == 0.5
    assert fp['padding_sets'] == ['c32'] and fp['mix_padding'] == 0.2 and fp['sets'] == ['a', 'b']
    with pytest.raises(_Reached):                              # more than the sets hold: the recorded size is what came out
        job.finetune(*sets, batch_size=8, epochs=1, moving_size=300, ood_mix=0.5, padding=0.5, seed=3,
                     padding_sets={'c32': stub(recorded, 'c32')})
    assert job.ft_params['moving_size'] == int(370 // 1.5) == 246 and job.ft_params['mix'] == 120 / 370
    with pytest.raises(_Reached):                              # no padding: no padding sets recorded, whatever was given
        job.finetune(*sets, batch_size=8, epochs=1, moving_size=40, padding_sets={'c32': stub(recorded, 'c32')})
    assert job.ft_params['padding_sets'] == [] and job.ft_params['padding'] == 0. and job.ft_params['mix'] == 0.5
    with pytest.raises(NotImplementedError, match='named torchvision datasets'):
        job.finetune(*sets, batch_size=8, epochs=1, moving_size=40, padding=0.5, padding_sets={'const32': 'const32'})
    with pytest.raises(NotImplementedError, match='named torchvision datasets'):
        job.finetune(*sets, batch_size=8, epochs=1, moving_size=40, padding=0.5)
    # no padding set given: the uniform* and const* siblings of the model's set, by name
    job.DATA_ROOT = 'nowhere'                                  # the synthetic sets read no file
    job.training_parameters['set'] = 'cifar10'
    with pytest.raises(_Reached):
        job.finetune(*sets, batch_size=8, epochs=1, moving_size=40, padding=0.5, seed=3)
    assert job.ft_params['padding_sets'] == ['uniform32', 'const32'] and job.ft_params['moving_size'] == 40
    assert job.ft_params['mix'] == 20 / 60
    with pytest.raises(_Reached):                              # a list with a short name and a data set
        job.finetune(*sets, batch_size=8, epochs=1, moving_size=40, padding=0.5, seed=3, padding_sets=['const', stub(recorded, 'c32')])
    assert job.ft_params['padding_sets'] == ['const32', 'c32']
