"""Host side of WIMJob.finetune(): the MovingSet, the loop's epoch arithmetic and the C ABI of the new kernels (no GPU)."""
import os
import re

import pytest
import torch

from jvae_compat.ft_datasets import MovingSet, NamedView, TaggedConcat, finetune_schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Set(torch.utils.data.Dataset):
    """n items (x, y): x = [base + i], y = i % 3."""

    def __init__(self, n, base, name):
        self.n, self.base, self.name = n, base, name

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return torch.tensor([float(self.base + i)]), i % 3


def moving():
    return MovingSet(_Set(5, 0, 'cifar'), {'svhn': _Set(3, 100, 'a'), 'lsun': _Set(4, 200, 'b')})


def test_moving_set_items_carry_their_group():
    m = moving()
    assert len(m) == 12 and m.classes == ('ind', 'ood')
    assert m.mix == [5 / 12, 7 / 12] and abs(sum(m.mix) - 1) < 1e-15
    items = [m[i] for i in range(12)]
    assert [t for _, t in items] == [0] * 5 + [1] * 7 == [MovingSet.IND] * 5 + [MovingSet.OOD] * 7
    assert [float(x) for x, _ in items] == [0, 1, 2, 3, 4, 100, 101, 102, 200, 201, 202, 203]
    assert m[-1][1] == 1 and float(m[-1][0]) == 203
    for bad in (12, -13):
        with pytest.raises(IndexError):
            m[bad]
    assert [m.locate(i) for i in (0, 4, 5, 11)] == [(0, 0), (0, 4), (1, 0), (1, 6)]


def test_membership_by_tag():
    m = moving()
    tags = torch.tensor([0, 1, 1, 0])
    assert list(m.which_subsets(*tags, which='ind')) == [True, False, False, True]
    assert list(m.which_subsets(*tags, which='ood')) == [False, True, True, False]
    assert list(m.which_subsets(*tags)) == ['ind', 'ood', 'ood', 'ind']


def test_extract_subdataset():
    m = moving()
    ind = m.extract_subdataset('ind', new_name='cifar10')
    assert isinstance(ind, NamedView) and ind.name == 'cifar10' and len(ind) == 5
    assert float(ind[2][0]) == 2 and ind[2][1] == 2                      # the set's own (x, y) items
    assert m.extract_subdataset('ind').name == 'cifar'                    # no new name: the set itself
    ood = m.extract_subdataset('ood')
    assert isinstance(ood, TaggedConcat) and ood.classes == ('svhn', 'lsun') and len(ood) == 7 and ood.mix == [3 / 7, 4 / 7]
    assert [ood[i][1] for i in range(7)] == [0, 0, 0, 1, 1, 1, 1]
    lsun = ood.extract_subdataset('lsun', new_name='lsun')
    assert lsun.name == 'lsun' and len(lsun) == 4 and float(lsun[0][0]) == 200 and lsun[1][1] == 1
    with pytest.raises(ValueError):
        m.extract_subdataset('nope')
    with pytest.raises(ValueError):
        MovingSet(_Set(2, 0, 'x'), {})


def test_a_loader_collates_the_tags():
    x, tags = next(iter(torch.utils.data.DataLoader(moving(), batch_size=12)))
    assert x.shape == (12, 1) and tags.dtype == torch.int64 and tags.tolist() == [0] * 5 + [1] * 7


@pytest.mark.parametrize('args,want', [
    # (train_size, moving_size, batch_size, epochs) -> (recorded train_size, batches per epoch), by hand:
    ((100000, 16, 8, 2), (32, [2, 2])),                    # epochs override: 2 x 16 samples
    ((32, 16, 8, None), (32, [2, 2])),
    ((100, 16, 8, None), (100, [2, 2, 2, 2, 2, 2, 0])),    # ceil(100 / 16) = 7 epochs; 6 x 16 = 96 used, 4 left: no full batch
    ((40, 20, 8, None), (40, [2, 2])),                     # drop_last: 16 of 20 per epoch, 40 -> 24 -> 8; two epochs planned
    ((50, 20, 8, None), (50, [2, 2, 2])),                  # 50 -> 34 -> 18 -> 2
    ((10, 100, 4, None), (10, [2])),                       # less than one pass: min(10, 100) // 4
    ((3, 100, 4, None), (3, [0])),
    ((0, 16, 8, None), (0, [])),
])
def test_finetune_schedule(args, want):
    assert finetune_schedule(*args) == want


def test_finetune_schedule_rejects_empty_sets():
    with pytest.raises(ValueError):
        finetune_schedule(10, 0, 4)
    with pytest.raises(ValueError):
        finetune_schedule(10, 8, 0)


NEW_SYMBOLS = ('jvae_latent_mixed_fwd_f32', 'jvae_latent_mixed_bwd_f32', 'jvae_group_tally_f32')


@pytest.mark.parametrize('name', NEW_SYMBOLS)
def test_new_symbols_are_declared_and_bound(name):
    from jvae_hip import lib
    with open(os.path.join(REPO, 'include', 'jvae_hip.h')) as f:
        header = f.read()
    decl = re.search(r'^int ' + name + r'\(([^;]*)\);', header, re.M | re.S)
    assert decl, name + ' is not declared in include/jvae_hip.h'
    table = getattr(lib, '_SIGNATURES', None) or next(v for v in vars(lib).values() if isinstance(v, dict) and 'jvae_latent_fwd_f32' in v)
    assert name in table, name + ' is not bound in jvae_hip/lib.py'
    restype, argtypes = table[name]
    assert len(argtypes) == len(decl.group(1).split(',')), (name, len(argtypes))


def test_wimjob_has_the_fine_tuning_interface():
    from jvae_compat.wim import WIMJob
    assert WIMJob.WIM_FUSED_STEP is True and WIMJob.last_finetune_route is None
    assert callable(WIMJob.finetune_step) and callable(WIMJob.finetune)
    assert WIMJob.printed_loss == ('zdist',) and WIMJob.TALLY_GROUPS == ('ind', 'ood', 'in')
