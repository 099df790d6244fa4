"""Data sets of the WIM fine-tuning loop (`WIMJob.finetune`), over data-set OBJECTS.

`MovingSet` is the set the fine-tuning moves towards the alternate prior: the in-distribution test set followed by the
out-of-distribution sets, as one data set whose items are `(x, tag)` - tag 0 for an in-distribution item, 1 for an OOD one - so
that the loop knows each sample's group without reading labels back.  The reference builds it by name, sub-sampled by seed /
task and optionally padded (ft/datasets.py: SubSampledDataset, MixtureDataset, create_moving_set); none of that is here: every
item of every set is used, in order.

`finetune_schedule` is the loop's epoch arithmetic (ft/job.py:328-345) as a pure function.
"""
import bisect
import math

import torch


class NamedView(torch.utils.data.Dataset):
    """`dataset` under another `name`, items unchanged (the scoring passes key their results by `name`)."""

    def __init__(self, dataset, name):
        self.dataset, self.name = dataset, name

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, i):
        return self.dataset[i]


class TaggedConcat(torch.utils.data.Dataset):
    """Named data sets one after the other; item i is (x, k) with k the position of the set that index i falls into."""

    def __init__(self, **datasets):
        if not datasets:
            raise ValueError('at least one data set')
        self._classes = tuple(datasets)
        self._datasets = list(datasets.values())
        self._starts = [0]
        for d in self._datasets:
            self._starts.append(self._starts[-1] + len(d))
        self.name = '-'.join(self._classes)

    @property
    def classes(self):
        return self._classes

    @property
    def mix(self):
        """The share of each class in the whole."""
        n = max(len(self), 1)
        return [len(d) / n for d in self._datasets]

    def __len__(self):
        return self._starts[-1]

    def locate(self, i):
        """Index -> (position of its set, index inside that set)."""
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(f'index {i} for length {len(self)}')
        k = bisect.bisect_right(self._starts, i) - 1
        return k, i - self._starts[k]

    def __getitem__(self, i):
        k, j = self.locate(int(i))
        return self._datasets[k][j][0], k

    def which_subsets(self, *tags, which=None):
        """Per tag: the name of its class, or with `which` whether it is that class."""
        for t in tags:
            name = self._classes[int(t)]
            yield name == which if which else name

    def extract_subdataset(self, name, new_name=None):
        """The set of class `name` itself (items as it yields them), called `new_name` when one is given."""
        d = self._datasets[self._classes.index(name)]
        return d if new_name is None else NamedView(d, new_name)


class MovingSet(TaggedConcat):
    """`ind_set` then the sets of `ood_sets` (name -> data set): classes ('ind', 'ood'), items (x, 0) / (x, 1).
    `extract_subdataset('ood')` is the `TaggedConcat` of the OOD sets, whose own `extract_subdataset(name)` gives each back."""

    IND, OOD = 0, 1

    def __init__(self, ind_set, ood_sets):
        if not ood_sets:
            raise ValueError('at least one out-of-distribution set')
        super().__init__(ind=ind_set, ood=TaggedConcat(**ood_sets))


def finetune_schedule(train_size, moving_size, batch_size, epochs=None):
    """The epochs of a fine-tuning run -> (train_size as recorded in ft_params, [batches of each epoch]).

    `epochs` overrides train_size by epochs x moving_size.  There are ceil(train_size / moving_size) epochs; an epoch has
    min(what is left of train_size, moving_size) // batch_size batches (the moving loader drops its last, partial batch) and
    takes that many full batches off train_size."""
    if moving_size <= 0 or batch_size <= 0:
        raise ValueError('an empty moving set or batch')
    if epochs:
        train_size = epochs * moving_size
    recorded = left = int(train_size)
    per_epoch = []
    for _ in range(int(math.ceil(left / moving_size))):
        n = min(left, moving_size) // batch_size
        per_epoch.append(n)
        left -= n * batch_size
    return recorded, per_epoch
