"""Data sets of the WIM fine-tuning loop (`WIMJob.finetune`), over data-set OBJECTS.

`MovingSet` is the set the fine-tuning moves towards the alternate prior when no `moving_size` is asked for: the
in-distribution test set followed by the out-of-distribution sets, as one data set whose items are `(x, tag)` - tag 0 for an
in-distribution item, 1 for an OOD one - so that the loop knows each sample's group without reading labels back.  Every item
of every set is used, in order.

`SubSampledDataset`, `MixtureDataset` and `create_moving_set` are the reference's seeded moving sets (ft/datasets.py) with its
arithmetic: a permutation of every source set drawn by `np.random.default_rng(seed)`, the `task` number selecting a disjoint
slice of it, an `ood_mix` ratio, padding with further sets (`padding`), padding with held-back in / out samples
(`mix_padding`) and `bar()`, which flips every sub-set to its complement.  `create_moving_set` takes data-set objects, not
names.  Every such set has `resolve()` -> `(leaves, leaf, index, tag)`: the distinct underlying data sets and, per item, the
number of its leaf, the sample index inside that leaf and the top-level class position - the arrays
`ops.ImagesetMixTable` keeps on the device so that a whole mixed batch comes from one launch (`torch_load.mixed_loader`).
`__getitem__` reads the same arrays.  Every index is checked against the length of its leaf when the arrays are built.

Three things the reference does not do, because it raises there:
  * `task=None` (TypeError in the reference) is task 0;
  * `padding == 0` (ZeroDivisionError / ValueError in the reference, whatever the padding sets) builds the moving set without
    the 'pad' class: classes ('ood', 'ind'[, 'padmix']);
  * a `moving_size` the sets cannot fill (ZeroDivisionError in the reference) raises ValueError naming the set that ran out.

`finetune_schedule` is the loop's epoch arithmetic (ft/job.py:328-345) as a pure function.
"""
import bisect
import logging
import math

import numpy as np
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


# ------------------------------------------------------------------------------------------------- seeded moving sets
def _frozen(*arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a, np.int64)
        a.flags.writeable = False
        out.append(a)
    return tuple(out)


class SubSampledDataset(torch.utils.data.Dataset):
    """`length` items of `dataset` after a permutation seeded by `seed`: item i is dataset[perm[(first + i) % n]] with
    first = task x length, so that tasks 0, 1, ... take disjoint slices.  `bar()` turns the set into its complement, the
    samples that follow the slice: first = (task + 1) x the length held before, length n - the length held before;
    `bar(False)` goes back.  `shrink(length)` sets another length (at most what is there), None = everything.  `task=None`
    is task 0."""

    def __init__(self, dataset, length=None, seed=0, task=0):
        self._source, self._seed = dataset, seed
        self._slice = 0 if task is None else int(task)
        self.maxlength = len(dataset)
        self._length = self.maxlength
        self._held = 0                            # while barred: the length of the slice this set is the complement of
        self.barred = False
        self.name = 'sub-{}'.format(getattr(dataset, 'name', 'dataset'))
        if hasattr(dataset, 'classes'):
            self.classes = dataset.classes
        self._perm = self._resolved = None
        self.shrink(length)

    def _room(self):
        return self.maxlength - self._held if self.barred else self.maxlength

    def shrink(self, length=None):
        room = self._room()
        self._length = room if length is None else max(0, min(int(length), room))

    def bar(self, b=True):
        if bool(b) == self.barred:
            return
        if b:
            self._held, self.barred = self._length, True
            self.shrink()
        else:
            self.barred = False
            self.shrink(self._held)

    def __len__(self):
        return self._length

    def _key(self):
        inner = self._source._key() if hasattr(self._source, '_key') else None
        return self._length, self.barred, self._held, inner

    def _positions(self):
        """The position in `dataset` of every item."""
        if self._perm is None:
            self._perm = np.random.default_rng(self._seed).permutation(self.maxlength)
        if self.barred:                           # behind the slice of this task
            first = (self._slice + 1) * self._held
        else:
            first = self._slice * self._length
        around = (first + np.arange(self._length, dtype=np.int64)) % max(self.maxlength, 1)
        return self._perm[around].astype(np.int64)

    def resolve(self):
        """-> (leaves, leaf, index, tag): see the module docstring; tag is 0 over a plain data set, the inner set's over a
        mixture.  The arrays are kept until the set is shrunk or barred and must not be written to."""
        key = self._key()
        if self._resolved is None or self._resolved[0] != key:
            pos, inner = self._positions(), self._source
            if hasattr(inner, 'resolve'):
                leaves, leaf, index, tag = inner.resolve()
                n = len(leaf)
            else:
                leaves, n = [inner], len(inner)
            if pos.size and (int(pos.min()) < 0 or int(pos.max()) >= n):
                raise IndexError('{}: sample {} of the {} of {}'.format(self.name, int(pos.max()), n, getattr(inner, 'name', 'set')))
            if hasattr(inner, 'resolve'):
                arrays = _frozen(leaf[pos], index[pos], tag[pos])
            else:
                arrays = _frozen(np.zeros(len(pos)), pos, np.zeros(len(pos)))
            self._resolved = (key, (leaves, *arrays))
        return self._resolved[1]

    def __getitem__(self, i):
        if isinstance(i, slice):
            raise NotImplementedError('slices of a sub-sampled data set')
        i = int(i)
        if not 0 <= i < self._length:
            raise IndexError('index {} for length {}'.format(i, self._length))
        leaves, leaf, index, tag = self.resolve()
        item = leaves[leaf[i]][int(index[i])]
        return (item[0], int(tag[i])) if hasattr(self._source, 'resolve') else item


def _unit(lengths, shares, rounded=math.floor):
    """The largest whole every part can serve at its share: min over the parts with a share of rounded(length / share)."""
    return min(int(rounded(n / s)) for n, s in zip(lengths, shares) if s > 0)


class MixtureDataset(torch.utils.data.Dataset):
    """Named sub-sets one after the other, each with the share `mix` of the whole; item i is (x, k), k the position of the
    sub-set i falls into (the sub-set's own label is dropped).  A plain data set becomes a `SubSampledDataset(seed, task)`.
    `mix`: None = by the sub-sets' lengths, an int = equal shares, a list, or a dict by name.  `shrink(length)` sets the
    lengths: floor(unit x share) with unit = min(length, min_k floor(len_k / share_k)), then one more for the sub-set furthest
    below length x share until `length` is reached (a sub-set that has no more gives what it has)."""

    def __init__(self, *datasets, mix=None, length=None, seed=0, task=None, **named):
        if datasets and named:
            raise ValueError('data sets either by position or by name')
        if not named:
            named = {str(getattr(d, 'name', i)): d for i, d in enumerate(datasets)}
        if not named:
            raise ValueError('at least one data set')
        self.barred = False
        self._classes = tuple(named)
        self._subsets = [d if isinstance(d, (MixtureDataset, SubSampledDataset)) else SubSampledDataset(d, seed=seed, task=task)
                         for d in named.values()]
        self.name = '-'.join('{}:{}'.format(i, getattr(d, 'name', 'set')) for i, d in enumerate(self._subsets))
        self.num_datasets = len(self._subsets)
        if not mix:
            mix = [len(d) for d in self._subsets]
        elif isinstance(mix, int):
            mix = [1] * self.num_datasets
        elif isinstance(mix, dict):
            mix = [mix[c] for c in self._classes]
        total = sum(mix)
        if len(mix) != self.num_datasets or min(mix) < 0 or not total > 0:
            raise ValueError('{}: no sample to share out (mix {})'.format(self.name, list(mix)))
        self._shares = [float(m / total) for m in mix]                   # as asked for; `mix` is what came out
        self.maxlength = _unit([d.maxlength for d in self._subsets], self._shares, rounded=math.ceil)
        self._resolved = None
        self.shrink(length)

    @property
    def classes(self):
        return self._classes

    @property
    def subdatasets(self):
        return self._subsets

    @property
    def mix(self):
        """The share of each class in the whole, as it came out."""
        return self._came_out

    def __len__(self):
        return self._length

    def _measure(self):
        sizes = [len(d) for d in self._subsets]
        self._length = sum(sizes)
        if not self._length:
            raise ValueError('{}: no sample is left of {}'.format(
                self.name, ', '.join('{} ({})'.format(c, getattr(d, 'name', 'set')) for c, d in zip(self._classes, self._subsets))))
        self._came_out = [n / self._length for n in sizes]

    def shrink(self, length=None):
        unit = _unit([len(d) for d in self._subsets], self._shares)
        if length is None:
            length = unit
        unit = min(unit, length)
        if length > self.maxlength:
            logging.warning('%s: length %d cannot be reached, stopping at %d', self.name, length, self.maxlength)
            length = self.maxlength
        if not length:
            for d in self._subsets:
                d.shrink(0)
            self._length, self._came_out = 0, list(self._shares)
            return
        wanted = [math.floor(unit * share) for share in self._shares]
        for d, n in zip(self._subsets, wanted):
            d.shrink(n)
        aims = [length * share for share in self._shares]
        while sum(wanted) < length:               # one more for the sub-set furthest below its aim (the first of equals)
            k = max(range(self.num_datasets), key=lambda j: aims[j] - wanted[j])
            wanted[k] += 1
            self._subsets[k].shrink(wanted[k])
        self._measure()
        if self._length < 0.9 * length:
            logging.warning('%s: wanted length %d, got %d', '-'.join(self._classes), length, self._length)

    def bar(self, b=True):
        """Every sub-set to its complement (b) or back: a change of the mixture's state flips each sub-set's own."""
        if bool(b) != self.barred:
            for d in self._subsets:
                d.bar(not d.barred)
            self.barred = bool(b)
        self._measure()

    def rename(self, *names, **renamed):
        if names and renamed or names and len(names) != len(self._classes):
            raise ValueError('a name for every class, or old=new pairs')
        self._classes = tuple(names) if names else tuple(renamed.get(c, c) for c in self._classes)

    def which_subsets(self, *tags, which=None):
        """Per tag: the name of its class, or with `which` whether it is that class."""
        for t in tags:
            name = self._classes[int(t)]
            yield name == which if which else name

    def extract_subdataset(self, name, new_name=None):
        """The sub-set of class `name` itself, renamed to `new_name` (None: to the class name)."""
        d = self._subsets[self._classes.index(name)]
        d.name = name if new_name is None else new_name
        return d

    def _key(self):
        return tuple(d._key() for d in self._subsets)

    def resolve(self):
        """-> (leaves, leaf, index, tag): see the module docstring; tag is the position of the sub-set."""
        key = self._key()
        if self._resolved is None or self._resolved[0] != key:
            leaves, parts = [], ([], [], [])
            for k, d in enumerate(self._subsets):
                sub, leaf, index, _ = d.resolve()
                number = []
                for s in sub:
                    where = [j for j, have in enumerate(leaves) if have is s]
                    if not where:
                        leaves.append(s)
                    number.append(where[0] if where else len(leaves) - 1)
                parts[0].append(np.asarray(number, np.int64)[leaf] if len(leaf) else leaf)
                parts[1].append(index)
                parts[2].append(np.full(len(index), k, np.int64))
            self._resolved = (key, (leaves, *_frozen(*(np.concatenate(p) for p in parts))))
        return self._resolved[1]

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError('index {} for length {}'.format(i, len(self)))
        leaves, leaf, index, tag = self.resolve()
        return leaves[leaf[i]][int(index[i])][0], int(tag[i])


def create_moving_set(ind_testset, ood_sets, padding_sets, moving_size, ood_mix, padding=0., mix_padding=0., seed=0, task=0,
                      ood_mix_pad=0.5):
    """The moving set of a fine-tuning run (ft/datasets.py: create_moving_set) from data-set objects: `ood_sets` and
    `padding_sets` are dicts name -> data set.  Classes, in this order:
      'ood'     int(ood_mix x moving_size) items, equal shares of the OOD sets;
      'ind'     the rest of moving_size from `ind_testset`;
      'pad'     int(padding x moving_size) items, equal shares of the padding sets - left out when padding == 0;
      'padmix'  when mix_padding > 0: int(mix_padding x moving_size) items of the COMPLEMENTS of 'ood' and 'ind' (share
                ood_mix_pad of them OOD), so that no sample of it is in 'ind' or 'ood'."""
    task = 0 if task is None else task
    ood_sets, padding_sets = dict(ood_sets), dict(padding_sets or {})
    if not ood_sets:
        raise ValueError('at least one out-of-distribution set')
    for name in padding_sets:
        if name in ood_sets:
            raise ValueError('{} is an out-of-distribution set and a padding set: use mix_padding'.format(name))
    if padding and not padding_sets:
        raise ValueError('padding {} without a padding set'.format(padding))

    ood_set = MixtureDataset(mix=1, seed=seed, task=task, length=int(ood_mix * moving_size), **ood_sets)
    ind_set = SubSampledDataset(ind_testset, seed=seed, task=task, length=moving_size - len(ood_set))
    parts = {'ood': ood_set, 'ind': ind_set}
    if padding:
        share = {name: padding / len(padding_sets) for name in padding_sets}
        parts['pad'] = MixtureDataset(mix=share, seed=seed, task=task, length=int(padding * moving_size), **padding_sets)
    if mix_padding:
        ind_bar = SubSampledDataset(ind_testset, seed=seed, task=task, length=len(ind_set))
        ind_bar.bar()
        ood_bar = MixtureDataset(mix=1, seed=seed, task=task, length=len(ood_set), **ood_sets)
        ood_bar.bar()
        out_share = mix_padding * ood_mix_pad
        parts['padmix'] = MixtureDataset(mix={'ood': out_share, 'ind': mix_padding - out_share}, seed=seed, task=task,
                                         length=int(mix_padding * moving_size), ood=ood_bar, ind=ind_bar)
    for name, part in parts.items():
        if len(part) == 0:
            raise ValueError('moving set of size {}: nothing is left for class {!r} ({})'.format(moving_size, name, part.name))
    return MixtureDataset(mix={name: len(part) for name, part in parts.items()}, seed=seed, task=task, **parts)
