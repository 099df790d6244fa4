"""Semi-supervised sets: a labelled dataset with most of its labels hidden (net.SEMI_SUPERVISED reads a negative label as "no
label").  No counterpart in the reference."""
import numpy as np
import torch


def _labels_of(dataset):
    """The label of every sample, as the dataset YIELDS it: `.targets` / `.labels` where nothing stands between them and the
    samples (no target_transform, no look-up table), else the samples' own."""
    labels = getattr(dataset, 'targets', None)
    if labels is None:
        labels = getattr(dataset, 'labels', None)
    if labels is None or getattr(dataset, 'target_transform', None) is not None or getattr(dataset, 'lut', None) is not None:
        return np.asarray([int(dataset[i][1]) for i in range(len(dataset))], dtype=np.int64)
    if torch.is_tensor(labels):
        labels = labels.cpu().numpy()
    return np.asarray(labels, dtype=np.int64)


class HiddenLabels(torch.utils.data.Dataset):
    """Map-style wrapper: sample i of `dataset` with its label replaced by -1 when it is hidden.

    keep_per_class: the number of labels every class keeps (a class with fewer samples keeps them all); keep_fraction: the share
    of its labels every class keeps, rounded to the nearest count; exactly one of the two.  Every class keeps at least one
    label.  The choice is drawn with numpy.random.RandomState(seed) over the sorted indices of each class, the classes in
    ascending order: the same seed hides the same samples.  Samples whose label is already negative stay hidden.

    .hidden (len,) bool - True where the label is hidden; .targets (len,) int64 - the labels as yielded (-1 where hidden)."""

    def __init__(self, dataset, keep_per_class=None, keep_fraction=None, seed=0):
        if (keep_per_class is None) == (keep_fraction is None):
            raise ValueError('HiddenLabels: give keep_per_class or keep_fraction, one of the two')
        if keep_per_class is not None and int(keep_per_class) < 1:
            raise ValueError('HiddenLabels: keep_per_class >= 1 expected, got {!r}'.format(keep_per_class))
        if keep_fraction is not None and not 0. <= float(keep_fraction) <= 1.:
            raise ValueError('HiddenLabels: keep_fraction in [0, 1] expected, got {!r}'.format(keep_fraction))
        self.dataset = dataset
        labels = _labels_of(dataset)
        if len(labels) != len(dataset):
            raise ValueError('HiddenLabels: {} labels for {} samples'.format(len(labels), len(dataset)))
        rng = np.random.RandomState(seed)
        hidden = np.ones(len(labels), dtype=bool)
        for cls in np.unique(labels[labels >= 0]):
            members = np.sort(np.flatnonzero(labels == cls))
            if keep_per_class is not None:
                keep = min(int(keep_per_class), len(members))
            else:
                keep = min(max(int(round(float(keep_fraction) * len(members))), 1), len(members))
            hidden[rng.permutation(members)[:keep]] = False
        self.hidden = torch.from_numpy(hidden)
        self.targets = torch.from_numpy(np.where(hidden, -1, labels).astype(np.int64))

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, i):
        x = self.dataset[i][0]
        return x, int(self.targets[i])
