"""Writes tests/golden/moving_sets/reference_indices.json: which samples the REFERENCE's moving sets hold.

    python tools/gen_moving_set_golden.py --reference <checkout of the reference> [--out FILE]

The reference's ft/datasets.py is imported from the checkout under a stub `utils.torch_load` (torchvision is not needed): the
stub's data sets are called ind (train 500, test 100), a (60), b (90), c32 and u32 (1000 each) and return
((set name, sample index), label) items, so that every item of a mixture names its leaf and its sample.  Recorded per
parameter combination: the classes, the mix, the per-class lengths and the (leaf, sample, tag) list of the moving set, the same
for its 'ood' class and each OOD sub-set, for one combination the list after bar(True); and one SubSampledDataset with its
bar() / bar(False) round trip.  The file holds recorded results only; tests/test_moving_sets_host.py reads nothing else."""
import argparse
import importlib.util
import json
import os
import sys
import types

SIZES = {'ind': (500, 100), 'a': (0, 60), 'b': (0, 90), 'c32': (0, 1000), 'u32': (0, 1000)}

# (moving_size, ood_mix, padding, padding_sets, mix_padding, seed, task)
CASES = [
    (40, 0.5, 0.5, ['c32'], 0., 3, 0), (40, 0.5, 0.5, ['c32'], 0., 3, 1),
    (40, 0.5, 0.5, ['c32'], 0.25, 3, 0), (40, 0.5, 0.5, ['c32'], 0.25, 3, 1),
    (40, 0.3, 0.5, ['c32'], 0.2, 7, 0), (40, 0.3, 0.5, ['c32'], 0.2, 7, 2),
    (64, 0.5, 0.5, ['c32'], 0.2, 7, 5),
    (33, 0.5, 0.5, ['c32'], 0.2, 7, 1),
    (40, 0.5, 0.25, ['c32'], 0., 0, 0),
    (40, 0.5, 1.0, ['c32', 'u32'], 0., 0, 0),
]
BARRED = 4                                                     # the case recorded once more after bar(True)


class Stub:
    def __init__(self, name, n):
        self.name, self.n = name, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < self.n:
            raise IndexError(i)
        return (self.name, i), i % 7


def load_reference(root):
    def get_dataset(name, transformer='default', data_augmentation=[], splits=['train', 'test']):
        train, test = SIZES[name]
        return Stub(name, train), Stub(name, test)
    utils = types.ModuleType('utils')
    utils.torch_load = types.ModuleType('utils.torch_load')
    utils.torch_load.get_dataset = get_dataset
    sys.modules['utils'], sys.modules['utils.torch_load'] = utils, utils.torch_load
    spec = importlib.util.spec_from_file_location('reference_ft_datasets', os.path.join(root, 'ft', 'datasets.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def items(dset):
    out = []
    for i in range(len(dset)):
        (leaf, sample), tag = dset[i]
        out.append([leaf, int(sample), int(tag)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                                                   'moving_sets', 'reference_indices.json'))
    args = ap.parse_args()
    R = load_reference(args.reference)
    doc = {'sizes': {k: {'train': v[0], 'test': v[1]} for k, v in SIZES.items()}, 'ood_sets': ['a', 'b'], 'cases': []}

    sub = R.SubSampledDataset(Stub('b', 90), length=20, seed=5, task=1)
    rec = {'set': 'b', 'length': 20, 'seed': 5, 'task': 1, 'items': items(sub)}
    sub.bar()
    rec.update(bar_length=len(sub), bar_items=items(sub))
    sub.bar(False)
    rec.update(unbar_items=items(sub))
    doc['subsampled'] = rec

    for k, (size, ood_mix, padding, pads, mix_padding, seed, task) in enumerate(CASES):
        m = R.create_moving_set('ind', 'default', [], size, ood_mix, ['a', 'b'], pads, padding=padding, mix_padding=mix_padding,
                                seed=seed, task=task)
        case = {'moving_size': size, 'ood_mix': ood_mix, 'padding': padding, 'padding_sets': pads, 'mix_padding': mix_padding,
                'seed': seed, 'task': task, 'classes': list(m.classes), 'mix': [float(v) for v in m.mix],
                'lengths': [len(d) for d in m.subdatasets], 'items': items(m)}
        ood = m.extract_subdataset('ood')
        case['ood'] = {'classes': list(ood.classes), 'mix': [float(v) for v in ood.mix], 'lengths': [len(d) for d in ood.subdatasets],
                       'items': items(ood), 'subsets': {n: items(ood.extract_subdataset(n)) for n in ood.classes}}
        if k == BARRED:
            m.bar(True)
            case['bar'] = {'lengths': [len(d) for d in m.subdatasets], 'items': items(m)}
        doc['cases'].append(case)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print(args.out, os.path.getsize(args.out), 'bytes,', len(doc['cases']), 'cases')


if __name__ == '__main__':
    main()
