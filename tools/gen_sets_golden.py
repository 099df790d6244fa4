"""Writes tests/golden/torch_load/names.json: what the REFERENCE's pure name functions (utils/torch_load.py:584-682) return for
the names tests/test_torch_load_host.py asks about.  The reference module imports torchvision and matplotlib at its top; neither
is needed by the name functions, so both are stubbed in sys.modules.  It reads data/sets.ini by a relative path: run with the
reference checkout as --ref (the working directory is moved there for the import and the calls).

    python tools/gen_sets_golden.py --ref /path/to/joint-vae
"""
import argparse
import json
import os
import sys
import types

NAMES = ['cifar10', 'cifar10-3', 'cifar10-0-1-2-3-4-5', 'cifar10+7+9', 'cifar1090', 'mnist', 'mnist90', 'fashion32p', 'fashion32r',
         'letters', 'svhn', 'mnist32r', 'const32', 'uniform28', 'cifar100']
HELDOUT_CALLS = [['cifar10'], ['cifar10', 3], ['cifar10', 5, 1], ['cifar10', 0, 1, 2, 3, 4], ['cifar10', 0, 1, 2, 3, 4, 5],
                 ['mnist', 9, 8, 7, 6, 5, 4, 3], ['cifar100', 99], ['svhn', 2, 0]]


class _AnyMeta(type):
    def __getattr__(cls, attr):
        if attr.startswith('__'):
            raise AttributeError(attr)
        return _AnyMeta(attr, (), {})


def _stub(name):
    class Anything(types.ModuleType):
        def __getattr__(self, attr):
            if attr.startswith('__'):
                raise AttributeError(attr)
            return sys.modules.get(self.__name__ + '.' + attr) or _AnyMeta(attr, (), {})
    sys.modules[name] = Anything(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                                                  'torch_load', 'names.json'))
    a = ap.parse_args()
    for m in ('torchvision', 'torchvision.datasets', 'torchvision.transforms', 'torchvision.utils', 'matplotlib',
              'matplotlib.pyplot'):
        _stub(m)
    out = os.path.abspath(a.out)
    os.chdir(a.ref)
    sys.path.insert(0, a.ref)
    from utils import torch_load as T
    rec = {'names': {}, 'name_by_heldout': []}
    for n in NAMES:
        rec['names'][n] = {'shape_default': T.get_shape_by_name(n), 'shape_pad': T.get_shape_by_name(n, 'pad'),
                           'same_size': T.get_same_size_by_name(n), 'heldout': T.get_heldout_classes_by_name(n),
                           'classes': T.get_classes_by_name(n)}
    rec['same_size_question'] = T.get_same_size_by_name('cifar10-?')
    for call in HELDOUT_CALLS:
        rec['name_by_heldout'].append({'args': call, 'name': T.get_name_by_heldout_classes(*call)})
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1)
    print('wrote', out)


if __name__ == '__main__':
    main()
