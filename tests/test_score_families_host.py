"""The recorded score families (`odin-T-eps`, `regret-steps-lr`, `knn-k`; module/score_rows.py) and the named read-back
(ops.read_back) on the host.  No GPU: the models are built on the CPU and nothing is launched.

The grid pins what `_ood_methods` and `score_rows.parse` answer for every name, model type and setting of the two opt-in switches.
EXPECTED holds the answers of the code as it stood before the families shared one table; the table has to give the same ones."""
import re

import numpy as np
import pytest
import torch

from oracle.cases import get_case

CASES = {'cvae': 'c1_n16_mlp', 'vae': 'a2_n8_vae', 'vib': 'b2_n8_vib'}
SWITCHES = [(False, False), (True, False), (False, True), (True, True)]             # (OOD_REGRET_METHODS, OOD_KNN_METHODS)
NAMES = ['odin', 'odinx', 'odin*', 'odin-1-0.0040', 'odin-3-0.0014', 'regret', 'regretful', 'regret*', 'regret-5-0.0500',
         'regret-5-0.0500-2s', 'regret-4-0.0500', 'knn', 'knn-', 'knn-x', 'knn*', 'knn-10', 'knn-7', 'knn-10-2s', 'elbo', ['elbo', 'knn*']]
ODIN_GRID = 210                                                                     # names: written as ('odin grid', 210) below


def outcome(call):
    """What `call()` returns, or ('raises', the exception's type, the attribute names its message carries)."""
    try:
        return call()
    except (NotImplementedError, ValueError) as err:
        return ('raises', type(err).__name__, tuple(re.findall(r'[A-Z]+_[A-Z_]+', str(err))))


def ood_methods(net, name):
    got = net._ood_methods(name)
    return ('odin grid', len(got)) if got == net._odin_names() else got


def parsed(net, name):
    from module import score_rows
    row = score_rows.parse(name, score_rows.traits_of(net))
    return (row.base, row.source, row.kind, row.const, row.roc_mode)


def record(mtype, regret, knn):
    """{name: (the outcome of _ood_methods, the outcome of parse - per name for a list)} at one grid point."""
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case(CASES[mtype])['net']))
    assert net.type == mtype
    net.OOD_REGRET_METHODS, net.OOD_KNN_METHODS = regret, knn
    return {str(name): (outcome(lambda: ood_methods(net, name)),
                        [outcome(lambda: parsed(net, n)) for n in name] if isinstance(name, list) else outcome(lambda: parsed(net, name)))
            for name in NAMES}


# {type: {name: [((what _ood_methods gives, what parse gives), the (regret, knn) switch settings with that answer), ...]}}
EXPECTED = {'cvae': {'odin': [((('raises', 'NotImplementedError', ()), ('odin', 'odin', None, None, False)),
                    [(False, False), (True, False), (False, True), (True, True)])],
          'odinx': [((('raises', 'NotImplementedError', ()), ('odinx', 'odinx', None, None, False)),
                     [(False, False), (True, False), (False, True), (True, True)])],
          'odin*': [((('raises', 'NotImplementedError', ()), ('odin*', 'odin*', None, None, False)),
                     [(False, False), (True, False), (False, True), (True, True)])],
          'odin-1-0.0040': [((('raises', 'NotImplementedError', ()), ('odin-1-0.0040', 'odin-1-0.0040', None, None, False)),
                             [(False, False), (True, False), (False, True), (True, True)])],
          'odin-3-0.0014': [((('raises', 'NotImplementedError', ()), ('odin-3-0.0014', 'odin-3-0.0014', None, None, False)),
                             [(False, False), (True, False), (False, True), (True, True)])],
          'regret': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                      [(False, False), (False, True)]),
                     ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('raises', 'NotImplementedError', ())), [(True, False), (True, True)])],
          'regretful': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                         [(False, False), (False, True)]),
                        ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('raises', 'NotImplementedError', ())), [(True, False), (True, True)])],
          'regret*': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                       [(False, False), (False, True)]),
                      ((['regret-5-0.0500', 'regret-20-0.0200'], ('raises', 'NotImplementedError', ())), [(True, False), (True, True)])],
          'regret-5-0.0500': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                               [(False, False), (False, True)]),
                              ((['regret-5-0.0500'], ('regret-5-0.0500', 'regret-5-0.0500', None, None, False)), [(True, False), (True, True)])],
          'regret-5-0.0500-2s': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                                  [(False, False), (False, True)]),
                                 ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('regret-5-0.0500', 'regret-5-0.0500', None, None, 'around-mean')),
                                  [(True, False), (True, True)])],
          'regret-4-0.0500': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                               [(False, False), (False, True)]),
                              ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('regret-4-0.0500', 'regret-4-0.0500', None, None, False)),
                               [(True, False), (True, True)])],
          'knn': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())), [(False, False), (True, False)]),
                  ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
          'knn-': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                    [(False, False), (True, False)]),
                   ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
          'knn-x': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                     [(False, False), (True, False)]),
                    ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
          'knn*': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                    [(False, False), (True, False)]),
                   ((['knn-1', 'knn-10', 'knn-50'], ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
          'knn-10': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                      [(False, False), (True, False)]),
                     ((['knn-10'], ('knn-10', 'knn-10', None, None, False)), [(False, True), (True, True)])],
          'knn-7': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                     [(False, False), (True, False)]),
                    ((('raises', 'ValueError', ('KNN_K',)), ('knn-7', 'knn-7', None, None, False)), [(False, True), (True, True)])],
          'knn-10-2s': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                         [(False, False), (True, False)]),
                        ((('raises', 'ValueError', ('KNN_K',)), ('knn-10', 'knn-10', None, None, 'around-mean')), [(False, True), (True, True)])],
          'elbo': [((['elbo'], ('elbo', 'total', 'max-', 1.0, False)), [(False, False), (True, False), (False, True), (True, True)])],
          "['elbo', 'knn*']": [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)),
                                 [('elbo', 'total', 'max-', 1.0, False), ('raises', 'NotImplementedError', ())]),
                                [(False, False), (True, False)]),
                               ((['elbo', 'knn-1', 'knn-10', 'knn-50'],
                                 [('elbo', 'total', 'max-', 1.0, False), ('raises', 'NotImplementedError', ())]),
                                [(False, True), (True, True)])]},
 'vae': {'odin': [((('raises', 'NotImplementedError', ()), ('odin', 'odin', None, None, False)),
                   [(False, False), (True, False), (False, True), (True, True)])],
         'odinx': [((('raises', 'NotImplementedError', ()), ('odinx', 'odinx', None, None, False)),
                    [(False, False), (True, False), (False, True), (True, True)])],
         'odin*': [((('raises', 'NotImplementedError', ()), ('odin*', 'odin*', None, None, False)),
                    [(False, False), (True, False), (False, True), (True, True)])],
         'odin-1-0.0040': [((('raises', 'NotImplementedError', ()), ('odin-1-0.0040', 'odin-1-0.0040', None, None, False)),
                            [(False, False), (True, False), (False, True), (True, True)])],
         'odin-3-0.0014': [((('raises', 'NotImplementedError', ()), ('odin-3-0.0014', 'odin-3-0.0014', None, None, False)),
                            [(False, False), (True, False), (False, True), (True, True)])],
         'regret': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                     [(False, False), (False, True)]),
                    ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('raises', 'NotImplementedError', ())), [(True, False), (True, True)])],
         'regretful': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                        [(False, False), (False, True)]),
                       ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('raises', 'NotImplementedError', ())), [(True, False), (True, True)])],
         'regret*': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                      [(False, False), (False, True)]),
                     ((['regret-5-0.0500', 'regret-20-0.0200'], ('raises', 'NotImplementedError', ())), [(True, False), (True, True)])],
         'regret-5-0.0500': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                              [(False, False), (False, True)]),
                             ((['regret-5-0.0500'], ('regret-5-0.0500', 'regret-5-0.0500', None, None, False)), [(True, False), (True, True)])],
         'regret-5-0.0500-2s': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                                 [(False, False), (False, True)]),
                                ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('regret-5-0.0500', 'regret-5-0.0500', None, None, 'around-mean')),
                                 [(True, False), (True, True)])],
         'regret-4-0.0500': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                              [(False, False), (False, True)]),
                             ((('raises', 'ValueError', ('REGRET_PARAMS',)), ('regret-4-0.0500', 'regret-4-0.0500', None, None, False)),
                              [(True, False), (True, True)])],
         'knn': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())), [(False, False), (True, False)]),
                 ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn-': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())), [(False, False), (True, False)]),
                  ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn-x': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                    [(False, False), (True, False)]),
                   ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn*': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())), [(False, False), (True, False)]),
                  ((['knn-1', 'knn-10', 'knn-50'], ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn-10': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                     [(False, False), (True, False)]),
                    ((['knn-10'], ('knn-10', 'knn-10', None, None, False)), [(False, True), (True, True)])],
         'knn-7': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                    [(False, False), (True, False)]),
                   ((('raises', 'ValueError', ('KNN_K',)), ('knn-7', 'knn-7', None, None, False)), [(False, True), (True, True)])],
         'knn-10-2s': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                        [(False, False), (True, False)]),
                       ((('raises', 'ValueError', ('KNN_K',)), ('knn-10', 'knn-10', None, None, 'around-mean')), [(False, True), (True, True)])],
         'elbo': [((['elbo'], ('elbo', 'total', 'neg', 0.0, False)), [(False, False), (True, False), (False, True), (True, True)])],
         "['elbo', 'knn*']": [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)),
                                [('elbo', 'total', 'neg', 0.0, False), ('raises', 'NotImplementedError', ())]),
                               [(False, False), (True, False)]),
                              ((['elbo', 'knn-1', 'knn-10', 'knn-50'], [('elbo', 'total', 'neg', 0.0, False), ('raises', 'NotImplementedError', ())]),
                               [(False, True), (True, True)])]},
 'vib': {'odin': [((('raises', 'ValueError', ('ODIN_TEMPS', 'ODIN_EPS')), ('odin', 'odin', None, None, False)),
                   [(False, False), (True, False), (False, True), (True, True)])],
         'odinx': [((('raises', 'ValueError', ('ODIN_TEMPS', 'ODIN_EPS')), ('odinx', 'odinx', None, None, False)),
                    [(False, False), (True, False), (False, True), (True, True)])],
         'odin*': [((('odin grid', 210), ('odin*', 'odin*', None, None, False)), [(False, False), (True, False), (False, True), (True, True)])],
         'odin-1-0.0040': [((['odin-1-0.0040'], ('odin-1-0.0040', 'odin-1-0.0040', None, None, False)),
                            [(False, False), (True, False), (False, True), (True, True)])],
         'odin-3-0.0014': [((('raises', 'ValueError', ('ODIN_TEMPS', 'ODIN_EPS')), ('odin-3-0.0014', 'odin-3-0.0014', None, None, False)),
                            [(False, False), (True, False), (False, True), (True, True)])],
         'regret': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                     [(False, False), (True, False), (False, True), (True, True)])],
         'regretful': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                        [(False, False), (True, False), (False, True), (True, True)])],
         'regret*': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                      [(False, False), (True, False), (False, True), (True, True)])],
         'regret-5-0.0500': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                              [(False, False), (False, True)]),
                             ((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('regret-5-0.0500', 'regret-5-0.0500', None, None, False)),
                              [(True, False), (True, True)])],
         'regret-5-0.0500-2s': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                                 [(False, False), (False, True)]),
                                ((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)),
                                  ('regret-5-0.0500', 'regret-5-0.0500', None, None, 'around-mean')),
                                 [(True, False), (True, True)])],
         'regret-4-0.0500': [((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('raises', 'NotImplementedError', ())),
                              [(False, False), (False, True)]),
                             ((('raises', 'NotImplementedError', ('OOD_REGRET_METHODS',)), ('regret-4-0.0500', 'regret-4-0.0500', None, None, False)),
                              [(True, False), (True, True)])],
         'knn': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())), [(False, False), (True, False)]),
                 ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn-': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())), [(False, False), (True, False)]),
                  ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn-x': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                    [(False, False), (True, False)]),
                   ((('raises', 'ValueError', ('KNN_K',)), ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn*': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())), [(False, False), (True, False)]),
                  ((['knn-1', 'knn-10', 'knn-50'], ('raises', 'NotImplementedError', ())), [(False, True), (True, True)])],
         'knn-10': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                     [(False, False), (True, False)]),
                    ((['knn-10'], ('knn-10', 'knn-10', None, None, False)), [(False, True), (True, True)])],
         'knn-7': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                    [(False, False), (True, False)]),
                   ((('raises', 'ValueError', ('KNN_K',)), ('knn-7', 'knn-7', None, None, False)), [(False, True), (True, True)])],
         'knn-10-2s': [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)), ('raises', 'NotImplementedError', ())),
                        [(False, False), (True, False)]),
                       ((('raises', 'ValueError', ('KNN_K',)), ('knn-10', 'knn-10', None, None, 'around-mean')), [(False, True), (True, True)])],
         'elbo': [((['elbo'], ('elbo', 'total', 'neg', 0.0, False)), [(False, False), (True, False), (False, True), (True, True)])],
         "['elbo', 'knn*']": [((('raises', 'NotImplementedError', ('OOD_KNN_METHODS',)),
                                [('elbo', 'total', 'neg', 0.0, False), ('raises', 'NotImplementedError', ())]),
                               [(False, False), (True, False)]),
                              ((['elbo', 'knn-1', 'knn-10', 'knn-50'], [('elbo', 'total', 'neg', 0.0, False), ('raises', 'NotImplementedError', ())]),
                               [(False, True), (True, True)])]}}


@pytest.mark.parametrize('mtype', list(CASES))
@pytest.mark.parametrize('regret,knn', SWITCHES)
def test_pinned_grid(mtype, regret, knn):
    got = record(mtype, regret, knn)
    assert list(got) == list(EXPECTED[mtype])
    for name, answers in EXPECTED[mtype].items():
        want, = [answer for answer, switches in answers if (regret, knn) in switches]
        assert got[name] == want, (mtype, regret, knn, name)


def test_read_back_is_exact_and_one_copy(monkeypatch):
    from jvae_hip import ops
    g = torch.Generator().manual_seed(1)
    fields = {'a': torch.randn(3, 4, generator=g, dtype=torch.float64), 'b': torch.randn(3, generator=g),
              'c': torch.full((3, 2), 2 ** 31 - 1, dtype=torch.int32), 'd': torch.tensor([-7], dtype=torch.int32)}
    fields['c'][1, 0] = -2 ** 31
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda t, *a, **k: copies.append(tuple(t.shape)) or real(t, *a, **k))
    host = ops.read_back(fields)
    monkeypatch.undo()
    assert copies == [(12 + 3 + 6 + 1,)]                                            # ONE transfer, of everything
    assert list(host) == list(fields)
    for k, v in fields.items():
        assert isinstance(host[k], np.ndarray) and host[k].dtype == np.float64 and host[k].shape == tuple(v.shape)
        assert np.array_equal(host[k], v.double().numpy())                          # the widening is exact
    assert host['c'][0, 0] == 2 ** 31 - 1 and host['c'][1, 0] == -2 ** 31 and int(host['d'][0]) == -7
