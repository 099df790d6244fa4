"""The grid of tests/test_family_table_host.py and tools/gen_family_table_golden.py: what `_ood_methods` and `score_rows.parse`
answer for every name, model case and setting of the six opt-in switches of the recorded score families.  No GPU: the models are
built on the CPU and nothing is launched."""
import json
import re

from oracle.cases import get_case

CASES = ('c1_n16_mlp', 'a2_n8_vae', 'b2_n8_vib')
SWITCHES = ('OOD_REGRET_METHODS', 'OOD_KNN_METHODS', 'OOD_MAHA_METHODS', 'OOD_IC_METHODS', 'OOD_DOSE_METHODS', 'OOD_SSIM_METHODS')
TYPES = ('REGRET_TYPES', 'IC_TYPES', 'SSIM_TYPES', 'DOSE_TYPES')
# (the switches that are on, whether the four *_TYPES are emptied): all off, each one alone, all on, all on for no type
SETTINGS = [((), False)] + [((s,), False) for s in SWITCHES] + [(SWITCHES, False), (SWITCHES, True)]
# per family: the starred name, a listed row, a well-formed row the model does not list (`maha*`, `ic*` and `ssim*` have none on
# these models: a second listed row), a malformed name, a row with `-2s`
PER_FAMILY = {'odin': ['odin*', 'odin-1-0.0040', 'odin-3-0.0014', 'odinx', 'odin-1-0.0040-2s'],
              'regret': ['regret*', 'regret-5-0.0500', 'regret-4-0.0500', 'regretful', 'regret-5-0.0500-2s'],
              'knn': ['knn*', 'knn-10', 'knn-7', 'knn-x', 'knn-10-2s'],
              'maha': ['maha*', 'maha', 'maha-rel', 'maha-x', 'maha-2s'],
              'ic-': ['ic*', 'ic-bits', 'ic-iws', 'ic-x', 'ic-bits-2s'],
              'dose': ['dose*', 'dose-kl', 'dose-nope', 'dosex', 'dose-2s'],
              'ssim': ['ssim*', 'ssim-mu', 'ssim-cs', 'ssim-x', 'ssim-2s']}
NAMES = ([n for names in PER_FAMILY.values() for n in names] + ['elbo', 'all']
         + [['elbo', names[0], names[1]] for names in PER_FAMILY.values()])


def outcome(call):
    """What `call()` returns, or ('raises', the exception's type, the attribute names its message carries)."""
    try:
        return call()
    except (NotImplementedError, ValueError) as err:
        return ('raises', type(err).__name__, tuple(re.findall(r'[A-Z]+_[A-Z_]+', str(err))))


def ood_methods(net, name):
    got = net._ood_methods(name)
    return ('long', len(got), got[-40:]) if len(got) > 40 else got         # 'all', the ODIN grid: the length and the last 40 names


def parsed(net, name):
    from module import score_rows
    row = score_rows.parse(name, score_rows.traits_of(net))
    return (row.base, row.source, row.kind, row.const, row.roc_mode)


def record(case, setting):
    """{name: (the outcome of _ood_methods, the outcome of parse - per name for a list)} at one grid point, as JSON holds it."""
    from cvae import ClassificationVariationalNetwork as Net
    net = Net(**dict(get_case(case)['net']))
    on, no_types = SETTINGS[setting]
    for s in SWITCHES:
        setattr(net, s, s in on)
    for t in TYPES * no_types:
        setattr(net, t, ())
    got = {str(name): (outcome(lambda: ood_methods(net, name)),
                       [outcome(lambda: parsed(net, n)) for n in name] if isinstance(name, list) else outcome(lambda: parsed(net, name)))
           for name in NAMES}
    return json.loads(json.dumps(got))
