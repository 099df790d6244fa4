"""The seven recorded score families (`odin*`, `regret*`, `knn*`, `maha*`, `ic*`, `dose*`, `ssim*`; module/score_rows.py) on the
host.  No GPU: the models are built on the CPU and nothing is launched.

tests/golden/family_table.json holds what `_ood_methods` and `score_rows.parse` answered, on the grid of family_table_cases.py,
while the families stood in four tables (tools/gen_family_table_golden.py); the one table has to give the same answers."""
import json
import os

import pytest

import family_table_cases as G


@pytest.fixture(scope='module')
def expected(golden_dir):
    with open(os.path.join(golden_dir, 'family_table.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.CASES)
def test_pinned_grid(case, expected):
    assert list(expected[case]) == [str(name) for name in G.NAMES]
    for setting in range(len(G.SETTINGS)):
        got = G.record(case, setting)
        assert list(got) == list(expected[case])
        for name, answers in expected[case].items():
            want, = [answer for answer, settings in answers if setting in settings]
            assert got[name] == want, (case, G.SETTINGS[setting], name)


def test_the_grid_says_something(expected):
    """Every family is listed somewhere and refused somewhere; the opt-ins answer differently with their switch on and off."""
    from module import score_rows
    assert [f.prefix for f in score_rows.FAMILIES] == list(G.PER_FAMILY)
    for prefix, names in G.PER_FAMILY.items():
        answers = [a[0][0] for case in G.CASES for a in expected[case][names[1]]]
        assert [names[1]] in answers and any(a[0] == 'raises' for a in answers), names[1]
        assert prefix == 'odin' or any(len(expected[case][names[0]]) > 1 for case in G.CASES), names[0]
