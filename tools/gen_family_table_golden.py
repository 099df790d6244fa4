"""Writes tests/golden/family_table.json: what `_ood_methods` and `score_rows.parse` answer on the grid of
tests/family_table_cases.py (three model cases x nine settings of the six opt-in switches x the names), for
tests/test_family_table_host.py.  Equal answers are grouped: {case: {name: [[answer, [the settings with that answer]], ...]}}.

Run it on the code whose answers are to be pinned - the commit BEFORE a change of the family table, not the changed code.  No GPU.

    python tools/gen_family_table_golden.py
"""
import json
import logging
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)
import family_table_cases as G  # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden', 'family_table.json')


def main():
    logging.disable(logging.WARNING)                           # 'all' says what it leaves out, at every grid point
    grid = {}
    for case in G.CASES:
        by_name = grid[case] = {str(name): [] for name in G.NAMES}
        for setting in range(len(G.SETTINGS)):
            for name, answer in G.record(case, setting).items():
                same = [g for g in by_name[name] if g[0] == answer]
                if same:
                    same[0][1].append(setting)
                else:
                    by_name[name].append([answer, [setting]])
    with open(OUT, 'w') as f:
        json.dump(grid, f, separators=(',', ':'))
        f.write('\n')
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
